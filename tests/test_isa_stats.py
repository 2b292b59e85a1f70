"""Register statistics of the headline Winograd F(4x4) instantiations, read from the AMDGPU metadata of the built library (no GPU needed).

The twelve-wave kernels run at three waves per SIMD, i.e. at most 168 VGPRs; a spill there puts scratch traffic into the same vmcnt as the K loop's
prefetching DMAs.  Every instantiation of the wide and the tall block shape must stay out of scratch, and the SGPRs it keeps in VGPR lanes must not grow
(conv_wino4.h).  Skipped when the library or llvm-readelf is not there."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "libeigen_hip.so")
READELF = shutil.which("llvm-readelf") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")

# wino4_kernel<NI, EPI, TALL, HALF, PACK, NSPLIT> of the two full block shapes, wide and tall (EPI 1 ConvLSTM, 2 ConvA, 3 ConvP), with the SGPRs each may keep in
# VGPR lanes: no more than the build before the spill-free K loop
SGPR_SPILL_CAP = {(4, 1, False): 30, (3, 2, False): 11, (4, 2, False): 11, (3, 3, False): 5, (4, 3, False): 5,
                  (4, 1, True): 8, (3, 2, True): 0, (4, 2, True): 0, (3, 3, True): 0, (4, 3, True): 0}
MAX_VGPR = 168          # three waves per SIMD


def _mangled(ni, epi, tall):
    return "_ZN3eig12wino4_kernelILi%dELi%dELb%dELb0ELb0ELb0EEEvNS_8ConvArgsE" % (ni, epi, int(tall))


def _gfx950_code_objects(blob):
    """The gfx950 entries of every clang offload bundle embedded in the library (one bundle per translation unit)."""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    i = blob.find(magic)
    while i >= 0:
        n = struct.unpack_from("<Q", blob, i + len(magic))[0]
        p = i + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield blob[i + off:i + off + size]
        i = blob.find(magic, i + 1)


def _kernel_stats():
    stats = {}
    blob = open(LIB, "rb").read()
    with tempfile.TemporaryDirectory() as d:
        for k, co in enumerate(_gfx950_code_objects(blob)):
            path = os.path.join(d, "co%d.elf" % k)
            with open(path, "wb") as f:
                f.write(co)
            notes = subprocess.check_output([READELF, "--notes", path], text=True)
            # amdhsa.kernels: one mapping per kernel, its entry starting at "  - ." and its scalar keys indented by four spaces
            for entry in re.split(r"^  - ", notes, flags=re.M)[1:]:
                fields = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)\s*$", entry, re.M))
                if "name" in fields:   # (a kernel instantiated in more than one unit: every copy is checked)
                    stats.setdefault(fields["name"], []).append({k: int(v) for k, v in fields.items() if v.isdigit()})
    return stats


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(LIB):
        pytest.skip("libeigen_hip.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    return _kernel_stats()


@pytest.mark.parametrize("ni,epi,tall", sorted(SGPR_SPILL_CAP))
def test_full_block_wino4_kernels_do_not_spill(stats, ni, epi, tall):
    name = _mangled(ni, epi, tall)
    assert name in stats, "%s not in the library" % name
    for s in stats[name]:
        assert s["private_segment_fixed_size"] == 0, (name, s)
        assert s["vgpr_spill_count"] == 0, (name, s)
        assert s["vgpr_count"] + s.get("agpr_count", 0) <= MAX_VGPR, (name, s)
        assert s["sgpr_spill_count"] <= SGPR_SPILL_CAP[(ni, epi, tall)], (name, s)
