"""Every kernel header goes into exactly one translation unit (no GPU, no library needed).

A non-template, non-static ``__global__`` is a strong external symbol on the host side, so a header that defines one and reaches two units
of ``HIP_UNITS`` through their ``#include "..."`` closures is a duplicate-symbol error at link time, which names a mangled kernel and
not the header.  This names the header."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")


def _code(path):
    """the file's text without its comments"""
    text = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _closure(path, seen=None):
    """path and every file it reaches through #include "...", resolved against the including file's directory"""
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _code(path), re.M):
        _closure(os.path.join(os.path.dirname(path), name), seen)
    return seen


def _strong_kernels(path):
    """The guards of every __global__ of the file that is neither static nor a template (what stands between the end of the previous
    declaration and the keyword says which): one set per kernel of the NAMEs of the `#ifdef NAME` blocks around it, empty outside any."""
    found, stack, decl = [], [], ""
    for line in _code(path).split("\n"):
        d = re.match(r"\s*#\s*(ifdef|ifndef|if|endif)\b\s*(\w*)", line)
        if d:
            if d.group(1) == "endif":
                stack.pop()
            else:
                stack.append(d.group(2) if d.group(1) == "ifdef" else None)
            continue
        for part in re.split(r"(__global__)", line):
            if part == "__global__":
                if not re.search(r"\b(static|template)\b", re.split(r"[;}]", decl)[-1]):
                    found.append({g for g in stack if g})
            decl = (decl + " " + part)[-4000:]
    return found


def _homes(header, guards, closures):
    """the units a kernel of `header` under `guards` is compiled into: those that reach the header and define every guard"""
    defined = lambda unit, g: any(re.search(r"^\s*#\s*define\s+%s\b" % g, _code(f), re.M) for f in closures[unit])
    return sorted(u for u, c in closures.items() if header in c and all(defined(u, g) for g in guards))


def test_every_kernel_header_lies_in_exactly_one_unit():
    import __graft_entry__ as ge
    closures = {u: _closure(os.path.join(CSRC, u)) for u in ge.HIP_UNITS}
    headers = sorted(os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith(".h"))
    strong = {h: k for h in headers for k in [_strong_kernels(h)] if k}
    assert strong, "no kernel header found: the scan is broken"
    for h, kernels in strong.items():
        for guards in kernels:
            homes = _homes(h, guards, closures)
            assert len(homes) == 1, "%s defines a non-static, non-template __global__ and is compiled into %s: it must reach exactly one unit" % (
                os.path.basename(h), homes or "no unit")
    # the scan tells the kinds apart: a strong kernel header, one whose kernels are all static (two units include it), one with none
    names = [os.path.basename(h) for h in strong]
    assert "train_kernels.h" in names and "flow_obj_kernels.h" in names and "flow_kernels.h" not in names and "train_common.h" not in names
    assert sum(os.path.join(CSRC, "flow_kernels.h") in c for c in closures.values()) == 2
