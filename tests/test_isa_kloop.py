"""The steady-state K loops of the full-block Winograd F(4x4) instantiations, read from the disassembly of the built library (no GPU needed).

All twelve waves of a block leave the K loop's barrier together, so what a wave executes between the s_barrier and the first MFMA of the next K-block is hidden
behind nothing: it must be an MFMA, after at most the wait for the B operand that was read in front of the barrier.  In particular the U fetch (buffer_load ... lds),
the B read of chunk 1 (ds_read), address arithmetic (VALU) and the loop's back-edge stay out of there (conv_wino4.h: khead / ktail / run).
And the K-block a wave executes again and again carries one taken branch, the back-edge: the plane cursor's change of source is out of line.
Skipped when the library or llvm-objdump is not there.

    python tests/test_isa_kloop.py [LIB]     prints, per instantiation and loop, what stands between the barrier and the MFMA, the loop's branches and its hot path."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_isa_stats import LIB, READELF, SGPR_SPILL_CAP, _gfx950_code_objects, _mangled  # noqa: E402

OBJDUMP = os.path.join(os.path.dirname(READELF), "llvm-objdump")
MFMA = "v_mfma_f32_16x16x4_f32"
MIN_MFMA = 12            # a loop over K-blocks carries at least three chunks of four (NI = 3: four of three) MFMAs
# Scalar instructions between the s_barrier and the MFMA, a cap against regressions.  Parent build, wide ConvLSTM: 18 scalar instructions (loop counters, seven moves of the
# ring rotation, m0 / offset set-up, s_waitcnt) around the exit branch not taken and the taken back-edge, 3 buffer_loads, 1 ds_read and 1 VALU; tall shape: the
# column pass of the A operands (9 to 14 VALU) as well.  This build, all 170 loops: the s_waitcnt for the B operand and nothing else.
MAX_SCALAR = 1


def _is_branch(m):
    return m.startswith("s_cbranch") or m in ("s_branch", "s_setpc_b64", "s_swappc_b64")


def disassemble(lib=LIB):
    """{kernel name: [(address, mnemonic, branch target or None)]} of every gfx950 code object in the library."""
    out = {}
    blob = open(lib, "rb").read()
    with tempfile.TemporaryDirectory() as d:
        for k, co in enumerate(_gfx950_code_objects(blob)):
            path = os.path.join(d, "co%d.elf" % k)
            with open(path, "wb") as f:
                f.write(co)
            text = subprocess.check_output([OBJDUMP, "-d", path], text=True)
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-fA-F]+ <(\S+)>:\s*$", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                    del cur[:]   # (a kernel instantiated in more than one unit: the last copy)
                    continue
                m = re.match(r"^\s+(\S+)(.*?)//\s*([0-9A-Fa-f]+):\s*([0-9A-Fa-f]{8})", line)
                if m and cur is not None:
                    mn, addr, word = m.group(1), int(m.group(3), 16), int(m.group(4), 16)
                    tgt = None
                    if _is_branch(mn) and mn.startswith(("s_cbranch", "s_branch")):   # SOPP: target = next instruction + 4 * simm16
                        simm = word & 0xFFFF
                        tgt = addr + 4 + 4 * (simm - 0x10000 if simm & 0x8000 else simm)
                    cur.append((addr, mn, tgt))
    return out


def _blocks(ins):
    """Basic blocks [(first, last instruction index)], successors per block (indices into the list)."""
    index = {a: i for i, (a, _, _) in enumerate(ins)}
    leaders = {0}
    for i, (_, m, t) in enumerate(ins):
        if _is_branch(m) or m == "s_endpgm":
            if i + 1 < len(ins):
                leaders.add(i + 1)
            if t in index:
                leaders.add(index[t])
    starts = sorted(leaders)
    blocks = [(s0, (starts[k + 1] if k + 1 < len(starts) else len(ins)) - 1) for k, s0 in enumerate(starts)]
    of = {s0: k for k, (s0, _) in enumerate(blocks)}
    succ = []
    for k, (s0, e) in enumerate(blocks):
        _, m, t = ins[e]
        out = []
        if t in index:
            out.append(of[index[t]])
        if not (m in ("s_branch", "s_endpgm", "s_setpc_b64")) and k + 1 < len(blocks):
            out.append(k + 1)   # (falls through: no branch at the end, or a conditional one)
        succ.append(out)
    return blocks, succ


def _dominators(succ):
    """Immediate-dominator sets by the iterative algorithm (entry = block 0); unreachable blocks dominate nothing."""
    n = len(succ)
    order, seen, stack = [], [False] * n, [(0, 0)]
    seen[0] = True
    while stack:
        b, i = stack.pop()
        if i < len(succ[b]):
            stack.append((b, i + 1))
            c = succ[b][i]
            if not seen[c]:
                seen[c] = True
                stack.append((c, 0))
        else:
            order.append(b)
    rpo = order[::-1]
    num = {b: i for i, b in enumerate(rpo)}
    pred = [[] for _ in range(n)]
    for b in rpo:
        for c in succ[b]:
            pred[c].append(b)
    idom = {0: 0}
    changed = True
    while changed:
        changed = False
        for b in rpo[1:]:
            new = None
            for p_ in pred[b]:
                if p_ in idom:
                    if new is None:
                        new = p_
                    else:
                        x, y = p_, new
                        while x != y:
                            while num[x] > num[y]:
                                x = idom[x]
                            while num[y] > num[x]:
                                y = idom[y]
                        new = x
            if idom.get(b) != new:
                idom[b] = new
                changed = True
    return idom, pred


def k_loops(ins):
    """The innermost natural loops, as (header block, sorted blocks [(first, last)]), that contain an s_barrier and at least MIN_MFMA MFMAs."""
    blocks, succ = _blocks(ins)
    idom, pred = _dominators(succ)

    def dominates(a, b):
        while True:
            if a == b:
                return True
            if b not in idom or idom[b] == b:
                return False
            b = idom[b]

    loops = {}
    for b in idom:
        for h in succ[b]:
            if dominates(h, b):   # back edge b -> h
                body, work = loops.setdefault(h, {h}), [b]
                while work:
                    x = work.pop()
                    if x not in body:
                        body.add(x)
                        work.extend(p_ for p_ in pred[x] if p_ in idom)
    res = []
    for h, body in sorted(loops.items()):
        if any(o != h and o in body for o in loops):
            continue   # not innermost
        mn = [ins[i][1] for k in body for i in range(blocks[k][0], blocks[k][1] + 1)]
        if "s_barrier" in mn and mn.count(MFMA) >= MIN_MFMA:
            res.append((blocks[h], sorted(blocks[k] for k in body)))
    return res


def loop_mnemonics(ins, loop):
    return [ins[i][1] for s0, e in loop[1] for i in range(s0, e + 1)]


def loop_branches(ins, loop):
    """(mnemonic, 'back' or 'fwd' or 'exit') of every branch of the loop."""
    inside = {i for s0, e in loop[1] for i in range(s0, e + 1)}
    index = {a: i for i, (a, _, _) in enumerate(ins)}
    res = []
    for i in sorted(inside):
        a, m, t = ins[i]
        if t is not None:
            res.append((m, "exit" if index.get(t) not in inside else ("back" if t <= a else "fwd")))
    return res


def behind_barrier(ins, loop):
    """Per s_barrier of the loop: the mnemonics from it to the next MFMA, straight on in address order (the walk ends behind the first branch it meets: there is
    no telling from the code which way it goes, and none belongs there)."""
    res = []
    for s0, e in loop[1]:
        for i in range(s0, e + 1):
            if ins[i][1] == "s_barrier":
                mns, j = [], i + 1
                while j < len(ins) and not ins[j][1].startswith("v_mfma"):
                    mns.append(ins[j][1])
                    if _is_branch(ins[j][1]):
                        break
                    j += 1
                res.append(mns)
    return res


def hot_path(ins, loop):
    """The branches met from the loop's header straight on, conditional branches on the scalar / vector condition codes falling through, up to the first one that is
    taken whatever the data: s_branch, or s_cbranch_exec(n)z (the compiler's always-taken branch over a block laid out in line).  -> ([mnemonics], target index)"""
    index = {a: i for i, (a, _, _) in enumerate(ins)}
    met, j = [], loop[0][0]
    while j < len(ins):
        _, m, t = ins[j]
        if _is_branch(m):
            met.append(m)
            if m == "s_branch" or m.startswith("s_cbranch_exec"):
                return met, index.get(t)
        j += 1
    return met, None


def classify(mns):
    c = {"buffer_load": 0, "ds": 0, "valu": 0, "branch": 0, "scalar": 0, "other": 0}
    for m in mns:
        if m.startswith("buffer_load"):
            c["buffer_load"] += 1
        elif m.startswith("ds_"):
            c["ds"] += 1
        elif _is_branch(m):
            c["branch"] += 1
        elif m.startswith("v_"):
            c["valu"] += 1
        elif m.startswith("s_"):
            c["scalar"] += 1
        else:
            c["other"] += 1
    return c


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("libeigen_hip.so not built")
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not found")
    return disassemble()


@pytest.mark.parametrize("ni,epi,tall", sorted(SGPR_SPILL_CAP))
def test_an_mfma_is_first_behind_the_k_loop_barrier(kernels, ni, epi, tall):
    name = _mangled(ni, epi, tall)
    assert name in kernels, "%s not in the library" % name
    ins = kernels[name]
    loops = k_loops(ins)
    # six rows xi of the position grid, each with a loop over full K-blocks; the ConvLSTM also one over unpooled-source K-blocks (xi = 2 multiplies nothing there)
    assert len(loops) >= 6, (name, len(loops))
    for loop in loops:
        for mns in behind_barrier(ins, loop):
            c = classify(mns)
            where = (name, hex(ins[loop[0][0]][0]), mns)
            assert c["buffer_load"] == 0 and c["ds"] == 0 and c["valu"] == 0 and c["branch"] == 0 and c["other"] == 0, where
            assert c["scalar"] <= MAX_SCALAR, where
        # one taken branch per K-block: from the header straight on, the first branch taken whatever the data is the back-edge (parent build: an s_cbranch_execnz
        # over the plane cursor's source switch, and the back-edge behind it)
        met, target = hot_path(ins, loop)
        assert met and met[-1] == "s_branch" and target == loop[0][0], (name, hex(ins[loop[0][0]][0]), met)
        assert not any(m.startswith("s_cbranch_exec") for m in met), (name, met)


if __name__ == "__main__":
    ks = disassemble(sys.argv[1] if len(sys.argv) > 1 else LIB)
    for key in sorted(SGPR_SPILL_CAP):
        ins = ks[_mangled(*key)]
        print("wino4_kernel<%d, %d, tall=%d>" % key)
        for loop in k_loops(ins):
            mn = loop_mnemonics(ins, loop)
            for mns in behind_barrier(ins, loop):
                print("  loop at %#x: %d instructions, %d MFMAs, branches %s; hot path %s; behind the barrier %s %s"
                      % (ins[loop[0][0]][0], len(mn), mn.count(MFMA), loop_branches(ins, loop), hot_path(ins, loop)[0], {k: n for k, n in classify(mns).items() if n}, mns))
