"""The WIDE block shape of the F(4x4) Winograd kernel (csrc/conv_wino4.h) in the launch forms of the headline plan -- walks of two and three N-blocks, blocks that
start at a later part of their tile's N-blocks, NI = 3 and NI = 4 ConvA / ConvP, maps ragged at the right and bottom edge -- against the CPU oracle, bit for bit,
under weights that keep every layer alive.

At test sizes the default plan takes half, tall or packed blocks, so the other state tests (tests/test_gpu_state_parity.py) reach these forms in one roll-out only.
Here EIGEN_W4_TALL=0 / EIGEN_W4_HALF=0 force the wide shape and EIGEN_W4_PARTS the split on nine small nets at batch 3; R_l, c_l, P_l, E_l of every layer after each
of 2 fed + 1 self-fed steps and all frames are compared by np.array_equal with the oracle's under the same operator-form mask; no tolerance is chosen.  Before a
net runs, the child asks the planner what ITS process is about to launch (engine.plan_text(switches=None), the device's compute-unit count) and asserts the cells
tests/test_wino_wide_host.py counted.  Cases, settings and cells are tests/wino_wide_support.py; profiles/wino_wide_cells.txt holds a run's record."""
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import state_support as ss
from tests import wino_wide_support as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

_CHILD_TIMEOUT = 300


def _npz(d, i, mask):
    return os.path.join(d, "wide_%d_%08x.npz" % (i, mask))


@pytest.fixture(scope="module")
def oracle_dir(tmp_path_factory, oracle_lib):
    """The oracle's frames and states after steps 1, 2, 3, computed once by the parent: one .npz per (net, operator-form mask)."""
    d = str(tmp_path_factory.mktemp("oracle_wide"))
    for i, mask in sorted({(i, ws.SETTINGS[name].mask) for name, i in ws.CASES}):
        np.savez(_npz(d, i, mask), **ss.pack_states(*ws.oracle_states(oracle_lib, i, mask)))
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run_pieces(e, d_seq, frame):
    """the sequence in pieces: ([B, T, C0, H, W] frames, {step count: state})"""
    import torch
    frames, states, fed, steps = [], {}, 0, 0
    for reset, n_in, n_ext in ws.PIECES:
        out = torch.zeros((ws.BATCH, n_in + n_ext, e.c_dim, e.height, e.width), dtype=torch.uint8, device="cuda")
        e.prednet_sequence(d_seq[:, fed:] if n_in else None, ws.N_FED * frame, ws.BATCH, n_in, n_ext, bool(reset), 0, out)
        fed, steps = fed + n_in, steps + n_in + n_ext
        states[steps] = e.debug_state(ws.BATCH)   # (synchronises the stream)
        frames.append(out.cpu().numpy())
    return np.concatenate(frames, axis=1), states


def _child(name, oracle_dir):
    """One setting in a fresh process (the switches are read from the environment once): each of its nets, in pieces and in one call."""
    import torch
    import oracle
    from evolutionary_illusion_generator_amd import engine
    mask = ws.SETTINGS[name].mask
    assert oracle.wino_mask_default() == mask and engine.load_library().eigen_winograd_mask() == mask
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ok = True
    for i in ws.SETTINGS[name].nets:
        w, h, ch = ws.NETS[i]
        # what this process is about to launch (its own switches and mask, this device) is wide, walks no further than the planner's rule, and holds the census's cells
        cells = ws.case_cells(engine.plan_text, name, i, ws.BATCH, n_cu, switches=None)
        assert cells.keys() == ws.case_cells(engine.plan_text, name, i).keys(), (name, ws.NETS[i], sorted(cells))
        for c, ops in sorted(cells.items()):
            print("CELL|%s|%dx%d %s|%s|%s" % (name, w, h, ch, ws.cell_name(c), " ".join("%s_%d" % o for o in ops)), flush=True)
        imgs = ws.images(i)
        frame = imgs[0].size
        d_seq = torch.from_numpy(np.ascontiguousarray(np.repeat(imgs[:, None], ws.N_FED, axis=1))).cuda()   # [B, N_FED, C0, H, W]: the still image as a sequence
        with np.load(_npz(oracle_dir, i, mask)) as z:
            ref_fr, ref_st = ss.unpack_states({k: z[k] for k in z.files}, len(ch), ws.STATE_STEPS)
        bad = []
        e = engine.Engine(w, h, ch, ws.BATCH)
        e.set_weights(ws.weights(i))
        got_fr, got_st = _run_pieces(e, d_seq, frame)
        for s in ws.STATE_STEPS:
            ss.compare_states(got_st[s], ref_st[s], s, bad)
        for t in range(got_fr.shape[1]):
            if not np.array_equal(got_fr[:, t], ref_fr[:, t]):
                bad.append("frame of step %d: %d bytes differ" % (t + 1, int((got_fr[:, t] != ref_fr[:, t]).sum())))
        # the whole sequence in one call (profiled launches): the final state and the frames of the pieces, bit for bit
        T = ws.N_FED + ws.N_SELF
        one = torch.zeros((ws.BATCH, T, ch[0], h, w), dtype=torch.uint8, device="cuda")
        e.conv_profile(True)
        e.prednet_sequence(d_seq, ws.N_FED * frame, ws.BATCH, ws.N_FED, ws.N_SELF, True, 0, one)
        one_st = e.debug_state(ws.BATCH)
        took = sorted({(r["epi"], r["layer"]) for r in e.conv_profile(False) if r["wino"] and r["launches"]})
        n_bad = len(bad)
        ss.compare_states(one_st, got_st[T], T, bad)
        bad[n_bad:] = ["one call against the pieces, " + ln for ln in bad[n_bad:]]
        if not np.array_equal(one.cpu().numpy(), got_fr):
            bad.append("one call against the pieces: %d frame bytes differ" % int((one.cpu().numpy() != got_fr).sum()))
        e.close()
        assert len(took) == len({op for ops in cells.values() for op in ops}), (took, cells)   # as many operators ran in F(4x4) as the plan has
        n_tensors = len(ws.STATE_STEPS) * len(ch) * len(ss.TENSORS)
        print("WIDE", name, (w, h, ch, ws.BATCH), ("all %d tensors bit-exact at steps %s, frames and the one-call state too" % (n_tensors, ws.STATE_STEPS)) if not bad
              else "MISMATCH in %d; FIRST: %s" % (len(bad), bad[0]), "| Winograd operators:", took, flush=True)
        for ln in bad[1:]:
            print("    also:", ln, flush=True)
        ok = ok and not bad
    print("WIDE_OK" if ok else "WIDE_FAIL", flush=True)


_RUNS = {}
_stop = threading.Event()


def _start_child(name, oracle_dir):
    """(returncode or None, output).  After a child that ended by a signal or at its time limit, no further child is started."""
    if _stop.is_set():
        return None, "not started: an earlier child process ended by a signal or at its time limit"
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_wino_wide as t; t._child(%r, %r)" % (ROOT, name, oracle_dir)
    try:
        r = subprocess.run([sys.executable, "-c", code], env=ws.setting_env(name, os.environ), capture_output=True, text=True, timeout=_CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as x:
        _stop.set()
        return None, "time limit of %d s: %s\n%s" % (_CHILD_TIMEOUT, x.stdout, x.stderr)
    if r.returncode < 0:
        _stop.set()
    return r.returncode, r.stdout[-80000:] + ("\n" + r.stderr[-3000:] if r.returncode else "")


def _runs(oracle_dir):
    if not _RUNS:   # independent fresh processes, started together (three: at most four at a time), each under its own time limit; none is started twice
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=4) as pool:
            _RUNS.update(zip(ws.SETTINGS, pool.map(lambda s: _start_child(s, oracle_dir), ws.SETTINGS)))
    return _RUNS


@pytest.mark.parametrize("name", list(ws.SETTINGS))
def test_wide_blocks_state_of_every_layer_bit_exact(cuda, oracle_dir, name):
    """The nets of this setting on forced wide blocks: reset / 1 step (the step-0 twins alone), 1 fed step, 1 self-fed step on the kept state; R_l, c_l, P_l, E_l of
    every layer and image after each piece and every frame equal the oracle's, and one call over the whole sequence leaves the state and the frames of the pieces.
    A mismatch names the first differing (step, layer, tensor), image and channel, the box of differing pixels in 4 x 4 tiles -- an edge tile and an N-block look
    different there -- and the largest difference in ulps."""
    rc, out = _runs(oracle_dir)[name]
    print(out)
    assert rc == 0, (rc, out)
    assert "WIDE_OK" in out and "MISMATCH" not in out, out
    assert out.count("bit-exact") == len(ws.SETTINGS[name].nets), out


def test_the_cells_that_ran_are_the_census(cuda, oracle_dir):
    """The union of the cells the children planned for their own process on this device is the union the host census plans (tests/test_wino_wide_host.py), and it
    holds every required cell."""
    from evolutionary_illusion_generator_amd import engine
    ran = {ln.split("|")[3] for _, out in _runs(oracle_dir).values() for ln in out.splitlines() if ln.startswith("CELL|")}
    census = {c for name, i in ws.CASES for c in ws.case_cells(engine.plan_text, name, i)}
    assert ran == {ws.cell_name(c) for c in census}, sorted(ran ^ {ws.cell_name(c) for c in census})
    assert ws.missing_cells(engine.plan_text, census) == []
