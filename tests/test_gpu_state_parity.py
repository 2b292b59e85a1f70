"""The float32 state of EVERY layer of the inference path against the CPU oracle, bit for bit, in every launch form of the
Winograd F(4x4, 3x3) kernel (csrc/conv_wino4.h) and under weights that keep every layer alive.

The frame tests (test_gpu_parity.py, test_gpu_sequence.py) compare uint8 frames of layer 0 under the synthetic weights, which leave the
layers >= 1 nearly dead: a top-layer output channel can be zeroed without a byte changing (test_state_parity_host.py pins that).  Here R_l,
c_l, P_l and E_l of every layer and image are read back (eigen_debug_state) after steps 1, 2, 4 and 6 of the six roll-outs of the frame test,
under its seven switch settings, with dense random weights -- every bias and peephole non-zero -- and compared by np.array_equal; no
tolerance is chosen.  Cases, weights and the comparison are tests/state_support.py."""
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import state_support as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

EIGEN_ERR_INVALID, EIGEN_ERR_STATE = -1, -3
# what a switch setting runs: the dense weights everywhere, the synthetic ones and both feedbacks of the self-fed piece under the default only
_WSETS = {s: ["dense", "synthetic"] if s is None else ["dense"] for s in ss.SWITCHES}
_REQUANTS = {s: [False, True] if s is None else [False] for s in ss.SWITCHES}
_CHILD_TIMEOUT = 600


def _npz(d, i, wset, mask):
    return os.path.join(d, "oracle_%d_%s_%08x.npz" % (i, wset, mask))


@pytest.fixture(scope="module")
def oracle_dir(tmp_path_factory, oracle_lib):
    """The oracle's states, computed once by the parent: they depend on (roll-out, weights, mask, feedback) only, and three masks serve the seven
    settings.  One .npz per (roll-out, weights, mask): frames and the states after steps 1, 2, 4, 6 under float feedback; where the requantised
    feedback runs, its frames and its state after step 6 (the fed steps do not depend on it)."""
    d = str(tmp_path_factory.mktemp("oracle_states"))
    todo = sorted({(wset, ss.switch_mask(s), len(_REQUANTS[s]) > 1) for s in ss.SWITCHES for wset in _WSETS[s]}, key=lambda t: (t[0], t[1], not t[2]))
    seen = set()
    for wset, mask, both in todo:
        if (wset, mask) in seen:   # (the default setting, which asks for both feedbacks, sorts first)
            continue
        seen.add((wset, mask))
        for i, (w, h, ch, B) in enumerate(ss.ROLLOUTS):
            wts, imgs = ss.WEIGHT_SETS[wset](ch, w, h), ss.images(w, h, ch, B)
            out = ss.pack_states(*ss.oracle_states(oracle_lib, wts, ch, w, h, imgs, mask, False))
            if both:
                fr, st = ss.oracle_states(oracle_lib, wts, ch, w, h, imgs, mask, True, steps=ss.STATE_STEPS[-1:])
                out.update({"q_" + k: v for k, v in ss.pack_states(fr, st).items()})
            np.savez(_npz(d, i, wset, mask), **out)
    yield d
    shutil.rmtree(d, ignore_errors=True)   # (hundreds of MB: not kept with the session's other temporary files)


def _run_pieces(e, d_seq, B, frame, n_fed):
    """the sequence in pieces: ([B, T, C0, H, W] frames, {step count: state})"""
    import torch
    frames, states, fed, steps = [], {}, 0, 0
    for reset, n_in, n_ext in ss.PIECES:
        out = torch.zeros((B, n_in + n_ext, e.c_dim, e.height, e.width), dtype=torch.uint8, device="cuda")
        e.prednet_sequence(d_seq[:, fed:] if n_in else None, n_fed * frame, B, n_in, n_ext, bool(reset), 0, out)
        fed, steps = fed + n_in, steps + n_in + n_ext
        states[steps] = e.debug_state(B)   # (synchronises the stream)
        frames.append(out.cpu().numpy())
    return np.concatenate(frames, axis=1), states


def _child(switch, oracle_dir):
    """One switch setting in a fresh process (the switches are read from the environment once): every roll-out, in pieces and in one call."""
    import torch
    import oracle
    from evolutionary_illusion_generator_amd.engine import Engine
    mask = ss.switch_mask(switch)
    assert oracle.wino_mask_default() == mask
    ok = True
    for i, (w, h, ch, B) in enumerate(ss.ROLLOUTS):
        imgs = ss.images(w, h, ch, B)
        frame = imgs[0].size
        d_seq = torch.from_numpy(np.ascontiguousarray(np.repeat(imgs[:, None], ss.N_FED, axis=1))).cuda()   # [B, N_FED, C0, H, W]: the still image as a sequence
        for wset in _WSETS[switch]:
            wts = ss.WEIGHT_SETS[wset](ch, w, h)
            with np.load(_npz(oracle_dir, i, wset, mask)) as z:
                ref = {k: z[k] for k in z.files}
            ref_fr, ref_st = ss.unpack_states(ref, len(ch), ss.STATE_STEPS)
            for requant in _REQUANTS[switch]:
                if requant:   # the self-fed piece under the requantised feedback: its own frames and final state
                    q_fr, q_st = ss.unpack_states({k[2:]: v for k, v in ref.items() if k.startswith("q_")}, len(ch), ss.STATE_STEPS[-1:])
                    ref_fr, ref_st = q_fr, {**ref_st, **q_st}
                bad = []
                e = Engine(w, h, ch, B, requant_feedback=requant)
                e.set_weights(wts)
                got_fr, got_st = _run_pieces(e, d_seq, B, frame, ss.N_FED)
                for s in ss.STATE_STEPS:
                    ss.compare_states(got_st[s], ref_st[s], s, bad)
                for t in range(got_fr.shape[1]):
                    if not np.array_equal(got_fr[:, t], ref_fr[:, t]):
                        bad.append("frame of step %d: %d bytes differ" % (t + 1, int((got_fr[:, t] != ref_fr[:, t]).sum())))
                # the whole sequence in one call (profiled launches: nothing forks onto the side stream): the final state of the pieces, bit for bit
                one = torch.zeros((B, ss.N_FED + ss.N_SELF, ch[0], h, w), dtype=torch.uint8, device="cuda")
                e.conv_profile(True)
                e.prednet_sequence(d_seq, ss.N_FED * frame, B, ss.N_FED, ss.N_SELF, True, 0, one)
                one_st = e.debug_state(B)
                took = sorted({(r["epi"], r["layer"]) for r in e.conv_profile(False) if r["wino"] and r["launches"]})
                n_bad = len(bad)
                ss.compare_states(one_st, got_st[ss.STATE_STEPS[-1]], ss.STATE_STEPS[-1], bad)
                bad[n_bad:] = ["one call against the pieces, " + ln for ln in bad[n_bad:]]
                if not np.array_equal(one.cpu().numpy(), got_fr):
                    bad.append("one call against the pieces: %d frame bytes differ" % int((one.cpu().numpy() != got_fr).sum()))
                e.close()
                n_tensors = len(ss.STATE_STEPS) * len(ch) * len(ss.TENSORS)
                print("STATE", switch, (w, h, ch, B), wset, "requant" if requant else "float",
                      ("all %d tensors bit-exact at steps %s, frames and the one-call state too" % (n_tensors, ss.STATE_STEPS)) if not bad
                      else "MISMATCH in %d; FIRST: %s" % (len(bad), bad[0]), "| Winograd operators:", took, flush=True)
                for ln in bad[1:]:
                    print("    also:", ln, flush=True)
                ok = ok and not bad
    print("STATE_OK" if ok else "STATE_FAIL", flush=True)


_RUNS = {}
_stop = threading.Event()


def _start_child(switch, oracle_dir):
    """(returncode or None, output).  After a child that ended by a signal or at its time limit, no further child is started."""
    if _stop.is_set():
        return None, "not started: an earlier child process ended by a signal or at its time limit"
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_state_parity as t; t._child(%r, %r)" % (ROOT, switch, oracle_dir)
    try:
        r = subprocess.run([sys.executable, "-c", code], env=ss.switch_env(switch, os.environ), capture_output=True, text=True, timeout=_CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as x:
        _stop.set()
        return None, "time limit of %d s: %s\n%s" % (_CHILD_TIMEOUT, x.stdout, x.stderr)
    if r.returncode < 0:
        _stop.set()
    return r.returncode, r.stdout[-20000:] + ("\n" + r.stderr[-3000:] if r.returncode else "")


@pytest.mark.parametrize("switch", ss.SWITCHES)
def test_state_of_every_layer_bit_exact(cuda, oracle_dir, switch):
    """Six roll-outs x this switch setting (what each setting forces: test_winograd_operators_frames_bit_exact; "parts=1" changes no launch at these shapes,
    whose F(4x4) blocks are all half, tall or packed and do not walk -- test_wino_wide_host.py pins it, test_gpu_wino_wide.py runs the walking wide forms): the sequence of 4 fed + 2 self-fed
    steps runs in pieces -- reset / 1 step, then 1, 2 and the 2 self-fed steps on the kept state -- and R_l, c_l, P_l, E_l of every layer and
    image after each piece equal the oracle's state after steps 1 (the step-0 operators alone), 2, 4 (E_0 live) and 6 (E_0 exactly zero), as do
    the frames; one call over the whole sequence leaves the state of the pieces.  Dense weights under every setting; under the default also
    the synthetic ones and the requantised feedback.  A mismatch names the first differing (step, layer, tensor), image and channel, the box of
    differing pixels in 4 x 4 tiles and the largest difference in ulps, for every differing tensor of the roll-out."""
    if not _RUNS:   # independent fresh processes, started together, four at a time, each under its own time limit; none is started twice
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=4) as pool:
            _RUNS.update(zip(ss.SWITCHES, pool.map(lambda s: _start_child(s, oracle_dir), ss.SWITCHES)))
    rc, out = _RUNS[switch]
    print(out)
    assert rc == 0, (rc, out)
    assert "STATE_OK" in out and "MISMATCH" not in out, out
    assert out.count("bit-exact") == len(ss.ROLLOUTS) * len(_WSETS[switch]) * len(_REQUANTS[switch]), out


def test_default_plan_walking_n_blocks_state_bit_exact(cuda, oracle_lib):
    """What no switch gives: the DEFAULT plan walking N-blocks on its own (csrc/conv_plan.h: walks of three or two N-blocks once the launch
    gives every compute unit four blocks), which at 64 x 64 [3, 48, 96] takes a batch of hundreds.  The batch is eight distinct images repeated,
    plus three, so the last group of blocks is ragged: every copy's state equals its first copy's bit for bit (the batch position does not
    show), and the eight distinct images and the last image of the batch equal the oracle's, after 2 fed + 1 self-fed steps."""
    import torch
    from evolutionary_illusion_generator_amd import engine
    assert not _stop.is_set(), "a child process of this module ended by a signal or at its time limit: nothing more is started on the GPU"
    w, h, ch = ss.WALK_SHAPE
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    walks = lambda B: [r for r in engine.plan_text(ch, w, h, B, n_cu) if r["kernel"] == "wino" and r["nwalk"] > 1]
    B = next((b for b in range(ss.WALK_DISTINCT, 8193, ss.WALK_DISTINCT) if any(r["op"] == "lstm" and r["layer"] == 1 for r in walks(b))), None)
    assert B is not None, "no batch up to 8192 makes ConvLSTM_1 walk on %d compute units" % n_cu
    B += 3
    plan = walks(B)
    print("WALK batch %d on %d compute units:" % (B, n_cu), [(r["op"], r["layer"], r["shape"], "n_nblk=%d" % r["n_nblk"], "nwalk=%d" % r["nwalk"]) for r in plan])
    lstm1 = [r for r in plan if r["op"] == "lstm" and r["layer"] == 1]
    assert lstm1 and lstm1[0]["nwalk"] > 1 and (lstm1[0]["n_nblk"] // lstm1[0]["nwalk"]) * lstm1[0]["tilesX"] * lstm1[0]["tilesY"] * B >= 4 * n_cu, plan
    distinct = ss.images(w, h, ch, ss.WALK_DISTINCT)
    imgs = distinct[np.arange(B) % ss.WALK_DISTINCT]
    wts = ss.dense_weights(ch, w, h)
    T = ss.WALK_FED + ss.WALK_SELF
    e = engine.Engine(w, h, ch, B)
    e.set_weights(wts)
    d_seq = torch.from_numpy(np.ascontiguousarray(np.repeat(imgs[:, None], ss.WALK_FED, axis=1))).to(cuda)
    out = torch.zeros((B, T, ch[0], h, w), dtype=torch.uint8, device=cuda)
    e.prednet_sequence(d_seq, ss.WALK_FED * imgs[0].size, B, ss.WALK_FED, ss.WALK_SELF, True, 0, out)
    got, got_fr = e.debug_state(B), out.cpu().numpy()
    e.close()
    ref_fr, ref = ss.oracle_states(oracle_lib, wts, ch, w, h, distinct, ss.MASK_DEFAULT, False, steps=[T], n_fed=ss.WALK_FED, n_self=ss.WALK_SELF)
    first = np.arange(B) % ss.WALK_DISTINCT
    bad = []
    # the batch position must not show: every image against the first copy of the same image
    ss.compare_states(got, [{k: v[first] for k, v in t.items()} for t in got], T, bad)
    bad = ["copies against their first copy, " + ln for ln in bad]
    if not np.array_equal(got_fr, got_fr[first]):
        bad.append("copies against their first copy: %d frame bytes differ" % int((got_fr != got_fr[first]).sum()))
    # the distinct images and the last image of the batch against the oracle
    pick = list(range(ss.WALK_DISTINCT)) + [B - 1]
    ss.compare_states([{k: v[pick] for k, v in t.items()} for t in got], [{k: v[first[pick]] for k, v in t.items()} for t in ref[T]], T, bad)
    if not np.array_equal(got_fr[pick], ref_fr[first[pick]]):
        bad.append("frames: %d bytes differ from the oracle's" % int((got_fr[pick] != ref_fr[first[pick]]).sum()))
    assert not bad, "\n".join(bad)
    assert all(t["R"].std() > 0.05 for t in got[1:])


def test_debug_state_refusals(cuda):
    """eigen_debug_state: EIGEN_ERR_STATE wherever a reset = 0 call would be refused, EIGEN_ERR_INVALID for a bad layer, `which` or pointer;
    reading the state does not change it."""
    import ctypes
    import torch
    from evolutionary_illusion_generator_amd.engine import Engine, EngineError
    assert not _stop.is_set(), "a child process of this module ended by a signal or at its time limit: nothing more is started on the GPU"
    w, h, ch, B = 32, 16, [3, 8, 12], 3
    e = Engine(w, h, ch, B, n_repeat=2, n_ext=1)
    e.set_weights(ss.dense_weights(ch, w, h))
    buf = np.zeros((B, 2 * ch[1], h // 2, w // 2), np.float32)
    raw = lambda batch, layer, which, p=buf: e.lib.eigen_debug_state(e._h, ctypes.c_int32(batch), ctypes.c_int32(layer), ctypes.c_int32(which),
                                                                       None if p is None else ctypes.c_void_p(p.ctypes.data), None)
    assert raw(B, 1, 0) == EIGEN_ERR_STATE   # no sequence call yet
    imgs = ss.images(w, h, ch, B)
    d = torch.from_numpy(np.ascontiguousarray(np.repeat(imgs[:, None], 2, axis=1))).to(cuda)
    out = torch.zeros((B, 2, ch[0], h, w), dtype=torch.uint8, device=cuda)
    e.prednet_sequence(d, 2 * imgs[0].size, B, 2, 0, True, 0, out)
    assert raw(B, 1, 3) == 0 and buf.any()
    assert raw(B - 1, 1, 0) == EIGEN_ERR_STATE and b"batch of 3" in e.lib.eigen_last_error()   # another batch
    for layer, which, p in [(-1, 0, buf), (len(ch), 0, buf), (1, -1, buf), (1, 4, buf), (1, 0, None)]:
        assert raw(B, layer, which, p) == EIGEN_ERR_INVALID, (layer, which)
    a = e.debug_state(B)
    assert [t["E"].shape for t in a] == [(B, 2 * c, h >> l, w >> l) for l, c in enumerate(ch)] and np.array_equal(a[1]["E"], buf)
    # reading changes nothing: the sequence continues as if it had not been read
    ext = torch.zeros((B, 1, ch[0], h, w), dtype=torch.uint8, device=cuda)
    e.prednet_sequence(None, 0, B, 0, 1, False, 0, ext)
    whole = torch.zeros((B, 3, ch[0], h, w), dtype=torch.uint8, device=cuda)
    e.prednet_sequence(d, 2 * imgs[0].size, B, 2, 1, True, 0, whole)
    torch.cuda.synchronize()
    assert np.array_equal(whole[:, 2].cpu().numpy(), ext[:, 0].cpu().numpy())
    fr = torch.zeros((B, 3, ch[0], h, w), dtype=torch.uint8, device=cuda)
    e.prednet_rollout(torch.from_numpy(imgs).to(cuda), B, 3, 0, fr)   # a roll-out overwrites the kept state
    assert raw(B, 1, 0) == EIGEN_ERR_STATE
    with pytest.raises(EngineError):
        e.debug_state(B)
    e.close()
