"""CPU side of the state-parity tests (tests/test_gpu_state_parity.py): the oracle's state export, the liveness condition of the dense
weights on every case, the gap the state comparison closes, and the mismatch report.  No GPU."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import state_support as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(w, h, ch, B, ss.N_FED, ss.N_SELF) for w, h, ch, B in ss.ROLLOUTS] + [ss.WALK_SHAPE + (ss.WALK_DISTINCT, ss.WALK_FED, ss.WALK_SELF)]
CASE_IDS = ["%dx%d-%s" % (c[0], c[1], "_".join(map(str, c[2]))) for c in CASES]


@functools.lru_cache(maxsize=None)
def _final_state(i, wset):
    """the oracle's final state of case i (all its images, default mask, float feedback), computed once; read-only by convention"""
    import oracle
    oracle.build()
    w, h, ch, B, n_fed, n_self = CASES[i]
    _, st = ss.oracle_states(oracle, ss.WEIGHT_SETS[wset](ch, w, h), ch, w, h, ss.images(w, h, ch, B), ss.MASK_DEFAULT, False, steps=[n_fed + n_self], n_fed=n_fed, n_self=n_self)
    return st[n_fed + n_self]


def test_the_cases_are_those_of_the_frame_test():
    """the roll-outs and switch settings are restated in state_support.py (the frame test keeps its own inside a script string): they must not drift apart"""
    text = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    assert "for (w, h, ch, B) in [%s]:" % ", ".join(repr(r) for r in ss.ROLLOUTS) in text
    assert "_WINO_SWITCHES = [%s]" % ", ".join("None" if s is None else '"%s"' % s for s in ss.SWITCHES) in text
    assert "synthetic_prednet_weights(ch, w, h, seed=5)" in text and "default_rng(11)" in text and "n_repeat=4, n_ext=2" in text
    assert sorted({ss.switch_mask(s) for s in ss.SWITCHES}) == [0x03FFFFFE, 0x0C0E0E00, 0x0FFFFFFE]   # three oracle runs serve seven settings
    assert [sum(p[1] + p[2] for p in ss.PIECES[:i + 1]) for i in range(len(ss.PIECES))] == ss.STATE_STEPS
    assert ss.STATE_STEPS[-1] == ss.N_FED + ss.N_SELF and ss.N_FED in ss.STATE_STEPS


def test_dense_draw_is_the_training_tests_random_draw():
    from tests import train_support
    w, h, ch = 16, 8, [3, 4, 6]
    a, b = ss.dense_weights(ch, w, h), train_support._random_weights(ch, w, h, seed=2)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]) if k != "ConvP0/b" else (a[k] == 0.5).all(), k
    for k, v in a.items():   # no bias and no peephole is zero: every bias read of every epilogue meets a value
        if v.ndim != 4:
            assert (v != 0).all(), k


def test_debug_state_is_declared_and_exported():
    from evolutionary_illusion_generator_amd import engine
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    assert "int eigen_debug_state(eigen_engine* e, int32_t batch, int32_t layer, int32_t which, float* h_out, void* stream);" in header
    assert "eigen_debug_state" in engine.EXPORTS and engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header
    import oracle
    assert tuple(oracle.STATE_TENSORS) == ss.TENSORS   # `which` 0..3 on both sides


@pytest.mark.parametrize("requant", [False, True])
def test_oracle_state_export(oracle_lib, requant):
    w, h, ch = 32, 16, [3, 8, 12]
    wts = ss.dense_weights(ch, w, h)
    img = ss.images(w, h, ch, 1)[0]
    kw = dict(n_repeat=4, n_ext=2, requant=requant)
    fr, p0, st = oracle_lib.prednet_rollout(wts, ch, w, h, img, return_float=True, state_steps=[1, 2, 4, 5, 6], **kw)
    assert sorted(st) == [1, 2, 4, 5, 6]
    for s, layers in st.items():
        assert [t["R"].shape for t in layers] == [(c, h >> l, w >> l) for l, c in enumerate(ch)]
        assert [t["E"].shape for t in layers] == [(2 * c, h >> l, w >> l) for l, c in enumerate(ch)]
        # P_0 of the state after s steps is the float plane of step s - 1, and the frame its quantisation
        assert np.array_equal(layers[0]["P"], p0[s - 1])
        assert np.array_equal((layers[0]["P"] * np.float32(255.0)).astype(np.int32).astype(np.uint8), fr[s - 1])
        assert all(np.abs(t[k]).max() > 0 for t in layers for k in ("R", "c", "P"))
    # E_0 is what the last executed step CONSUMED: err(its input, P_0 of the step before) -- eigen_debug_state returns the same tensor
    x = img.astype(np.float32) / np.float32(255.0)
    for s in (2, 4):
        assert np.array_equal(st[s][0]["E"], np.concatenate([np.maximum(x - p0[s - 2], 0), np.maximum(p0[s - 2] - x, 0)]))
        assert st[s][0]["E"].any()
    assert np.array_equal(st[1][0]["E"], np.concatenate([x, np.zeros_like(x)]))   # (P_0 = 0 after reset_state())
    for s in (5, 6):   # self-fed: the input IS the previous prediction, or its byte over 255
        fed = fr[s - 2].astype(np.float32) / np.float32(255.0) if requant else p0[s - 2]
        assert np.array_equal(st[s][0]["E"], np.concatenate([np.maximum(fed - p0[s - 2], 0), np.maximum(p0[s - 2] - fed, 0)]))
        assert st[s][0]["E"].any() == requant   # exactly zero under float feedback
    # the states on the way are the final states of shorter runs (steps 1, 2, 4 are fed steps)
    for s in (1, 2, 4):
        fr_s, st_s = oracle_lib.prednet_rollout(wts, ch, w, h, img, n_repeat=s, n_ext=0, requant=requant, state_steps=[s])
        assert np.array_equal(fr_s, fr[:s])
        for l in range(len(ch)):
            for k in ss.TENSORS:
                assert np.array_equal(st_s[s][l][k], st[s][l][k]), (s, l, k)
    # an empty list: the frames of the export there was before, byte for byte, from the plain call and from the C entry itself
    assert np.array_equal(oracle_lib.prednet_rollout(wts, ch, w, h, img, **kw), fr)
    fr0, st0 = oracle_lib.prednet_rollout(wts, ch, w, h, img, state_steps=[], **kw)
    assert st0 == {} and np.array_equal(fr0, fr)
    names = oracle_lib.tensor_names(len(ch))
    arrs = [np.ascontiguousarray(wts[n], dtype=np.float32) for n in names]
    tab = (ctypes.POINTER(ctypes.c_float) * len(arrs))(*[a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in arrs])
    chs = np.asarray(ch, np.int32)
    old = np.zeros_like(fr)
    rc = oracle_lib.lib().eig_oracle_prednet_rollout_wino(
        ctypes.c_int(len(ch)), chs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.c_int(w), ctypes.c_int(h), tab, img.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        ctypes.c_int(4), ctypes.c_int(2), ctypes.c_int(int(requant)), old.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None, ctypes.c_int(0),
        ctypes.c_int(oracle_lib.wino_mask_default()))
    assert rc == 0 and np.array_equal(old, fr)
    with pytest.raises(ValueError):
        oracle_lib.prednet_rollout(wts, ch, w, h, img, state_steps=[7], **kw)
    with pytest.raises(ValueError):
        oracle_lib.prednet_rollout(wts, ch, w, h, img, state_steps=[0], **kw)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_dense_weights_keep_every_layer_alive_and_synthetic_ones_do_not(oracle_lib, i):
    """The condition the dense set must meet in the oracle's final state of every case (state_support.is_live): per layer l >= 1 the share of
    E_l > 0 in [0.2, 0.6], the share of |R_l| in (1e-3, 0.9) >= 0.9, std(R_l) >= 0.05; at most 10 % of P_0 at the clamp.  The synthetic set
    fails the std condition at every layer >= 1 -- the reason there is a second set.  (-s prints the table.)"""
    rows, clamp = ss.liveness(_final_state(i, "dense"))
    syn, syn_clamp = ss.liveness(_final_state(i, "synthetic"))
    for name, rr, cl in (("dense", rows, clamp), ("synthetic", syn, syn_clamp)):
        print("LIVENESS %-28s %-9s P0 at clamp %.3f | " % (CASE_IDS[i], name, cl)
              + " | ".join("l%d: E>0 %.2f, |R| in (1e-3, 0.9) %.3f, std(R) %.3f" % ((l + 1,) + r) for l, r in enumerate(rr)))
    assert ss.is_live(rows, clamp), (CASE_IDS[i], rows, clamp)
    for l, (e, r, s) in enumerate(rows):   # (is_live, spelled out for the report)
        assert 0.2 <= e <= 0.6 and r >= 0.9 and s >= 0.05, (CASE_IDS[i], l + 1, e, r, s)
    assert clamp <= 0.1
    assert all(s < 0.05 for _, _, s in syn), (CASE_IDS[i], syn)
    assert not ss.is_live(syn, syn_clamp)


def _zero_top_convp(wts, L):
    out = dict(wts)
    out["ConvP%d/W" % (L - 1)] = out["ConvP%d/W" % (L - 1)].copy()
    out["ConvP%d/W" % (L - 1)][-1] = 0.0   # the whole last output channel: a dropped N-tile, a skipped edge tile, a mis-indexed bias look like this
    return out


def test_the_gap_frames_miss_a_zeroed_top_channel_under_synthetic_weights(oracle_lib):
    """Why the state is compared at all, pinned: at 64 x 64 [3, 16, 32] under the synthetic weights, zeroing the last output channel of
    ConvP2 leaves every byte of every frame of the 4 + 2 roll-out as it was, while the float state changes at every layer; under the dense
    weights frames and state both change."""
    w, h, ch, B = ss.ROLLOUTS[0]
    assert (w, h, ch) == (64, 64, [3, 16, 32])
    imgs = ss.images(w, h, ch, B)
    seen = {}
    for name, make in ss.WEIGHT_SETS.items():
        wts = make(ch, w, h)
        fr, st = ss.oracle_states(oracle_lib, wts, ch, w, h, imgs, ss.MASK_DEFAULT, False, steps=[ss.STATE_STEPS[-1]])
        fr_z, st_z = ss.oracle_states(oracle_lib, _zero_top_convp(wts, len(ch)), ch, w, h, imgs, ss.MASK_DEFAULT, False, steps=[ss.STATE_STEPS[-1]])
        a, b = st[ss.STATE_STEPS[-1]], st_z[ss.STATE_STEPS[-1]]
        seen[name] = (int((fr != fr_z).sum()), [sum(int((a[l][k] != b[l][k]).sum()) for k in ss.TENSORS) for l in range(len(ch))])
        print("GAP", name, "bytes changed %d of %d; state elements changed per layer %s" % (seen[name][0], fr.size, seen[name][1]))
    assert seen["synthetic"][0] == 0 and all(n > 0 for n in seen["synthetic"][1]), seen
    assert seen["dense"][0] > 0 and all(n > 0 for n in seen["dense"][1]), seen
    # and the comparison of the GPU test reports it: the first differing tensor of the faulty run is at the top layer
    out = []
    ss.compare_states(b, a, ss.STATE_STEPS[-1], out)
    assert len(out) >= len(ch) and all(any(ln.startswith("step 6 layer %d " % l) for ln in out) for l in range(len(ch))), out


def test_mismatch_report_tells_an_edge_tile_from_an_n_block():
    rng = np.random.default_rng(0)
    ref = rng.normal(0, 1, (3, 40, 15, 20)).astype(np.float32)
    got = ref.copy()
    assert ss.ulp_distance(np.float32([1.0, -1.0, 0.0, 1e-45]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0, -1e-45])).tolist() == [1, 0, 0, 2]
    # a wrong ragged bottom tile row (rows 12..14 of 15) in every channel of image 2
    got[2, :, 12:, 16:] = np.nextafter(got[2, :, 12:, 16:], np.float32(9))
    s = ss.describe_mismatch(got, ref)
    assert "first at image 2 channel 0" in s and "rows 3..3 of 4, columns 4..4 of 5" in s and "channels 0..39 (40 of 40)" in s and s.endswith("max 1 ulp"), s
    # a wrong block of output channels over the whole map
    got = ref.copy()
    got[:, 32:] += np.float32(0.5)
    s = ss.describe_mismatch(got, ref)
    assert "first at image 0 channel 32" in s and "rows 0..3 of 4, columns 0..4 of 5" in s and "channels 32..39 (8 of 40)" in s, s
    out = []
    ss.compare_states([{"R": ref, "c": ref, "P": got, "E": ref}], [{k: ref for k in ss.TENSORS}], 4, out)
    assert len(out) == 1 and out[0].startswith("step 4 layer 0 P: first at image 0 channel 32"), out
