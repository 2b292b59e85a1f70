"""The flow objective's score mode on the GPU (eigen_trainer_flow_term_score, eigen_trainer_loss_grad_flow_score, train.FlowScore);
DESIGN.md section 13, "The score mode".  The stage alone is compared with the numpy restatement of tests/flow_score_support.py: the
solve's field bit for bit, the per-sample record within the bound of a double-precision sum, and everything that follows the record
(q, the seed, the reference gradient) bit for bit once the restatement is fed the device's own record.  A training call is compared with
`run_flow(term=...)`, float64 autograd of the same score on the predictions, which tests/test_flow_score_host.py keeps under the float32
yardstick; `score=None` through the new entry gives the bits of eigen_trainer_loss_grad_flow_pair."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.train import FlowObjective, FlowScoreSettings, FlowSettings, PredictionFlow, PredNetTrainer
from tests import flow_obj_support as fs
from tests import flow_ref_support as rs
from tests import flow_score_support as ss
from tests.flow_gpu_support import SENT, _p, _padded, _raw_loss_grad, _unpad
from tests.frame_grad_support import case_inputs, check_frame_grads, fold_tied, zero_steps
from tests.train_support import _check_grads, case_weights

pytestmark = pytest.mark.gpu

WORST = {"norm": 0.0, "element": 0.0, "loss": 0.0, "frames": 0.0}
STAGE = [(w, h, C, r, masked, ref_kind, mc) for w, h, C, r, masked in ss.STAGE_CASES for ref_kind, _ in ss.REFS for mc in ss.MIN_COUNTS]
stage_id = lambda c: "%dx%dx%d-r%d-%s-min%d" % (c[0], c[1], c[2], c[3], c[5], c[6])


def _settings(sc):
    return FlowScoreSettings(sc.max_norm, sc.min_norm, sc.r_min, sc.r_max, sc.w_direction, sc.w_strength, sc.min_count, 0)


def _raw_score(tr, d_pred, p_b, d_ref, float_ref, r_b, B, radius, eps, d_mask, score, scale, value, stats, d_flow, d_seed, s_b, d_rg, rg_b, flags=0, both=False):
    """eigen_trainer_flow_term_score called directly on device buffers; score: FlowScoreSettings or None; stats: numpy [B, 10] or None"""
    cfg = FlowSettings(radius, flags, eps)
    ref = (_p(d_ref), _p(d_ref)) if both else (None, _p(d_ref)) if float_ref else (_p(d_ref), None)
    return tr.lib.eigen_trainer_flow_term_score(tr._h, _p(d_pred), p_b, ref[0], ref[1], r_b, B, ctypes.byref(cfg), _p(d_mask), None if score is None else ctypes.byref(score),
                                                ctypes.c_double(scale), None if value is None else ctypes.byref(value),
                                                None if stats is None else ctypes.c_void_p(stats.ctypes.data), _p(d_flow), _p(d_seed), s_b, _p(d_rg), rg_b, None)


def _sum_bound(terms):
    """(the exact sum, N 2^-53 sum |terms|: the bound of a double-precision sum of the N terms in any order)"""
    t = np.asarray(terms, np.float64).ravel().tolist()
    return math.fsum(t), len(t) * 2.0 ** -53 * math.fsum(abs(v) for v in t)


@pytest.mark.parametrize("case", STAGE, ids=stage_id)
def test_the_stage_is_the_numpy_restatement(cuda, case):
    """`flow_term` (a byte reference) and `flow_term_pair` (a float one) with a score, B = 2, scale 0.75:
    u `np.array_equal` the restatement's; N exact; every first-pass sum N m of the record within N 2^-53 sum |terms| of the exactly
    summed one, and every N V likewise against the exactly summed squared deviations from the device's own means; S_b and f within 1e-10
    of the restatement, and exactly what the restatement forms from the device's record; with that record the seed and the reference
    gradient are the restatement's bit for bit; the seed is within 2^-23 |ref| + 1e-9 max |ref| of float64 autograd (the float rounding of
    the output, and float64 sums under the 1 / min_norm amplification); a sample below min_count has value 0 and an exactly zero seed
    and reference gradient; on padded strides the entry returns the same bits and leaves the padding alone; every output is optional."""
    w, h, C, r, masked, ref_kind, mc = case
    B = ss.B_STAGE
    pred, ref, ref64, mask, sc = ss.stage_case(w, h, C, r, masked, ref_kind, mc)
    float_ref = ref_kind == "floats"
    flow = ss.flow_of(sc, r, mask=mask, pairing="prediction" if float_ref else "frame")
    want = ss.score_stage_ref(pred, ref64, r, 1e-2, mask, sc, scale=0.75)
    per = C * h * w
    with PredNetTrainer("synthetic", [C, 4], w, h, B + 1, 2) as tr:
        stage = tr.flow_term_pair if float_ref else tr.flow_term
        v0, u0, s0 = stage(pred, ref, flow, scale=0.75)
        v, u, seed, rg = stage(pred, ref, flow, scale=0.75, reference_grad=True)
        rec = tr.last_flow_stats
        if not float_ref:    # flow_term also returns the record
            again = tr.flow_term(pred, ref, flow, scale=0.75, reference_grad=True, stats=True)
            assert again[0] == v and again[3].tobytes() == rg.tobytes() and again[4].tobytes() == rec.tobytes() and again[4] is tr.last_flow_stats
        assert v == v0 and u.tobytes() == u0.tobytes() and seed.tobytes() == s0.tobytes()
        assert np.array_equal(u, want.u), np.abs(u - want.u).max()
        pts = want.score.points
        assert rec.shape == (B, ss.REC) and np.array_equal(rec[:, 0], want.score.record[:, 0]) and not rec[:, 9].any()
        for b in range(B):
            m, N = pts.member[b], rec[b, 0]
            cols = [pts.rho[b][m], pts.tau[b][m], np.abs(want.u[b, 0][m]), pts.nrm[b][m]]
            for k, t in enumerate(cols):
                exact, bound = _sum_bound(t)
                assert abs(N * rec[b, 1 + k] - exact) <= bound, (b, k, N * rec[b, 1 + k], exact, bound)
            for k, (t, mean) in enumerate(((cols[0], rec[b, 1]), (cols[1], rec[b, 2]), (cols[3], rec[b, 4]))):
                exact, bound = _sum_bound((t - mean) * (t - mean))
                assert abs(N * rec[b, 5 + k] - exact) <= bound, (b, k, N * rec[b, 5 + k], exact, bound)
            assert abs(rec[b, 8] - want.score.S[b]) <= 1e-10 and rec[b, 8] == ss.sample_value(rec[b], sc)
        assert abs(v - want.value) <= 1e-10, (v, want.value)
        fed = ss.score_stage_ref(pred, ref64, r, 1e-2, mask, sc, scale=0.75, record=rec)
        assert v == fed.value
        assert np.array_equal(seed, fed.seed), np.abs(seed - fed.seed).max()
        assert np.array_equal(rg, fed.grad), np.abs(rg - fed.grad).max()
        P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
        f, _, _ = ss.torch_score_term(P, torch.from_numpy(ref64.copy()), r, 1e-2, mask, sc)
        (g,) = torch.autograd.grad(0.75 * f, P)
        g = g.numpy()
        assert (np.abs(seed - g) <= 2.0 ** -23 * np.abs(g) + 1e-9 * np.abs(g).max()).all(), np.abs(seed - g).max() / np.abs(g).max()
        below = rec[:, 0] < mc
        assert below.sum() == (1 if mc == 25 and (w, h) == (12, 8) else 0)
        for b in range(B):
            if below[b]:
                assert rec[b, 8] == 0.0 and not seed[b].any() and not rg[b].any()
            else:
                assert rec[b, 8] > 0 and seed[b].any() and rg[b].any()
        # the entry itself on padded strides, with and without the optional outputs
        p_b, r_b, s_b, g_b = per + 5, per + 3, per + 7, per + 11
        d_pred = _padded(pred, p_b, np.float32(np.nan), cuda)
        d_ref = _padded(ref, r_b, np.float32(np.nan) if float_ref else np.uint8(7), cuda)
        d_mask = None if mask is None else torch.from_numpy(mask).to(cuda)
        for with_all in (True, False):
            d_rg = torch.full((B * g_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
            d_seed = torch.full((B * s_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
            d_flow = torch.full((B * 2 * h * w + 4,), float(SENT), dtype=torch.float64, device=cuda) if with_all else None
            value, stats = ctypes.c_double(), np.full((B + 1, ss.REC), float(SENT))
            assert _raw_score(tr, d_pred, p_b, d_ref, float_ref, r_b, B, r, 1e-2, d_mask, _settings(sc), 0.75, value if with_all else None, stats if with_all else None,
                              d_flow, d_seed if with_all else None, s_b, d_rg, g_b) == 0, tr.lib.eigen_last_error()
            got, clean = _unpad(d_rg, g_b, B, (C, h, w))
            assert clean and np.array_equal(got, rg), with_all
            if with_all:
                got, clean = _unpad(d_seed, s_b, B, (C, h, w))
                assert clean and np.array_equal(got, seed) and value.value == v
                assert stats[:B].tobytes() == rec.tobytes() and (stats[B] == float(SENT)).all()
                uu = d_flow.cpu().numpy()
                assert (uu[B * 2 * h * w:] == float(SENT)).all() and np.array_equal(uu[:B * 2 * h * w].reshape(B, 2, h, w), u)
        assert _raw_score(tr, d_pred, p_b, d_ref, float_ref, r_b, B, r, 1e-2, d_mask, _settings(sc), 0.75, None, None, None, None, 0, None, 0) == 0
    print("score stage %s: N %s S %s f %.17g, |f - restatement| %.1e, max |seed| %.3e, max |ref grad| %.3e" % (
        stage_id(case), rec[:, 0].astype(int).tolist(), rec[:, 8].tolist(), v, abs(v - want.value), np.abs(seed).max(), np.abs(rg).max()))


@functools.lru_cache(maxsize=None)
def _gpu_and_ref(c):
    """the training call of a case and its float64 reference, made once.  max_norm comes from the float64 reference's fields
    (`case_max_norm`), with a requantised case fed the bytes of the GPU's own float32 predictions on both sides"""
    frames, wts, call = ss.train_case_frames(c), ss.train_case_weights(c), ss.train_case_call(c)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, fs.B_CASE, frames.shape[1]) as tr:
        _, pred0 = tr.forward_backward(frames, pred=True, **call)       # the predictions do not depend on the objective
        feed = pred0 if c.form == "still_requant" else None
        _, fields = ss.train_case_reference(c, ss.train_case_score(c, 1.0), pred=feed, leaf=None)
        max_norm, half = ss.case_max_norm(fields, c.h)
        sc = ss.train_case_score(c, max_norm)
        score = ss.as_flow_score(sc)
        flow = PredictionFlow(c.r, 1e-2).scored(score) if c.pairing == "prediction" else FlowObjective(c.r, 1e-2, reference="moving", score=score)
        kw = dict(objective="flow", flow=flow, **call)
        loss, pred, per, terms = tr.forward_backward(frames, pred=True, frame_grads="frames", flow_terms=True, **kw)
        grads, seq = tr.grads(), tr.state_dict()["seq"]
        loss_t, tied = tr.forward_backward(frames, frame_grads="tied", **kw)
        loss_0, terms_0 = tr.forward_backward(frames, flow_terms=True, **kw)
        grads_0, seq_0 = tr.grads(), tr.state_dict()["seq"]
    assert pred.tobytes() == pred0.tobytes()
    # loss, terms, weight gradients and state are the same bits with and without a frame-gradient buffer
    assert loss == loss_t == loss_0 and terms.tobytes() == terms_0.tobytes()
    assert all(grads[k].tobytes() == grads_0[k].tobytes() for k in grads)
    assert all(a.tobytes() == b.tobytes() for k in seq for a, b in zip(seq[k], seq_0[k]))
    r, ref_fields = ss.train_case_reference(c, sc, pred=feed, leaf="frames")
    return (loss, pred, per, tied, terms, grads), r, ref_fields, sc, half


@pytest.mark.parametrize("c", ss.TRAIN_CASES, ids=ss.train_case_id)
def test_a_training_call_matches_float64_autograd_of_the_score(cuda, c):
    """Both pairings ("moving": the frame pairing with the frame in the graph), the three forms, r = 2 and 7, B = 2, "live" weights.
    Every sample of every weighted term has at least min_count members on the reference; the loss within 1e-5 of its un-cancelled scale
    and every term within that of its own (S_b is a sum of two non-negative products, so the scale is the value); every weight gradient
    within `_check_grads` of tests/train_support.py, unchanged; the per-frame and the tied frame gradient within the same rule per step
    (`check_frame_grads`), the tied output being the float32 fold of the per-frame one under the prediction pairing."""
    (loss, pred, per, tied, terms, grads), r, fields, sc, half = _gpu_and_ref(c)
    what = ss.train_case_id(c)
    call = ss.train_case_call(c)
    T = per.shape[1]
    for u in fields:
        assert (ss.score_ref(u, None, sc).record[:, 0] >= sc.min_count).all(), what
    assert np.abs(pred - r.pred).max() <= 1e-5
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss, r.scale)
    assert terms.shape == r.terms.shape and (np.abs(terms - r.terms) <= 1e-5 * r.term_scales).all(), (terms, r.terms)
    assert (terms == 0).tolist() == (r.terms == 0).tolist()
    norm, element = _check_grads(grads, r.grads, what=what)
    n_fed = call["n_fed"] or T
    if c.pairing == "prediction":
        zero = {t for t in range(T) if t >= n_fed or t == T - 1}
        assert np.array_equal(tied, fold_tied(per))
    else:
        zero = zero_steps(T, call["n_fed"], call["step_weights"])
    for t in zero:
        assert not per[:, t].any() and not r.frame_grad[:, t].any(), t
    ratio = check_frame_grads(per, r.frame_grad, what, tied=tied, zero=zero)
    lossr = abs(loss - r.loss) / (1e-5 * r.scale)
    for k, v in (("norm", norm), ("element", element), ("loss", lossr), ("frames", ratio)):
        WORST[k] = max(WORST[k], v)
    print("score mode %s: max_norm %.4g (half gap %.1e) loss %.6f; error / bound norm %.4f element %.4f loss %.4f frames %.4f (worst so far %.4f %.4f %.4f %.4f)" % (
        what, sc.max_norm, half, loss, norm, element, lossr, ratio, WORST["norm"], WORST["element"], WORST["loss"], WORST["frames"]))


def _raw_flow_score(tr, d, B, T, n, flags, pairing, loss, terms, buf=None, objective=2, score=None, d_dir=None):
    """eigen_trainer_loss_grad_flow_score: the arguments of tests/flow_gpu_support.py `_raw_loss_grad`, then the score"""
    cfg = FlowSettings(7, flags, 1e-2)
    return tr.lib.eigen_trainer_loss_grad_flow_score(tr._h, _p(d), T * n, B, T, T, 0, 1, None, objective, None, ctypes.byref(loss), None, None, _p(buf),
                                                     T * n if buf is not None else 0, n if buf is not None else 0, ctypes.byref(cfg), _p(d_dir), None, terms, pairing,
                                                     None if score is None else ctypes.byref(score), None)


def test_without_a_score_the_new_entry_is_the_old_one(cuda):
    """16x12 [3, 4, 6], "live" weights: `eigen_trainer_loss_grad_flow_score(score=NULL)` equals `eigen_trainer_loss_grad_flow_pair` bit for
    bit in loss, terms, all weight gradients and the per-frame frame gradients, under the frame pairing with the constant and with the
    moving reference and under the prediction pairing; with a score the call differs, repeats its bits, and leaves nothing behind: the
    old entry returns its bits again afterwards."""
    w, h, ch = 16, 12, (3, 4, 6)
    c = fs.FlowCase(w, h, ch, "live", "energy", 7, "drifting")
    frames, wts = fs.flow_case_frames(c), case_weights(w, h, ch, "live")
    B, T = frames.shape[:2]
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    score = _settings(ss.score_for(h, 1.5))
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        def run(entry, flags, pairing, sc=None):
            buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
            terms, loss = (ctypes.c_double * (T - 1))(), ctypes.c_double()
            rc = _raw_loss_grad(tr, "pair", d, B, T, n, flags, pairing, loss, terms, buf) if entry == "pair" else _raw_flow_score(tr, d, B, T, n, flags, pairing, loss, terms, buf, score=sc)
            assert rc == 0, tr.lib.eigen_last_error()
            return loss.value, list(terms), tr.grads(), buf.cpu().numpy()

        same = lambda a, b: a[0] == b[0] and a[1] == b[1] and a[3].tobytes() == b[3].tobytes() and all(a[2][k].tobytes() == b[2][k].tobytes() for k in a[2])
        for flags, pairing in ((0, 0), (1, 0), (0, 1)):
            old = run("pair", flags, pairing)
            assert same(old, run("score", flags, pairing)) and not (old[3] == SENT).any() and old[0] != 0 and any(g.any() for g in old[2].values())
            with_score = run("score", flags, pairing, score)
            assert not same(old, with_score) and with_score[0] > 0 and any(g.any() for g in with_score[2].values())
            assert same(with_score, run("score", flags, pairing, score))
            assert same(old, run("pair", flags, pairing))


def test_refusals(cuda):
    """Every rule of the score's settings, a direction field or another objective together with a score, both or neither reference, a
    NULL score on the stage-alone entry and flags on it: refused with EIGEN_ERR_INVALID before any launch, and nothing is written."""
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 4
    frames, _ = case_inputs(w, h, tuple(ch), B, T)
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    pred = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    prev = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    ref = d[:, 0].contiguous()
    good = ss.score_for(h, 1.5)
    nan, inf = float("nan"), float("inf")
    bad = [good._replace(max_norm=0.0), good._replace(max_norm=-1.0), good._replace(max_norm=nan), good._replace(max_norm=inf), good._replace(min_norm=-1e-3),
           good._replace(min_norm=1.5), good._replace(min_norm=nan), good._replace(r_min=-1.0), good._replace(r_min=7.0), good._replace(r_max=inf),
           good._replace(r_min=nan), good._replace(min_count=1), good._replace(min_count=0), good._replace(w_direction=-0.1), good._replace(w_strength=nan),
           good._replace(w_direction=inf), good._replace(w_direction=0.0, w_strength=0.0)]
    with PredNetTrainer("synthetic", ch, w, h, B, T) as tr:
        buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
        terms = (ctypes.c_double * (T - 1))(*([float(SENT)] * (T - 1)))
        loss, value = ctypes.c_double(float(SENT)), ctypes.c_double(float(SENT))
        seed = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        rg = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        u = torch.full((B * 2 * h * w,), float(SENT), dtype=torch.float64, device=cuda)
        stats = np.full((B, ss.REC), float(SENT))
        d_dir = torch.from_numpy(train.flow_direction("tangent", w, h)).to(cuda)
        stage = lambda sc, float_ref=False, **kw: _raw_score(tr, pred, n, prev if float_ref else ref, float_ref, n, B, 7, 1e-2, None, sc, 1.0, value, stats, u, seed, n, rg, n, **kw)
        call = lambda sc, **kw: _raw_flow_score(tr, d, B, T, n, 0, kw.pop("pairing", 0), loss, terms, buf, score=sc, **kw)

        def refused(rc, word):
            msg = tr.lib.eigen_last_error().decode()
            assert rc == -1 and word in msg, (rc, msg)

        for sc in bad:
            for float_ref in (False, True):
                refused(stage(_settings(sc), float_ref), "flow score")
            for pairing in (0, 1):
                refused(call(_settings(sc), pairing=pairing), "flow score")
        reserved = _settings(good)
        reserved.reserved = 1
        refused(stage(reserved), "reserved")
        refused(call(reserved), "reserved")
        refused(stage(None), "null")
        refused(stage(_settings(good), both=True), "reference")
        refused(_raw_score(tr, pred, n, None, False, n, B, 7, 1e-2, None, _settings(good), 1.0, value, stats, u, seed, n, rg, n), "reference")
        for flags in (1, 2, -1):
            refused(stage(_settings(good), flags=flags), "flags")
        refused(call(_settings(good), d_dir=d_dir), "direction")
        refused(call(_settings(good), objective=0), "EIGEN_OBJ_FLOW")
        refused(call(_settings(good), objective=1), "EIGEN_OBJ_FLOW")
        refused(call(_settings(good), pairing=7), "pairing")
        torch.cuda.synchronize()
        assert (buf == float(SENT)).all() and (seed == float(SENT)).all() and (u == float(SENT)).all() and (rg == float(SENT)).all()
        assert loss.value == float(SENT) and value.value == float(SENT) and list(terms) == [float(SENT)] * (T - 1) and (stats == float(SENT)).all()
        assert all(not g.any() for g in tr.grads().values())
        with pytest.raises(ValueError):
            tr.flow_term(pred, ref, FlowObjective(), stats=True)
        assert tr.flow_term(pred, ref, FlowObjective())[0] > 0 and tr.last_flow_stats is None
        # and the accepted edges are accepted
        edges = good._replace(min_norm=0.0, r_min=6.0, r_max=6.0, min_count=2, w_direction=0.0)
        assert stage(_settings(edges)) == 0 and stage(_settings(good), True) == 0 and not (rg == float(SENT)).any() and not (stats == float(SENT)).any()
        assert call(_settings(good)) == 0 and call(_settings(good), pairing=1) == 0 and not (buf == float(SENT)).any() and loss.value != float(SENT)


@pytest.mark.parametrize("w,h,ch", ss.RISING_SHAPES)
def test_refinement_climbs_as_on_the_reference(cuda, w, h, ch):
    """refine_stills under PredictionFlow(score=...) with its default step weights, at the settings of tests/test_flow_score_host.py
    test_refinement_on_the_reference_alone (n_repeat=4, n_ext=2, 8 steps of 2 bytes, float feedback, the left quarter kept), at the
    shapes where the score term rises on the float64 reference alone and at those only: reproducible from numpy and device input, kept
    columns untouched, no byte moves by more than 16, and the term rises.  At 12x8 it does not rise on the reference (a sample's members
    fall below min_count on the way), so nothing is asserted there."""
    B = 2
    frames, sets = case_inputs(w, h, tuple(ch), B, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    mask = rs.refine_mask(w, h)
    flow = PredictionFlow().scored(ss.as_flow_score(ss.refine_score(w, h, tuple(ch))))
    kw = dict(requant=False, objective="flow", flow=flow, mask=mask, **ss.REFINE)
    with PredNetTrainer(sets["live"], list(ch), w, h, B, 6) as tr:
        out, hist = train.refine_stills(tr, stills, **kw)
        out2, hist2 = train.refine_stills(tr, torch.from_numpy(stills).to(cuda), **kw)
    _, ref_hist = ss.refine_reference(w, h, tuple(ch))
    print("refine score mode %dx%d: %s (reference: %s)" % (w, h, " ".join("%.4e" % v for v in hist), " ".join("%.4e" % v for v in ref_hist)))
    assert out.dtype == np.uint8 and out.shape == stills.shape and hist.shape == (9,) and hist.dtype == np.float64
    assert np.array_equal(out, out2) and np.array_equal(hist, hist2)
    assert np.array_equal(out[..., :w // 4], stills[..., :w // 4]) and (out != stills).any()
    assert np.abs(out.astype(np.int32) - stills).max() <= 8 * 2
    assert abs(hist[0] - ref_hist[0]) <= 1e-5 * ref_hist[0]
    assert ref_hist[-1] > ref_hist[0] and hist[-1] > hist[0], hist


def test_step_and_refine_genomes_take_the_score(cuda):
    """`step` and `refine_genomes` take a FlowObjective with a score as they take any: two Adam steps change the weights and the loss;
    refine_genomes at the setting of tests/cppn_grad_support.py is reproducible, moves the genomes, and its history's last entry is the
    loss a direct call gives for the returned images.  Whether the loss rises is printed, not asserted: no CPU statement of that loop
    exists."""
    from tests import cppn_grad_support as S
    from tests.train_support import _weight_sets
    SIM = S.SIM
    w, h, ch = SIM["w"], SIM["h"], list(SIM["ch"])
    n_repeat, n_ext = SIM["n_repeat"], max(SIM["n_ext"], 2)
    flow = PredictionFlow(radius=3).scored(train.FlowScore(max_norm=1.0, min_count=4))
    kw = dict(n_repeat=n_repeat, n_ext=n_ext, iters=SIM["iters"], lr=SIM["lr"], requant=False, objective="flow")
    cfg, genomes = S.sim_genomes()
    params = lambda g: ({k: (n.bias, n.response) for k, n in g.nodes.items()}, {k: c.weight for k, c in g.connections.items()})
    before = [params(g) for g in genomes]
    wts = dict(_weight_sets(ch, w, h))["live"]
    with PredNetTrainer(wts, ch, w, h, batch=len(genomes), max_steps=n_repeat + n_ext) as tr:
        out, history, images = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        out2, history2, images2 = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        frames = np.ascontiguousarray(np.broadcast_to(images[:, None], (len(genomes), n_repeat + n_ext) + images.shape[1:]))
        weights = [0.0] * n_repeat + [1.0] * (n_ext - 1)
        direct = tr.forward_backward(frames, n_fed=n_repeat, requant=False, step_weights=weights, objective="flow", flow=flow)
        losses = [tr.step(frames, n_fed=n_repeat, step_weights=weights, objective="flow", flow=flow) for _ in range(2)]
        moved = tr.weights()
    print("refine_genomes score mode: %s; rose: %s; two Adam steps: %s" % (" ".join("%.4e" % v for v in history), history[-1] > history[0], losses))
    assert np.isfinite(history).all() and history.tobytes() == history2.tobytes() and images.tobytes() == images2.tobytes()
    assert [params(g) for g in out] == [params(g) for g in out2] and [params(g) for g in genomes] == before
    assert any(params(a) != b for a, b in zip(out, before)) and history[-1] == direct and direct > 0
    assert losses[0] == direct and losses[1] != losses[0] and any(not np.array_equal(moved[k], wts[k]) for k in wts)
