"""The flow objective's structure scores on the GPU (eigen_trainer_flow_term_structure, eigen_trainer_loss_grad_flow_structure,
train.BandsScore, train.FreeScore); DESIGN.md section 13, "The structure scores".  The stage alone is compared with the numpy restatement
of tests/flow_struct_support.py: the solve's field bit for bit, the per-sample record within the bound of a double-precision sum, and
everything that follows the record (g, q, the seed, the reference gradient) bit for bit once the restatement is fed the device's own
record.  For Free that includes the integer sign sums of the pair pass: the gradient reads nothing else of it, and
tests/test_flow_struct_host.py asserts the margins under which the device's arccos cannot move one.  The device's theta itself is not
read back there; `test_the_pair_pass_read_back` reads theta, L and the sign sums back (eigen_trainer_debug_free_planes) and checks them
directly.  The seed is also held against float64 autograd within 2^-23 |ref| + 1e-9 max |ref|, as the score mode's.  A training call is compared with `run_flow(term=...)`; a NULL struct
through the new entry gives the bits of eigen_trainer_loss_grad_flow_pair."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.train import FlowObjective, FlowSettings, FlowStructureSettings, PredictionFlow, PredNetTrainer
from tests import flow_obj_support as fs
from tests import flow_ref_support as rs
from tests import flow_score_support as ss
from tests import flow_struct_support as st
from tests.flow_gpu_support import SENT, _p, _padded, _raw_loss_grad, _unpad
from tests.frame_grad_support import case_inputs, check_frame_grads, fold_tied, zero_steps
from tests.train_support import _check_grads, case_weights

pytestmark = pytest.mark.gpu

WORST = {"norm": 0.0, "element": 0.0, "loss": 0.0, "frames": 0.0}


def _settings(sc):
    return st.as_score(sc).settings(0)      # the limits of a Bands are always given here, so the height plays no part


def _raw_struct(tr, d_pred, p_b, d_ref, float_ref, r_b, B, radius, eps, d_mask, score, scale, value, stats, d_flow, d_seed, s_b, d_rg, rg_b, flags=0, both=False):
    """eigen_trainer_flow_term_structure called directly on device buffers; score: FlowStructureSettings or None; stats: numpy [B, 10] or None"""
    cfg = FlowSettings(radius, flags, eps)
    ref = (_p(d_ref), _p(d_ref)) if both else (None, _p(d_ref)) if float_ref else (_p(d_ref), None)
    return tr.lib.eigen_trainer_flow_term_structure(tr._h, _p(d_pred), p_b, ref[0], ref[1], r_b, B, ctypes.byref(cfg), _p(d_mask), None if score is None else ctypes.byref(score),
                                                    ctypes.c_double(scale), None if value is None else ctypes.byref(value),
                                                    None if stats is None else ctypes.c_void_p(stats.ctypes.data), _p(d_flow), _p(d_seed), s_b, _p(d_rg), rg_b, None)


def _sum_bound(terms):
    """(the exact sum, N 2^-53 sum |terms|: the bound of a double-precision sum of the N terms in any order)"""
    t = np.asarray(terms, np.float64).ravel().tolist()
    return math.fsum(t), len(t) * 2.0 ** -53 * math.fsum(abs(v) for v in t)


@pytest.mark.parametrize("c", st.STAGE_CASES, ids=st.stage_id)
def test_the_stage_is_the_numpy_restatement(cuda, c):
    """`flow_term` (a byte reference) and `flow_term_pair` (a float one) with a structure score, B = 2, scale 0.75:
    u `np.array_equal` the restatement's; N exact; every first-pass sum N m of the record within N 2^-53 sum |terms| of the exactly
    summed one, and the variance sum likewise against the exactly summed terms formed from the device's own mean (Free's swarm sum is made
    of the device's L_i and is checked where they are read back, `test_the_pair_pass_read_back`).
    S_b and f within 1e-10 of the restatement, and exactly what the restatement forms from the device's record; with that record the seed
    and the reference gradient are the restatement's bit for bit, which for Free means every integer sign sum is the restatement's; the
    seed is within 2^-23 |ref| + 1e-9 max |ref| of float64 autograd; a sample below min_count or without a member has value 0 and an
    exactly zero seed and reference gradient, and nothing is non-finite; on padded strides the entry returns the same bits and leaves the
    padding alone; every output is optional."""
    B = st.B_STAGE
    w, h, C, r = c.w, c.h, c.C, c.r
    pred, ref, ref64, mask, sc = st.stage_case(c)
    float_ref = c.ref_kind == "floats"
    flow = st.flow_of(sc, r, mask=mask, pairing="prediction" if float_ref else "frame")
    want = st.struct_stage_ref(pred, ref64, r, 1e-2, mask, sc, scale=0.75)
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
        assert np.isfinite(rec).all() and np.isfinite(seed).all() and np.isfinite(rg).all() and np.isfinite(v)
        pts = want.score.points
        assert rec.shape == (B, st.REC) and np.array_equal(rec[:, 0], want.score.record[:, 0]) and not rec[:, 6:8].any() and not rec[:, 9].any()
        for b in range(B):
            N = rec[b, 0]
            if N == 0:
                assert not rec[b].any()
                continue
            first, second = st.sample_columns(want.u, pts, sc, b, None if c.kind == "bands" else want.score.pairs[b], rec[b])
            for k, t in enumerate(first):
                exact, bound = _sum_bound(t)
                assert abs(N * rec[b, 1 + k] - exact) <= bound, (b, k, N * rec[b, 1 + k], exact, bound)
            for k, t in enumerate(second[:1]):      # Free's swarm sum is made of the device's L: test_the_pair_pass_read_back
                exact, bound = _sum_bound(t)
                assert abs(N * rec[b, 3 + k] - exact) <= bound, (b, k, N * rec[b, 3 + k], exact, bound)
            mine = rec[b].copy()
            st.fill_value(mine, sc)
            assert abs(rec[b, 8] - want.score.S[b]) <= 1e-10 and rec[b, 8] == mine[8] and rec[b, 5] == mine[5] and (c.kind == "free" or not rec[b, 4:6].any())
        assert abs(v - want.value) <= 1e-10, (v, want.value)
        fed = st.struct_stage_ref(pred, ref64, r, 1e-2, mask, sc, scale=0.75, record=rec)
        assert v == fed.value
        assert np.array_equal(seed, fed.seed), np.abs(seed - fed.seed).max()
        assert np.array_equal(rg, fed.grad), np.abs(rg - fed.grad).max()
        P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
        f, _, _ = st.torch_struct_term(P, torch.from_numpy(ref64.copy()), r, 1e-2, mask, sc)
        (g,) = torch.autograd.grad(0.75 * f, P)
        g = g.numpy()
        assert (np.abs(seed - g) <= 2.0 ** -23 * np.abs(g) + 1e-9 * np.abs(g).max()).all(), np.abs(seed - g).max() / np.abs(g).max()
        below = (rec[:, 0] < c.min_count) | (rec[:, 0] == 0)
        assert below.tolist() == [bool(s == 0.0) for s in want.score.S] and below.sum() == (1 if c.empty or (c.min_count == 25 and (w, h) == (12, 8)) else below.sum()) <= 1
        for b in range(B):
            if below[b]:
                assert rec[b, 8] == 0.0 and not seed[b].any() and not rg[b].any()
            else:
                assert rec[b, 8] != 0 and seed[b].any() and rg[b].any()
        # the entry itself on padded strides, with and without the optional outputs
        p_b, r_b, s_b, g_b = per + 5, per + 3, per + 7, per + 11
        d_pred = _padded(pred, p_b, np.float32(np.nan), cuda)
        d_ref = _padded(ref, r_b, np.float32(np.nan) if float_ref else np.uint8(7), cuda)
        d_mask = None if mask is None else torch.from_numpy(mask).to(cuda)
        for with_all in (True, False):
            d_rg = torch.full((B * g_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
            d_seed = torch.full((B * s_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
            d_flow = torch.full((B * 2 * h * w + 4,), float(SENT), dtype=torch.float64, device=cuda) if with_all else None
            value, stats = ctypes.c_double(), np.full((B + 1, st.REC), float(SENT))
            assert _raw_struct(tr, d_pred, p_b, d_ref, float_ref, r_b, B, r, 1e-2, d_mask, _settings(sc), 0.75, value if with_all else None, stats if with_all else None,
                               d_flow, d_seed if with_all else None, s_b, d_rg, g_b) == 0, tr.lib.eigen_last_error()
            got, clean = _unpad(d_rg, g_b, B, (C, h, w))
            assert clean and np.array_equal(got, rg), with_all
            if with_all:
                got, clean = _unpad(d_seed, s_b, B, (C, h, w))
                assert clean and np.array_equal(got, seed) and value.value == v
                assert stats[:B].tobytes() == rec.tobytes() and (stats[B] == float(SENT)).all()
                uu = d_flow.cpu().numpy()
                assert (uu[B * 2 * h * w:] == float(SENT)).all() and np.array_equal(uu[:B * 2 * h * w].reshape(B, 2, h, w), u)
        assert _raw_struct(tr, d_pred, p_b, d_ref, float_ref, r_b, B, r, 1e-2, d_mask, _settings(sc), 0.75, None, None, None, None, 0, None, 0) == 0
    print("structure stage %s: max_norm %.4g N %s S %s f %.17g, |f - restatement| %.1e, max |seed| %.3e, max |ref grad| %.3e" % (
        st.stage_id(c), sc.max_norm, rec[:, 0].astype(int).tolist(), rec[:, 8].tolist(), v, abs(v - want.value), np.abs(seed).max(), np.abs(rg).max()))


@pytest.mark.parametrize("c", [c for c in st.STAGE_CASES if c.kind == "free"], ids=st.stage_id)
def test_the_pair_pass_read_back(cuda, c):
    """The planes of Free's pair pass after a stage call, read back through `PredNetTrainer.free_planes`: the member flags are the
    restatement's; theta is within two ulps of pi (8.9e-16) of numpy's arccos and 0 off the members; rowS and colS equal the restatement's
    integers exactly and are 0 off the members; with the DEVICE's theta in numpy's place every L_i is within
    (its number of close pairs) 2^-53 sum |terms| of the exactly summed one; and the record's swarm sum is within N 2^-53 sum |terms| of
    the exactly summed terms (pi - L_i / N) / pi formed from the device's L_i."""
    B = st.B_STAGE
    pred, ref, ref64, mask, sc = st.stage_case(c)
    float_ref = c.ref_kind == "floats"
    flow = st.flow_of(sc, c.r, mask=mask, pairing="prediction" if float_ref else "frame")
    want = st.struct_stage_ref(pred, ref64, c.r, 1e-2, mask, sc, scale=0.75)
    with PredNetTrainer("synthetic", [c.C, 4], c.w, c.h, B + 1, 2) as tr:
        (tr.flow_term_pair if float_ref else tr.flow_term)(pred, ref, flow, scale=0.75)
        rec, pl = tr.last_flow_stats, tr.free_planes(B)
    pts = want.score.points
    assert np.array_equal(pl["member"], pts.member)
    worst_theta = worst_L = 0.0
    for b in range(B):
        m = pts.member[b]
        for k in ("theta", "L", "rowS", "colS"):
            assert not pl[k][b][~m].any(), (b, k)
        N = int(m.sum())
        if N == 0:
            continue
        mine = want.score.pairs[b]
        assert np.abs(pl["theta"][b][m] - mine.theta).max() <= 2 * 2.0 ** -51, np.abs(pl["theta"][b][m] - mine.theta).max()
        worst_theta = max(worst_theta, np.abs(pl["theta"][b][m] - mine.theta).max())
        assert np.array_equal(pl["rowS"][b][m], mine.rowS) and np.array_equal(pl["colS"][b][m], mine.colS)
        fed = st.free_pairs(pts.nx[b], m, sc.max_distance * sc.max_distance, theta=pl["theta"][b])
        assert np.array_equal(fed.rowS, mine.rowS) and np.array_equal(fed.colS, mine.colS)
        got = pl["L"][b][m]
        for i in range(N):
            t = fed.terms[i][fed.terms[i] != 0]
            exact = math.fsum(t.tolist())
            assert abs(got[i] - exact) <= len(t) * 2.0 ** -53 * exact, (b, i, got[i], exact)
            worst_L = max(worst_L, abs(got[i] - exact) / max(exact, 1e-300))
        exact, bound = _sum_bound((st.PI - got / rec[b, 0]) / st.PI)
        assert rec[b, 0] == N and abs(N * rec[b, 4] - exact) <= bound, (b, N * rec[b, 4], exact, bound)
    print("pair pass %s: max |theta - arccos| %.1e, max |L - exact| / L %.1e" % (st.stage_id(c), worst_theta, worst_L))


@functools.lru_cache(maxsize=None)
def _gpu_and_ref(c):
    """the training call of a case and its float64 reference, made once.  max_norm comes from the float64 reference's fields
    (`case_max_norm`), with a requantised case fed the bytes of the GPU's own float32 predictions on both sides"""
    b = c.base
    frames, wts, call = ss.train_case_frames(b), st.train_case_weights(c), ss.train_case_call(b)
    with PredNetTrainer(wts, list(b.ch), b.w, b.h, fs.B_CASE, frames.shape[1]) as tr:
        _, pred0 = tr.forward_backward(frames, pred=True, **call)       # the predictions do not depend on the objective
        feed = pred0 if b.form == "still_requant" else None
        probe = st.train_case_score(c, 1.0)
        _, fields = st.train_case_reference(c, probe, pred=feed, leaf=None)
        max_norm, half = st.case_max_norm(fields, probe)
        sc = st.train_case_score(c, max_norm)
        score = st.as_score(sc)
        flow = PredictionFlow(b.r, 1e-2).scored(score) if b.pairing == "prediction" else FlowObjective(b.r, 1e-2, reference="moving", score=score)
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
    assert all(x.tobytes() == y.tobytes() for k in seq for x, y in zip(seq[k], seq_0[k]))
    r, ref_fields = st.train_case_reference(c, sc, pred=feed, leaf="frames")
    return (loss, pred, per, tied, terms, grads), r, ref_fields, sc, half


@pytest.mark.parametrize("c", st.TRAIN_CASES, ids=st.train_case_id)
def test_a_training_call_matches_float64_autograd_of_the_structure_score(cuda, c):
    """Both structures, both pairings ("moving": the frame pairing with the frame in the graph), the three forms, r = 2 and 7, B = 2, "live"
    weights.  Every sample of every weighted term has members on the reference; the loss within 1e-5 of its un-cancelled scale and every
    term within that of its own; every weight gradient within `_check_grads` of tests/train_support.py, unchanged; the per-frame and the
    tied frame gradient within the same rule per step (`check_frame_grads`), the tied output being the float32 fold of the per-frame one
    under the prediction pairing."""
    (loss, pred, per, tied, terms, grads), r, fields, sc, half = _gpu_and_ref(c)
    b = c.base
    what = st.train_case_id(c)
    call = ss.train_case_call(b)
    T = per.shape[1]
    for u in fields:
        assert (st.struct_ref(u, None, sc).record[:, 0] >= 1).all(), what
    assert np.abs(pred - r.pred).max() <= 1e-5
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss, r.scale)
    assert terms.shape == r.terms.shape and (np.abs(terms - r.terms) <= 1e-5 * r.term_scales).all(), (terms, r.terms)
    assert (terms == 0).tolist() == (r.terms == 0).tolist()
    norm, element = _check_grads(grads, r.grads, what=what)
    n_fed = call["n_fed"] or T
    if b.pairing == "prediction":
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
    print("structure score %s: max_norm %.4g (half gap %.1e) loss %.6f; error / bound norm %.4f element %.4f loss %.4f frames %.4f (worst so far %.4f %.4f %.4f %.4f)" % (
        what, sc.max_norm, half, loss, norm, element, lossr, ratio, WORST["norm"], WORST["element"], WORST["loss"], WORST["frames"]))


def _raw_flow_struct(tr, d, B, T, n, flags, pairing, loss, terms, buf=None, objective=2, score=None, d_dir=None):
    """eigen_trainer_loss_grad_flow_structure: the arguments of tests/flow_gpu_support.py `_raw_loss_grad`, then the structure score"""
    cfg = FlowSettings(7, flags, 1e-2)
    return tr.lib.eigen_trainer_loss_grad_flow_structure(tr._h, _p(d), T * n, B, T, T, 0, 1, None, objective, None, ctypes.byref(loss), None, None, _p(buf),
                                                         T * n if buf is not None else 0, n if buf is not None else 0, ctypes.byref(cfg), _p(d_dir), None, terms, pairing,
                                                         None if score is None else ctypes.byref(score), None)


def test_without_a_struct_the_new_entry_is_the_old_one(cuda):
    """16x12 [3, 4, 6], "live" weights: `eigen_trainer_loss_grad_flow_structure(score=NULL)` equals `eigen_trainer_loss_grad_flow_pair` bit
    for bit in loss, terms, all weight gradients and the per-frame frame gradients, under the frame pairing with the constant and with the
    moving reference and under the prediction pairing; with either structure the call differs, repeats its bits, and leaves nothing
    behind: the old entry, and the score mode's entry with a Circles score, return their own bits again afterwards."""
    from tests.test_gpu_flow_score import _raw_flow_score, _settings as circles_settings
    w, h, ch = 16, 12, (3, 4, 6)
    c = fs.FlowCase(w, h, ch, "live", "energy", 7, "drifting")
    frames, wts = fs.flow_case_frames(c), case_weights(w, h, ch, "live")
    B, T = frames.shape[:2]
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    scores = [_settings(st.bands_for(h, 1.5)), _settings(st.Free(1.5, 1e-3, 5.0, 1, st.FREE_W))]
    circles = circles_settings(ss.score_for(h, 1.5))
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        def run(entry, flags, pairing, sc=None):
            buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
            terms, loss = (ctypes.c_double * (T - 1))(), ctypes.c_double()
            if entry == "pair":
                rc = _raw_loss_grad(tr, "pair", d, B, T, n, flags, pairing, loss, terms, buf)
            elif entry == "circles":
                rc = _raw_flow_score(tr, d, B, T, n, flags, pairing, loss, terms, buf, score=sc)
            else:
                rc = _raw_flow_struct(tr, d, B, T, n, flags, pairing, loss, terms, buf, score=sc)
            assert rc == 0, tr.lib.eigen_last_error()
            return loss.value, list(terms), tr.grads(), buf.cpu().numpy()

        same = lambda a, b: a[0] == b[0] and a[1] == b[1] and a[3].tobytes() == b[3].tobytes() and all(a[2][k].tobytes() == b[2][k].tobytes() for k in a[2])
        for flags, pairing in ((0, 0), (1, 0), (0, 1)):
            old = run("pair", flags, pairing)
            old_score = run("circles", flags, pairing, circles)
            assert same(old, run("struct", flags, pairing)) and not (old[3] == SENT).any() and old[0] != 0 and any(g.any() for g in old[2].values())
            for sc in scores:
                with_struct = run("struct", flags, pairing, sc)
                assert not same(old, with_struct) and not same(old_score, with_struct) and with_struct[0] > 0 and any(g.any() for g in with_struct[2].values())
                assert same(with_struct, run("struct", flags, pairing, sc))
                assert same(old, run("pair", flags, pairing))
                assert same(old_score, run("circles", flags, pairing, circles))


def test_refusals(cuda):
    """Every rule of the structure scores' settings, structures 1 and 3 (the message names eigen_flow_score), a direction field or another
    objective together with a score, both or neither reference, a NULL score on the stage-alone entry and flags on it: refused with
    EIGEN_ERR_INVALID before any launch, and nothing is written."""
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 4
    frames, _ = case_inputs(w, h, tuple(ch), B, T)
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    pred = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    prev = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    ref = d[:, 0].contiguous()
    nan, inf = float("nan"), float("inf")

    def make(structure=0, min_count=1, max_norm=1.5, min_norm=1e-3, lim_lo=0.0, lim_hi=6.0, max_distance=5.0, w=(0.5, 0.1, 0.4)):
        return FlowStructureSettings(structure, min_count, max_norm, min_norm, lim_lo, lim_hi, max_distance, (ctypes.c_double * 3)(*w))

    bad = []
    for s in (0, 2):
        bad += [make(s, max_norm=0.0), make(s, max_norm=-1.0), make(s, max_norm=nan), make(s, max_norm=inf), make(s, min_norm=-1e-3), make(s, min_norm=1.5),
                make(s, min_norm=nan), make(s, min_count=0), make(s, min_count=-3)]
    bad += [make(0, lim_lo=7.0), make(0, lim_hi=inf), make(0, lim_lo=nan), make(0, lim_lo=-inf), make(0, lim_hi=2.1e9), make(0, lim_lo=-3e9, lim_hi=-2.1e9)]
    bad += [make(2, max_distance=0.0), make(2, max_distance=-1.0), make(2, max_distance=nan), make(2, max_distance=inf), make(2, w=(-0.1, 1, 1)), make(2, w=(1, nan, 1)),
            make(2, w=(1, 1, inf)), make(2, w=(0, 0, 0))]
    bad += [make(4), make(-1), make(7)]
    with PredNetTrainer("synthetic", ch, w, h, B, T) as tr:
        buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
        terms = (ctypes.c_double * (T - 1))(*([float(SENT)] * (T - 1)))
        loss, value = ctypes.c_double(float(SENT)), ctypes.c_double(float(SENT))
        seed = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        rg = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        u = torch.full((B * 2 * h * w,), float(SENT), dtype=torch.float64, device=cuda)
        stats = np.full((B, st.REC), float(SENT))
        d_dir = torch.from_numpy(train.flow_direction("tangent", w, h)).to(cuda)
        stage = lambda sc, float_ref=False, **kw: _raw_struct(tr, pred, n, prev if float_ref else ref, float_ref, n, B, 7, 1e-2, None, sc, 1.0, value, stats, u, seed, n, rg, n, **kw)
        call = lambda sc, **kw: _raw_flow_struct(tr, d, B, T, n, 0, kw.pop("pairing", 0), loss, terms, buf, score=sc, **kw)

        def refused(rc, word):
            msg = tr.lib.eigen_last_error().decode()
            assert rc == -1 and word in msg, (rc, msg)

        for sc in bad:
            for float_ref in (False, True):
                refused(stage(sc, float_ref), "flow structure score")
            for pairing in (0, 1):
                refused(call(sc, pairing=pairing), "flow structure score")
        for s in (1, 3):
            refused(stage(make(s)), "eigen_flow_score")
            refused(call(make(s)), "eigen_flow_score")
        good = (make(0), make(2))
        refused(stage(None), "null")
        for sc in good:
            refused(stage(sc, both=True), "reference")
            refused(_raw_struct(tr, pred, n, None, False, n, B, 7, 1e-2, None, sc, 1.0, value, stats, u, seed, n, rg, n), "reference")
            for flags in (1, 2, -1):
                refused(stage(sc, flags=flags), "flags")
            refused(call(sc, d_dir=d_dir), "direction")
            refused(call(sc, objective=0), "EIGEN_OBJ_FLOW")
            refused(call(sc, objective=1), "EIGEN_OBJ_FLOW")
            refused(call(sc, pairing=7), "pairing")
        torch.cuda.synchronize()
        assert (buf == float(SENT)).all() and (seed == float(SENT)).all() and (u == float(SENT)).all() and (rg == float(SENT)).all()
        assert loss.value == float(SENT) and value.value == float(SENT) and list(terms) == [float(SENT)] * (T - 1) and (stats == float(SENT)).all()
        assert all(not g.any() for g in tr.grads().values())
        # and the accepted edges are accepted: the fields a structure does not read may hold anything
        edges = (make(0, min_norm=0.0, lim_lo=6.0, lim_hi=6.0, max_distance=nan, w=(0, 0, 0)), make(2, min_norm=0.0, lim_lo=nan, lim_hi=-inf, w=(0, 0, 1)))
        for sc in edges + good:
            assert stage(sc) == 0 and stage(sc, True) == 0, tr.lib.eigen_last_error()
        assert not (rg == float(SENT)).any() and not (stats == float(SENT)).any()
        for sc in good:
            assert call(sc) == 0 and call(sc, pairing=1) == 0
        assert not (buf == float(SENT)).any() and loss.value != float(SENT)


@pytest.mark.parametrize("kind,w,h,ch", [(kind, w, h, ch) for kind in ("bands", "free") for w, h, ch in st.RISING_SHAPES[kind]])
def test_refinement_climbs_as_on_the_reference(cuda, kind, w, h, ch):
    """refine_stills under PredictionFlow(score=...) with its default step weights, at the settings of tests/test_flow_struct_host.py
    test_refinement_on_the_reference_alone (n_repeat=4, n_ext=2, 8 steps of 2 bytes, float feedback, the left quarter kept), at the
    shapes where the term rises on the float64 reference alone and at those only: reproducible from numpy and device input, kept columns
    untouched, no byte moves by more than 16, and the term rises."""
    B = 2
    frames, sets = case_inputs(w, h, tuple(ch), B, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    mask = rs.refine_mask(w, h)
    flow = PredictionFlow().scored(st.as_score(st.refine_score(kind, w, h, tuple(ch))))
    kw = dict(requant=False, objective="flow", flow=flow, mask=mask, **st.REFINE)
    with PredNetTrainer(sets["live"], list(ch), w, h, B, 6) as tr:
        out, hist = train.refine_stills(tr, stills, **kw)
        out2, hist2 = train.refine_stills(tr, torch.from_numpy(stills).to(cuda), **kw)
    _, ref_hist = st.refine_reference(kind, w, h, tuple(ch))
    print("refine %s %dx%d: %s (reference: %s)" % (kind, w, h, " ".join("%.4e" % v for v in hist), " ".join("%.4e" % v for v in ref_hist)))
    assert out.dtype == np.uint8 and out.shape == stills.shape and hist.shape == (9,) and hist.dtype == np.float64
    assert np.array_equal(out, out2) and np.array_equal(hist, hist2)
    assert np.array_equal(out[..., :w // 4], stills[..., :w // 4]) and (out != stills).any()
    assert np.abs(out.astype(np.int32) - stills).max() <= 8 * 2
    assert abs(hist[0] - ref_hist[0]) <= 1e-5 * abs(ref_hist[0])
    assert ref_hist[-1] > ref_hist[0] and hist[-1] > hist[0], hist
