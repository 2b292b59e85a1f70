"""The flow objective's prediction pairing on the GPU (eigen_trainer_loss_grad_flow_pair, eigen_trainer_flow_term_pair,
train.PredictionFlow); DESIGN.md section 13, "The prediction pairing".  The stage on two float images is compared bit for bit with the
numpy restatement of tests/flow_pair_support.py and tied to eigen_trainer_flow_term_ref; a training call is compared with `run_pair`,
float64 autograd with the previous prediction in the graph, which tests/test_flow_pair_host.py keeps under the float32 yardstick."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.train import FlowObjective, PredictionFlow, PredNetTrainer
from tests import flow_obj_support as fs
from tests import flow_pair_support as ps
from tests import flow_ref_support as rs
from tests.flow_gpu_support import SENT, _padded, _raw_loss_grad, _raw_pair, _unpad
from tests.frame_grad_support import case_inputs, check_frame_grads, fold_tied
from tests.train_support import _check_grads, _grads_differ, case_weights

pytestmark = pytest.mark.gpu

WORST = {"norm": 0.0, "element": 0.0, "loss": 0.0, "frames": 0.0}


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("w,h,C,r,masked,modes", rs.FIELD_CASES)
def test_the_stage_is_the_numpy_restatement_bit_for_bit(cuda, w, h, C, r, masked, modes, kind):
    """`flow_term_pair` and the entry on padded strides: u, seed and prev_grad `np.array_equal` `pair_ref`, the padding is found
    untouched, and the value is within N 2^-53 sum |m v| / (B N_m), N = B H W summands, of the exactly summed one (the bound of
    tests/test_gpu_flow_obj.py).  Every output is optional."""
    B = 2
    pred, prev = ps.pair_field_inputs(w, h, C, kind, B)
    mask = fs.field_mask(w, h) if masked else None
    per = C * h * w
    p_b, r_b, s_b, g_b = per + 5, per + 3, per + 7, per + 11
    d_pred, d_prev = _padded(pred, p_b, np.float32(np.nan), cuda), _padded(prev, r_b, np.float32(np.nan), cuda)
    d_mask = None if mask is None else torch.from_numpy(mask).to(cuda)
    with PredNetTrainer("synthetic", [C, 4], w, h, B + 1, 2) as tr:
        for mode in modes:
            d = fs.direction_of(mode, w, h)
            want = ps.pair_ref(pred, prev, r, 1e-2, d, mask, scale=0.75)
            flow = PredictionFlow(r, 1e-2, d, mask)
            v0, u0, s0 = tr.flow_term_pair(pred, prev, flow, scale=0.75)
            v1, u1, s1, g1 = tr.flow_term_pair(pred, prev, flow, scale=0.75, reference_grad=True)
            assert v1 == v0 and u1.tobytes() == u0.tobytes() and s1.tobytes() == s0.tobytes()
            assert g1.dtype == np.float32 and g1.shape == pred.shape and np.isfinite(g1).all() and np.abs(g1).max() > 0 and np.abs(u1).max() > 0
            assert np.array_equal(u1, want.u), (mode, np.abs(u1 - want.u).max())
            assert np.array_equal(s1, want.seed), (mode, np.abs(s1 - want.seed).max())
            assert np.array_equal(g1, want.prev_grad), (mode, np.abs(g1 - want.prev_grad).max(), np.abs(want.prev_grad).max())
            assert abs(v1 - want.value) <= want.bound, (mode, v1, want.value, want.bound)
            d_dir = None if d is None else torch.from_numpy(d).to(cuda)
            for with_u in (True, False):
                d_pg = torch.full((B * g_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
                d_seed = torch.full((B * s_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
                d_flow = torch.full((B * 2 * h * w + 4,), float(SENT), dtype=torch.float64, device=cuda) if with_u else None
                value = ctypes.c_double()
                assert _raw_pair(tr, d_pred, p_b, d_prev, r_b, B, r, 1e-2, d_dir, d_mask, 0.75, value, d_flow, d_seed if with_u else None, s_b, d_pg, g_b) == 0
                got, clean = _unpad(d_pg, g_b, B, (C, h, w))
                assert clean and np.array_equal(got, want.prev_grad), (mode, with_u)
                assert value.value == v0
                if with_u:
                    seed, clean = _unpad(d_seed, s_b, B, (C, h, w))
                    assert clean and np.array_equal(seed, want.seed)
                    uu = d_flow.cpu().numpy()
                    assert (uu[B * 2 * h * w:] == float(SENT)).all() and np.array_equal(uu[:B * 2 * h * w].reshape(B, 2, h, w), want.u)
            assert _raw_pair(tr, d_pred, p_b, d_prev, r_b, B, r, 1e-2, d_dir, d_mask, 0.75, None, None, None, 0, None, 0) == 0
            print("%dx%dx%d r=%d %s %s: value %.17g, |error| %.2e of the bound %.2e, max |prev_grad| %.3e, max |seed| %.3e" % (
                w, h, C, r, kind, mode, v1, abs(v1 - want.value), want.bound, np.abs(g1).max(), np.abs(s1).max()))


@pytest.mark.parametrize("w,h,C,r,masked,modes", rs.FIELD_CASES)
def test_on_a_frame_the_stage_is_flow_term_ref(cuda, w, h, C, r, masked, modes):
    """with prev = (float)byte / 255.0f of a uint8 frame, `flow_term_pair` returns the bits of `flow_term(reference_grad=True)` on it"""
    B = 2
    mask = fs.field_mask(w, h) if masked else None
    with PredNetTrainer("synthetic", [C, 4], w, h, B, 2) as tr:
        for kind in ("random", "smooth"):
            pred, ref = fs.field_inputs(w, h, C, kind, B)
            prev = ref.astype(np.float32) / np.float32(255.0)
            for mode in modes:
                flow = FlowObjective(r, 1e-2, fs.direction_of(mode, w, h), mask)
                a = tr.flow_term(pred, ref, flow, scale=0.75, reference_grad=True)
                b = tr.flow_term_pair(pred, prev, flow, scale=0.75, reference_grad=True)
                assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])) and a[3].any()


@functools.lru_cache(maxsize=None)
def _gpu_and_ref(c):
    """the training call of a case under the prediction pairing and its float64 reference, made once"""
    frames, wts, call = ps.pair_case_frames(c), ps.pair_case_weights(c), ps.pair_case_call(c)
    flow = PredictionFlow(**ps.pair_case_settings(c))
    kw = dict(objective="flow", flow=flow, **call)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, ps.B_CASE, frames.shape[1]) as tr:
        if c.form == "continued":
            tr.forward_backward(frames, **kw)
            seq = tr.state_dict()["seq"]
            kw["reset"] = False
        loss, pred, per, terms = tr.forward_backward(frames, pred=True, frame_grads="frames", flow_terms=True, **kw)
        grads = tr.grads()
        if c.form == "continued":
            tr.load_state_dict(dict(tr.state_dict(), seq=seq))
        loss_t, tied = tr.forward_backward(frames, frame_grads="tied", **kw)
    assert loss == loss_t
    # with requant both sides read the bytes of the GPU's own float32 predictions, as tests/test_gpu_flow_obj.py does
    feed = pred if c.form == "still_requant" else None
    return (loss, pred, per, tied, terms, grads), ps.pair_case_reference(c, pred=feed, leaf="frames"), ps.pair_case_reference(c, pred=feed, run=ps.frame_pairing)


@pytest.mark.parametrize("c", ps.PAIR_CASES, ids=ps.pair_case_id)
def test_a_training_call_matches_float64_autograd_with_the_previous_prediction_in_the_graph(cuda, c):
    """Loss within 1e-5 sum m |v| / (B N_m), the un-cancelled scale, and every term within that of its own; every weight gradient within
    `_check_grads` of tests/train_support.py, unchanged; the per-frame and the tied frame gradient, the input path alone, within the
    same rule per step (`check_frame_grads`); a step that reads no frame and the last step are exactly zero.  The frame-pairing
    reference of the same call is outside the bounds.
    Measured on MI355X over the 64 cases: at worst 0.025 of the norm bound, 0.031 of the element-wise bound, 0.092 of the loss bound and
    0.0055 of a frame-gradient bound."""
    (loss, pred, per, tied, terms, grads), r, frame = _gpu_and_ref(c)
    what = ps.pair_case_id(c)
    T = per.shape[1]
    assert np.abs(pred - r.pred).max() <= 1e-5
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss, r.scale)
    assert terms.shape == r.terms.shape and (np.abs(terms - r.terms) <= 1e-5 * r.term_scales).all(), (terms, r.terms)
    assert (terms == 0).tolist() == (r.terms == 0).tolist()
    norm, element = _check_grads(grads, r.grads, what=what)
    n_fed = ps.pair_case_call(c)["n_fed"] or T
    zero = {t for t in range(T) if t >= n_fed or t == T - 1}
    for t in zero:
        assert not per[:, t].any() and not r.frame_grad[:, t].any(), t
    assert np.array_equal(tied, fold_tied(per))
    ratio = check_frame_grads(per, r.frame_grad, what, tied=tied, zero=zero)
    assert _grads_differ(frame.grads, grads) and abs(loss - frame.loss) > 1e-5 * r.scale
    lossr = abs(loss - r.loss) / (1e-5 * r.scale)
    for k, v in (("norm", norm), ("element", element), ("loss", lossr), ("frames", ratio)):
        WORST[k] = max(WORST[k], v)
    print("prediction pairing %s: error / bound norm %.4f element %.4f loss %.4f frames %.4f (worst so far %.4f %.4f %.4f %.4f)" % (
        what, norm, element, lossr, ratio, WORST["norm"], WORST["element"], WORST["loss"], WORST["frames"]))


def test_the_new_entry_with_the_frame_pairing_is_the_old_one_and_calls_repeat(cuda):
    """16x12 [3, 4, 6]: `eigen_trainer_loss_grad_flow_pair(pairing=0)` equals `eigen_trainer_loss_grad_flow` bit for bit in loss, terms,
    all weight gradients and frame gradients, with the constant and with the moving reference; a second identical PredictionFlow call
    repeats its bits, and differs from the frame pairing's."""
    w, h, ch = 16, 12, (3, 4, 6)
    c = ps.PairCase(w, h, ch, "live", "tangent", 7, "drifting")
    frames, wts = ps.pair_case_frames(c), case_weights(w, h, ch, "live")
    B, T = frames.shape[:2]
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        for flags in (0, 1):
            out = []
            for entry in ("flow", "pair"):
                buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
                terms, loss = (ctypes.c_double * (T - 1))(), ctypes.c_double()
                assert _raw_loss_grad(tr, entry, d, B, T, n, flags, 0, loss, terms, buf) == 0
                out.append((loss.value, list(terms), tr.grads(), buf.cpu().numpy()))
            (l0, t0, g0, f0), (l1, t1, g1, f1) = out
            assert l0 == l1 and t0 == t1 and f0.tobytes() == f1.tobytes() and not (f0 == SENT).any() and l0 != 0
            assert all(g0[k].tobytes() == g1[k].tobytes() for k in g0) and any(g.any() for g in g0.values())
        flow = PredictionFlow(**ps.pair_case_settings(c))
        a = tr.forward_backward(frames, pred=True, objective="flow", flow=flow, frame_grads="frames", flow_terms=True)
        ga = tr.grads()
        b = tr.forward_backward(frames, pred=True, objective="flow", flow=flow, frame_grads="frames", flow_terms=True)
        gb = tr.grads()
        assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
        assert all(ga[k].tobytes() == gb[k].tobytes() for k in ga)
        assert a[0] != l0 and a[1].tobytes() == tr.forward_backward(frames, pred=True, objective="flow", flow=FlowObjective(**ps.pair_case_settings(c)))[1].tobytes()
        assert any(not np.array_equal(ga[k], g0[k]) for k in ga)


@pytest.mark.parametrize("form", ["still_requant", "drifting"])
def test_nothing_held_over_leaks_into_a_later_call(cuda, form):
    """an "mse" call after a PredictionFlow call returns the bits it returned before it: loss, predictions, weight and frame gradients
    and the kept state; so does a frame-pairing "flow" call with the moving reference"""
    w, h, ch = 40, 24, (3, 4)
    c = ps.PairCase(w, h, ch, "live", "energy", 7, form)
    frames, wts, call = ps.pair_case_frames(c), case_weights(w, h, ch, "live"), ps.pair_case_call(c)
    call["step_weights"] = None
    T = frames.shape[1]
    moving = FlowObjective(reference="moving", **ps.pair_case_settings(c))
    with PredNetTrainer(wts, list(ch), w, h, ps.B_CASE, T) as tr:
        def snapshot(**kw):
            out = tr.forward_backward(frames, pred=True, frame_grads="frames", **kw, **call)
            return out, tr.grads(), tr.state_dict()["seq"]
        before = snapshot(objective="mse"), snapshot(objective="flow", flow=moving)
        pair = tr.forward_backward(frames, objective="flow", flow=PredictionFlow(**ps.pair_case_settings(c)), frame_grads="frames", **call)
        assert pair[1].any() and any(g.any() for g in tr.grads().values())
        after = snapshot(objective="mse"), snapshot(objective="flow", flow=moving)
    for (o0, g0, s0), (o1, g1, s1) in zip(before, after):
        assert o0[0] == o1[0] and all(x.tobytes() == y.tobytes() for x, y in zip(o0[1:], o1[1:]))
        assert all(g0[k].tobytes() == g1[k].tobytes() for k in g0)
        assert all(x.tobytes() == y.tobytes() for k in s0 for x, y in zip(s0[k], s1[k]))


@pytest.mark.parametrize("w,h,ch,mode", ps.RISING_ROWS)
def test_refinement_climbs_as_on_the_reference(cuda, w, h, ch, mode):
    """refine_stills under a PredictionFlow with its default step weights, at the settings of tests/test_flow_pair_host.py
    test_refinement_on_the_reference_alone (n_repeat=4, n_ext=2, 8 steps of 2 bytes, float feedback, the left quarter kept) on the rows
    that rise there: reproducible from numpy and device input, kept columns untouched, no byte moves by more than 16, and the term rises.  On the float64 reference every row rises on every
    step, by x1.3 to x5 in all, so no tolerance is taken."""
    B = 2
    frames, sets = case_inputs(w, h, tuple(ch), B, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    mask = rs.refine_mask(w, h)
    flow = PredictionFlow(direction=fs.direction_of(mode, w, h))
    kw = dict(requant=False, objective="flow", flow=flow, mask=mask, **ps.REFINE)
    with PredNetTrainer(sets["live"], list(ch), w, h, B, 6) as tr:
        out, hist = train.refine_stills(tr, stills, **kw)
        out2, hist2 = train.refine_stills(tr, torch.from_numpy(stills).to(cuda), **kw)
        explicit = train.refine_stills(tr, stills, step_weights=[0.0] * 4 + [1.0], **dict(kw, iters=1))[1]
    _, ref_hist = ps.pair_refine_reference(w, h, tuple(ch), mode)
    print("refine prediction pairing %dx%d %s: %s (reference: %s)" % (w, h, mode, " ".join("%.4e" % v for v in hist), " ".join("%.4e" % v for v in ref_hist)))
    assert out.dtype == np.uint8 and out.shape == stills.shape and hist.shape == (9,) and hist.dtype == np.float64
    assert np.array_equal(out, out2) and np.array_equal(hist, hist2) and explicit[0] == hist[0] and explicit[1] == hist[1]
    assert np.array_equal(out[..., :w // 4], stills[..., :w // 4]) and (out != stills).any()
    assert np.abs(out.astype(np.int32) - stills).max() <= 8 * 2
    assert ref_hist[-1] > ref_hist[0] and hist[-1] > hist[0], hist


def test_refine_genomes_takes_the_pairing(cuda):
    """refine_genomes under a PredictionFlow at the setting of tests/cppn_grad_support.py: reproducible, the genomes move and differently
    than under the frame pairing, and the history's last entry is the loss a direct call with the pairing's default weights gives for the
    returned images.  Whether the loss rises is printed, not asserted: no CPU statement of that loop exists."""
    from tests import cppn_grad_support as S
    from tests.train_support import _weight_sets
    SIM = S.SIM
    w, h, ch = SIM["w"], SIM["h"], list(SIM["ch"])
    n_repeat, n_ext = SIM["n_repeat"], max(SIM["n_ext"], 2)
    settings = dict(radius=3, direction=train.flow_direction("tangent", w, h))
    flow, frame = PredictionFlow(**settings), FlowObjective(**settings)
    kw = dict(n_repeat=n_repeat, n_ext=n_ext, iters=SIM["iters"], lr=SIM["lr"], requant=False, objective="flow")
    cfg, genomes = S.sim_genomes()
    params = lambda g: ({k: (n.bias, n.response) for k, n in g.nodes.items()}, {k: c.weight for k, c in g.connections.items()})
    before = [params(g) for g in genomes]
    with PredNetTrainer(dict(_weight_sets(ch, w, h))["live"], ch, w, h, batch=len(genomes), max_steps=n_repeat + n_ext) as tr:
        out, history, images = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        out2, history2, images2 = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        out_f, history_f, _ = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=frame, **kw)
        frames = np.ascontiguousarray(np.broadcast_to(images[:, None], (len(genomes), n_repeat + n_ext) + images.shape[1:]))
        direct = tr.forward_backward(frames, n_fed=n_repeat, requant=False, step_weights=[0.0] * n_repeat + [1.0] * (n_ext - 1), objective="flow", flow=flow)
        with pytest.raises(ValueError):
            train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **dict(kw, n_ext=1))
    print("refine_genomes prediction pairing: %s; rose: %s" % (" ".join("%.4e" % v for v in history), history[-1] > history[0]))
    assert np.isfinite(history).all() and history.tobytes() == history2.tobytes() and images.tobytes() == images2.tobytes()
    assert [params(g) for g in out] == [params(g) for g in out2] and [params(g) for g in genomes] == before
    assert any(params(a) != b for a, b in zip(out, before)) and any(params(a) != params(b) for a, b in zip(out, out_f))
    assert history[0] != history_f[0] and history[-1] == direct


def test_refusals(cuda):
    """an unknown pairing, the prediction pairing with the moving-reference flag or under another objective, flags on
    eigen_trainer_flow_term_pair, too small a pg_bstride, a NULL prev, and n_ext = 1 under a PredictionFlow: each refused with
    EIGEN_ERR_INVALID (ValueError in Python), eigen_last_error set, and nothing launched or written"""
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 4
    frames, _ = case_inputs(w, h, tuple(ch), B, T)
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    pred = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    prev = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    with PredNetTrainer("synthetic", ch, w, h, B, T) as tr:
        buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
        terms = (ctypes.c_double * (T - 1))(*([float(SENT)] * (T - 1)))
        loss = ctypes.c_double(float(SENT))
        seed = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        pg = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        u = torch.full((B * 2 * h * w,), float(SENT), dtype=torch.float64, device=cuda)
        value = ctypes.c_double(float(SENT))
        call = lambda flags, pairing, grad=True, **kw: _raw_loss_grad(tr, "pair", d, B, T, n, flags, pairing, loss, terms, buf if grad else None, **kw)
        term = lambda flags=0, pg_b=n, out=pg, prv=prev: _raw_pair(tr, pred, n, prv, n, B, 7, 1e-2, None, None, 1.0, value, u, seed, n, out, pg_b, flags)

        def refused(rc, word):
            msg = tr.lib.eigen_last_error().decode()
            assert rc == -1 and word in msg, (rc, msg)

        for pairing in (2, 3, -1, 1 << 30):
            for flags in (0, 1):
                refused(call(flags, pairing), "pairing")
                refused(call(flags, pairing, grad=False), "pairing")
        refused(call(1, 1), "EIGEN_FLOW_MOVING_REFERENCE")
        refused(call(1, 1, grad=False), "EIGEN_FLOW_MOVING_REFERENCE")
        refused(call(2, 1), "flags")
        refused(call(0, 1, objective=0, settings=False), "EIGEN_OBJ_FLOW")
        refused(call(0, 1, objective=1, settings=False), "EIGEN_OBJ_FLOW")
        for flags in (1, 2, 3, -1):
            refused(term(flags), "flags")
        refused(term(pg_b=n - 1), "stride")
        refused(term(pg_b=0), "stride")
        refused(term(prv=None), "null")
        torch.cuda.synchronize()
        assert (buf == float(SENT)).all() and (seed == float(SENT)).all() and (u == float(SENT)).all() and (pg == float(SENT)).all()
        assert loss.value == float(SENT) and value.value == float(SENT) and list(terms) == [float(SENT)] * (T - 1)
        assert all(not g.any() for g in tr.grads().values())
        stills = np.ascontiguousarray(frames[:, 0])
        for given in (None, [1.0, 1.0, 1.0]):
            with pytest.raises(ValueError, match="n_ext"):
                train.refine_stills(tr, stills, n_repeat=3, n_ext=1, iters=1, objective="flow", flow=PredictionFlow(), step_weights=given)
        assert all(not g.any() for g in tr.grads().values())
        # and the accepted edges are accepted: both pairings through the new entry, the stage with and without the gradient buffer
        assert call(0, 1) == 0 and not (buf == float(SENT)).any() and loss.value != float(SENT)
        assert call(0, 0, grad=False) == 0 and call(1, 0) == 0
        assert term() == 0 and not (pg == float(SENT)).any()
        assert term(out=None, pg_b=0) == 0
