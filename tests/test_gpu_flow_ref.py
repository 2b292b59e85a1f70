"""The flow objective's moving reference on the GPU (eigen_trainer_flow_term_ref, EIGEN_FLOW_MOVING_REFERENCE,
FlowObjective(reference="moving")); DESIGN.md section 13, "The moving reference".  The reference gradient of one term is compared bit for
bit with the numpy restatement of tests/flow_ref_support.py, a training call with `run_flow(constant_reference=False)`, which
tests/test_flow_ref_host.py keeps under the float32 yardstick, and its composition with the float32 folds stated there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.train import FlowObjective, FlowSettings, PredNetTrainer
from tests import flow_obj_support as fs
from tests import flow_ref_support as rs
from tests.flow_gpu_support import SENT, _p, _padded, _raw_ref
from tests.frame_grad_support import case_inputs, check_frame_grads, zero_steps
from tests.train_support import case_weights

pytestmark = pytest.mark.gpu

WORST = {"frames": 0.0}


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("w,h,C,r,masked,modes", rs.FIELD_CASES)
def test_the_reference_gradient_is_the_numpy_restatement_bit_for_bit(cuda, w, h, C, r, masked, modes, kind):
    """`flow_term(..., reference_grad=True)` and the entry on padded strides `np.array_equal` `flow_ref_grad`; the padding is found
    untouched; value, u and seed are the bits of the call without the reference gradient."""
    B = 2
    pred, ref = fs.field_inputs(w, h, C, kind, B)
    mask = fs.field_mask(w, h) if masked else None
    per = C * h * w
    p_b, r_b, s_b, g_b = per + 5, per + 3, per + 7, per + 11
    d_pred, d_ref = _padded(pred, p_b, np.float32(np.nan), cuda), _padded(ref, r_b, np.uint8(255), cuda)
    d_mask = None if mask is None else torch.from_numpy(mask).to(cuda)
    with PredNetTrainer("synthetic", [C, 4], w, h, B + 1, 2) as tr:
        for mode in modes:
            d = fs.direction_of(mode, w, h)
            want = rs.flow_ref_grad(pred, ref, r, 1e-2, d, mask, scale=0.75)
            flow = FlowObjective(r, 1e-2, d, mask)
            v0, u0, s0 = tr.flow_term(pred, ref, flow, scale=0.75)
            v1, u1, s1, g1 = tr.flow_term(pred, ref, flow, scale=0.75, reference_grad=True)
            assert v1 == v0 and u1.tobytes() == u0.tobytes() and s1.tobytes() == s0.tobytes()
            assert g1.dtype == np.float32 and g1.shape == pred.shape and np.isfinite(g1).all() and np.abs(g1).max() > 0
            assert np.array_equal(g1, want.grad), (mode, np.abs(g1 - want.grad).max(), np.abs(want.grad).max())
            assert np.array_equal(u1, want.u) and np.array_equal(s1, want.seed)
            # the entry itself: every stride padded, u into the caller's buffer or into the workspace
            d_dir = None if d is None else torch.from_numpy(d).to(cuda)
            for with_u in (True, False):
                d_rg = torch.full((B * g_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
                d_seed = torch.full((B * s_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
                d_flow = torch.full((B * 2 * h * w + 4,), float(SENT), dtype=torch.float64, device=cuda) if with_u else None
                value = ctypes.c_double()
                assert _raw_ref(tr, d_pred, p_b, d_ref, r_b, B, r, 1e-2, d_dir, d_mask, 0.75, value, d_flow, d_seed if with_u else None, s_b, d_rg, g_b) == 0
                buf = d_rg.cpu().numpy()
                got = np.stack([buf[b * g_b:b * g_b + per].reshape(C, h, w) for b in range(B)])
                written = np.zeros(buf.shape, bool)
                for b in range(B):
                    written[b * g_b:b * g_b + per] = True
                assert (buf[~written] == SENT).all()
                assert np.array_equal(got, want.grad), (mode, with_u)
                assert value.value == v0
                if with_u:
                    uu = d_flow.cpu().numpy()
                    assert (uu[B * 2 * h * w:] == float(SENT)).all() and np.array_equal(uu[:B * 2 * h * w].reshape(B, 2, h, w), want.u)
            print("%dx%dx%d r=%d %s %s: max |reference gradient| %.3e, max |seed| %.3e" % (w, h, C, r, kind, mode, np.abs(g1).max(), np.abs(s1).max()))


@functools.lru_cache(maxsize=None)
def _gpu_and_ref(c):
    """the training calls of a case with the moving reference and their float64 references, made once"""
    frames, wts, call = fs.flow_case_frames(c), case_weights(c.w, c.h, c.ch, c.wset), fs.flow_case_call(c)
    flow = FlowObjective(reference="moving", **fs.flow_case_settings(c))
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, fs.B_CASE, frames.shape[1]) as tr:
        loss, pred, per = tr.forward_backward(frames, pred=True, objective="flow", flow=flow, frame_grads="frames", **call)
        grads = tr.grads()
        loss_t, tied = tr.forward_backward(frames, objective="flow", flow=flow, frame_grads="tied", **call)
    assert loss == loss_t
    # with requant both sides read the bytes of the GPU's own float32 predictions, as tests/test_gpu_flow_obj.py does
    r = fs.flow_case_reference(c, pred=pred, leaf="frames", constant_reference=False)
    rt = fs.flow_case_reference(c, pred=pred, leaf="tied", constant_reference=False) if c.form != "drifting" else None
    return (loss, per, tied, grads), r, rt


@pytest.mark.parametrize("c", rs.LIVE_CASES + rs.DEAD_CASES, ids=fs.flow_case_id)
def test_a_training_call_matches_float64_autograd_with_the_reference_in_the_graph(cuda, c):
    """ "frames" and "tied" against `run_flow(constant_reference=False)` with the frames, and for a still the still, as the leaf, by
    tests/frame_grad_support.py `check_frame_grads` with `zero_steps(T, n_fed, step_weights)`.  At the dead cases ("random" weights at
    the gray shapes) P0 sits at the clamp, every weight gradient is exactly zero and the frame gradient is the reference path alone,
    within the same bounds; the steps without a target path are then exactly zero.
    Measured on MI355X over the 72 cases: at worst 0.0008 of a bound."""
    (loss, per, tied, grads), r, rt = _gpu_and_ref(c)
    call = fs.flow_case_call(c)
    T = per.shape[1]
    dead = fs.is_dead(c)
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale
    if dead:
        assert all(not g.any() for g in grads.values()) and all(not g.any() for g in r.grads.values())
    zero = zero_steps(T, call["n_fed"], call["step_weights"], dead=dead)
    for t in zero:
        assert not per[:, t].any(), t
    ratio = check_frame_grads(per, r.frame_grad, fs.flow_case_id(c), tied=tied, zero=zero)
    if rt is not None:
        assert np.abs(rt.frame_grad - r.frame_grad.sum(1)).max() <= 1e-12 * np.abs(rt.frame_grad).max()
        ratio = max(ratio, check_frame_grads(tied[:, None], rt.frame_grad[:, None], fs.flow_case_id(c) + " tied leaf"))
    WORST["frames"] = max(WORST["frames"], ratio)
    print("moving reference %s: miss / bound %.4f (worst so far %.4f)" % (fs.flow_case_id(c), ratio, WORST["frames"]))


COMPOSE = [(12, 8, (1, 4), "tangent", "still", None), (16, 12, (3, 4, 6), "energy", "still_requant", None), (24, 16, (1, 4, 8), "energy", "drifting", None),
           (40, 24, (3, 4), "tangent", "drifting", [1.0, 0.0, 2.0, 0.5])]


@pytest.mark.parametrize("w,h,ch,mode,form,weights", COMPOSE)
def test_composition_and_invariance(cuda, w, h, ch, mode, form, weights):
    """Per frame g_t(moving) == fl(g_t(constant) + ref_{t-1}) bit for bit, ref_{t-1} from `flow_term` on the returned P0_{t-1} with
    scale = w_{t-1} / sum w; the tied output is the stated float32 fold; a term of weight zero adds nothing.  Loss, terms, weight
    gradients, predictions and the kept state are the same bits with the mode on and off, with and without a frame gradient."""
    c = fs.FlowCase(w, h, tuple(ch), "live", mode, 7, form)
    frames, wts, call = fs.flow_case_frames(c), case_weights(w, h, tuple(ch), "live"), fs.flow_case_call(c)
    if weights is not None:
        call["step_weights"] = weights
    B, T = frames.shape[:2]
    settings = fs.flow_case_settings(c)
    const, moving = FlowObjective(**settings), FlowObjective(reference="moving", **settings)
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        out = {}
        for name, flow in (("constant", const), ("moving", moving)):
            loss, pred, per, terms = tr.forward_backward(frames, pred=True, objective="flow", flow=flow, frame_grads="frames", flow_terms=True, **call)
            grads, seq = tr.grads(), tr.state_dict()["seq"]
            loss_t, tied = tr.forward_backward(frames, objective="flow", flow=flow, frame_grads="tied", **call)
            loss_0 = tr.forward_backward(frames, objective="flow", flow=flow, **call)
            assert loss == loss_t == loss_0
            assert all(np.array_equal(g, tr.grads()[k]) for k, g in grads.items())
            out[name] = (loss, pred, per, terms, grads, seq, tied)
        (l0, p0, per0, t0, g0, s0, tied0), (l1, p1, per1, t1, g1, s1, tied1) = out["constant"], out["moving"]
        assert l0 == l1 and p0.tobytes() == p1.tobytes() and t0.tobytes() == t1.tobytes()
        assert sorted(g0) == sorted(g1) and all(g0[k].tobytes() == g1[k].tobytes() for k in g0)
        assert all(a.tobytes() == b.tobytes() for k in s0 for a, b in zip(s0[k], s1[k]))
        w_s = call["step_weights"] or [1.0] * (T - 1)
        refs = {}
        for s in range(T - 1):
            if w_s[s] != 0:
                refs[s] = tr.flow_term(p1[:, s], frames[:, s + 1], const, scale=w_s[s] / sum(w_s), reference_grad=True)[3]
                assert refs[s].any()
    assert len(refs) < T - 1 or weights is None and form == "drifting"
    assert np.array_equal(per1, rs.add_reference_paths(per0, refs))
    assert np.array_equal(tied1, rs.fold_tied_moving(per0, refs))
    for s in range(T - 1):
        if s not in refs:
            assert per1[:, s + 1].tobytes() == per0[:, s + 1].tobytes()
    assert per1[:, 0].tobytes() == per0[:, 0].tobytes() and not np.array_equal(per1, per0) and not np.array_equal(tied1, tied0)


def test_two_adam_steps_do_not_depend_on_the_mode(cuda):
    w, h, ch = 16, 12, (3, 4, 6)
    c = fs.FlowCase(w, h, ch, "live", "tangent", 7, "drifting")
    frames, wts = fs.flow_case_frames(c), case_weights(w, h, ch, "live")
    got = []
    for reference in ("constant", "moving"):
        flow = FlowObjective(reference=reference, **fs.flow_case_settings(c))
        with PredNetTrainer(wts, list(ch), w, h, fs.B_CASE, frames.shape[1]) as tr:
            losses = [tr.step(frames, objective="flow", flow=flow) for _ in range(2)]
            got.append((losses, tr.weights()))
    assert got[0][0] == got[1][0] and got[0][0][0] != got[0][0][1]
    assert all(got[0][1][k].tobytes() == got[1][1][k].tobytes() for k in got[0][1])
    assert any(not np.array_equal(got[0][1][k], wts[k]) for k in wts)


@pytest.mark.parametrize("mode", ["tangent", "energy"])
@pytest.mark.parametrize("w,h,ch", rs.REFINE_SHAPES)
def test_refinement_climbs_with_the_moving_reference(cuda, w, h, ch, mode):
    """refine_stills(objective="flow", reference="moving") at the settings of tests/test_flow_ref_host.py
    test_refinement_on_the_reference_alone_climbs (n_repeat=4, n_ext=2, 8 steps of 2 bytes, float feedback, the left quarter kept), at all
    four shapes and in both modes: reproducible from numpy and device input, kept columns untouched, no byte moves by more than 16, and
    the term rises.  On the float64 reference alone it rises by x1.3 to x6, so no tolerance is taken."""
    B = 2
    frames, sets = case_inputs(w, h, tuple(ch), B, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    mask = rs.refine_mask(w, h)
    flow = FlowObjective(direction=fs.direction_of(mode, w, h), reference="moving")
    kw = dict(requant=False, objective="flow", flow=flow, mask=mask, **rs.REFINE)
    with PredNetTrainer(sets["live"], list(ch), w, h, B, 6) as tr:
        out, hist = train.refine_stills(tr, stills, **kw)
        out2, hist2 = train.refine_stills(tr, torch.from_numpy(stills).to(cuda), **kw)
    print("refine moving reference %dx%d %s: %s" % (w, h, mode, " ".join("%.4e" % v for v in hist)))
    assert out.dtype == np.uint8 and out.shape == stills.shape and hist.shape == (9,) and hist.dtype == np.float64
    assert np.array_equal(out, out2) and np.array_equal(hist, hist2)
    assert np.array_equal(out[..., :w // 4], stills[..., :w // 4]) and (out != stills).any()
    assert np.abs(out.astype(np.int32) - stills).max() <= 8 * 2
    assert hist[-1] > hist[0], hist


def test_refine_genomes_takes_the_mode(cuda):
    """refine_genomes(objective="flow") with reference="moving" at the setting of tests/cppn_grad_support.py: reproducible, the inputs
    untouched, the genomes move and differently than with the constant reference, the history finite and its last entry the loss a direct
    call gives for the returned images.  Whether the loss rises is printed, not asserted: no CPU statement of that loop exists."""
    import copy
    from tests import cppn_grad_support as S
    from tests.train_support import _weight_sets
    SIM = S.SIM
    w, h, ch = SIM["w"], SIM["h"], list(SIM["ch"])
    n_repeat, n_ext = SIM["n_repeat"], SIM["n_ext"]
    settings = dict(radius=3, direction=train.flow_direction("tangent", w, h))
    flow, const = FlowObjective(reference="moving", **settings), FlowObjective(**settings)
    kw = dict(n_repeat=n_repeat, n_ext=n_ext, iters=SIM["iters"], lr=SIM["lr"], requant=False, objective="flow")
    cfg, genomes = S.sim_genomes()
    before = copy.deepcopy(genomes)
    params = lambda g: ({k: (n.bias, n.response) for k, n in g.nodes.items()}, {k: c.weight for k, c in g.connections.items()})
    with PredNetTrainer(dict(_weight_sets(ch, w, h))["live"], ch, w, h, batch=len(genomes), max_steps=n_repeat + n_ext) as tr:
        out, history, images = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        out2, history2, images2 = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        out_c, history_c, _ = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=const, **kw)
        frames = np.ascontiguousarray(np.broadcast_to(images[:, None], (len(genomes), n_repeat + n_ext) + images.shape[1:]))
        direct = tr.forward_backward(frames, n_fed=n_repeat, requant=False, step_weights=[0.0] * (n_repeat - 1) + [1.0] * n_ext, objective="flow", flow=flow)
    print("refine_genomes moving reference: %s; rose: %s (constant reference: %s; rose: %s)" % (
        " ".join("%.4e" % v for v in history), history[-1] > history[0], " ".join("%.4e" % v for v in history_c), history_c[-1] > history_c[0]))
    assert np.isfinite(history).all() and history.tobytes() == history2.tobytes() and images.tobytes() == images2.tobytes()
    assert [params(g) for g in out] == [params(g) for g in out2] and [params(g) for g in genomes] == [params(g) for g in before]
    assert any(params(a) != params(b) for a, b in zip(out, before))
    assert history[0] == history_c[0] and any(params(a) != params(b) for a, b in zip(out, out_c))
    assert history[-1] == direct


def test_refusals(cuda):
    """unknown flag bits, flags on the stage-alone entries, too small an rg_bstride, an unknown reference: refused with nothing launched
    or written"""
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 4
    frames, _ = case_inputs(w, h, tuple(ch), B, T)
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    pred = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    ref = d[:, 0].contiguous()
    with PredNetTrainer("synthetic", ch, w, h, B, T) as tr:
        buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
        terms = (ctypes.c_double * (T - 1))(*([float(SENT)] * (T - 1)))
        loss = ctypes.c_double(float(SENT))

        def call(flags, grad=True):
            cfg = FlowSettings(7, flags, 1e-2)
            return tr.lib.eigen_trainer_loss_grad_flow(tr._h, _p(d), T * n, B, T, T, 0, 1, None, 2, None, ctypes.byref(loss), None, None, _p(buf) if grad else None,
                                                       T * n if grad else 0, n if grad else 0, ctypes.byref(cfg), None, None, terms, None)

        seed = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        rg = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        u = torch.full((B * 2 * h * w,), float(SENT), dtype=torch.float64, device=cuda)
        value = ctypes.c_double(float(SENT))

        def term(flags):
            cfg = FlowSettings(7, flags, 1e-2)
            return tr.lib.eigen_trainer_flow_term(tr._h, _p(pred), n, _p(ref), n, B, ctypes.byref(cfg), None, None, ctypes.c_double(1.0), ctypes.byref(value), _p(u),
                                                  _p(seed), n, None)

        term_ref = lambda flags=0, rg_b=n, out=rg: _raw_ref(tr, pred, n, ref, n, B, 7, 1e-2, None, None, 1.0, value, u, seed, n, out, rg_b, flags)
        for flags in (2, 3, 4, 1 << 30, -1, -2):
            assert call(flags) == -1 and call(flags, grad=False) == -1
        for flags in (1, 2, 3, -1):
            assert term(flags) == -1 and term_ref(flags) == -1
        assert term_ref(rg_b=n - 1) == -1 and term_ref(rg_b=0) == -1 and term_ref(out=None) == -1
        torch.cuda.synchronize()
        assert (buf == float(SENT)).all() and (seed == float(SENT)).all() and (u == float(SENT)).all() and (rg == float(SENT)).all()
        assert loss.value == float(SENT) and value.value == float(SENT) and list(terms) == [float(SENT)] * (T - 1)
        assert all(not g.any() for g in tr.grads().values())
        with pytest.raises(ValueError):
            FlowObjective(reference="other")
        # and the accepted edges are accepted: the flag with and without a frame-gradient buffer, where it changes nothing
        assert call(1) == 0 and not (buf == float(SENT)).any()
        with_grad = (loss.value, list(terms), {k: g.copy() for k, g in tr.grads().items()})
        assert call(1, grad=False) == 0 and call(0, grad=False) == 0
        assert (loss.value, list(terms)) == with_grad[:2] and all(np.array_equal(g, with_grad[2][k]) for k, g in tr.grads().items())
        assert term(0) == 0 and term_ref() == 0 and not (rg == float(SENT)).any()
