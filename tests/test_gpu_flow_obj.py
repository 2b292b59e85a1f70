"""The flow objective of the trainer (eigen_trainer_flow_term, eigen_trainer_loss_grad_flow, forward_backward(objective="flow"));
DESIGN.md section 13, "The flow objective".  The fields are compared bit for bit with the numpy restatement of
tests/flow_obj_support.py, a training call with its float64 autograd statement `run_flow`, which tests/test_flow_obj_host.py pins to
oracle/prednet_train_ref.py and keeps under the float32 yardstick of the gradient rule."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.engine import EngineError
from evolutionary_illusion_generator_amd.train import FlowObjective, FlowSettings, PredNetTrainer
from tests import flow_obj_support as fs
from tests.flow_gpu_support import SENT, _p, _padded, _raw_term
from tests.frame_grad_support import case_inputs, check_frame_grads, fold_tied
from tests.train_support import _check_grads, _grads_differ, case_weights

pytestmark = pytest.mark.gpu

WORST = {"norm": 0.0, "element": 0.0, "loss": 0.0, "frames": 0.0}


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("w,h,C,r,masked,modes", fs.FIELD_CASES)
def test_flow_and_seed_are_the_numpy_restatement_bit_for_bit(cuda, w, h, C, r, masked, modes, kind):
    """u and seed `np.array_equal` the float64 restatement; the value is within N 2^-53 sum |m v| / (B N_m), N = B H W summands, of the
    exactly summed one.  Every batch stride is padded and the padding is found untouched."""
    B = 2
    pred, ref = fs.field_inputs(w, h, C, kind, B)
    mask = fs.field_mask(w, h) if masked else None
    per = C * h * w
    p_b, r_b, s_b = per + 5, per + 3, per + 7
    d_pred, d_ref = _padded(pred, p_b, np.float32(np.nan), cuda), _padded(ref, r_b, np.uint8(255), cuda)
    d_mask = None if mask is None else torch.from_numpy(mask).to(cuda)
    with PredNetTrainer("synthetic", [C, 4], w, h, B + 1, 2) as tr:
        for mode in modes:
            d = fs.direction_of(mode, w, h)
            want = fs.flow_ref(pred, ref, r, 1e-2, d, mask, scale=0.75)
            d_dir = None if d is None else torch.from_numpy(d).to(cuda)
            d_seed = torch.full((B * s_b + 3,), float(SENT), dtype=torch.float32, device=cuda)
            d_flow = torch.full((B * 2 * h * w + 4,), float(SENT), dtype=torch.float64, device=cuda)
            value = ctypes.c_double()
            assert _raw_term(tr, d_pred, p_b, d_ref, r_b, B, r, 1e-2, d_dir, d_mask, 0.75, value, d_flow, d_seed, s_b) == 0
            u = d_flow.cpu().numpy()
            assert (u[B * 2 * h * w:] == float(SENT)).all()
            u = u[:B * 2 * h * w].reshape(B, 2, h, w)
            seed_buf = d_seed.cpu().numpy()
            seed = np.stack([seed_buf[b * s_b:b * s_b + per].reshape(C, h, w) for b in range(B)])
            written = np.zeros(seed_buf.shape, bool)
            for b in range(B):
                written[b * s_b:b * s_b + per] = True
            assert (seed_buf[~written] == SENT).all()
            assert np.isfinite(u).all() and np.abs(u).max() > 0 and np.abs(seed).max() > 0
            assert np.array_equal(u, want.u), (mode, np.abs(u - want.u).max())
            assert np.array_equal(seed, want.seed), (mode, np.abs(seed - want.seed).max())
            assert abs(value.value - want.value) <= want.bound, (mode, value.value, want.value, want.bound)
            print("%dx%dx%d r=%d %s %s: value %.17g, |error| %.2e of the bound %.2e, mean |u| %.3f" % (w, h, C, r, kind, mode, value.value,
                                                                                                   abs(value.value - want.value), want.bound, np.abs(u).mean()))
            # the Python call gives the same three and each output is optional
            v2, u2, s2 = tr.flow_term(pred, ref, FlowObjective(r, 1e-2, d, mask), scale=0.75)
            assert v2 == value.value and np.array_equal(u2, u) and np.array_equal(s2, seed)
            assert _raw_term(tr, d_pred, p_b, d_ref, r_b, B, r, 1e-2, d_dir, d_mask, 0.75, None, None, None, 0) == 0


@functools.lru_cache(maxsize=None)
def _gpu_and_ref(c):
    """one training call of a case and its float64 reference, made once"""
    frames, wts, call = fs.flow_case_frames(c), case_weights(c.w, c.h, c.ch, c.wset), fs.flow_case_call(c)
    flow = FlowObjective(**fs.flow_case_settings(c))
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, fs.B_CASE, frames.shape[1]) as tr:
        loss, pred, terms = tr.forward_backward(frames, pred=True, objective="flow", flow=flow, flow_terms=True, **call)
        grads = tr.grads()
    # with requant both sides read the bytes of the GPU's own float32 predictions, as tests/test_gpu_train_ext.py does
    return (loss, pred, terms, grads), fs.flow_case_reference(c, pred=pred)


@pytest.mark.parametrize("c", fs.FLOW_CASES, ids=fs.flow_case_id)
def test_a_training_call_matches_float64_autograd(cuda, c):
    """Gradients: `_check_grads` of tests/train_support.py, unchanged, per tensor.  Predictions within 1e-5 absolute.  Loss and every term
    within 1e-5 sum m |v| / (B N_m), the un-cancelled scale (a directed term can cancel to near zero).  The "random" weights at the
    gray shapes are the declared all-zero cases: P0 sits at the clamp everywhere, every gradient is exactly zero and the loss, which
    is not, still matches.
    Measured on MI355X over the 84 cases: at worst 0.0071 of the norm bound, 0.0087 of the element-wise bound and 0.0036 of the loss bound."""
    (loss, pred, terms, grads), r = _gpu_and_ref(c)
    assert np.abs(pred - r.pred).max() <= 1e-5
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss, r.scale)
    assert terms.shape == r.terms.shape and (np.abs(terms - r.terms) <= 1e-5 * r.term_scales).all(), (terms, r.terms)
    assert (terms == 0).tolist() == (r.terms == 0).tolist()
    if fs.is_dead(c):
        assert loss != 0 and all(not g.any() for g in grads.values()) and all(not g.any() for g in r.grads.values())
    norm, element = _check_grads(grads, r.grads, zero_allowed=fs.is_dead(c), what=fs.flow_case_id(c))
    lossr = abs(loss - r.loss) / (1e-5 * r.scale)
    for k, v in (("norm", norm), ("element", element), ("loss", lossr)):
        WORST[k] = max(WORST[k], v)
    print("flow %s: error / bound norm %.4f element %.4f loss %.4f (worst so far %.4f %.4f %.4f)" % (fs.flow_case_id(c), norm, element, lossr, WORST["norm"],
                                                                                                 WORST["element"], WORST["loss"]))


@pytest.mark.parametrize("w,h,ch", fs.FLOW_SHAPES)
def test_the_objective_cannot_vanish_or_flip_unnoticed(cuda, w, h, ch):
    """Against the reference of the other mode, and against the reference with the direction negated, the GPU's gradients are outside
    the bound they meet against their own reference."""
    energy, tangent = (fs.FlowCase(w, h, tuple(ch), "live", mode, 7, "still") for mode in ("energy", "tangent"))
    (_, _, _, g_e), r_e = _gpu_and_ref(energy)
    (_, _, _, g_t), r_t = _gpu_and_ref(tangent)
    _check_grads(g_e, r_e.grads)
    _check_grads(g_t, r_t.grads)
    assert _grads_differ(r_t.grads, g_e) and _grads_differ(r_e.grads, g_t)
    wts, frames = case_weights(w, h, tuple(ch), "live"), fs.flow_case_frames(tangent)
    args = dict(fs.flow_case_call(tangent), **fs.flow_case_settings(tangent))
    args["direction"] = -args["direction"]
    flipped = fs.run_flow(wts, ch, frames, **args)
    assert _grads_differ(flipped.grads, g_t)


@pytest.mark.parametrize("form", ["still", "drifting"])
@pytest.mark.parametrize("mode", fs.MODES)
@pytest.mark.parametrize("w,h,ch", fs.FLOW_SHAPES)
def test_frame_gradients_are_the_input_path_alone(cuda, w, h, ch, mode, form):
    """ "frames" and "tied" against `run_flow` with the frames as the leaf, by tests/frame_grad_support.py `check_frame_grads`; the tied
    output is the float32 fold of the per-frame one.  The reference frame is a constant of every term: a step that reads no frame, and
    the last step, whose prediction enters no term, are exactly zero, and the reference with a target path added misses the bound."""
    c = fs.FlowCase(w, h, tuple(ch), "live", mode, 7, form)
    frames, wts, call = fs.flow_case_frames(c), case_weights(w, h, tuple(ch), "live"), fs.flow_case_call(c)
    T = frames.shape[1]
    flow = FlowObjective(**fs.flow_case_settings(c))
    with PredNetTrainer(wts, ch, w, h, fs.B_CASE, T) as tr:
        loss, per = tr.forward_backward(frames, objective="flow", flow=flow, frame_grads="frames", **call)
        loss_t, tied = tr.forward_backward(frames, objective="flow", flow=flow, frame_grads="tied", **call)
        loss_0 = tr.forward_backward(frames, objective="flow", flow=flow, **call)
    assert loss == loss_t == loss_0
    assert np.array_equal(tied, fold_tied(per))
    r = fs.flow_case_reference(c, leaf="frames")
    zero = {4, 5} if form == "still" else {T - 1}
    for t in zero:
        assert not per[:, t].any() and not r.frame_grad[:, t].any(), t
    ratio = check_frame_grads(per, r.frame_grad, fs.flow_case_id(c), tied=tied, zero=zero)
    WORST["frames"] = max(WORST["frames"], ratio)
    print("flow frame gradient %s: miss / bound %.4f (worst so far %.4f)" % (fs.flow_case_id(c), ratio, WORST["frames"]))
    if form == "still":
        rt = fs.flow_case_reference(c, leaf="tied")
        assert np.abs(rt.frame_grad - r.frame_grad.sum(1)).max() <= 1e-12 * np.abs(rt.frame_grad).max()
    with_target = fs.flow_case_reference(c, leaf="frames", constant_reference=False)
    with pytest.raises(AssertionError):
        check_frame_grads(per, with_target.frame_grad, "with a target path", tied=tied, zero=range(T))


def test_refinement_raises_the_flow_term_and_is_reproducible(cuda):
    """refine_stills(objective="flow") along the tangent with the "live" weights and the settings of tests/test_gpu_frame_grad.py
    test_refinement_raises_the_stand_in_loss_and_is_reproducible: n_repeat=4, n_ext=2, iters=8, step=2, requant=False, the left
    quarter kept.
    The shapes: 12 x 8 gray alone.  On the float64 reference alone (`run_flow` with the tied leaf, tests/frame_grad_support.py
    `still_step_ref`) the term rose on every one of the 8 steps there, 0.3741 -> 0.4258; at 16 x 12 colour, 24 x 16 gray and 40 x 24
    colour it FELL (0.348 -> 0.309, 0.465 -> 0.265, 0.0682 -> 0.0640), and in the energy mode it fell at all four.  The gradient this
    objective gives by a still is the input path alone: the still is also the reference frame of every term, a constant of the graph,
    so the step ignores how the term moves with its reference.  Those shapes are left out of this test for that reason."""
    w, h, ch = 12, 8, [1, 4]
    B = 2
    frames, sets = case_inputs(w, h, tuple(ch), B, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    mask = np.ones((h, w), np.uint8)
    mask[:, :w // 4] = 0
    flow = FlowObjective(direction=train.flow_direction("tangent", w, h))
    kw = dict(n_repeat=4, n_ext=2, iters=8, step=2, requant=False, objective="flow", flow=flow, mask=mask)
    with PredNetTrainer(sets["live"], ch, w, h, B, 6) as tr:
        out, hist = train.refine_stills(tr, stills, **kw)
        out2, hist2 = train.refine_stills(tr, torch.from_numpy(stills).to(cuda), **kw)
    print("refine flow %dx%d tangent: %s" % (w, h, " ".join("%.4e" % v for v in hist)))
    assert out.dtype == np.uint8 and out.shape == stills.shape and hist.shape == (9,) and hist.dtype == np.float64
    assert hist[-1] > hist[0], hist
    assert np.array_equal(out, out2) and np.array_equal(hist, hist2)
    assert np.array_equal(out[..., :w // 4], stills[..., :w // 4]) and (out != stills).any()
    assert np.abs(out.astype(np.int32) - stills).max() <= 8 * 2


def test_refine_genomes_takes_the_objective(cuda):
    """refine_genomes(objective="flow") at the setting of tests/cppn_grad_support.py: reproducible, the inputs untouched, the genomes move,
    and the history is the flow loss of the images it rendered (its last entry is the loss a direct call gives for the returned images).
    Whether the loss rises is not asserted: the gradient by a still is the input path alone (see the refinement test above)."""
    import copy
    from tests import cppn_grad_support as S
    from tests.train_support import _weight_sets
    SIM = S.SIM
    w, h, ch = SIM["w"], SIM["h"], list(SIM["ch"])
    n_repeat, n_ext = SIM["n_repeat"], SIM["n_ext"]
    flow = FlowObjective(radius=3, direction=train.flow_direction("tangent", w, h))
    kw = dict(n_repeat=n_repeat, n_ext=n_ext, iters=SIM["iters"], lr=SIM["lr"], requant=False, objective="flow", flow=flow)
    cfg, genomes = S.sim_genomes()
    before = copy.deepcopy(genomes)
    params = lambda g: ({k: (n.bias, n.response) for k, n in g.nodes.items()}, {k: c.weight for k, c in g.connections.items()})
    with PredNetTrainer(dict(_weight_sets(ch, w, h))["live"], ch, w, h, batch=len(genomes), max_steps=n_repeat + n_ext) as tr:
        out, history, images = train.refine_genomes(tr, genomes, cfg, SIM["structure"], **kw)
        out2, history2, images2 = train.refine_genomes(tr, genomes, cfg, SIM["structure"], **kw)
        frames = np.ascontiguousarray(np.broadcast_to(images[:, None], (len(genomes), n_repeat + n_ext) + images.shape[1:]))
        direct = tr.forward_backward(frames, n_fed=n_repeat, requant=False, step_weights=[0.0] * (n_repeat - 1) + [1.0] * n_ext, objective="flow", flow=flow)
        other = tr.forward_backward(frames, n_fed=n_repeat, requant=False, step_weights=[0.0] * (n_repeat - 1) + [1.0] * n_ext)
    print("refine_genomes flow: %s" % " ".join("%.4e" % v for v in history))
    assert np.isfinite(history).all() and history.tobytes() == history2.tobytes() and images.tobytes() == images2.tobytes()
    assert [params(g) for g in out] == [params(g) for g in out2] and [params(g) for g in genomes] == [params(g) for g in before]
    assert any(params(a) != params(b) for a, b in zip(out, before))
    assert history[-1] == direct and direct != other


def test_error_returns(cuda):
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 4
    frames, _ = case_inputs(w, h, tuple(ch), B, T)
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    good_dir = torch.from_numpy(train.flow_direction("tangent", w, h)).to(cuda)
    bad_dirs = []
    for bad in (float("nan"), float("inf")):
        t = good_dir.clone()
        t[1, h - 1, w - 1] = bad
        bad_dirs.append(t)
    zero_mask = torch.zeros((h, w), dtype=torch.uint8, device=cuda)
    one_mask = zero_mask.clone()
    one_mask[3, 5] = 1
    pred = torch.rand((B, ch[0], h, w), dtype=torch.float32, device=cuda)
    ref = d[:, 0].contiguous()
    with PredNetTrainer("synthetic", ch, w, h, B, T) as tr:
        buf = torch.full((B * T * n,), float(SENT), dtype=torch.float32, device=cuda)
        terms = (ctypes.c_double * (T - 1))(*([float(SENT)] * (T - 1)))
        loss = ctypes.c_double(float(SENT))

        def call(objective=2, radius=7, eps=1e-2, d_dir=None, d_mask=None, settings=True):
            cfg = FlowSettings(radius, 0, eps)
            return tr.lib.eigen_trainer_loss_grad_flow(tr._h, _p(d), T * n, B, T, T, 0, 1, None, objective, None, ctypes.byref(loss), None, None, _p(buf), T * n, n,
                                                       ctypes.byref(cfg) if settings else None, _p(d_dir), _p(d_mask), terms, None)

        seed = torch.full((B * n,), float(SENT), dtype=torch.float32, device=cuda)
        u = torch.full((B * 2 * h * w,), float(SENT), dtype=torch.float64, device=cuda)
        value = ctypes.c_double(float(SENT))
        term = lambda radius=7, eps=1e-2, d_dir=None, d_mask=None, settings=True, batch=B, p_b=n, r_b=n, s_b=n, scale=1.0: _raw_term(
            tr, pred, p_b, ref, r_b, batch, radius, eps, d_dir, d_mask, scale, value, u, seed, s_b, settings)
        for fn in (call, term):
            for radius in (0, 17, -3):
                assert fn(radius=radius) == -1
            for eps in (0.0, -1e-2, float("nan"), float("inf")):
                assert fn(eps=eps) == -1
            for bad in bad_dirs:
                assert fn(d_dir=bad) == -1
            assert fn(d_mask=zero_mask) == -1
            assert fn(settings=False) == -1
        assert term(batch=0) == -1 and term(batch=B + 1) == -4
        assert term(p_b=n - 1) == -1 and term(r_b=n - 1) == -1 and term(s_b=n - 1) == -1 and term(scale=float("nan")) == -1
        assert call(objective=3) == -1 and call(objective=-1) == -1
        # settings, a direction or a mask with another objective
        assert call(objective=0) == -1 and call(objective=1, settings=False, d_mask=one_mask) == -1 and call(objective=0, settings=False, d_dir=good_dir) == -1
        # the entries without settings refuse the objective
        assert tr.lib.eigen_trainer_loss_grad_obj(tr._h, _p(d), T * n, B, T, T, 0, 1, None, 2, None, ctypes.byref(loss), None, None, None) == -1
        assert tr.lib.eigen_trainer_loss_grad_frames(tr._h, _p(d), T * n, B, T, T, 0, 1, None, 2, None, ctypes.byref(loss), None, None, _p(buf), T * n, n, None) == -1
        # a refused call writes nothing
        torch.cuda.synchronize()
        assert (buf == float(SENT)).all() and (seed == float(SENT)).all() and (u == float(SENT)).all()
        assert loss.value == float(SENT) and value.value == float(SENT) and list(terms) == [float(SENT)] * (T - 1)
        assert all(not g.any() for g in tr.grads().values())
        # and the accepted edges are accepted
        assert call(radius=1, d_mask=one_mask, d_dir=good_dir) == 0 and call(radius=16) == 0 and call(objective=0, settings=False) == 0
        assert term(radius=16, d_mask=one_mask) == 0 and np.isfinite(value.value)
        assert not (buf == float(SENT)).any() and all(np.isfinite(v) for v in terms)
        flow = FlowObjective()
        with pytest.raises(ValueError):
            tr.forward_backward(frames, objective="flow")
        with pytest.raises(ValueError):
            tr.step(frames, objective="flow")
        for objective in ("mse", "error"):
            with pytest.raises(ValueError):
                tr.forward_backward(frames, objective=objective, flow=flow)
        with pytest.raises(ValueError):
            tr.forward_backward(frames, flow_terms=True)
        with pytest.raises(ValueError):
            train.refine_stills(tr, frames[:, 0], n_repeat=2, n_ext=2, objective="flow")
        with pytest.raises(ValueError):
            tr.forward_backward(frames, objective="flow", flow=FlowObjective(mask=np.ones((h + 1, w), np.uint8)))
        with pytest.raises(ValueError):
            tr.flow_term(np.zeros((B, ch[0], h, w), np.float32), frames[:, 0], None)
        # every existing rule of a call holds under the objective
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, objective="flow", flow=flow, step_weights=[0.0, 0.0, 0.0])
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, objective="flow", flow=flow, n_fed=T + 1)
        with pytest.raises(EngineError, match="error -4"):
            tr.forward_backward(np.concatenate([frames, frames[:, :1]], 1), objective="flow", flow=flow)
        loss2, terms2 = tr.forward_backward(frames, objective="flow", flow=flow, flow_terms=True, step_weights=[1.0, 0.0, 2.0])
        assert terms2[1] == 0.0 and terms2[0] != 0 and terms2[2] != 0 and loss2 == (1.0 * terms2[0] + 0.0 * terms2[1] + 2.0 * terms2[2]) / 3.0
        tr.step(frames, objective="flow", flow=flow)
