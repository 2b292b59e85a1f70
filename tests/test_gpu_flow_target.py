"""The flow objective against a target field on the GPU (eigen_trainer_flow_term_target, eigen_trainer_loss_grad_flow_target,
``forward_backward(flow_target=)``, ``flow_term(target=)``, ``train.flow_epe``; DESIGN.md section 13, "The target field").  The field
and the value are compared bit for bit with the numpy restatement of tests/flow_target_support.py; the seed and the reference gradient,
float32 out of float64 arithmetic, tensor by tensor with its float64 autograd statement under the bound of tests/test_gpu_flow_iter.py,
max |got - ref| <= 2^-23 max |ref|; a training call meets `flow_obj_support.run_flow` under `TargetTerm` by the unchanged gradient
rules."""
import ctypes

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.train import FlowObjective, PredictionFlow, PredNetTrainer
from tests import flow_iter_support as fi
from tests import flow_target_support as ft
from tests.frame_grad_support import check_frame_grads
from tests.train_support import _check_grads, _grads_differ

pytestmark = pytest.mark.gpu

SCALE = 0.75
WORST = {"stage": 0.0}


def _trainer(name):
    """a trainer for the stage alone on a shape's image: two layers where the image halves, one where it is odd"""
    _, w, h, C, seeds, _ = next(s for s in ft.STAGE_SHAPES if s[0] == name)
    return PredNetTrainer("synthetic", [C, 4] if w % 2 == 0 and h % 2 == 0 else [C], w, h, len(seeds), 2)


def _objective(r, solve, mask=None):
    return FlowObjective(r, ft.EPS, mask=mask).solved(*solve)


def _check_tensor(got, ref64, what):
    """the bound of tests/test_gpu_flow_iter.py: `flow_iter_support.within`, 2^-23 of the tensor's maximum"""
    err, bound = fi.within(got, ref64)
    assert bound > 0, what
    WORST["stage"] = max(WORST["stage"], err / bound)
    print("%s: max |got - ref| %.3e, bound %.3e (ratio %.3f, worst so far %.3f)" % (what, err, bound, err / bound, WORST["stage"]))
    assert err <= bound, (what, err, bound)


def _stage_calls(tr, name, r, solve, mask, target):
    """the stage under both pairings: `flow_term` on the byte reference and `flow_term_pair` / `flow_term_pair_target` on the same
    bytes as floats"""
    img0, img1, _ = ft.stage_inputs(name)
    pred, prev = fi.as_floats(img1), fi.as_floats(img0)
    flow = _objective(r, solve, mask)
    by_pair = tr.flow_term_pair(pred, prev, flow, scale=SCALE, reference_grad=True) if target is None else \
        tr.flow_term_pair_target(pred, prev, flow, target, scale=SCALE, reference_grad=True)
    return tr.flow_term(pred, img0, flow, scale=SCALE, reference_grad=True, target=target), by_pair


@pytest.mark.parametrize("case", ft.STAGE_CASES, ids=ft.stage_case_id)
def test_the_stage_alone_meets_the_restatement_and_the_autograd_statement(cuda, case):
    """Per shape, radius and solve, with and without the shared mask, under both pairings (a byte and a float reference), against the
    exact flow of the pair: the field and the value are the numpy restatement's bit for bit, the seed and the reference gradient are
    within 2^-23 of their tensor's maximum of float64 autograd, and both entries return the same bytes."""
    name, r, solve = case
    img0, _, truth = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    with _trainer(name) as tr:
        for masked in (False, True):
            rest, stmt = ft.stage_reference(name, r, solve, masked)
            by_frame, by_pair = _stage_calls(tr, name, r, solve, ft.stage_mask(w, h) if masked else None, truth)
            what = "%s %s" % (ft.stage_case_id(case), "masked" if masked else "whole")
            assert by_frame[0] == by_pair[0] and all(x.tobytes() == y.tobytes() for x, y in zip(by_frame[1:], by_pair[1:])), what
            value, u, seed, rg = by_frame
            assert np.array_equal(u, rest.u), (what, np.abs(u - rest.u).max())
            print("%s: value %.17g, restatement %.17g" % (what, value, rest.value))
            assert np.array_equal(value, rest.value), (what, value, rest.value)
            assert seed.dtype == np.float32 and rg.dtype == np.float32
            _check_tensor(seed, SCALE * stmt.seed64, what + " seed")
            _check_tensor(rg, SCALE * stmt.ref64, what + " reference gradient")


@pytest.mark.parametrize("solve", ft.SOLVES, ids=lambda s: "%dx%d" % s)
def test_a_zero_target_is_the_mean_squared_displacement(cuda, solve):
    """every shape at radius 3 under the mask, both pairings: a target of zeros returns the value, field, seed and reference gradient of
    the call without a target, bit for bit"""
    for name, w, h, _, _, _ in ft.STAGE_SHAPES:
        _, _, truth = ft.stage_inputs(name)
        mask = ft.stage_mask(w, h)
        with _trainer(name) as tr:
            plain = _stage_calls(tr, name, 3, solve, mask, None)
            zero = _stage_calls(tr, name, 3, solve, mask, np.zeros_like(truth))
        for a, b in zip(plain, zero):
            assert a[0] == b[0] != 0.0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), (name, solve)
            assert np.abs(a[2]).max() > 0 and np.abs(a[3]).max() > 0


@pytest.mark.parametrize("solve", ft.SOLVES, ids=lambda s: "%dx%d" % s)
def test_the_field_itself_as_the_target_gives_exact_zeros(cuda, solve):
    """a target equal to the field the first call returned: the value is exactly 0.0 and the seed and the reference gradient are all
    zero, on every shape, with a numpy target and with a device tensor"""
    import torch
    for name, w, h, _, _, _ in ft.STAGE_SHAPES:
        with _trainer(name) as tr:
            first = _stage_calls(tr, name, 3, solve, None, None)
            for own in (first[0][1], torch.from_numpy(first[0][1]).to(cuda)):
                for value, u, seed, rg in _stage_calls(tr, name, 3, solve, None, own):
                    assert value == 0.0 and np.array_equal(u, first[0][1]) and not seed.any() and not rg.any(), (name, solve, value)


# ---- the entries themselves
def _raw_term(tr, cuda, entry, pred, ref, flow, solve, tail=()):
    """eigen_trainer_flow_term_iter ("iter") or eigen_trainer_flow_term_target ("target", with `tail`: d_target, t_bstride) called
    directly -> (rc, value, u, seed, reference gradient)"""
    import torch
    from evolutionary_illusion_generator_amd.engine import DenseSolveC, _ptr
    n, C, h, w = pred.shape
    per = C * h * w
    p, r = torch.from_numpy(pred).to(cuda), torch.from_numpy(ref).to(cuda)
    float_ref = ref.dtype == np.float32
    d_dir, d_mask = flow.on_device(torch, tr.device, h, w)
    cfg = flow.settings(stage_alone=True)
    sc = flow.score.settings(h) if flow.score is not None else None
    by_circles = isinstance(flow.score, train.FlowScore)
    mem = flow.members_settings(n, h, w) if flow.score is not None else None
    by = lambda x: None if x is None else ctypes.byref(x)
    value = ctypes.c_double()
    u = torch.zeros((n, 2, h, w), dtype=torch.float64, device=cuda)
    seed, rg = (torch.zeros((n, C, h, w), dtype=torch.float32, device=cuda) for _ in range(2))
    s = None if solve is None else DenseSolveC(*solve)
    fn = getattr(tr.lib, "eigen_trainer_flow_term_" + entry)
    rc = fn(tr._h, _ptr(p), ctypes.c_int64(per), None if float_ref else _ptr(r), _ptr(r) if float_ref else None, ctypes.c_int64(per), ctypes.c_int32(n),
            ctypes.byref(cfg), _ptr(d_mask), by(sc if by_circles else None), by(None if by_circles else sc), by(mem), ctypes.c_double(SCALE), ctypes.byref(value), None,
            _ptr(u), _ptr(seed), ctypes.c_int64(per), _ptr(rg), ctypes.c_int64(per), None, _ptr(d_dir), by(s), *tail)
    return rc, value.value, u.cpu().numpy(), seed.cpu().numpy(), rg.cpu().numpy()


def _raw_loss_grad(tr, cuda, entry, frames, flow, solve, objective=2, tail=()):
    """eigen_trainer_loss_grad_flow_iter / _target called directly: one reset, teacher-forced call with per-frame frame gradients
    -> (rc, loss, terms, frame gradient)"""
    import torch
    from evolutionary_illusion_generator_amd.engine import DenseSolveC, _ptr
    B, T, C, h, w = frames.shape
    per = C * h * w
    d = torch.from_numpy(frames).to(cuda)
    by = lambda x: None if x is None else ctypes.byref(x)
    d_dir, d_mask, cfg, sc, mem, by_circles = None, None, None, None, None, False
    if flow is not None:
        d_dir, d_mask = flow.on_device(torch, tr.device, h, w)
        cfg = flow.settings()
        sc = flow.score.settings(h) if flow.score is not None else None
        by_circles = isinstance(flow.score, train.FlowScore)
        mem = flow.members_settings(B, h, w) if flow.score is not None else None
    loss, terms = ctypes.c_double(), np.zeros(T - 1, np.float64)
    buf = torch.zeros((B, T, C, h, w), dtype=torch.float32, device=cuda)
    s = None if solve is None else DenseSolveC(*solve)
    fn = getattr(tr.lib, "eigen_trainer_loss_grad_flow_" + entry)
    rc = fn(tr._h, _ptr(d), ctypes.c_int64(T * per), ctypes.c_int32(B), ctypes.c_int32(T), ctypes.c_int32(T), ctypes.c_int32(0), ctypes.c_int32(1), None,
            ctypes.c_int32(objective), None, ctypes.byref(loss), None, None, _ptr(buf), ctypes.c_int64(T * per), ctypes.c_int64(per), by(cfg), _ptr(d_dir), _ptr(d_mask),
            _ptr(terms), ctypes.c_int32(train.FLOW_PAIRINGS[flow.pairing] if flow is not None else 0), by(sc if by_circles else None), by(None if by_circles else sc),
            by(mem), None, None, by(s), *tail)
    return rc, loss.value, terms, buf.cpu().numpy()


def _null_tail(n):
    """a NULL target and strides that would be refused with one: they are not read"""
    return (None,) + (ctypes.c_int64(0),) * n


def test_a_null_target_is_the_iter_entry_bit_for_bit(cuda):
    """20 x 15 colour: `eigen_trainer_flow_term_target` with d_target NULL returns the bytes of `eigen_trainer_flow_term_iter` under the
    energy mode, a direction field and the Circles score, with a byte and a float reference, without a solve and under 2 x 2; 16 x 12:
    `eigen_trainer_loss_grad_flow_target` likewise returns the loss, terms, frame gradient and weight gradients of
    `eigen_trainer_loss_grad_flow_iter` under both pairings and the moving reference; a handle that saw no real solve holds no workspace."""
    name = "20x15"
    img0, img1, _ = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    pred, prev = fi.as_floats(img1), fi.as_floats(img0)
    flows = [FlowObjective(3, ft.EPS), FlowObjective(3, ft.EPS, train.flow_direction("horizontal", w, h), ft.stage_mask(w, h)),
             FlowObjective(3, ft.EPS, score=train.FlowScore(min_count=4, **fi.SCORE_LIMITS))]
    with _trainer(name) as tr:
        for solve in (None, (2, 2)):
            for flow in flows:
                for ref in (img0, prev):
                    want = _raw_term(tr, cuda, "iter", pred, ref, flow, solve)
                    got = _raw_term(tr, cuda, "target", pred, ref, flow, solve, _null_tail(1))
                    assert want[0] == got[0] == 0 and want[1] == got[1], tr.lib.eigen_last_error()
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(want[2:], got[2:])) and np.abs(got[3]).max() > 0
            if solve is None:
                assert tr.debug_flow_iter() == 0
    frames, _, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    sha = lambda g: b"".join(np.ascontiguousarray(g[k]).tobytes() for k in sorted(g))
    with PredNetTrainer(wts, list(ch), w, h, ft.TRAIN_B, ft.TRAIN_T) as tr:
        for flow in (FlowObjective(3, ft.EPS), PredictionFlow(3, ft.EPS), FlowObjective(3, ft.EPS, reference="moving")):
            for solve in (None, (2, 2)):
                want = _raw_loss_grad(tr, cuda, "iter", frames, flow, solve)
                want_g = sha(tr.grads())
                got = _raw_loss_grad(tr, cuda, "target", frames, flow, solve, tail=_null_tail(2))
                assert want[0] == got[0] == 0 and want[1] == got[1] != 0, tr.lib.eigen_last_error()
                assert want[2].tobytes() == got[2].tobytes() and want[3].tobytes() == got[3].tobytes() and sha(tr.grads()) == want_g


def test_refusals_return_invalid_and_leave_the_handle_working(cuda):
    """every refusal of the two entries is EIGEN_ERR_INVALID (-1) before any launch or allocation: a target with a score, a structure
    score, members or a direction field; t_bstride below 2 H W; t_tstride below 2 H W with more than one term (and accepted with one);
    a target under another objective.  The outputs are untouched, no workspace is made, and the handle then runs a target call."""
    import torch
    from evolutionary_illusion_generator_amd.engine import _ptr
    name = "20x15"
    img0, img1, truth = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    pred = fi.as_floats(img1)
    d_t = torch.from_numpy(np.array(truth)).to(cuda)
    field = 2 * h * w
    tail = lambda b=field: (_ptr(d_t), ctypes.c_int64(b))
    score = train.FlowScore(min_count=4, **fi.SCORE_LIMITS)
    carrying = [FlowObjective(3, ft.EPS, train.flow_direction("horizontal", w, h)), FlowObjective(3, ft.EPS, score=score),
                FlowObjective(3, ft.EPS, score=train.BandsScore(min_count=4, **fi.SCORE_LIMITS)),
                FlowObjective(3, ft.EPS, score=score, members=train.CornerMembers()),
                FlowObjective(3, ft.EPS, score=score, mask=np.ones((len(img0), h, w), np.uint8))]
    with _trainer(name) as tr:
        for solve in (None, (2, 2)):
            for flow in carrying:
                got = _raw_term(tr, cuda, "target", pred, img0, flow, solve, tail())
                assert got[0] == -1 and not got[2].any() and not got[3].any(), (got[0], tr.lib.eigen_last_error())
            got = _raw_term(tr, cuda, "target", pred, img0, FlowObjective(3, ft.EPS), solve, tail(field - 1))
            assert got[0] == -1 and b"t_bstride" in tr.lib.eigen_last_error() and not got[2].any()
        assert tr.debug_flow_iter() == 0
        value, u, seed = tr.flow_term(pred, img0, FlowObjective(3, ft.EPS).solved(2, 2), target=truth)
        assert value > 0 and np.abs(seed).max() > 0
    frames, flow_truth, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = ft.TRAIN_B, ft.TRAIN_T
    field = 2 * h * w
    d_t = torch.from_numpy(flow_truth).to(cuda)
    tail = lambda b=(T - 1) * field, t=field: (_ptr(d_t), ctypes.c_int64(b), ctypes.c_int64(t))
    score = train.FlowScore(min_count=4, max_norm=8.0)
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        before = tr.grads()
        refused = [(FlowObjective(3, ft.EPS, train.flow_direction("horizontal", w, h)), 2, tail()), (FlowObjective(3, ft.EPS, score=score), 2, tail()),
                   (PredictionFlow(3, ft.EPS).scored(train.FreeScore(min_count=4, max_norm=8.0)), 2, tail()),
                   (FlowObjective(3, ft.EPS, score=score, members=train.CornerMembers()), 2, tail()),
                   (FlowObjective(3, ft.EPS), 2, tail(b=field - 1)), (FlowObjective(3, ft.EPS), 2, tail(t=field - 1)), (PredictionFlow(3, ft.EPS), 2, tail(t=0)),
                   (None, 0, tail()), (None, 1, tail())]
        for flow, objective, tl in refused:
            for solve in (None, (2, 2)) if flow is not None else (None,):
                got = _raw_loss_grad(tr, cuda, "target", frames, flow, solve, objective, tl)
                assert got[0] == -1 and not got[3].any() and not got[2].any(), (got[0], objective, tr.lib.eigen_last_error())
        assert tr.debug_flow_iter() == 0
        after = tr.grads()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        # two steps have one term: its t_tstride is not read
        got = _raw_loss_grad(tr, cuda, "target", np.ascontiguousarray(frames[:, :2]), FlowObjective(3, ft.EPS), None, 2, tail(t=0))
        assert got[0] == 0 and got[1] > 0, tr.lib.eigen_last_error()
        loss = tr.forward_backward(frames, objective="flow", flow=PredictionFlow(3, ft.EPS), flow_target=flow_truth)
        assert np.isfinite(loss) and loss > 0
        for kw in (dict(objective="mse", flow_target=flow_truth), dict(objective="flow", flow=FlowObjective(3, ft.EPS, score=score), flow_target=flow_truth),
                   dict(objective="flow", flow=FlowObjective(3, ft.EPS), flow_target=flow_truth[:, :2]),
                   dict(objective="flow", flow=FlowObjective(3, ft.EPS), flow_target=flow_truth.astype(np.float32))):
            with pytest.raises(ValueError):
                tr.forward_backward(frames, **kw)


# ---- the training call
def _train_call(tr, pairing, reference, frames, target, **kw):
    return tr.forward_backward(frames, n_fed=ft.TRAIN_FED, requant=False, objective="flow", flow=ft.train_objective(pairing, reference), flow_target=target, **kw)


@pytest.mark.parametrize("pairing,reference", ft.TRAIN_FORMS, ids=["%s-%s" % f for f in ft.TRAIN_FORMS])
def test_a_training_call_matches_float64_autograd_under_the_target(cuda, pairing, reference):
    """[1, 8, 16] at 16 x 12, B = 2, T = 4, two fed and two self-fed steps, the video's exact flow as the target: loss and terms within
    1e-5 of their scale, every weight gradient within `_check_grads` and the per-frame gradient within `check_frame_grads` of
    `run_flow` under `TargetTerm`, both unchanged; against the same reference with a zero target the loss, the terms and the weight
    gradients all fail those checks.  A strided device view of the target gives the same bytes."""
    import torch
    frames, flow, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        loss, pred, per, terms = _train_call(tr, pairing, reference, frames, flow, pred=True, frame_grads="frames", flow_terms=True)
        grads = tr.grads()
        wide = torch.zeros((2 * B, 2 * T, 2, h, w), dtype=torch.float64, device=cuda)
        view = wide[::2, 1:T]
        view.copy_(torch.from_numpy(flow))
        again = _train_call(tr, pairing, reference, torch.from_numpy(frames).to(cuda), view, frame_grads="frames", flow_terms=True)
        assert again[0] == loss and again[1].tobytes() == per.tobytes() and again[2].tobytes() == terms.tobytes()
        assert all(np.array_equal(grads[k], v) for k, v in tr.grads().items())
    r, z = ft.train_reference(pairing, reference), ft.train_reference(pairing, reference, "zero")
    what = "target %s %s" % (pairing, reference)
    assert np.abs(pred - r.pred).max() <= 1e-5
    print("%s: loss %.9g against %.9g (zero target: %.9g), terms %s against %s" % (what, loss, r.loss, z.loss, terms, r.terms))
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss, r.scale)
    assert (np.abs(terms - r.terms) <= 1e-5 * r.term_scales).all(), (terms, r.terms)
    norm, element = _check_grads(grads, r.grads, what=what)
    ratio = check_frame_grads(per, r.frame_grad, what, zero=set() if reference == "moving" else set(range(ft.TRAIN_FED, T)))
    print("%s: error / bound norm %.4f element %.4f frames %.4f" % (what, norm, element, ratio))
    # liveness: the plain mean squared displacement's reference is outside every one of these checks
    assert abs(loss - z.loss) > 1e-5 * z.scale and (np.abs(terms - z.terms) > 1e-5 * z.term_scales).all()
    assert _grads_differ(z.grads, grads), "the gradient is the mean squared displacement's"


def test_micro_batches_slice_the_target_with_the_frames(cuda):
    """`step(micro_batches=2)` on a handle of batch 1 under the prediction pairing and the target: the accumulated gradient is held to the
    float64 reference of the batch of 2 by `_check_grads`, the loss to 1e-5 of its scale, as tests/test_gpu_optim.py asks of the other
    objectives; two runs give the same weight bytes, which are those of the steps taken by hand; the chunks read their own slice of
    the target (a target whose samples are swapped fails the check).  How far the weights are from the single call's on a handle of
    batch 2 is printed."""
    frames, flow, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    kw = dict(n_fed=ft.TRAIN_FED, objective="flow", flow=ft.train_objective("prediction", "constant"))
    r = ft.train_reference("prediction", "constant")
    with PredNetTrainer(wts, list(ch), w, h, 1, T) as tr:
        loss = tr.accumulate_micro_batches(frames, 2, flow_target=flow, **kw)
        tr.load_accumulated()
        got = tr.grads()
        tr.adam()
        by_hand = tr.weights()
        tr.accumulate_micro_batches(frames, 2, flow_target=np.ascontiguousarray(flow[::-1]), **kw)
        tr.load_accumulated()
        swapped = tr.grads()
    worst = _check_grads(got, r.grads, what="target micro_batches=2")
    assert abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss)
    assert _grads_differ(r.grads, swapped), "the chunks do not read their own slice of the target"
    runs = []
    for _ in range(2):
        with PredNetTrainer(wts, list(ch), w, h, 1, T) as tr:
            assert tr.step(frames, micro_batches=2, flow_target=flow, **kw) == loss
            runs.append(tr.weights())
    with PredNetTrainer(wts, list(ch), w, h, 2, T) as tr:
        whole_loss = tr.step(frames, flow_target=flow, **kw)
        whole = tr.weights()
    for k in wts:
        assert runs[0][k].tobytes() == runs[1][k].tobytes() == by_hand[k].tobytes(), k
    assert any(not np.array_equal(runs[0][k], wts[k]) for k in wts)
    # the same comparison under "mse": what the accumulator's own float32 additions do to any objective
    with PredNetTrainer(wts, list(ch), w, h, 1, T) as tr:
        tr.step(frames, micro_batches=2)
        mse_micro = tr.weights()
    with PredNetTrainer(wts, list(ch), w, h, 2, T) as tr:
        tr.step(frames)
        mse_whole = tr.weights()
    print("under mse the weights of micro_batches=2 %s the single call's" % ("are" if all(mse_micro[k].tobytes() == mse_whole[k].tobytes() for k in wts) else "are not"))
    apart = max(float(np.abs(runs[0][k].astype(np.float64) - whole[k]).max()) for k in wts)
    same = all(runs[0][k].tobytes() == whole[k].tobytes() for k in wts)
    print("micro_batches=2: gradient error / bound %.4f in norm, %.4f element-wise; loss %.17g, the single call's %.17g; weights %s the single call's (max apart %.3e)"
          % (worst[0], worst[1], loss, whole_loss, "are" if same else "are not", apart))
    assert abs(whole_loss - r.loss) <= 1e-5 * r.scale


def test_the_truth_halves_the_term_on_frames_from_the_device_source(cuda):
    """The 16 x 12 exact binary shift (0.25, -0.125) rendered by the moving-texture kernel itself, radius 3, eps 1e-4, the pixels at least
    3 from the border: `flow_epe` against the rendered flow (a device tensor) is below half of `flow_epe` against zeros, on both frame
    pairs, and is the value tests/test_flow_target_host.py holds to the same condition on the restatement."""
    import torch
    from evolutionary_illusion_generator_amd.engine import Engine
    from tests import flow_obj_support as fs
    from tests import moving_support as ms
    name, b = ms.SHIFT_SAMPLE
    c = ms.case(name)
    eng = Engine(c["w"], c["h"], [c["c_dim"]], 1)
    try:
        frames, flow, _ = eng.render_moving_cppn(c["gb"], c["affine"], c["affine_inv"], flow=True, layer=True)
        torch.cuda.synchronize()
    finally:
        eng.close()
    host_frames, host_flow, mask = ft.truth_case()
    assert np.array_equal(frames[b:b + 1].cpu().numpy(), host_frames) and np.array_equal(flow[b:b + 1].cpu().numpy(), host_flow)
    obj = FlowObjective(ft.TRUTH_RADIUS, ft.TRUTH_EPS, mask=mask)
    with PredNetTrainer("synthetic", [c["c_dim"]], c["w"], c["h"], 1, 2) as tr:
        for t in range(c["T"] - 1):
            pred = fi.as_floats(frames[b:b + 1, t + 1].cpu().numpy())      # (float)byte / 255.0f, as the host case forms it
            truth = train.flow_epe(tr, pred, frames[b:b + 1, t], obj, flow[b:b + 1, t])
            zero = train.flow_epe(tr, pred, frames[b:b + 1, t], obj, torch.zeros_like(flow[b:b + 1, t]))
            want = ft.target_stage_ref(fi.as_floats(host_frames[:, t + 1]), fs.byte_reference(host_frames[:, t]), ft.TRUTH_RADIUS, ft.TRUTH_EPS, host_flow[:, t], mask)
            print("pair %d: term against the truth %.6f, against zeros %.6f, ratio %.4f" % (t, truth, zero, truth / zero))
            assert truth == want.value and zero > 0 and truth < 0.5 * zero, (t, truth, zero, want.value)


def test_twenty_adam_steps_repeat_bit_for_bit(cuda):
    """two runs of 20 Adam steps under the prediction pairing and the target from one seed give identical weight bytes, and the weights
    have moved"""
    frames, flow, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    runs = []
    for _ in range(2):
        with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
            losses = [tr.step(frames, n_fed=ft.TRAIN_FED, objective="flow", flow=ft.train_objective("prediction", "constant"), flow_target=flow) for _ in range(20)]
            runs.append((losses, tr.weights()))
    assert runs[0][0] == runs[1][0] and np.isfinite(runs[0][0]).all()
    for k in wts:
        assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k
    assert any(not np.array_equal(runs[0][1][k], wts[k]) for k in wts)
    print("20 Adam steps under the target: loss %.6f -> %.6f" % (runs[0][0][0], runs[0][0][-1]))


# held-out mean squared endpoint error between consecutive predictions before -> after 200 Adam steps under the target, as
# scripts/flow_target_train.py printed them on an MI355X (profiles/flow_target_train.txt); the assertion asks for half of the measured
# reduction, the margin of tests/test_gpu_moving.py::test_adam_steps_on_moving_textures_cut_the_held_out_loss.  Under "mse" the same
# metric rose, 0.939249 -> 1.080614.
MEASURED_TARGET_TRAINING = (0.939249, 0.812742)      # 13.5 % lower: 6.7 % is asked for


def test_adam_steps_under_the_target_cut_the_held_out_endpoint_error(cuda):
    """The setup of scripts/flow_target_train.py: 32 x 24 gray, [1, 8, 16], B = 4, T = 6 (3 fed + 3 self-fed), 200 Adam steps at alpha 3e-3
    under a PredictionFlow (radius 3) with the video's exact flow as the target, the terms 1 .. 4 weighted; one-layer textures, held-out
    batch 10**6, `train.flow_epe` on the tape-free predictions."""
    from evolutionary_illusion_generator_amd.train import MovingTextures
    from examples.train_prednet import held_out_epe
    w, h, ch = 32, 24, [1, 8, 16]
    B, T, fed = 4, 6, 3
    flow = PredictionFlow(3, 1e-2)
    with MovingTextures(w, h, 1, T, seed=0, layers=1) as src, PredNetTrainer("synthetic:0", ch, w, h, B, T, alpha=3e-3) as tr:
        held, truth, _ = src.batch(10 ** 6, B, flow=True)
        before = held_out_epe(tr, held, truth, 3, 1e-2, fed, False).mean()
        for k in range(200):
            frames, fl, _ = src.batch(k, B, flow=True)
            tr.step(frames, n_fed=fed, step_weights=[0.0, 1.0, 1.0, 1.0, 1.0], objective="flow", flow=flow, flow_target=fl)
        after = held_out_epe(tr, held, truth, 3, 1e-2, fed, False).mean()
    print("held-out squared endpoint error %.6f -> %.6f (%.1f %% lower)" % (before, after, 100 * (1 - after / before)))
    m_before, m_after = MEASURED_TARGET_TRAINING
    assert after < before, (before, after)
    assert after <= (1 - 0.5 * (1 - m_after / m_before)) * before, (before, after)
