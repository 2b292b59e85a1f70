"""The joint objective and the valid pixels on the GPU (eigen_moving_cppn_valid, eigen_trainer_flow_term_valid,
eigen_trainer_loss_grad_flow_joint; ``Engine.moving_cppn_valid``, ``MovingTextures.batch(valid=True)``, ``flow_term_valid``,
``forward_backward(frame_weight=, flow_valid=)``; DESIGN.md section 13, "The joint objective and the valid pixels").  The validity planes,
the field and the value are compared bit for bit with the numpy restatements of tests/flow_joint_support.py; the seed and the reference
gradient, float32 out of float64 arithmetic, tensor by tensor with their float64 autograd statement under the bound of
tests/test_gpu_flow_target.py, max |got - ref| <= 2^-23 max |ref|; a training call meets `flow_obj_support.run_flow` under `JointTerm`
by the unchanged gradient rules."""
import ctypes

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.engine import Engine
from evolutionary_illusion_generator_amd.train import FlowJointSettings, FlowObjective, MovingTextures, PredictionFlow, PredNetTrainer
from tests import flow_iter_support as fi
from tests import flow_joint_support as fj
from tests import flow_target_support as ft
from tests.frame_grad_support import check_frame_grads
from tests.test_flow_joint_host import KIND_FORMS
from tests.test_gpu_flow_target import _raw_loss_grad, _raw_term, _trainer
from tests.train_support import _check_grads, _grads_differ

pytestmark = pytest.mark.gpu

SCALE = 0.75
INVALID, CAPACITY = -1, -4


# ---- the validity planes
@pytest.mark.parametrize("name", fj.VALID_CASES)
def test_validity_planes_are_the_restatement_bit_for_bit(cuda, name):
    import torch
    c = fj.valid_case(name)
    e = Engine(c["w"], c["h"], [c["c_dim"]], 1)
    try:
        got = e.moving_cppn_valid(c["affine"], c["affine_inv"])
        torch.cuda.synchronize()
        want = fj.valid_ref(c)[0]
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (name, int((got.cpu().numpy() != want).sum()))
        # a sample's planes do not depend on the call they are in
        if c["n"] > 1:
            last = e.moving_cppn_valid(c["affine"][1:], c["affine_inv"][1:])
            assert np.array_equal(last.cpu().numpy(), want[1:])
    finally:
        e.close()


def test_the_validity_entry_refuses_and_the_handle_works_afterwards(cuda):
    import torch
    c = fj.valid_case("live")
    n, T, L, h, w = c["n"], c["T"], c["L"], c["h"], c["w"]
    A, I = np.ascontiguousarray(c["affine"]), np.ascontiguousarray(c["affine_inv"])
    out = torch.full((n, T - 1, h, w), 9, dtype=torch.uint8, device=cuda)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
    e = Engine(w, h, [1], 1)
    try:
        call = lambda handle=True, n=n, T=T, L=L, a=A, i=I, o=out: e.lib.eigen_moving_cppn_valid(e._h if handle else None, ctypes.c_int32(n), ctypes.c_int32(T), ctypes.c_int32(L),
                                                                                                   p(a), p(i), p(o), None)
        for kw in (dict(handle=False), dict(a=None), dict(i=None), dict(o=None), dict(L=0), dict(L=3), dict(T=1), dict(T=0), dict(n=0), dict(n=-1)):
            assert call(**kw) == INVALID, (kw, e.lib.eigen_last_error())
        assert call(n=65536) == CAPACITY
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 9).all()
        assert call() == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), fj.valid_ref(c)[0])
    finally:
        e.close()


def test_a_batch_without_valid_is_what_it_was_and_valid_adds_the_planes(cuda):
    """two-layer textures: `batch(k, n, flow=True)` returns three tensors, the bytes the render entry gives for the described samples;
    `valid=True` appends the planes of the restatement and leaves the three as they are; `batch(k, n)` is the frames alone"""
    import torch
    with MovingTextures(16, 12, 1, 3, seed=3, layers=2) as src:
        d = src.describe(5, 2)
        three = src.batch(5, 2, flow=True)
        four = src.batch(5, 2, flow=True, valid=True)
        alone = src.batch(5, 2)
        direct = src.engine.render_moving_cppn(d["gb"], d["affine"], d["affine_inv"], flow=True, layer=True)
        torch.cuda.synchronize()
        assert isinstance(three, tuple) and len(three) == 3 and len(four) == 4 and isinstance(alone, torch.Tensor)
        for a, b, c in zip(three, four, direct):
            assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
        assert np.array_equal(alone.cpu().numpy(), three[0].cpu().numpy())
        want = fj.valid_ref(d)[0]
        assert four[3].dtype == torch.uint8 and np.array_equal(four[3].cpu().numpy(), want) and 0 < want.mean() < 1


# ---- the stage alone
WORST = {"stage": 0.0}


def _check_tensor(got, ref64, what):
    """the bound of tests/test_gpu_flow_target.py: `flow_iter_support.within`, 2^-23 of the tensor's maximum"""
    err, bound = fi.within(got, ref64)
    assert bound > 0, what
    WORST["stage"] = max(WORST["stage"], err / bound)
    print("%s: max |got - ref| %.3e, bound %.3e (ratio %.3f, worst so far %.3f)" % (what, err, bound, err / bound, WORST["stage"]))
    assert err <= bound, (what, err, bound)


def _valid_calls(tr, name, r, solve, mask, valid):
    """the stage under both pairings: `flow_term_valid` on the byte reference and `flow_term_pair_valid` on the same bytes as floats"""
    img0, img1, truth = ft.stage_inputs(name)
    pred, prev = fi.as_floats(img1), fi.as_floats(img0)
    flow = FlowObjective(r, ft.EPS, mask=mask).solved(*solve)
    return (tr.flow_term_valid(pred, img0, flow, truth, valid, scale=SCALE, reference_grad=True),
            tr.flow_term_pair_valid(pred, prev, flow, truth, valid, scale=SCALE, reference_grad=True))


@pytest.mark.parametrize("case", fj.STAGE_CASES, ids=ft.stage_case_id)
def test_the_stage_alone_meets_the_restatement_and_the_autograd_statement(cuda, case):
    """Per shape, radius and solve, with and without the shared mask, a byte and a float reference, under planes that differ per sample
    and cut windows, rows and tiles: the field and the value are the numpy restatement's bit for bit (the value is the fixed-order sum of
    mv, so mv is); the seed and the reference gradient are within 2^-23 of their tensor's maximum of float64 autograd; the same
    statement without the planes misses that bound; all-ones planes return the bytes of `flow_term(target=)`; a sample with an all-zero
    plane gives a finite value, exact zeros in its seed and leaves the other sample's seed as it was."""
    import torch
    name, r, solve = case
    img0, img1, truth = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    valid = fj.stage_valid(w, h)
    pred = fi.as_floats(img1)
    with _trainer(name) as tr:
        for masked in (False, True):
            (rest, field), stmt = fj.stage_reference(name, r, solve, masked)
            mask = ft.stage_mask(w, h) if masked else None
            by_frame, by_pair = _valid_calls(tr, name, r, solve, mask, valid)
            what = "%s %s" % (ft.stage_case_id(case), "masked" if masked else "whole")
            assert by_frame[0] == by_pair[0] and all(x.tobytes() == y.tobytes() for x, y in zip(by_frame[1:], by_pair[1:])), what
            value, u, seed, rg = by_frame
            assert np.array_equal(u, field), (what, np.abs(u - field).max())
            print("%s: value %.17g, restatement %.17g" % (what, value, rest.value))
            assert value == rest.value, (what, value, rest.value)
            assert seed.dtype == np.float32 and rg.dtype == np.float32
            _check_tensor(seed, SCALE * stmt.seed64, what + " seed")
            _check_tensor(rg, SCALE * stmt.ref64, what + " reference gradient")
            # liveness: the statement without the planes is outside the bound
            # (but at 8 x 8 under radius 7: every window is the whole image and the shift is uniform, so the error is one vector, every sample's
            # r_b c_b is N_m and the seed does not depend on which pixels carry it; the two float64 statements themselves agree there)
            _, without = ft.stage_reference(name, r, solve, masked)
            apart = fi.within(stmt.seed64, without.seed64, 10 * fi.BOUND)
            assert apart[0] > apart[1] or (name, r) == ("8x8", 7), (what, apart)
            if apart[0] > apart[1]:
                err, bound = fi.within(seed, SCALE * without.seed64)
                assert err > bound and value != without.value, (what, err, bound)
            # all-ones planes, as bytes on the host and as bools on the device: the call without planes, bit for bit
            flow = FlowObjective(r, ft.EPS, mask=mask).solved(*solve)
            plain = tr.flow_term(pred, img0, flow, scale=SCALE, reference_grad=True, target=truth)
            for ones in (np.ones_like(valid), torch.ones(valid.shape, dtype=torch.bool, device=cuda)):
                got = tr.flow_term_valid(pred, img0, flow, truth, ones, scale=SCALE, reference_grad=True)
                assert got[0] == plain[0] and all(x.tobytes() == y.tobytes() for x, y in zip(got[1:], plain[1:])), what
            # a sample without a valid pixel
            gone = tr.flow_term_valid(pred, img0, flow, truth, np.stack([valid[0], np.zeros_like(valid[1])]), scale=SCALE, reference_grad=True)
            assert np.isfinite(gone[0]) and gone[0] > 0 and not gone[2][1].any() and not gone[3][1].any(), what
            assert gone[2][0].tobytes() == seed[0].tobytes() and gone[3][0].tobytes() == rg[0].tobytes() and np.abs(seed[0]).max() > 0, what
            assert train.flow_epe(tr, pred, img0, flow, truth, valid) == tr.flow_term_valid(pred, img0, flow, truth, valid)[0]


def test_the_stage_entry_refuses_and_a_null_plane_is_the_target_entry(cuda):
    """20 x 15: planes without a target and a v_bstride below H W are EIGEN_ERR_INVALID before any launch, under either solve, the outputs
    untouched; d_valid NULL returns the bytes of eigen_trainer_flow_term_target; a stride between the planes above H W is read"""
    import torch
    from evolutionary_illusion_generator_amd.engine import _ptr
    name = "20x15"
    img0, img1, truth = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    pred = fi.as_floats(img1)
    valid = fj.stage_valid(w, h)
    d_t, d_v = torch.from_numpy(np.array(truth)).to(cuda), torch.from_numpy(np.array(valid)).to(cuda)
    wide = torch.zeros((2, 2, h, w), dtype=torch.uint8, device=cuda)
    wide[:, 0].copy_(d_v)
    field, plane = 2 * h * w, h * w
    flow = FlowObjective(3, ft.EPS)
    with _trainer(name) as tr:
        for solve in (None, (2, 2)):
            got = _raw_term(tr, cuda, "valid", pred, img0, flow, solve, (None, ctypes.c_int64(0), _ptr(d_v), ctypes.c_int64(plane)))
            assert got[0] == INVALID and b"target" in tr.lib.eigen_last_error() and not got[2].any() and not got[3].any()
            got = _raw_term(tr, cuda, "valid", pred, img0, flow, solve, (_ptr(d_t), ctypes.c_int64(field), _ptr(d_v), ctypes.c_int64(plane - 1)))
            assert got[0] == INVALID and b"v_bstride" in tr.lib.eigen_last_error() and not got[2].any() and not got[3].any()
            want = _raw_term(tr, cuda, "target", pred, img0, flow, solve, (_ptr(d_t), ctypes.c_int64(field)))
            null = _raw_term(tr, cuda, "valid", pred, img0, flow, solve, (_ptr(d_t), ctypes.c_int64(field), None, ctypes.c_int64(0)))
            assert want[0] == null[0] == 0 and want[1] == null[1] and all(x.tobytes() == y.tobytes() for x, y in zip(want[2:], null[2:]))
            near = _raw_term(tr, cuda, "valid", pred, img0, flow, solve, (_ptr(d_t), ctypes.c_int64(field), _ptr(d_v), ctypes.c_int64(plane)))
            far = _raw_term(tr, cuda, "valid", pred, img0, flow, solve, (_ptr(d_t), ctypes.c_int64(field), _ptr(wide), ctypes.c_int64(2 * plane)))
            assert near[0] == far[0] == 0 and near[1] == far[1] != want[1] and all(x.tobytes() == y.tobytes() for x, y in zip(near[2:], far[2:]))
        value = tr.flow_term_valid(pred, img0, flow.solved(2, 2), truth, valid)[0]
        assert value > 0


# ---- the training call
def _call(tr, frames, kind, pairing, reference, solve, **extra):
    return tr.forward_backward(frames, n_fed=ft.TRAIN_FED, requant=False, objective="flow", flow=fj.train_flow(kind, pairing, reference, solve),
                               **fj.train_kwargs(kind, len(frames)), **extra)


@pytest.mark.parametrize("kind,pairing,reference,solve", KIND_FORMS, ids=["%s-%s-%s-%dx%d" % (k, p, r, s[0], s[1]) for k, p, r, s in KIND_FORMS])
def test_a_joint_training_call_matches_float64_autograd(cuda, kind, pairing, reference, solve):
    """[1, 8, 16] at 16 x 12, B = 2, T = 4, two fed and two self-fed steps; joint with a target, with a target and the renderer's validity
    planes, with the plain displacement term and with a FlowScore; the single step under the three forms, the 2 x 2 solve under the
    prediction pairing.  Loss within 1e-5 of its scale, every weight gradient within `_check_grads` and the per-frame gradient within
    `check_frame_grads` of `run_flow` under `JointTerm` (the flow term plus mu mean((P - x)^2), x in the graph), both unchanged; the
    same reference at mu = 0 fails them.  `last_loss_parts` are the losses of the call without frame_weight and of the "mse" call, bit for
    bit; the loss is fl(parts[0] + fl(mu parts[1])); the terms are the flow-only call's bytes."""
    frames, _, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    mu = fj.train_mu(kind, pairing, reference, solve)
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        assert tr.last_loss_parts is None
        loss, pred, per, terms = _call(tr, frames, kind, pairing, reference, solve, frame_weight=mu, pred=True, frame_grads="frames", flow_terms=True)
        grads, parts = tr.grads(), tr.last_loss_parts
        flow_loss, flow_terms = _call(tr, frames, kind, pairing, reference, solve, flow_terms=True)
        mse_loss = tr.forward_backward(frames, n_fed=ft.TRAIN_FED, requant=False)
        assert tr.last_loss_parts == parts        # other calls leave it alone
        # the same under step weights: the other squared-error reduction
        sw = [0.0, 1.0, 2.0]
        weighted = _call(tr, frames, kind, pairing, reference, solve, frame_weight=mu, step_weights=sw)
        w_parts = tr.last_loss_parts
        w_flow = _call(tr, frames, kind, pairing, reference, solve, step_weights=sw)
        w_mse = tr.forward_backward(frames, n_fed=ft.TRAIN_FED, requant=False, step_weights=sw)
    what = "joint %s %s %s %dx%d mu %g" % (kind, pairing, reference, solve[0], solve[1], mu)
    assert parts == (flow_loss, mse_loss) and terms.tobytes() == flow_terms.tobytes(), (what, parts, flow_loss, mse_loss)
    assert loss == parts[0] + mu * parts[1] and parts[0] != 0 and parts[1] > 0, (what, loss, parts)
    assert w_parts == (w_flow, w_mse) and weighted == w_parts[0] + mu * w_parts[1] and w_mse != mse_loss, (what, w_parts, w_flow, w_mse)
    r, z = fj.train_reference(kind, pairing, reference, solve), fj.train_reference(kind, pairing, reference, solve, 0.0)
    assert np.abs(pred - r.pred).max() <= 1e-5
    print("%s: loss %.9g against %.9g (mu = 0: %.9g), parts %s" % (what, loss, r.loss, z.loss, parts))
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale, (what, loss, r.loss, r.scale)
    norm, element = _check_grads(grads, r.grads, what=what)
    ratio = check_frame_grads(per, r.frame_grad, what)
    print("%s: error / bound norm %.4f element %.4f frames %.4f" % (what, norm, element, ratio))
    # liveness: the flow objective alone is outside every one of these checks
    assert abs(loss - z.loss) > 1e-5 * z.scale and _grads_differ(z.grads, grads), what
    with pytest.raises(AssertionError):
        check_frame_grads(per, z.frame_grad, what, zero=set(range(T)))


def _joint_tail(d_target, t_b, t_t, rec):
    from evolutionary_illusion_generator_amd.engine import _ptr
    return (_ptr(d_target), ctypes.c_int64(t_b), ctypes.c_int64(t_t), None if rec is None else ctypes.byref(rec))


def test_a_null_record_is_the_target_entry_and_a_strided_plane_view_reads_the_same_bytes(cuda):
    """16 x 12: `eigen_trainer_loss_grad_flow_joint` with joint NULL, and with a record that asks for nothing, returns the loss, terms,
    frame gradient and weight gradients of `eigen_trainer_loss_grad_flow_target`, with and without a target, under both pairings, the moving
    reference and both solves; a strided device view of flow_valid gives the bytes of a contiguous one"""
    import torch
    frames, flow_truth, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    field = 2 * h * w
    d_t = torch.from_numpy(flow_truth).to(cuda)
    sha = lambda g: b"".join(np.ascontiguousarray(g[k]).tobytes() for k in sorted(g))
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        for flow in (FlowObjective(3, ft.EPS), PredictionFlow(3, ft.EPS), FlowObjective(3, ft.EPS, reference="moving")):
            for solve in (None, (2, 2)):
                for target in ((d_t, (T - 1) * field, field), (None, 0, 0)):
                    want = _raw_loss_grad(tr, cuda, "target", frames, flow, solve, tail=_joint_tail(*target, None)[:3])
                    want_g = sha(tr.grads())
                    for rec in (None, FlowJointSettings(0.0, None, 0, 0, None)):
                        got = _raw_loss_grad(tr, cuda, "joint", frames, flow, solve, tail=_joint_tail(*target, rec))
                        assert want[0] == got[0] == 0 and want[1] == got[1] != 0, tr.lib.eigen_last_error()
                        assert want[2].tobytes() == got[2].tobytes() and want[3].tobytes() == got[3].tobytes() and sha(tr.grads()) == want_g
        valid = fj.train_valid()
        kw = dict(n_fed=ft.TRAIN_FED, requant=False, objective="flow", flow=PredictionFlow(3, ft.EPS), flow_target=flow_truth, frame_weight=2.0, frame_grads="frames",
                  flow_terms=True)
        near = tr.forward_backward(frames, flow_valid=valid, **kw)
        near_g = sha(tr.grads())
        wide = torch.zeros((2 * B, 2 * T, h, w), dtype=torch.uint8, device=cuda)
        view = wide[::2, 1:T]
        view.copy_(torch.from_numpy(valid))
        far = tr.forward_backward(torch.from_numpy(frames).to(cuda), flow_valid=view, **kw)
        assert near[0] == far[0] and near[1].tobytes() == far[1].tobytes() and near[2].tobytes() == far[2].tobytes() and sha(tr.grads()) == near_g
        whole = tr.forward_backward(frames, **kw)
        assert whole[0] != near[0] and whole[2].tobytes() != near[2].tobytes()


def test_refusals_return_invalid_and_leave_the_handle_working(cuda):
    """every refusal of the joint entry is EIGEN_ERR_INVALID (-1) before any launch or allocation: a frame_weight that is negative or not
    finite; a frame_weight under another objective; planes without a target; v_bstride below H W; v_tstride below H W with more than one
    term (and accepted with one).  The outputs and the gradients are untouched, no workspace is made, and the handle then trains."""
    import torch
    from evolutionary_illusion_generator_amd.engine import _ptr
    frames, flow_truth, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    field, plane = 2 * h * w, h * w
    d_t, d_v = torch.from_numpy(flow_truth).to(cuda), torch.from_numpy(fj.train_valid()).to(cuda)
    target, none = (d_t, (T - 1) * field, field), (None, 0, 0)
    rec = lambda mu=0.0, v=None, b=(T - 1) * plane, t=plane: FlowJointSettings(mu, None if v is None else v.data_ptr(), b, t, None)
    flow = FlowObjective(3, ft.EPS)
    with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
        before = tr.grads()
        refused = [(flow, 2, target, rec(-1.0)), (flow, 2, target, rec(float("nan"))), (flow, 2, none, rec(float("inf"))), (flow, 2, none, rec(-0.5)),
                   (None, 0, none, rec(1.0)), (None, 1, none, rec(1.0)),
                   (flow, 2, none, rec(1.0, d_v)), (PredictionFlow(3, ft.EPS), 2, none, rec(0.0, d_v)),
                   (flow, 2, target, rec(1.0, d_v, b=plane - 1)), (flow, 2, target, rec(0.0, d_v, t=plane - 1)), (PredictionFlow(3, ft.EPS), 2, target, rec(1.0, d_v, t=0))]
        for fl, objective, tg, r in refused:
            for solve in (None, (2, 2)) if fl is not None else (None,):
                got = _raw_loss_grad(tr, cuda, "joint", frames, fl, solve, objective, _joint_tail(*tg, r))
                assert got[0] == INVALID and not got[3].any() and not got[2].any() and got[1] == 0.0, (got[0], objective, tr.lib.eigen_last_error())
        assert tr.debug_flow_iter() == 0
        after = tr.grads()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        # two steps have one term: its v_tstride is not read
        two = np.ascontiguousarray(frames[:, :2])
        got = _raw_loss_grad(tr, cuda, "joint", two, flow, None, 2, _joint_tail(d_t, (T - 1) * field, 0, rec(1.0, d_v, t=0)))
        assert got[0] == 0 and got[1] > 0, tr.lib.eigen_last_error()
        loss = tr.forward_backward(frames, objective="flow", flow=PredictionFlow(3, ft.EPS), flow_target=flow_truth, flow_valid=fj.train_valid(), frame_weight=1.0)
        assert np.isfinite(loss) and loss > 0
        valid = fj.train_valid()
        for kw in (dict(objective="mse", frame_weight=1.0), dict(objective="error", frame_weight=1.0), dict(objective="flow", flow=flow, frame_weight=0.0),
                   dict(objective="flow", flow=flow, frame_weight=float("nan")), dict(objective="flow", flow=flow, flow_valid=valid),
                   dict(objective="flow", flow=flow, flow_target=flow_truth, flow_valid=valid[:, :2]),
                   dict(objective="flow", flow=flow, flow_target=flow_truth, flow_valid=valid.astype(np.float32))):
            with pytest.raises(ValueError):
                tr.forward_backward(frames, **kw)


# ---- micro-batches and repeatability, under (b): joint with a target and the renderer's validity planes
def _b_kwargs():
    _, flow, _ = ft.train_inputs()
    return dict(n_fed=ft.TRAIN_FED, objective="flow", flow=ft.train_objective("prediction", "constant"), flow_target=flow, flow_valid=fj.train_valid(),
                frame_weight=fj.train_mu("valid", "prediction", "constant"))


def test_micro_batches_slice_the_planes_with_the_frames(cuda):
    """`step(micro_batches=2)` on a handle of batch 1: the accumulated gradient is held to the float64 reference of the batch of 2 by
    `_check_grads`, the loss to 1e-5 of its scale (every sample's term is its own mean, so the chunks' mean is the batch's); two runs give
    the same weight bytes; the chunks read their own slice of the planes (planes whose samples are swapped fail the check)"""
    frames, flow, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    kw = _b_kwargs()
    r = fj.train_reference("valid", "prediction", "constant")
    with PredNetTrainer(wts, list(ch), w, h, 1, T) as tr:
        loss = tr.accumulate_micro_batches(frames, 2, **kw)
        tr.load_accumulated()
        got = tr.grads()
        swapped_kw = dict(kw, flow_valid=np.ascontiguousarray(kw["flow_valid"][::-1]))
        tr.accumulate_micro_batches(frames, 2, **swapped_kw)
        tr.load_accumulated()
        swapped = tr.grads()
    worst = _check_grads(got, r.grads, what="joint micro_batches=2")
    assert abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss)
    assert _grads_differ(r.grads, swapped), "the chunks do not read their own slice of the planes"
    runs = []
    for _ in range(2):
        with PredNetTrainer(wts, list(ch), w, h, 1, T) as tr:
            assert tr.step(frames, micro_batches=2, **kw) == loss
            runs.append(tr.weights())
    for k in wts:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert any(not np.array_equal(runs[0][k], wts[k]) for k in wts)
    print("joint micro_batches=2: gradient error / bound %.4f in norm, %.4f element-wise; loss %.17g" % (worst[0], worst[1], loss))


def test_ten_adam_steps_repeat_bit_for_bit(cuda):
    """two runs of ten Adam steps from one seed give identical losses, parts and weight bytes, and the weights have moved"""
    frames, flow, wts = ft.train_inputs()
    w, h, ch = ft.TRAIN_SHAPE
    B, T = frames.shape[:2]
    kw = _b_kwargs()
    runs = []
    for _ in range(2):
        with PredNetTrainer(wts, list(ch), w, h, B, T) as tr:
            losses = [(tr.step(frames, **kw), tr.last_loss_parts) for _ in range(10)]
            runs.append((losses, tr.weights()))
    assert runs[0][0] == runs[1][0] and np.isfinite([v[0] for v in runs[0][0]]).all()
    for k in wts:
        assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k
    assert any(not np.array_equal(runs[0][1][k], wts[k]) for k in wts)
    print("10 Adam steps under the joint objective: loss %.6f -> %.6f, parts %s -> %s" % (runs[0][0][0][0], runs[0][0][-1][0], runs[0][0][0][1], runs[0][0][-1][1]))


# ---- the outcome
# held-out means before -> after 200 Adam steps under the joint objective at mu = 4, as scripts/flow_joint_train.py recorded them on an
# MI355X (profiles/flow_joint_train.txt): both metrics fell.  The assertion asks for half of each measured reduction, the margin of
# tests/test_gpu_flow_target.py.  Under the target alone the squared error rose 8.3 %, under "mse" the endpoint error rose 15.1 %.
MEASURED_MU = 4.0
MEASURED_JOINT_EPE = (0.939249, 0.851750)        # 9.3 % lower: 4.7 % is asked for
MEASURED_JOINT_MSE = (0.052273, 0.041878)        # 19.9 % lower: 9.9 % is asked for


def test_adam_steps_under_the_joint_objective_cut_both_held_out_metrics(cuda):
    """The setup of scripts/flow_joint_train.py: 32 x 24 gray, [1, 8, 16], B = 4, T = 6 (3 fed + 3 self-fed), 200 Adam steps at alpha 3e-3
    under a PredictionFlow (radius 3) with the video's exact flow as the target, the terms 1 .. 4 weighted, frame_weight 4; one-layer
    textures, held-out batch 10**6: `train.flow_epe` on the tape-free predictions and the squared error of `evaluate`."""
    from examples.train_prednet import held_out_epe
    w, h, ch = 32, 24, [1, 8, 16]
    B, T, fed = 4, 6, 3
    flow = PredictionFlow(3, 1e-2)
    with MovingTextures(w, h, 1, T, seed=0, layers=1) as src, PredNetTrainer("synthetic:0", ch, w, h, B, T, alpha=3e-3) as tr:
        held, truth, _ = src.batch(10 ** 6, B, flow=True)
        measure = lambda: (held_out_epe(tr, held, truth, 3, 1e-2, fed, False).mean(), tr.evaluate(held, n_fed=fed).mean())
        before = measure()
        for k in range(200):
            frames, fl, _ = src.batch(k, B, flow=True)
            tr.step(frames, n_fed=fed, step_weights=[0.0, 1.0, 1.0, 1.0, 1.0], objective="flow", flow=flow, flow_target=fl, frame_weight=MEASURED_MU)
        after = measure()
    for name, b, a, (m_before, m_after) in (("squared endpoint error", before[0], after[0], MEASURED_JOINT_EPE), ("squared error", before[1], after[1], MEASURED_JOINT_MSE)):
        print("held-out %s %.6f -> %.6f (%.1f %% lower)" % (name, b, a, 100 * (1 - a / b)))
        assert a < b and a <= (1 - 0.5 * (1 - m_after / m_before)) * b, (name, b, a)
