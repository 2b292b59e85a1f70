"""CPU: the flow objective's references and host side ("The flow objective").  tests/flow_obj_support.py's
`run_flow` is pinned to oracle/prednet_train_ref.py, its numpy restatement of the kernels to torch autograd, and the float32 yardstick of
the gradient rule is kept over every case tests/test_gpu_flow_obj.py compares."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, train
from oracle import prednet_train_ref
from tests import flow_obj_support as fs
from tests.train_support import SHAPES, _fed_from, case_weights, check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
# the deviation of the float32 restatement tests/train_support.py ELEMENT_BOUND was derived from: the rule keeps its factor 10 only
# while the flow cases stay at or under it
YARDSTICK = 8.07e-5


@pytest.mark.parametrize("form", ["drifting", "still", "still_requant"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_run_flow_under_the_squared_error_is_the_oracle_to_the_bit(w, h, ch, form):
    c = fs.FlowCase(w, h, tuple(ch), "live", "energy", 2, form)
    wts, frames, call = case_weights(w, h, tuple(ch), "live"), fs.flow_case_frames(c), fs.flow_case_call(c)
    fed = _fed_from(prednet_train_ref.run(wts, ch, frames).pred.astype(np.float32)) if call["requant"] else None
    want = prednet_train_ref.run(wts, ch, frames, objective="mse", fed=fed, **call)
    got = fs.run_flow(wts, ch, frames, term=fs.squared_error_term, fed=fed, **call)
    assert got.loss == want.loss and np.array_equal(got.pred, want.pred)
    assert sorted(got.grads) == sorted(want.grads)
    for k in want.grads:
        assert np.array_equal(got.grads[k], want.grads[k]), k
    assert any(g.any() for g in want.grads.values())


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("w,h,C,r,masked,modes", fs.FIELD_CASES)
def test_the_analytic_seed_is_autograds_gradient(w, h, C, r, masked, modes, kind):
    """steps 1-7 of the semantics in numpy against torch autograd of the same value by the prediction: within 1e-12 of the largest
    element.  Both modes, a mask, r = 2 and 7, a window wider than the image (12 x 8 at r = 7), C = 1 and 3."""
    pred, ref = fs.field_inputs(w, h, C, kind)
    mask = fs.field_mask(w, h) if masked else None
    for mode in modes:
        d = fs.direction_of(mode, w, h)
        got = fs.flow_ref(pred, ref, r, 1e-2, d, mask, scale=0.75)
        P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
        x = torch.from_numpy((ref.astype(np.float32) / np.float32(255.0)).astype(np.float64))
        f, _, u = fs.torch_flow_term(P, x, r, 1e-2, d, mask)
        (g,) = torch.autograd.grad(0.75 * f, P)
        g = g.numpy()
        assert np.abs(g).max() > 0
        assert np.abs(got.seed64 - g).max() <= 1e-12 * np.abs(g).max(), (mode, np.abs(got.seed64 - g).max(), np.abs(g).max())
        assert np.array_equal(got.seed, got.seed64.astype(np.float32))
        assert abs(got.value - float(f.detach())) <= 1e-12 * abs(got.value) + got.bound
        assert np.abs(got.u - u.detach().numpy()).max() <= 1e-11 * np.abs(got.u).max()
        if masked:   # a pixel that is not counted adds nothing to the value
            assert not got.mv[:, mask == 0].any() and got.mv[:, mask != 0].any()


def test_the_restatement_truncates_its_windows():
    """a window sum of ones counts the in-image pixels of every window"""
    ones = np.ones((1, 5, 9))
    for r in (1, 2, 7):
        cnt = fs.window_sum(ones, r)[0]
        yy, xx = np.mgrid[0:5, 0:9]
        want = (np.minimum(yy + r, 4) - np.maximum(yy - r, 0) + 1) * (np.minimum(xx + r, 8) - np.maximum(xx - r, 0) + 1)
        assert np.array_equal(cnt, want)


@pytest.mark.parametrize("c", fs.FLOW_CASES, ids=fs.flow_case_id)
def test_the_float32_restatement_stays_under_the_yardstick(c):
    """The yardstick condition, for every gradient case of tests/test_gpu_flow_obj.py: `run_flow` with the network in float32 against
    float64 stays at or under 8.07e-5 per tensor, in norm and in the largest element (the deviation `ELEMENT_BOUND` is 10 x of), its loss
    and terms within a tenth of the loss bound 1e-5 sum m |v| / (B N_m), and every tensor has a non-zero reference gradient unless the
    case is a declared dead one (there every gradient is exactly zero on both sides and the loss is not).

    The float32 run keeps the flow term in float64 on the widened prediction, as the semantics state it and as the kernels compute it.
    Measured over these 84 cases on the CPU: worst deviation 1.2e-5 of a tensor's largest element or norm, worst loss deviation 0.008
    of the loss bound.  An all-float32 statement (flow_dtype=None) was measured too: 3.1e-5 for the gradients, still under the
    yardstick, and up to 0.21 of the loss bound (12x8 gray, energy, r = 7): the float32 window sums and the cancellation in det, which
    the device does not have, and which is why that variant is not the one asserted."""
    r64 = fs.flow_case_reference(c)
    r32 = fs.flow_case_reference(c, dtype=torch.float32)
    assert r64.scale > 0 and r64.loss != 0
    assert abs(r32.loss - r64.loss) <= 0.1 * 1e-5 * r64.scale, (r32.loss, r64.loss, r64.scale)
    live = r64.term_scales > 0
    assert (np.abs(r32.terms - r64.terms)[live] <= 0.1 * 1e-5 * r64.term_scales[live]).all()
    if c.form != "drifting":
        assert not r64.terms[:3].any() and r64.terms[3:].all()     # a term of weight zero reports 0.0
    for k, r in r64.grads.items():
        a = r32.grads[k]
        if fs.is_dead(c):
            assert not r.any() and not a.any(), k
            continue
        assert r.any(), "%s: the reference gradient is zero" % k
        assert np.abs(a - r).max() <= YARDSTICK * np.abs(r).max(), (k, np.abs(a - r).max() / np.abs(r).max())
        assert np.linalg.norm((a - r).ravel()) <= YARDSTICK * np.linalg.norm(r.ravel()), k
    if fs.is_dead(c):
        assert ((r64.pred <= 0) | (r64.pred >= 1)).all()


def test_the_case_list_is_what_the_gpu_test_states():
    ids = [fs.flow_case_id(c) for c in fs.FLOW_CASES]
    assert len(ids) == len(set(ids)) == 84
    assert {(c.w, c.h) for c in fs.FLOW_CASES} == {(12, 8), (16, 12), (24, 16), (40, 24)}
    assert sum(fs.is_dead(c) for c in fs.FLOW_CASES) == 24 and not any(c.wset == "synthetic" for c in fs.FLOW_CASES)
    assert {c.wset for c in fs.FLOW_CASES if (c.w, c.h) == (40, 24)} == {"live"}
    # (40, 24) is three tiles across with a ragged last one and two down
    assert -(-40 // fs.TILE) == 3 and 40 % fs.TILE != 0 and -(-24 // fs.TILE) == 2


def test_flow_direction_values():
    for kind in train.FLOW_DIRECTIONS:
        d = train.flow_direction(kind, 7, 5)
        assert d.shape == (2, 5, 7) and d.dtype == np.float32
    assert np.array_equal(train.flow_direction("horizontal", 4, 3), np.stack([np.ones((3, 4)), np.zeros((3, 4))]).astype(np.float32))
    assert np.array_equal(train.flow_direction("vertical", 4, 3), np.stack([np.zeros((3, 4)), np.ones((3, 4))]).astype(np.float32))
    rad, tan = train.flow_direction("radial", 7, 5), train.flow_direction("tangent", 7, 5)
    assert not rad[:, 2, 3].any() and not tan[:, 2, 3].any()          # zero at the centre pixel
    norm = np.hypot(rad[0], rad[1])
    norm[2, 3] = 1.0
    assert np.abs(norm - 1.0).max() < 1e-6
    assert rad[0, 2, 6] == 1.0 and rad[1, 2, 6] == 0.0 and rad[1, 4, 3] == 1.0    # away from the centre
    # counter-clockwise in image coordinates: (-dy, dx) / |.|
    assert np.array_equal(tan[0], -rad[1]) and np.array_equal(tan[1], rad[0])
    assert tan[1, 2, 6] == 1.0 and tan[0, 4, 3] == -1.0
    even = train.flow_direction("tangent", 4, 2)                       # no centre pixel: every vector is a unit vector
    assert np.abs(np.hypot(even[0], even[1]) - 1.0).max() < 1e-6
    with pytest.raises(ValueError):
        train.flow_direction("diagonal", 4, 3)


def test_flow_objective_and_keyword_validation():
    f = train.FlowObjective()
    assert (f.radius, f.eps, f.direction, f.mask) == (7, 1e-2, None, None)
    s = f.settings()
    assert (s.radius, s.eps) == (7, 1e-2)
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError):
            train.FlowObjective(radius=bad)
    assert train.FlowObjective(radius=1).radius == 1 and train.FlowObjective(radius=16).radius == 16
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            train.FlowObjective(eps=bad)
    d = train.flow_direction("tangent", 6, 4)
    assert train.FlowObjective(direction=d).direction.dtype == np.float32
    for bad in (d[0], d[:1], np.where(d == d[0, 0, 0], np.nan, d), np.where(d == d[0, 0, 0], np.inf, d)):
        with pytest.raises(ValueError):
            train.FlowObjective(direction=bad)
    m = np.zeros((4, 6), np.uint8)
    with pytest.raises(ValueError):
        train.FlowObjective(mask=m)
    with pytest.raises(ValueError):
        train.FlowObjective(mask=np.ones(6))
    m[1, 2] = 7
    assert train.FlowObjective(mask=m).mask[1, 2] == 1
    # a direction or mask of another size than the trainer's image
    with pytest.raises(ValueError):
        train.FlowObjective(direction=d).on_device(torch, 0, 8, 12)
    # flow goes with objective="flow" and with nothing else
    train._check_flow("flow", f)
    train._check_flow("mse", None)
    for objective, flow in (("flow", None), ("flow", {"radius": 7}), ("mse", f), ("error", f)):
        with pytest.raises(ValueError):
            train._check_flow(objective, flow)
    assert train.OBJECTIVES == {"mse": 0, "error": 1, "flow": 2}
    # the keyword is the last parameter of every call that takes an objective, and its default is None
    for fn in (train.PredNetTrainer.forward_backward, train.PredNetTrainer.step, train.PredNetTrainer._loss_grad, train.refine_stills, train.refine_genomes):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "flow" and params[-1].default is None, fn
    assert inspect.signature(train.PredNetTrainer.forward_backward).parameters["flow_terms"].default is False
    with pytest.raises(ValueError):
        train.refine_stills(None, None, objective="flow")
    with pytest.raises(ValueError):
        train.refine_genomes(None, [], None, 0, objective="mse", flow=f)


def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    for name in ("eigen_trainer_flow_term", "eigen_trainer_loss_grad_flow"):
        assert name in declared and name in engine.EXPORTS, name
    assert re.search(r"EIGEN_OBJ_FLOW\s*=\s*2\b", header) and "eigen_flow_settings" in header
    assert engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header
    assert ctypes.sizeof(train.FlowSettings) == 16     # {int32 radius, int32 reserved, double eps}


def test_the_kernels_live_in_their_own_header():
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    assert set(re.findall(pat, open(os.path.join(CSRC, "flow_obj_kernels.h")).read())) == set(fs.FLOW_OBJ_KERNELS)
    unit = open(os.path.join(CSRC, "flow_stage.hip")).read()
    assert '#include "flow_obj_kernels.h"' in unit
    header = open(os.path.join(CSRC, "flow_obj_kernels.h")).read()
    assert re.search(r"FLOW_TILE\s*=\s*%d\b" % fs.TILE, header) and re.search(r"FLOW_MAX_R\s*=\s*%d\b" % train.FLOW_MAX_RADIUS, header)


@pytest.mark.parametrize("kernel", fs.FLOW_OBJ_KERNELS)
def test_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)
