"""CPU: the flow objective's prediction pairing ("The prediction pairing").  The numpy restatement of the flow
stage on two float images is pinned to torch autograd by the reference image, `run_pair` is kept under the float32 yardstick of the
gradient rule on every case tests/test_gpu_flow_pair.py compares, the two gradients the trainer must NOT return are shown to miss the
rule, and the refinement the pairing exists for is shown to climb on the float64 reference alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, train
from tests import flow_obj_support as fs
from tests import flow_pair_support as ps
from tests import flow_ref_support as rs
from tests.train_support import _check_grads, _grads_differ, check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
YARDSTICK = 8.07e-5   # tests/test_flow_obj_host.py: the deviation tests/train_support.py ELEMENT_BOUND is 10 x of


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("w,h,C,r,masked,modes", rs.FIELD_CASES)
def test_the_analytic_gradients_are_autograds(w, h, C, r, masked, modes, kind):
    """`pair_ref` against torch autograd of `torch_flow_term` by both images: max |delta| <= 1e-12 max |ref| for the gradient by `prev`
    (measured 7.0e-15 at worst) and for the seed ahead of its rounding.  With prev = (float32)byte / 255 of a frame, u, seed and the
    reference gradient are those of `flow_ref_grad` on the frame to the bit."""
    pred, prev = ps.pair_field_inputs(w, h, C, kind)
    _, ref = fs.field_inputs(w, h, C, kind)
    mask = fs.field_mask(w, h) if masked else None
    assert not np.array_equal(prev, (prev * np.float32(255.0)).round() / np.float32(255.0))   # a float image, not bytes
    for mode in modes:
        d = fs.direction_of(mode, w, h)
        got = ps.pair_ref(pred, prev, r, 1e-2, d, mask, scale=0.75)
        P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
        x = torch.from_numpy(prev.astype(np.float64)).requires_grad_(True)
        f, _, u = fs.torch_flow_term(P, x, r, 1e-2, d, mask)
        gP, gx = (g.numpy() for g in torch.autograd.grad(0.75 * f, [P, x]))
        dev = np.abs(got.prev_grad64 - gx).max() / np.abs(gx).max()
        dev_seed = np.abs(got.seed - gP).max() / np.abs(gP).max()
        print("%dx%dx%d r=%d %s %s: |delta| / max |ref| %.2e (seed, after its rounding to float: %.2e)" % (w, h, C, r, kind, mode, dev, dev_seed))
        assert np.abs(gx).max() > 0 and dev <= 1e-12, (mode, dev)
        assert dev_seed <= 2.0 ** -23 and np.abs(got.u - u.detach().numpy()).max() <= 1e-12 * np.abs(got.u).max()
        assert np.array_equal(got.prev_grad, got.prev_grad64.astype(np.float32))
        assert abs(got.value - float(f.detach())) <= 1e-12 * np.abs(got.mv).sum()
        tie = ps.pair_ref(pred, ref.astype(np.float32) / np.float32(255.0), r, 1e-2, d, mask, scale=0.75)
        want = rs.flow_ref_grad(pred, ref, r, 1e-2, d, mask, scale=0.75)
        assert np.array_equal(tie.u, want.u) and np.array_equal(tie.seed, want.seed) and np.array_equal(tie.prev_grad, want.grad)


def _deviation(a, r):
    return max(np.abs(a - r).max() / np.abs(r).max(), np.linalg.norm((a - r).ravel()) / np.linalg.norm(r.ravel()))


@pytest.mark.parametrize("c", ps.PAIR_CASES, ids=ps.pair_case_id)
def test_the_yardstick_and_the_gradients_that_must_not_match(c):
    """On the 64 cases, all with "live" weights.
    The yardstick: the float32 network (float64 flow term on the widened images) against float64, per weight tensor, per frame and for
    the tied sum, element-wise and in norm, stays under 8.07e-5 (measured 5.3e-5 at worst; five cases take weight seed 3,
    tests/flow_pair_support.py PAIR_SEEDS says why), so tests/test_gpu_flow_pair.py applies `_check_grads` unchanged.  A requantised case feeds both runs the bytes of the float32 run's predictions.
    The two gradients the trainer must not return miss `_check_grads` against the true one: the frame-pairing gradient of the same call,
    and the prediction-pairing gradient with every reference detached."""
    r32 = ps.pair_case_reference(c, dtype=torch.float32, leaf="frames")
    pred = r32.pred.astype(np.float32) if c.form.endswith("requant") else None
    r64 = ps.pair_case_reference(c, pred=pred, leaf="frames")
    worst = 0.0
    for k, r in r64.grads.items():
        assert r.any(), k
        worst = max(worst, _deviation(r32.grads[k], r))
    T = r64.frame_grad.shape[1]
    n_fed = ps.pair_case_call(c)["n_fed"] or T
    for t in range(T):
        # frames are no references: a step that reads no frame, and the last step of a call, have no frame gradient at all
        r = r64.frame_grad[:, t]
        feeds_a_term = t < n_fed and t < T - 1
        assert r.any() == feeds_a_term, t
        if feeds_a_term:
            worst = max(worst, _deviation(r32.frame_grad[:, t], r))
    worst = max(worst, _deviation(r32.frame_grad.sum(1), r64.frame_grad.sum(1)))
    print("%s: float32 deviation %.2e" % (ps.pair_case_id(c), worst))
    assert worst <= YARDSTICK, worst
    assert r64.scale > 0 and abs(r32.loss - r64.loss) <= 1e-5 * r64.scale
    _check_grads(r64.grads, r64.grads)
    assert ps.has_reference_term(c)
    frame = ps.pair_case_reference(c, pred=pred, run=ps.frame_pairing)
    detached = ps.pair_case_reference(c, pred=pred, detach_prev=True)
    assert _grads_differ(r64.grads, frame.grads) and _grads_differ(r64.grads, detached.grads)
    assert detached.loss == r64.loss and frame.loss != r64.loss


@pytest.mark.parametrize("w,h,ch,mode", ps.REFINE_ROWS)
def test_refinement_on_the_reference_alone(w, h, ch, mode):
    """`run_pair(leaf="tied")` with the population term's weights [0] * n_repeat + [1] * (n_ext - 1) and `still_step_ref`, 8 steps of 2
    bytes with the left quarter kept (REFINE of tests/flow_ref_support.py, unchanged): the term rises in all eight rows, on every single
    step (DESIGN.md has the table).  RISING_ROWS is what tests/test_gpu_flow_pair.py runs; it lists exactly the rows that rise."""
    stills, hist = ps.pair_refine_reference(w, h, ch, mode)
    print("refine on the reference %dx%d %s: %s" % (w, h, mode, " ".join("%.4e" % v for v in hist)))
    assert hist.shape == (ps.REFINE["iters"] + 1,) and np.isfinite(hist).all()
    assert (hist[-1] > hist[0]) == ((w, h, ch, mode) in ps.RISING_ROWS), hist


def test_case_lists():
    assert len(ps.PAIR_CASES) == 64 and all(c.wset == "live" for c in ps.PAIR_CASES)
    assert [(w, h, ch[0]) for w, h, ch in ps.FLOW_SHAPES] == [(12, 8, 1), (16, 12, 3), (24, 16, 1), (40, 24, 3)]
    assert 40 % fs.TILE == 8 and 40 // fs.TILE == 2
    assert ps.MODES == ("energy", "tangent") and ps.RADII == (2, 7) and ps.B_CASE == 2
    assert {c.form for c in ps.PAIR_CASES} == set(ps.FORMS) and all(ps.has_reference_term(c) for c in ps.PAIR_CASES)
    assert ps.POPULATION_WEIGHTS == [0.0] * 4 + [1.0] and ps.pair_case_frames(ps.PAIR_CASES[0]).shape[1] == 6
    assert len(ps.RISING_ROWS) >= 4 and set(ps.RISING_ROWS) <= set(ps.REFINE_ROWS) and len(ps.REFINE_ROWS) == 8
    assert set(ps.PAIR_SEEDS) <= {ps.pair_case_id(c) for c in ps.PAIR_CASES}


def test_python_argument_checks():
    f = train.PredictionFlow()
    assert isinstance(f, train.FlowObjective) and f.pairing == "prediction" and train.FlowObjective().pairing == "frame"
    assert train.FlowObjective(reference="moving").pairing == "frame"
    assert (f.radius, f.eps, f.direction, f.mask, f.settings().flags) == (7, 1e-2, None, None, 0)
    assert list(inspect.signature(train.PredictionFlow.__init__).parameters) == ["self", "radius", "eps", "direction", "mask"]
    with pytest.raises(TypeError):
        train.PredictionFlow(reference="moving")
    for bad in (dict(radius=0), dict(radius=17), dict(eps=0.0), dict(direction=np.zeros((3, 4, 4), np.float32)), dict(mask=np.zeros((4, 4)))):
        with pytest.raises(ValueError):
            train.PredictionFlow(**bad)
    assert train.FLOW_PAIRINGS == {"frame": 0, "prediction": 1} and "PredictionFlow" in train.__all__
    params = list(inspect.signature(train.FlowObjective.__init__).parameters.values())
    assert params[-1].name == "reference" and params[-1].default == "constant"
    for fn in (train.PredNetTrainer.forward_backward, train.PredNetTrainer.step, train.refine_stills, train.refine_genomes):
        assert list(inspect.signature(fn).parameters)[-1] == "flow"
    sig = inspect.signature(train.PredNetTrainer.flow_term_pair)
    assert list(sig.parameters) == ["self", "pred", "prev", "flow", "scale", "reference_grad"] and sig.parameters["reference_grad"].default is False
    # the command lines' constructor
    assert type(train.make_flow()) is train.FlowObjective and train.make_flow("frame", reference="moving").reference == "moving"
    g = train.make_flow("prediction", 3, 0.5, None, np.ones((4, 4)))
    assert type(g) is train.PredictionFlow and (g.radius, g.eps) == (3, 0.5) and g.mask.shape == (4, 4)
    for bad in (dict(pairing="other"), dict(pairing="prediction", reference="moving"), dict(pairing="frame", reference="other")):
        with pytest.raises(ValueError):
            train.make_flow(**bad)
    # the default step weights of the refinement loops, and the rule that goes with them
    assert train._still_weights(None, 20, 2, f) == [0.0] * 20 + [1.0]
    assert train._still_weights(None, 4, 3, f) == [0.0] * 4 + [1.0] * 2
    assert train._still_weights(None, 20, 2, train.FlowObjective()) == train._still_weights(None, 20, 2, None) == [0.0] * 19 + [1.0] * 2
    assert train._still_weights([1.0, 2.0], 1, 2, f) == [1.0, 2.0]
    for given in (None, [1.0]):
        with pytest.raises(ValueError):
            train._still_weights(given, 4, 1, f)
    assert train._still_weights(None, 4, 1, train.FlowObjective()) == [0.0] * 3 + [1.0]
    for fn in (train.refine_stills, train.refine_genomes):
        assert "PredictionFlow" in fn.__doc__ and "PAIR_POPULATION" in fn.__doc__ and "PAIR_SINGLE" in fn.__doc__


def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    for name in ("eigen_trainer_loss_grad_flow_pair", "eigen_trainer_flow_term_pair"):
        assert name in declared and name in engine.EXPORTS
    assert re.search(r"enum\s*\{\s*EIGEN_FLOW_PAIR_FRAME\s*=\s*0\s*,\s*EIGEN_FLOW_PAIR_PREDICTION\s*=\s*1\s*\}", header)
    assert engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header
    assert ctypes.sizeof(train.FlowSettings) == 16 and [n for n, _ in train.FlowSettings._fields_] == ["radius", "flags", "eps"]
    flat = re.sub(r"\s+", " ", header)
    assert "const uint8_t* d_mask, double* h_terms, int32_t pairing, void* stream);" in flat
    assert "float* d_prev_grad, int64_t pg_bstride, void* stream);" in flat and "const float* d_prev, int64_t r_bstride" in flat


def test_the_kernels_live_in_their_own_header():
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    found = lambda name: set(re.findall(pat, open(os.path.join(CSRC, name)).read()))
    assert found("flow_pair_kernels.h") == set(ps.FLOW_PAIR_KERNELS)
    assert found("flow_ref_kernels.h") == set(rs.FLOW_REF_KERNELS) and found("flow_obj_kernels.h") == set(fs.FLOW_OBJ_KERNELS)
    unit, trainer = (open(os.path.join(CSRC, name)).read() for name in ("flow_stage.hip", "prednet_train.hip"))
    assert '#include "flow_pair_kernels.h"' in unit and not re.search(pat, unit) and not re.search(pat, trainer)


@pytest.mark.parametrize("kernel", ps.FLOW_PAIR_KERNELS)
def test_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)
