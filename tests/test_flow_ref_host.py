"""CPU: the flow objective's moving reference ("The moving reference").  The numpy restatement of
csrc/flow_ref_kernels.h is pinned to torch autograd with the reference frame as a leaf, `run_flow(constant_reference=False)` is kept
under the float32 yardstick of the gradient rule on every case tests/test_gpu_flow_ref.py compares, and the refinement the mode exists for
is shown to climb on the float64 reference alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, train
from tests import flow_obj_support as fs
from tests import flow_ref_support as rs
from tests.frame_grad_support import check_frame_grads, zero_steps
from tests.train_support import check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
YARDSTICK = 8.07e-5   # tests/test_flow_obj_host.py: the deviation tests/train_support.py ELEMENT_BOUND is 10 x of


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("w,h,C,r,masked,modes", rs.FIELD_CASES)
def test_the_analytic_reference_gradient_is_autograds(w, h, C, r, masked, modes, kind):
    """`flow_ref_grad` against torch autograd of `torch_flow_term` by the frame: max |delta| <= 1e-12 max |ref| (measured 7.6e-15).  Its
    u and seed are `flow_ref`'s to the bit."""
    pred, ref = fs.field_inputs(w, h, C, kind)
    mask = fs.field_mask(w, h) if masked else None
    for mode in modes:
        d = fs.direction_of(mode, w, h)
        got = rs.flow_ref_grad(pred, ref, r, 1e-2, d, mask, scale=0.75)
        base = fs.flow_ref(pred, ref, r, 1e-2, d, mask, scale=0.75)
        assert np.array_equal(got.u, base.u) and np.array_equal(got.seed, base.seed)
        P = torch.from_numpy(pred.astype(np.float64))
        x = torch.from_numpy((ref.astype(np.float32) / np.float32(255.0)).astype(np.float64)).requires_grad_(True)
        f, _, _ = fs.torch_flow_term(P, x, r, 1e-2, d, mask)
        (g,) = torch.autograd.grad(0.75 * f, x)
        g = g.numpy()
        dev = np.abs(got.grad64 - g).max() / np.abs(g).max()
        print("%dx%dx%d r=%d %s %s: |delta| / max |ref| %.2e" % (w, h, C, r, kind, mode, dev))
        assert np.abs(g).max() > 0 and dev <= 1e-12, (mode, dev)
        assert np.array_equal(got.grad, got.grad64.astype(np.float32))


def test_the_scharr_adjoint_is_the_transpose():
    """<S a, (rx, ry)> == <a, S^T(rx, ry)> on images that have corners, borders and, at 1 x 3 and 1 x 1, nothing else"""
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (1, 3), (2, 2), (3, 1), (5, 7)):
        a, rx, ry = rng.standard_normal((1, h, w)), rng.standard_normal((1, h, w)), rng.standard_normal((1, h, w))
        ap = np.pad(a, ((0, 0), (1, 1), (1, 1)), mode="edge")
        s = lambda dy, dx: ap[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        Ix = ((3.0 * (s(-1, 1) - s(-1, -1)) + 10.0 * (s(0, 1) - s(0, -1))) + 3.0 * (s(1, 1) - s(1, -1))) / 32.0
        Iy = ((3.0 * (s(1, -1) - s(-1, -1)) + 10.0 * (s(1, 0) - s(-1, 0))) + 3.0 * (s(1, 1) - s(-1, 1))) / 32.0
        lhs, rhs = (Ix * rx).sum() + (Iy * ry).sum(), (a * rs.scharr_adjoint(rx, ry)).sum()
        assert abs(lhs - rhs) <= 1e-13 * (np.abs(a).sum() * (np.abs(rx).max() + np.abs(ry).max())), (h, w, lhs, rhs)


@pytest.mark.parametrize("c", rs.LIVE_CASES, ids=fs.flow_case_id)
def test_the_yardstick_and_the_missing_path(c):
    """On the 48 live cases, the frames as the leaf and the reference in the graph.
    The yardstick: the float32 network (float64 flow term) against float64 stays under 8.07e-5 per step and for the tied sum, element-wise
    and in norm (measured 6.7e-7 and 4.2e-7 at worst).
    The path cannot be dropped unnoticed: on every step that has a target path, and on the tied sum, the constant-reference gradient
    misses `check_frame_grads`' bounds against the moving-reference one (least relative distance measured: 0.99)."""
    r64 = fs.flow_case_reference(c, leaf="frames", constant_reference=False)
    r32 = fs.flow_case_reference(c, leaf="frames", constant_reference=False, dtype=torch.float32)
    const = fs.flow_case_reference(c, leaf="frames")
    call = fs.flow_case_call(c)
    T = r64.frame_grad.shape[1]
    w_s = call["step_weights"] or [1.0] * (T - 1)
    parts = [(t, r32.frame_grad[:, t], r64.frame_grad[:, t], const.frame_grad[:, t]) for t in range(T)]
    parts.append(("tied", r32.frame_grad.sum(1), r64.frame_grad.sum(1), const.frame_grad.sum(1)))
    zero = zero_steps(T, call["n_fed"], call["step_weights"])
    worst, least = 0.0, np.inf
    for t, a, r, k in parts:
        if not r.any():
            assert t in zero and not a.any(), t
            continue
        worst = max(worst, np.abs(a - r).max() / np.abs(r).max(), np.linalg.norm((a - r).ravel()) / np.linalg.norm(r.ravel()))
        if t == "tied" or (t >= 1 and w_s[t - 1] != 0):
            least = min(least, np.linalg.norm((k - r).ravel()) / np.linalg.norm(r.ravel()))
        else:
            assert np.array_equal(k, r), t    # no target path: the two references are one computation
    print("%s: float32 deviation %.2e, least distance of the constant-reference gradient %.3f" % (fs.flow_case_id(c), worst, least))
    assert worst <= YARDSTICK, worst
    has_target = [t for t in range(1, T) if w_s[t - 1] != 0]
    assert has_target
    for t in has_target:
        got = np.zeros_like(r64.frame_grad)
        got[:, t] = const.frame_grad[:, t]
        ref = np.zeros_like(r64.frame_grad)
        ref[:, t] = r64.frame_grad[:, t]
        with pytest.raises(AssertionError):
            check_frame_grads(got, ref, "constant against moving, t=%d" % t, zero=range(T))
    with pytest.raises(AssertionError):
        check_frame_grads(r64.frame_grad, r64.frame_grad, "the tied sum", tied=const.frame_grad.sum(1), zero=zero)
    check_frame_grads(r64.frame_grad, r64.frame_grad, "itself", zero=zero)


@pytest.mark.parametrize("mode", ["tangent", "energy"])
@pytest.mark.parametrize("w,h,ch", rs.REFINE_SHAPES)
def test_refinement_on_the_reference_alone_climbs(w, h, ch, mode):
    """`run_flow(leaf="tied", constant_reference=False)` and `still_step_ref`, 8 steps of 2 bytes with the left quarter kept: the term
    rises at all four shapes in both modes (with the reference a constant it falls in seven of the eight; DESIGN.md has the table)."""
    stills, hist = rs.refine_reference(w, h, ch, mode)
    print("refine on the reference %dx%d %s: %s" % (w, h, mode, " ".join("%.4e" % v for v in hist)))
    assert hist.shape == (rs.REFINE["iters"] + 1,) and np.isfinite(hist).all()
    assert hist[-1] > hist[0], hist


def test_the_folds():
    """the two float32 folds a training call is stated by, on numbers whose order of addition shows"""
    per = np.zeros((1, 3, 1, 1, 2), np.float32)
    per[0, :, 0, 0, 0] = [1.0, 2.0 ** -24, 2.0 ** -24]
    refs = {0: np.full((1, 1, 1, 2), 2.0 ** -24, np.float32), 1: np.full((1, 1, 1, 2), 3.0, np.float32)}
    out = rs.add_reference_paths(per, refs)
    assert out[0, 1, 0, 0, 0] == np.float32(2.0 ** -24) + np.float32(2.0 ** -24) and out[0, 2, 0, 0, 0] == np.float32(2.0 ** -24) + np.float32(3.0)
    assert out[0, 0, 0, 0, 0] == 1.0
    tied = rs.fold_tied_moving(per, refs)
    acc = np.float32(0)
    for v in (2.0 ** -24, 3.0, 2.0 ** -24, 2.0 ** -24, 1.0):     # input_2, ref_1, input_1, ref_0, input_0
        acc = np.float32(acc + np.float32(v))
    assert tied[0, 0, 0, 0] == acc
    assert np.array_equal(rs.fold_tied_moving(per, {}), np.asarray([[[[1.0 + 2.0 ** -23, 0.0]]]], np.float32))


def test_case_lists():
    assert len(rs.LIVE_CASES) == 48 and len(rs.FIELD_CASES) == 6 and rs.FIELD_CASES[-1][:4] == (18, 18, 1, 1)
    assert {(c.w, c.h) for c in rs.DEAD_CASES} == {(12, 8), (24, 16)} and all(c.ch[0] == 1 for c in rs.DEAD_CASES)
    assert 18 % fs.TILE == 2


def test_python_argument_checks():
    f = train.FlowObjective()
    assert f.reference == "constant" and f.settings().flags == 0
    m = train.FlowObjective(reference="moving")
    assert m.reference == "moving" and m.settings().flags == train.FLOW_MOVING_REFERENCE == 1 and m.settings(stage_alone=True).flags == 0
    for bad in ("other", None, 1, "Moving"):
        with pytest.raises(ValueError):
            train.FlowObjective(reference=bad)
    params = list(inspect.signature(train.FlowObjective.__init__).parameters.values())
    assert params[-1].name == "reference" and params[-1].default == "constant"
    p = inspect.signature(train.PredNetTrainer.flow_term).parameters["reference_grad"]
    assert p.default is False
    for fn in (train.PredNetTrainer.forward_backward, train.PredNetTrainer.step, train.refine_stills, train.refine_genomes):
        assert list(inspect.signature(fn).parameters)[-1] == "flow"


def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    assert "eigen_trainer_flow_term_ref" in declared and "eigen_trainer_flow_term_ref" in engine.EXPORTS
    assert re.search(r"#define\s+EIGEN_FLOW_MOVING_REFERENCE\s+1\b", header)
    assert engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header
    assert ctypes.sizeof(train.FlowSettings) == 16
    assert [n for n, _ in train.FlowSettings._fields_] == ["radius", "flags", "eps"]
    assert train.FlowSettings.flags.offset == 4 and train.FlowSettings.eps.offset == 8
    assert re.search(r"int32_t\s+flags;", header) and not re.search(r"int32_t\s+reserved;", header)


def test_the_kernels_live_in_their_own_header():
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    assert set(re.findall(pat, open(os.path.join(CSRC, "flow_ref_kernels.h")).read())) == set(rs.FLOW_REF_KERNELS)
    assert set(re.findall(pat, open(os.path.join(CSRC, "flow_obj_kernels.h")).read())) == set(fs.FLOW_OBJ_KERNELS)
    assert '#include "flow_ref_kernels.h"' in open(os.path.join(CSRC, "flow_stage.hip")).read()


@pytest.mark.parametrize("kernel", rs.FLOW_REF_KERNELS)
def test_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)
