"""The flow objective's target field without a GPU ("The target field"): the ABI surface, the rules and the routing
of ``flow_target=`` / ``target=``, the resources of the new kernel in the built library, the restatements of
tests/flow_target_support.py against each other, and the liveness of the chosen cases on the references alone."""
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, train
from tests import flow_obj_support as fs
from tests import flow_target_support as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eigen_trainer_flow_term_target", "eigen_trainer_loss_grad_flow_target")


def test_the_two_exports_exist_and_bind():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    one_line = lambda n: re.sub(r"\s+", " ", re.search(r"^int %s\([^;]*;" % n, header, re.M).group(0))
    it, tg = one_line("eigen_trainer_flow_term_iter"), one_line("eigen_trainer_flow_term_target")
    assert tg == it.replace("_iter(", "_target(").replace("solve);", "solve, const double* d_target, int64_t t_bstride);")
    it, tg = one_line("eigen_trainer_loss_grad_flow_iter"), one_line("eigen_trainer_loss_grad_flow_target")
    assert tg == it.replace("_iter(", "_target(").replace("solve);", "solve, const double* d_target, int64_t t_bstride, int64_t t_tstride);")
    for n in NEW:
        assert engine.EXPORTS.count(n) == 1
    assert re.search(r"#define EIGEN_ABI_VERSION 4\b", header) and engine.ABI_VERSION == 4
    assert train._ENTRIES[True, "target"][0] == "eigen_trainer_loss_grad_flow_target"
    if os.path.exists(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "libeigen_hip.so")):
        lib = engine.load_library()
        train._bind(lib)
        assert lib.eigen_abi_version() == 4
        assert list(lib.eigen_trainer_flow_term_target.argtypes) == list(lib.eigen_trainer_flow_term_iter.argtypes) + [ctypes_p(), ctypes_i64()]
        assert list(lib.eigen_trainer_loss_grad_flow_target.argtypes) == list(lib.eigen_trainer_loss_grad_flow_iter.argtypes) + [ctypes_p(), ctypes_i64(), ctypes_i64()]


def ctypes_p():
    import ctypes
    return ctypes.c_void_p


def ctypes_i64():
    import ctypes
    return ctypes.c_int64


def test_entry_key_routes_a_target_and_nothing_else():
    score, mem = train.FlowScore(), train.CornerMembers()
    plain = [train.FlowObjective(), train.PredictionFlow(), train.FlowObjective(score=score), train.FlowObjective(score=train.BandsScore()),
             train.FlowObjective(score=score, members=mem), train.FlowObjective().solved(2, 2), train.FlowObjective(reference="moving")]
    keys = ["frame", "prediction", "score", "structure", "members", "iter", "frame"]
    assert [train._entry_key(f) for f in plain] == keys == [train._entry_key(f, None) for f in plain]
    tg = np.zeros((1, 2, 4, 4))
    for f in (train.FlowObjective(), train.PredictionFlow(), train.FlowObjective().solved(2, 2), train.FlowObjective(reference="moving")):
        assert train._entry_key(f, tg) == "target"
    assert {k: v for k, v in train._ENTRIES.items() if k != (True, "target")}[True, "iter"][0] == "eigen_trainer_loss_grad_flow_iter"


def test_every_value_error():
    H, W, n, T = 6, 8, 2, 4
    ok = np.zeros((n, T - 1, 2, H, W))
    shape = ok.shape
    flow = train.FlowObjective(3, 1e-2)
    assert train.check_flow_target("flow", flow, None, shape) is None and train.check_flow_target("mse", None, None, shape) is None
    assert train.check_flow_target("flow", flow, ok, shape) == [(T - 1) * 2 * H * W, 2 * H * W]
    assert train.check_flow_target("flow", train.PredictionFlow(3, 1e-2).solved(2, 2), ok, shape) == [(T - 1) * 2 * H * W, 2 * H * W]
    assert train.check_flow_target("flow", train.FlowObjective(3, 1e-2, mask=np.ones((H, W)), reference="moving"), ok, shape) is not None
    # the strides of the first two dimensions are passed through: a view along n and along the terms, a torch tensor alike
    wide = np.zeros((2 * n, 2 * T, 2, H, W))
    assert train.check_flow_target("flow", flow, wide[::2, 1:T], shape) == [2 * 2 * T * 2 * H * W, 2 * H * W]
    assert train.check_flow_target("flow", flow, torch.from_numpy(wide)[::2, 1:T], shape) == [2 * 2 * T * 2 * H * W, 2 * H * W]
    assert train.check_flow_target("flow", flow, ok[:, 0], (n, 2, H, W)) == [(T - 1) * 2 * H * W]
    # a target without objective="flow"
    for objective in ("mse", "error"):
        with pytest.raises(ValueError, match="goes with objective='flow'"):
            train.check_flow_target(objective, None, ok, shape)
    # an objective that carries a direction, a score, members or a per-sample mask
    score = train.FlowScore()
    carrying = [train.FlowObjective(3, 1e-2, direction=train.flow_direction("horizontal", W, H)), train.FlowObjective(3, 1e-2, score=score),
                train.FlowObjective(3, 1e-2, score=train.BandsScore()), train.FlowObjective(3, 1e-2, score=score, members=train.CornerMembers()),
                train.FlowObjective(3, 1e-2, score=score, mask=np.ones((n, H, W))), train.PredictionFlow(3, 1e-2).scored(score),
                train.PredictionFlow(3, 1e-2, mask=np.ones((n, H, W)))]
    for f in carrying:
        with pytest.raises(ValueError, match="takes no direction, score, members or per-sample mask"):
            train.check_flow_target("flow", f, ok, shape)
    # a wrong dtype or shape; last dimensions that are not contiguous; something that is no array
    for bad in (ok.astype(np.float32), torch.zeros(shape, dtype=torch.float32), np.zeros(shape, np.int64)):
        with pytest.raises(ValueError, match="must be float64"):
            train.check_flow_target("flow", flow, bad, shape)
    for bad in (ok[:, :2], ok[:1], ok[:, :, :1], np.zeros((n, T - 1, 2, W, H)), ok[:, 0], ok.reshape(-1), torch.zeros((n, T, 2, H, W), dtype=torch.float64)):
        with pytest.raises(ValueError, match="the flow target must be"):
            train.check_flow_target("flow", flow, bad, shape)
    for bad in (np.zeros((n, T - 1, 2, H, 2 * W))[..., ::2], np.zeros((n, T - 1, H, W, 2)).transpose(0, 1, 4, 2, 3),
                torch.zeros((n, T - 1, 2, 2 * H, W), dtype=torch.float64)[:, :, :, ::2]):
        with pytest.raises(ValueError, match="must be contiguous"):
            train.check_flow_target("flow", flow, bad, shape)
    with pytest.raises(ValueError, match="numpy array or torch tensor"):
        train.check_flow_target("flow", flow, ok.tolist(), shape)
    with pytest.raises(ValueError, match="needs a target"):
        train.flow_epe(None, None, None, flow, None)
    with pytest.raises(ValueError, match="needs a target"):
        train.PredNetTrainer.flow_term_pair_target(None, None, None, flow, None)
    import inspect
    assert list(inspect.signature(train.PredNetTrainer.flow_term).parameters)[-1] == "target"
    assert list(inspect.signature(train.PredNetTrainer.flow_term_pair_target).parameters) == ["self", "pred", "prev", "flow", "target", "scale", "reference_grad"]
    assert "mean squared endpoint error" in train.flow_epe.__doc__
    assert "flow[:, s]" in train.PredNetTrainer.forward_backward.__doc__


@pytest.mark.parametrize("kernel", ft.FLOW_TARGET_KERNELS)
def test_new_kernel_has_no_scratch_and_no_spills(kernel):
    from tests.train_support import check_no_scratch_and_no_spills
    check_no_scratch_and_no_spills(kernel)


def test_the_new_kernel_file_names_its_kernel_and_adds_nothing_atomically():
    src = open(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc", "flow_target_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert sorted(set(re.findall(r"\b(tflow_\w+_kernel)\(", code))) == sorted(ft.FLOW_TARGET_KERNELS)
    assert "atomic" not in code.lower()


def test_device_sum_is_a_sum():
    """the restated reduction adds every element once: an exact case, a case longer than one pass of the grid, and the fsum bound"""
    import math
    assert ft.device_sum(np.arange(1, 1001, dtype=np.float64), 2.0) == 1000 * 1001 / 4.0
    v = np.random.default_rng(0).random(3 * ft.SUM_BLOCKS * ft.SUM_THREADS + 17)
    exact = math.fsum(v.tolist())
    assert abs(ft.device_sum(v, 1.0) - exact) <= v.size * 2.0 ** -53 * exact
    assert ft.device_sum(np.zeros((2, 5, 7)), 70.0) == 0.0


@pytest.mark.parametrize("solve", ft.SOLVES, ids=lambda s: "%dx%d" % s)
def test_the_restatement_and_the_statement_agree_and_a_zero_target_is_the_plain_term(solve):
    """20 x 15 colour r 3 under the mask: the numpy restatement's field and value are the torch statement's to 1e-12; against a zero
    target the restatement's mv, g and q are `flow_stage_ref`'s own bits (the plain mean squared displacement); against the field itself
    everything is exactly zero; the truth's gradient is alive and differs from the zero target's."""
    name, r = "20x15", 3
    rest, stmt = ft.stage_reference(name, r, solve, True)
    assert np.abs(rest.u - stmt.u).max() <= 1e-12 and abs(rest.value - stmt.value) <= 1e-12 * max(1.0, abs(stmt.value))
    zero, zstmt = ft.stage_reference(name, r, solve, True, "zero")
    assert np.array_equal(zero.u, rest.u) and zero.value != rest.value
    img0, img1, truth = ft.stage_inputs(name)
    mask = ft.stage_mask(20, 15)
    if solve == (1, 1):
        plain = fs.flow_stage_ref(ft.fi.as_floats(img1), fs.byte_reference(img0), r, ft.EPS, mask=mask)
        assert np.array_equal(zero.mv, plain.mv)
        Ix, Iy, aa, bb, cc, det, u = ft.solve_planes(ft.fi.as_floats(img1), fs.byte_reference(img0), r, ft.EPS)
        m = mask != 0
        assert np.array_equal(zero.qx, np.where(m, (cc * (2.0 * u[:, 0]) - bb * (2.0 * u[:, 1])) / det, 0.0))
        assert np.array_equal(zero.qy, np.where(m, (aa * (2.0 * u[:, 1]) - bb * (2.0 * u[:, 0])) / det, 0.0))
    own = ft.target_value_ref(rest.u, rest.u, mask)
    assert own.value == 0.0 and not own.mv.any() and not own.gx.any() and not own.gy.any()
    for a, b in ((stmt.seed64, zstmt.seed64), (stmt.ref64, zstmt.ref64)):
        assert np.abs(a).max() > 0 and np.abs(a - b).max() >= 0.05 * np.abs(a).max()


def test_the_truth_halves_the_term_of_a_zero_target_on_the_exact_shift():
    """The 16 x 12 exact binary shift (0.25, -0.125), radius 3, eps 1e-4, the pixels at least 3 from the border, on the numpy restatement
    alone: the term against the true flow is below half the term against a zero target on both frame pairs.  DESIGN.md records a
    mean-error ratio of 0.20 for this case; the squared ratios are printed."""
    frames, flow, mask = ft.truth_case()
    assert (flow[0, :, 0] == 0.25).all() and (flow[0, :, 1] == -0.125).all()
    for t in range(frames.shape[1] - 1):
        pred, ref64 = ft.fi.as_floats(frames[:, t + 1]), fs.byte_reference(frames[:, t])
        truth = ft.target_stage_ref(pred, ref64, ft.TRUTH_RADIUS, ft.TRUTH_EPS, flow[:, t], mask).value
        zero = ft.target_stage_ref(pred, ref64, ft.TRUTH_RADIUS, ft.TRUTH_EPS, np.zeros_like(flow[:, t]), mask).value
        print("pair %d: term against the truth %.6f, against zeros %.6f, ratio %.4f" % (t, truth, zero, truth / zero))
        assert zero > 0 and truth < 0.5 * zero, (t, truth, zero)


@pytest.mark.parametrize("pairing,reference", ft.TRAIN_FORMS, ids=["%s-%s" % f for f in ft.TRAIN_FORMS])
def test_the_training_cases_are_live_on_the_reference_alone(pairing, reference):
    """the float64 reference of the training call under the truth differs from the one under a zero target by more than `_check_grads`
    allows, in its weight gradients and in its terms, and every gradient is alive"""
    from tests.train_support import _grads_differ
    r, z = ft.train_reference(pairing, reference), ft.train_reference(pairing, reference, "zero")
    print("%s %s: loss %.6e (zero target %.6e), terms %s" % (pairing, reference, r.loss, z.loss, r.terms))
    assert r.scale > 0 and all(np.abs(g).max() > 0 for g in r.grads.values()) and np.abs(r.frame_grad).max() > 0
    assert _grads_differ(z.grads, r.grads) and (np.abs(r.terms - z.terms) > 1e-3 * r.term_scales).all()


def test_the_command_lines_state_the_target():
    """--flow-target reaches the trainer through `examples/flow_args.py`; `truth` without `--data textures` is an argparse error"""
    import argparse
    from examples import flow_args
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="flow")
    ap.add_argument("--data", default="synthetic")
    flow_args.add_flow_arguments(ap)
    assert not hasattr(ap.parse_args([]), "flow_target")        # the refinement scripts' options: a still has no truth
    flow_args.add_flow_target_argument(ap)
    assert ap.parse_args([]).flow_target == "none"
    a = ap.parse_args(["--data", "textures", "--flow-target", "truth"])
    flow_args.check_flow_target(ap, a)
    assert a.flow_target == "truth"
    with pytest.raises(SystemExit):
        flow_args.check_flow_target(ap, ap.parse_args(["--flow-target", "truth"]))
    for script in (os.path.join("examples", "train_prednet.py"), os.path.join("scripts", "train_bench.py")):
        src = open(os.path.join(ROOT, script)).read()
        assert "check_flow_target(ap, a" in src and "flow_target" in src, script
