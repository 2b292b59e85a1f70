"""The joint objective and the valid pixels without a GPU ("The joint objective and the valid pixels"): the ABI
surface, the rules and the routing of ``frame_weight=`` / ``flow_valid=``, the resources of the new kernels in the built library, the
restatements of tests/flow_joint_support.py against each other, and the liveness of the chosen cases on the references alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, train
from tests import flow_joint_support as fj
from tests import flow_target_support as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
NEW = ("eigen_moving_cppn_valid", "eigen_trainer_flow_term_valid", "eigen_trainer_loss_grad_flow_joint")


def test_the_three_exports_exist_and_bind():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    one_line = lambda n: re.sub(r"\s+", " ", re.search(r"^int %s\([^;]*;" % n, header, re.M).group(0))
    tg, vd = one_line("eigen_trainer_flow_term_target"), one_line("eigen_trainer_flow_term_valid")
    assert vd == tg.replace("_target(", "_valid(").replace("t_bstride);", "t_bstride, const uint8_t* d_valid, int64_t v_bstride);")
    tg, jt = one_line("eigen_trainer_loss_grad_flow_target"), one_line("eigen_trainer_loss_grad_flow_joint")
    assert jt == tg.replace("_target(", "_joint(").replace("t_tstride);", "t_tstride, const eigen_flow_joint* joint);")
    assert one_line("eigen_moving_cppn_valid") == ("int eigen_moving_cppn_valid(eigen_engine* e, int32_t n, int32_t n_frames, int32_t n_layers, const double* h_affine, "
                                                   "const double* h_affine_inv, uint8_t* d_valid, void* stream);")
    record = re.search(r"typedef struct eigen_flow_joint \{(.*?)\} eigen_flow_joint;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", record)) == [f[0] for f in train.FlowJointSettings._fields_]
    assert ctypes.sizeof(train.FlowJointSettings) == 40
    for n in NEW:
        assert engine.EXPORTS.count(n) == 1
    assert re.search(r"#define EIGEN_ABI_VERSION 4\b", header) and engine.ABI_VERSION == 4
    assert train._ENTRIES[True, "joint"][0] == "eigen_trainer_loss_grad_flow_joint"
    if os.path.exists(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "libeigen_hip.so")):
        lib = engine.load_library()
        train._bind(lib)
        assert lib.eigen_abi_version() == 4 and lib.eigen_moving_cppn_valid is not None
        assert list(lib.eigen_trainer_flow_term_valid.argtypes) == list(lib.eigen_trainer_flow_term_target.argtypes) + [ctypes.c_void_p, ctypes.c_int64]
        assert list(lib.eigen_trainer_loss_grad_flow_joint.argtypes) == list(lib.eigen_trainer_loss_grad_flow_target.argtypes) + [ctypes.c_void_p]


def test_calls_without_the_new_arguments_keep_their_entry():
    score, mem = train.FlowScore(), train.CornerMembers()
    plain = [train.FlowObjective(), train.PredictionFlow(), train.FlowObjective(score=score), train.FlowObjective(score=train.BandsScore()),
             train.FlowObjective(score=score, members=mem), train.FlowObjective().solved(2, 2), train.FlowObjective(reference="moving")]
    keys = ["frame", "prediction", "score", "structure", "members", "iter", "frame"]
    tg = np.zeros((1, 2, 4, 4))
    assert [train._entry_key(f) for f in plain] == keys == [train._entry_key(f, None, False) for f in plain]
    assert all(train._entry_key(f, tg) == "target" == train._entry_key(f, tg, False) for f in plain[:2])
    assert all(train._entry_key(f, None, True) == "joint" == train._entry_key(f, tg, True) for f in plain)
    before = {(True, k): n for k, n in (("frame", "eigen_trainer_loss_grad_flow"), ("prediction", "eigen_trainer_loss_grad_flow_pair"),
                                        ("score", "eigen_trainer_loss_grad_flow_score"), ("structure", "eigen_trainer_loss_grad_flow_structure"),
                                        ("members", "eigen_trainer_loss_grad_flow_members"), ("iter", "eigen_trainer_loss_grad_flow_iter"),
                                        ("target", "eigen_trainer_loss_grad_flow_target"))}
    assert all(train._ENTRIES[k][0] == n for k, n in before.items()) and sorted(train.OBJECTIVES) == ["error", "flow", "mse"]
    # `flow` stays the last parameter, the new ones stand ahead of it and default to None
    for fn in (train.PredNetTrainer.forward_backward, train.PredNetTrainer.step, train.PredNetTrainer._loss_grad):
        params = inspect.signature(fn).parameters
        assert list(params)[-3:] == ["frame_weight", "flow_valid", "flow"] and params["frame_weight"].default is None and params["flow_valid"].default is None
    assert list(inspect.signature(train.PredNetTrainer.flow_term_valid).parameters) == ["self", "pred", "ref", "flow", "target", "valid", "scale", "reference_grad"]
    assert list(inspect.signature(train.PredNetTrainer.flow_term_pair_valid).parameters) == ["self", "pred", "prev", "flow", "target", "valid", "scale", "reference_grad"]
    assert list(inspect.signature(train.flow_epe).parameters) == ["trainer", "pred", "prev_or_ref", "flow", "target", "valid"]
    assert inspect.signature(train.flow_epe).parameters["valid"].default is None
    assert inspect.signature(train.MovingTextures.batch).parameters["valid"].default is False
    assert list(inspect.signature(engine.Engine.moving_cppn_valid).parameters) == ["self", "affine", "affine_inv", "stream"]


def test_every_value_error():
    H, W, n, T = 6, 8, 2, 4
    flow = train.FlowObjective(3, 1e-2)
    tg = np.zeros((n, T - 1, 2, H, W))
    ok = np.ones((n, T - 1, H, W), np.uint8)
    shape = ok.shape
    # the frame weight: None is no frame term; a finite float > 0 under objective="flow" only
    assert train.check_frame_weight("flow", None) is None and train.check_frame_weight("mse", None) is None
    assert train.check_frame_weight("flow", 4) == 4.0 and train.check_frame_weight("flow", np.float32(0.5)) == 0.5
    for bad in (0, 0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and > 0"):
            train.check_frame_weight("flow", bad)
    for bad in (True, "1", [1.0]):
        with pytest.raises(ValueError, match="must be a number"):
            train.check_frame_weight("flow", bad)
    for objective in ("mse", "error"):
        with pytest.raises(ValueError, match="goes with objective='flow'"):
            train.check_frame_weight(objective, 1.0)
    # the planes: only together with a target
    assert train.check_flow_valid("flow", flow, None, None, shape) is None and train.check_flow_valid("mse", None, None, None, shape) is None
    assert train.check_flow_valid("flow", flow, tg, ok, shape) == [(T - 1) * H * W, H * W]
    assert train.check_flow_valid("flow", train.PredictionFlow(3, 1e-2).solved(2, 2), tg, ok.astype(bool), shape) == [(T - 1) * H * W, H * W]
    assert train.check_flow_valid("flow", flow, tg, torch.ones(shape, dtype=torch.bool), shape) == [(T - 1) * H * W, H * W]
    wide = np.ones((2 * n, 2 * T, H, W), np.uint8)
    assert train.check_flow_valid("flow", flow, tg, wide[::2, 1:T], shape) == [2 * 2 * T * H * W, H * W]
    assert train.check_flow_valid("flow", flow, tg, torch.from_numpy(wide)[::2, 1:T], shape) == [2 * 2 * T * H * W, H * W]
    assert train.check_flow_valid("flow", flow, tg[:, 0], ok[:, 0], (n, H, W)) == [(T - 1) * H * W]
    with pytest.raises(ValueError, match="a flow target"):
        train.check_flow_valid("flow", flow, None, ok, shape)
    for objective in ("mse", "error"):
        with pytest.raises(ValueError, match="goes with objective='flow'"):
            train.check_flow_valid(objective, None, tg, ok, shape)
    for bad in (ok.astype(np.float32), ok.astype(np.int32), torch.ones(shape, dtype=torch.float64)):
        with pytest.raises(ValueError, match="must be uint8 or bool"):
            train.check_flow_valid("flow", flow, tg, bad, shape)
    for bad in (ok[:, :2], ok[:1], np.ones((n, T - 1, W, H), np.uint8), ok[:, 0], ok.reshape(-1), np.ones((n, T - 1, 2, H, W), np.uint8)):
        with pytest.raises(ValueError, match="the validity planes must be"):
            train.check_flow_valid("flow", flow, tg, bad, shape)
    for bad in (np.ones((n, T - 1, H, 2 * W), np.uint8)[..., ::2], np.ones((n, T - 1, W, H), np.uint8).transpose(0, 1, 3, 2),
                torch.ones((n, T - 1, 2 * H, W), dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError, match="must be contiguous"):
            train.check_flow_valid("flow", flow, tg, bad, shape)
    with pytest.raises(ValueError, match="numpy array or torch tensor"):
        train.check_flow_valid("flow", flow, tg, ok.tolist(), shape)
    # a per-sample mask on the objective is still refused with a target, planes or not
    with pytest.raises(ValueError, match="per-sample mask"):
        train.check_flow_target("flow", train.PredictionFlow(3, 1e-2, mask=np.ones((n, H, W))), tg, tg.shape)
    # the stage alone and the metric need both a target and planes; the source states planes of its flow only
    for fn in (train.PredNetTrainer.flow_term_valid, train.PredNetTrainer.flow_term_pair_valid):
        for target, valid in ((None, ok[:, 0]), (tg[:, 0], None)):
            with pytest.raises(ValueError, match="needs a target field and validity planes"):
                fn(None, None, None, flow, target, valid)
    with pytest.raises(ValueError, match="needs a target"):
        train.flow_epe(None, None, None, flow, None, ok[:, 0])
    with pytest.raises(ValueError, match="needs flow=True"):
        train.MovingTextures(16, 12, 1, 3).batch(0, 1, valid=True)
    assert "last_loss_parts" in train.PredNetTrainer.forward_backward.__doc__ and "flow_valid" in train.PredNetTrainer.step.__doc__


@pytest.mark.parametrize("kernel", fj.FLOW_VALID_KERNELS)
def test_the_trainer_kernels_have_no_scratch_and_no_spills(kernel):
    from tests.train_support import check_no_scratch_and_no_spills
    check_no_scratch_and_no_spills(kernel)


def test_the_validity_kernel_has_no_scratch_and_no_spills():
    from tests import test_isa_stats as isa
    from tests.train_support import _kernel_stats
    if not os.path.exists(isa.LIB):
        pytest.skip("libeigen_hip.so not built")
    if not os.path.exists(isa.READELF):
        pytest.skip("llvm-readelf not found")
    stats = _kernel_stats()
    names = [n for n in stats if re.match(r"_ZN3eig\d+cppn_valid_kernel", n)]
    assert names, "cppn_valid_kernel not in the library"
    for n in names:
        for s in stats[n]:
            assert s["private_segment_fixed_size"] == 0 and s["vgpr_spill_count"] == 0 and s["sgpr_spill_count"] == 0, (n, s)


def test_the_new_headers_name_their_kernels_and_add_nothing_atomically():
    code = lambda f: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
    trainer, renderer = code("flow_valid_kernels.h"), code("cppn_valid_kernel.h")
    assert sorted(set(re.findall(r"\b(tflow_\w+_kernel)\(", trainer))) == sorted(fj.FLOW_VALID_KERNELS)
    assert re.findall(r"\b(cppn_\w+_kernel)\(", renderer) == ["cppn_valid_kernel"]
    assert "atomic" not in trainer.lower() and "atomic" not in renderer.lower()
    # the headers whose kernel lists other tests pin are as they were: the new kernels are not in them
    assert "valid" not in code("flow_target_kernels.h") and "valid" not in code("cppn_motion_kernel.h")


@pytest.mark.parametrize("name", fj.VALID_CASES)
def test_the_validity_restatement_is_the_brute_force_statement(name):
    c = fj.valid_case(name)
    valid, cls = fj.valid_ref(c)
    assert valid.shape == (c["n"], c["T"] - 1, c["h"], c["w"]) and valid.dtype == np.uint8 and set(np.unique(valid)) <= {0, 1}
    assert np.array_equal(valid, fj.valid_brute(c))
    assert np.array_equal(valid != 0, cls == fj.VALID)


def test_the_live_case_holds_every_class():
    """two layers with explicit motions: some term holds at least 4 valid, 4 out-of-bounds and 4 occluded pixels, and the planes of the
    two samples and of the two terms differ; the one-layer case has out-of-bounds pixels alone; a NaN affine gives 0 everywhere"""
    c = fj.valid_case("live")
    assert (c["w"], c["h"], c["L"], c["T"], c["n"]) == (16, 12, 2, 3, 2)
    valid, cls = fj.valid_ref(c)
    counts = [[int((cls[b, t] == k).sum()) for k in (fj.VALID, fj.OUT_OF_BOUNDS, fj.OCCLUDED)] for b in range(c["n"]) for t in range(c["T"] - 1)]
    print("live: (valid, out of bounds, occluded) per sample and term:", counts)
    assert any(min(k) >= 4 for k in counts), counts
    assert not np.array_equal(valid[0], valid[1]) and not np.array_equal(valid[:, 0], valid[:, 1])
    one = fj.valid_ref(fj.valid_case("33x18"))[1]
    assert (one == fj.OUT_OF_BOUNDS).sum() >= 4 and not (one == fj.OCCLUDED).any() and (one == fj.VALID).sum() >= 4
    small = fj.valid_ref(fj.valid_case("8x8"))[1]
    assert all((small == k).sum() >= 4 for k in (fj.VALID, fj.OUT_OF_BOUNDS, fj.OCCLUDED))
    nan = dict(c, affine_inv=np.full_like(c["affine_inv"], np.nan))
    assert not fj.valid_ref(nan)[0].any() and not fj.valid_brute(nan).any()


@pytest.mark.parametrize("solve", ft.SOLVES, ids=lambda s: "%dx%d" % s)
def test_the_restatement_is_the_mean_of_the_samples_own_means(solve):
    """20 x 15 colour r 7, with and without the mask: the numpy restatement's value is the torch float64 statement's (the mean over the
    samples of per-sample valid means) to 1e-12; its counts are the planes' own; all-ones planes give `target_value_ref` bit for bit; a
    sample with an all-zero plane adds exactly 0 and leaves the other sample's mv and g as they were; the planes matter: the statement
    without them is elsewhere, in value and in gradient"""
    name, r = "20x15", 7
    img0, img1, truth = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    valid = fj.stage_valid(w, h)
    assert not np.array_equal(valid[0], valid[1]) and valid.all(axis=0).any() and not valid.all(axis=(1, 2)).any()
    for masked in (False, True):
        (rest, u), stmt = fj.stage_reference(name, r, solve, masked)
        mask = ft.stage_mask(w, h) if masked else None
        m = np.ones((h, w), bool) if mask is None else mask != 0
        assert np.abs(u - stmt.u).max() <= 1e-12 and abs(rest.value - stmt.value) <= 1e-12 * max(1.0, abs(stmt.value))
        assert list(rest.counts) == [int((m & (valid[b] != 0)).sum()) for b in range(2)] and 0 < rest.counts.min() < rest.n_mask
        plain = ft.target_value_ref(u, truth, mask)
        ones = fj.valid_value_ref(u, truth, np.ones_like(valid), mask)
        assert ones.value == plain.value and (ones.ratios == 1.0).all()
        assert all(a.tobytes() == b.tobytes() for a, b in zip((ones.mv, ones.gx, ones.gy), (plain.mv, plain.gx, plain.gy)))
        gone = fj.valid_value_ref(u, truth, np.stack([valid[0], np.zeros_like(valid[1])]), mask)
        assert np.isfinite(gone.value) and not gone.mv[1].any() and not gone.gx[1].any() and not gone.gy[1].any() and gone.ratios[1] == 0.0
        assert gone.mv[0].tobytes() == rest.mv[0].tobytes() and gone.gx[0].tobytes() == rest.gx[0].tobytes()
        _, without = ft.stage_reference(name, r, solve, masked)
        assert abs(without.value - stmt.value) > 1e-3 * stmt.value
        assert np.abs(without.seed64 - stmt.seed64).max() > 0.05 * np.abs(stmt.seed64).max()


KIND_FORMS = [(k, p, r, (1, 1)) for k in fj.KINDS for p, r in ft.TRAIN_FORMS] + [(k, "prediction", "constant", (2, 2)) for k in fj.KINDS]


@pytest.mark.parametrize("kind,pairing,reference,solve", KIND_FORMS, ids=["%s-%s-%s-%dx%d" % (k, p, r, s[0], s[1]) for k, p, r, s in KIND_FORMS])
def test_the_frame_weight_of_a_training_case_balances_the_two_parts(kind, pairing, reference, solve):
    """on the float64 references alone: the weight-gradient norm of the flow part and of mu times the squared error's lie within a factor of
    10 of each other, every gradient of the joint reference is alive, and the reference at mu = 0 is outside `_check_grads` of it"""
    from tests.train_support import _grads_differ
    mu = fj.train_mu(kind, pairing, reference, solve)
    flow_part = fj.grad_norm(fj.train_reference(kind, pairing, reference, solve, 0.0).grads)
    frame_part = mu * fj.grad_norm(fj.train_reference(kind, pairing, reference, solve, 0.0, part="mse").grads)
    print("%s %s %s %s: mu %g, |g flow| %.4e, mu |g mse| %.4e" % (kind, pairing, reference, solve, mu, flow_part, frame_part))
    assert mu > 0 and 0.1 <= flow_part / frame_part <= 10.0
    joint, alone = fj.train_reference(kind, pairing, reference, solve), fj.train_reference(kind, pairing, reference, solve, 0.0)
    assert joint.scale > 0 and all(np.abs(g).max() > 0 for g in joint.grads.values()) and np.abs(joint.frame_grad).max() > 0
    assert _grads_differ(joint.grads, alone.grads) and _grads_differ(alone.grads, joint.grads)


def test_the_validity_planes_of_the_training_video_are_live():
    """the planes `train_desc` states for the video of `flow_target_support.train_inputs`: both samples lose pixels, different ones, and
    the float64 reference under them is outside `_check_grads` of the one without"""
    from tests.train_support import _grads_differ
    v = fj.train_valid()
    assert v.shape == (ft.TRAIN_B, ft.TRAIN_T - 1, 12, 16) and all(0 < (v[b] == 0).sum() < v[b].size // 2 for b in range(ft.TRAIN_B))
    assert not np.array_equal(v[0], v[1])
    for pairing, reference in ft.TRAIN_FORMS:
        assert _grads_differ(fj.train_reference("valid", pairing, reference, mu=0.0).grads, fj.train_reference("target", pairing, reference, mu=0.0).grads)


def test_the_command_lines_state_the_frame_weight_and_the_valid_pixels():
    """--frame-weight and --flow-valid reach the trainer through `examples/flow_args.py`; each is an argparse error outside its mode"""
    import argparse
    from examples import flow_args
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="loss")
    ap.add_argument("--data", default="rings")
    flow_args.add_flow_arguments(ap)
    flow_args.add_flow_target_argument(ap)
    flow_args.add_flow_joint_arguments(ap)
    a = ap.parse_args([])
    assert a.frame_weight is None and a.flow_valid == "none"
    flow_args.check_flow_joint(ap, a)
    a = ap.parse_args(["--objective", "flow", "--frame-weight", "4", "--data", "textures", "--flow-target", "truth", "--flow-valid", "visible"])
    flow_args.check_flow_joint(ap, a)
    assert a.frame_weight == 4.0 and a.flow_valid == "visible"
    for bad in (["--frame-weight", "4"], ["--objective", "flow", "--frame-weight", "0"], ["--objective", "flow", "--frame-weight", "nan"],
                ["--objective", "flow", "--flow-valid", "visible"], ["--objective", "flow", "--data", "textures", "--flow-valid", "visible"],
                ["--objective", "flow", "--flow-target", "truth", "--flow-valid", "visible"]):
        with pytest.raises(SystemExit):
            flow_args.check_flow_joint(ap, ap.parse_args(bad))
    for script in (os.path.join("examples", "train_prednet.py"), os.path.join("scripts", "train_bench.py")):
        src = open(os.path.join(ROOT, script)).read()
        assert "add_flow_joint_arguments(ap)" in src and "check_flow_joint(ap, a" in src and "frame_weight" in src and "flow_valid" in src, script
