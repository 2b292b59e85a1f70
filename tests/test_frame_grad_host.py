"""CPU: the host side of the frame gradient and of the refinement of stills ("Frame gradients") -- the float64
restatement of tests/frame_grad_support.py pinned to the one reference, the structure of its frame gradient, the two entry points
in header, binding and library, the register metadata of the three kernels, and the Python argument checks."""
import os
import re
import types

import numpy as np
import pytest

from oracle import prednet_train_ref as ref
from tests.frame_grad_support import case_inputs, fold_tied, run_frames, still_step_ref, target_path
from tests.train_support import SHAPES, TRAIN_KERNELS, _kernel_stats, check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_HOST, B_HOST = 5, 2
FRAME_GRAD_KERNELS = ["tframe_grad_kernel", "tstill_absmax_kernel", "tstill_step_kernel"]
LALL = lambda L: [1.0] + [0.1] * (L - 1)


def _kw(objective, L, n_fed):
    return dict(objective=objective, layer_weights=LALL(L) if objective == "error" else None, n_fed=n_fed)


@pytest.mark.parametrize("n_fed", [T_HOST, 3])
@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("wset", ["synthetic", "random"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_the_restatement_is_the_one_reference_bit_for_bit(w, h, ch, wset, objective, n_fed):
    frames, sets = case_inputs(w, h, tuple(ch), B_HOST, T_HOST)
    kw = _kw(objective, len(ch), n_fed)
    r, f = ref.run(sets[wset], ch, frames, **kw), run_frames(sets[wset], ch, frames, **kw)
    assert f.loss == r.loss
    assert np.array_equal(f.pred, r.pred)
    for k in r.grads:
        assert np.array_equal(f.grads[k], r.grads[k]), k
    assert f.frame_grad.shape == frames.shape and f.frame_grad.dtype == np.float64


@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_the_gradient_by_a_repeated_still_is_the_sum_over_its_frames(w, h, ch, objective):
    frames, sets = case_inputs(w, h, tuple(ch), B_HOST, T_HOST)
    still = np.ascontiguousarray(np.repeat(frames[:, :1], T_HOST, 1))
    kw = _kw(objective, len(ch), 3)
    per = run_frames(sets["synthetic"], ch, still, **kw).frame_grad
    tied = run_frames(sets["synthetic"], ch, still, tied=True, **kw).frame_grad
    assert tied.shape == still[:, 0].shape and np.abs(tied).max() > 0
    assert np.abs(tied - per.sum(1)).max() <= 1e-12 * np.abs(tied).max()
    # and the float32 fold the library's tied mode is defined as is that sum, to float32 rounding
    assert np.abs(fold_tied(per) - tied).max() <= 1e-5 * np.abs(tied).max()


@pytest.mark.parametrize("objective", ["mse", "error"])
def test_frame_zero_has_no_target_part_and_only_term_zero_reaches_frame_one(objective):
    """All step weights but term 0 are zero, and part of frame 0 is black.  There E_0 of step 0 is relu(0 - 0) and relu'(0) = 0, so
    g_0, which has an input path only, is exactly zero; a target path would not be (g_1, which has one, is non-zero on those very
    pixels).  Term 0 ends in P0_0 (under "error" with the L_0 weights: a layer above would bring in E_l of step 1, which reads frame
    1): g_1 is its target path alone, and no later frame receives anything."""
    w, h, ch = SHAPES[1]
    frames, sets = case_inputs(w, h, tuple(ch), B_HOST, T_HOST)
    frames = frames.copy()
    frames[:, 0, :, :, :3] = 0
    sw = [1.0, 0.0, 0.0, 0.0]
    f = run_frames(sets["synthetic"], ch, frames, step_weights=sw, objective=objective)
    g = f.frame_grad
    assert not g[:, 0, :, :, :3].any() and g[:, 0, :, :, 3:].any()
    assert (g[:, 1, :, :, :3] != 0).mean() > 0.9
    tp = target_path(frames, f.pred, objective, sw)
    assert np.abs(g[:, 1] - tp[:, 1]).max() <= 1e-12 * np.abs(tp[:, 1]).max()
    assert not g[:, 2:].any()


@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("wset", ["synthetic", "random"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_a_self_fed_step_keeps_the_target_path_alone(w, h, ch, wset, objective):
    frames, sets = case_inputs(w, h, tuple(ch), B_HOST, T_HOST)
    sw = [0.5, 1.0, 0.0, 2.0]
    kw = _kw(objective, len(ch), 3)
    f = run_frames(sets[wset], ch, frames, step_weights=sw, **kw)
    tp = target_path(frames, f.pred, objective, sw, kw["layer_weights"])
    assert np.abs(tp[:, 4]).max() > 0 and not tp[:, 3].any()      # the zero weight is term 2, frame 3's
    for t in (3, 4):
        assert np.abs(f.frame_grad[:, t] - tp[:, t]).max() <= 1e-12 * np.abs(tp).max(), t
    if wset == "synthetic":   # a fed step has its input path as well (the random set saturates P0 at the gray shapes: nothing flows back there)
        assert np.abs(f.frame_grad[:, 1] - tp[:, 1]).max() > 1e-6 * np.abs(tp).max()


def test_still_step_ref_moves_free_pixels_by_at_most_the_step():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (3, 3, 6, 8)).astype(np.uint8)
    g = rng.normal(0, 1e-3, img.shape).astype(np.float32)
    g[2] = 0
    mask = np.ones((6, 8), np.uint8)
    mask[:, :2] = 0
    out = still_step_ref(img, g, 2.0, mask)
    assert out.dtype == np.uint8 and np.array_equal(out[2], img[2]) and np.array_equal(out[:, :, :, :2], img[:, :, :, :2])
    move = out.astype(np.int32) - img
    assert np.abs(move).max() == 2 and (move[:2][np.broadcast_to(mask != 0, img.shape)[:2]] * np.sign(g[:2][np.broadcast_to(mask != 0, img.shape)[:2]]) >= 0).all()


def test_header_binding_and_library_hold_the_two_entry_points():
    from evolutionary_illusion_generator_amd import engine
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    for name in ("eigen_trainer_loss_grad_frames", "eigen_trainer_still_step"):
        assert name in declared and name in engine.EXPORTS, name
    assert re.search(r"#define\s+EIGEN_ABI_VERSION\s+4\b", header) and engine.ABI_VERSION == 4
    if os.path.exists(engine.LIB_PATH):
        lib = engine.load_library()
        assert lib.eigen_abi_version() == 4
        assert hasattr(lib, "eigen_trainer_loss_grad_frames") and hasattr(lib, "eigen_trainer_still_step")


def test_the_kernels_live_in_their_own_header():
    csrc = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    assert set(re.findall(pat, open(os.path.join(csrc, "train_kernels.h")).read())) == set(TRAIN_KERNELS)
    assert set(re.findall(pat, open(os.path.join(csrc, "frame_grad_kernels.h")).read())) == set(FRAME_GRAD_KERNELS)
    assert '#include "frame_grad_kernels.h"' in open(os.path.join(csrc, "prednet_train.hip")).read()


@pytest.mark.parametrize("kernel", FRAME_GRAD_KERNELS)
def test_frame_gradient_kernels_have_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)
    if kernel == "tframe_grad_kernel":
        names = [n for n in _kernel_stats() if re.match(r"_ZN4eigt\d+tframe_grad_kernel", n)]
        for obj in (0, 1):
            assert any(re.match(r"_ZN4eigt\d+tframe_grad_kernelILi%dEE" % obj, n) for n in names), (obj, names)


def test_python_argument_errors_need_no_device():
    from evolutionary_illusion_generator_amd import train
    tr = train.PredNetTrainer.__new__(train.PredNetTrainer)   # no handle: the check comes before anything touches the device
    frames = np.zeros((1, 3, 1, 8, 12), np.uint8)
    for bad in ("all", "Tied", True, 1):
        with pytest.raises(ValueError, match="frame_grads"):
            tr.forward_backward(frames, frame_grads=bad)
    fake = types.SimpleNamespace(max_steps=5, channels=[1, 4], w=12, h=8)
    with pytest.raises(ValueError, match="max_steps"):
        train.refine_stills(fake, np.zeros((1, 1, 8, 12), np.uint8), n_repeat=4, n_ext=2)
    with pytest.raises(ValueError, match="max_steps"):
        train.refine_stills(fake, np.zeros((1, 1, 8, 12), np.uint8))       # the defaults: 22 frames
    assert "refine_stills" in train.__all__
