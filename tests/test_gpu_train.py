"""PredNet training on the GPU (eigen_trainer_*, train.PredNetTrainer) against the float64 torch-CPU autograd restatement of the
network and loss in oracle/prednet_train_ref.py (DESIGN.md section 13 states the semantics both follow)."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, fitness, weights
from evolutionary_illusion_generator_amd.engine import EngineError
from evolutionary_illusion_generator_amd.train import PredNetTrainer, TrainerConfig
from oracle import prednet_train_ref as ref
from tests.train_support import (SHAPES, WSETS, _check_grads, _drifting, case_frames, case_id, case_reference, case_weights, cases, is_all_zero,
                                 select)

pytestmark = pytest.mark.gpu


def _teacher_forced(c):
    """one teacher-forced squared-error call of the trainer against the reference: predictions, loss and every gradient"""
    wts, frames = case_weights(c.w, c.h, c.ch, c.wset), case_frames(c)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, c.B + c.room[0], c.T + c.room[1]) as tr:
        loss, pred = tr.forward_backward(frames, pred=True)
        got = tr.grads()
    r = case_reference(c)
    assert np.abs(pred - r.pred).max() <= 1e-5, (case_id(c), np.abs(pred - r.pred).max())
    assert abs(loss - r.loss) <= 1e-5 * r.loss, (case_id(c), loss, r.loss)
    if is_all_zero(c):
        # P0 sits at the clamp everywhere: the reference gradient of every tensor is exactly zero, and so is the trainer's
        assert all(not g.any() for g in r.grads.values()) and all(not g.any() for g in got.values()), case_id(c)
    worst = _check_grads(got, r.grads, zero_allowed=is_all_zero(c), what=case_id(c))
    print("%s: error / bound %.4f in norm, %.4f element-wise" % (case_id(c), worst[0], worst[1]))


@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_forward_loss_and_every_gradient_match_float64_autograd(cuda, w, h, ch):
    todo = select("teacher_forced", w, h, ch)
    assert [c.wset for c in todo] == WSETS and all((c.B, c.T) == (2, 5) for c in todo)
    for c in todo:
        _teacher_forced(c)


@pytest.mark.parametrize("c", cases("teacher_forced", wide=True), ids=case_id)
def test_every_gradient_matches_at_the_wide_shapes(cuda, c):
    """The MT = 4 tiles, gridDim.y > 1, partial M tiles, pixel counts off a multiple of 4 and a handle larger than the call
    (tests/train_support.py TILE_PROPERTIES)."""
    _teacher_forced(c)


@pytest.mark.parametrize("w,h,ch", [s for s in SHAPES if s[2][0] == 1])
def test_weights_that_saturate_every_prediction_give_exactly_zero_gradients(cuda, w, h, ch):
    """The random set at the gray shapes: every pixel of P0 at the clamp on every step, so no gradient reaches a weight under the
    squared error, teacher-forced or self-fed.  Exact zeros, not small numbers: whatever the kernels add up is a sum of zeros."""
    todo = [c for c in select("teacher_forced", w, h, ch, wset="random") + select("self_fed", w, h, ch, wset="random", requant=False, sw=None)]
    assert len(todo) == 2 and all(is_all_zero(c) for c in todo)
    for c in todo:
        wts, frames = case_weights(c.w, c.h, c.ch, c.wset), case_frames(c)
        with PredNetTrainer(wts, list(c.ch), c.w, c.h, c.B, c.T) as tr:
            loss, pred = tr.forward_backward(frames, pred=True, n_fed=c.n_fed)
            got = tr.grads()
        assert loss > 0 and ((pred == 0) | (pred == 1)).all()
        for k, g in got.items():
            assert not g.any(), (case_id(c), k)


@pytest.mark.parametrize("w,h,ch", SHAPES[1:])
def test_truncated_bptt_matches_the_reference_detached_at_the_split(cuda, w, h, ch):
    B, T, k = 2, 7, 3
    frames = _drifting(5, B, T, ch[0], h, w)
    wts = weights.synthetic_prednet_weights(ch, w, h, seed=4)
    with PredNetTrainer(wts, ch, w, h, B, T) as tr:
        l1, g1 = tr.loss_and_grad(frames[:, :k], reset=True)
        l2, pred2 = tr.forward_backward(frames[:, k:], reset=False, pred=True)
        g2 = tr.grads()
    first = ref.run(wts, ch, frames[:, :k])
    second = ref.run(wts, ch, frames[:, k:], state=first.state)
    r1, rg1, r2, rg2, rpred2 = first.loss, first.grads, second.loss, second.grads, second.pred
    assert abs(l1 - r1) <= 1e-5 * r1 and abs(l2 - r2) <= 1e-5 * r2, (l1, r1, l2, r2)
    assert np.abs(pred2 - rpred2).max() <= 1e-5
    _check_grads(g1, rg1)
    _check_grads(g2, rg2)


def test_adam_matches_numpy_and_training_is_bit_reproducible(cuda):
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 4
    frames = _drifting(8, B, T, ch[0], h, w)
    a, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-8
    runs = []
    for _ in range(2):
        with PredNetTrainer("synthetic:3", ch, w, h, B, T, alpha=a, beta1=b1, beta2=b2, eps=eps) as tr:
            p = tr.weights()
            m = {k: np.zeros(v.shape) for k, v in p.items()}
            v2 = {k: np.zeros(v.shape) for k, v in p.items()}
            for step in range(1, 4):
                _, g = tr.loss_and_grad(frames)
                tr.adam()
                got = tr.weights()
                lr = a * np.sqrt(1 - b2 ** step) / (1 - b1 ** step)
                for k in p:
                    gk = g[k].astype(np.float64)
                    m[k] += (1 - b1) * (gk - m[k])
                    v2[k] += (1 - b2) * (gk * gk - v2[k])
                    want = p[k].astype(np.float64) - lr * m[k] / (np.sqrt(v2[k]) + eps)
                    err = np.abs(got[k] - want)
                    assert (err <= 1e-6 * np.abs(want) + 1e-9).all(), (k, step, err.max())
                p = got  # the next step starts from the trainer's own float32 weights
            runs.append((got, g))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k


def test_trained_weights_drive_the_inference_engine(cuda):
    """weights() loaded into the inference path (prednet_sequence_predictions: its own kernels, Winograd on layers >= 1) reproduce the
    trainer forward's quantised predictions uint8(P0 * 255).  Measured on MI355X: max |diff| 1 in 1.8e-5 of the bytes; the bound (1e-3) leaves a 55x margin."""
    w, h, ch = 48, 32, [3, 8, 16, 32]
    B, T = 2, 6
    frames = _drifting(11, B, T, ch[0], h, w)
    with PredNetTrainer("synthetic:5", ch, w, h, B, T, alpha=3e-3) as tr:
        for _ in range(5):
            tr.step(frames)
        _, pred = tr.forward_backward(frames, pred=True)
        wts = tr.weights()
    mine = (pred * np.float32(255.0)).astype(np.uint8)
    theirs = fitness.prednet_sequence_predictions(frames, wts, ch, w, h)
    diff = np.abs(mine.astype(np.int16) - theirs.astype(np.int16))
    print("trained weights -> inference engine: max |diff| %d, fraction of bytes off %.2e" % (diff.max(), (diff > 0).mean()))
    assert diff.max() <= 1, diff.max()
    assert (diff > 0).mean() <= 1e-3, (diff > 0).mean()


def test_adam_steps_on_drifting_patterns_cut_the_held_out_loss(cuda):
    """200 Adam steps at 32x24 gray, 3 layers, batch 4, 6 frames: held-out next-frame loss must fall by >= 30 %.  Measured on MI355X:
    0.00453 -> 0.00095, 79 % lower, in under a second."""
    w, h, ch = 32, 24, [1, 8, 16]
    B, T = 4, 6
    held = _drifting(1000, B, T, 1, h, w)
    with PredNetTrainer("synthetic:0", ch, w, h, B, T, alpha=3e-3) as tr:
        before = tr.forward_backward(held)
        for i in range(200):
            tr.step(_drifting(i, B, T, 1, h, w))
        after = tr.forward_backward(held)
    print("held-out loss %.6f -> %.6f (%.1f %% lower)" % (before, after, 100 * (1 - after / before)))
    assert after <= 0.7 * before, (before, after)


def test_error_rules(cuda):
    w, h, ch = 12, 8, [1, 4]
    frames = _drifting(3, 2, 4, 1, h, w)
    with PredNetTrainer("synthetic", ch, w, h, 2, 4) as tr:
        with pytest.raises(EngineError, match="error -4"):
            tr.forward_backward(_drifting(3, 3, 4, 1, h, w))            # batch above the handle's
        with pytest.raises(EngineError, match="error -4"):
            tr.forward_backward(_drifting(3, 2, 5, 1, h, w))            # more steps than the handle's
        with pytest.raises(EngineError, match="error -3"):
            tr.forward_backward(frames, reset=False)                    # no previous call
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames[:, :1])                          # one frame: no loss term
        with pytest.raises(ValueError):
            tr.forward_backward(np.zeros((2, 4, 3, h, w), np.uint8))   # wrong frame shape
        with pytest.raises(ValueError):
            tr.forward_backward(frames.astype(np.float32))
        tr.forward_backward(frames)
        with pytest.raises(EngineError, match="error -3"):
            tr.forward_backward(frames[:1], reset=False)                # a different batch
        tr.forward_backward(frames[:, :2], reset=False)                 # the same batch continues
    lib = engine.load_library()
    cfg = TrainerConfig()
    cfg.device, cfg.width, cfg.height, cfg.n_layers, cfg.max_batch, cfg.max_steps = 0, w, h, 2, 2, 4
    cfg.channels[0], cfg.channels[1] = 1, 4
    hdl = ctypes.c_void_p()
    assert lib.eigen_trainer_create(ctypes.byref(cfg), ctypes.byref(hdl)) == 0
    try:
        d = torch.from_numpy(frames).to(cuda)
        loss = ctypes.c_double()
        rc = lib.eigen_trainer_loss_grad(hdl, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(4 * h * w), 2, 4, 1, ctypes.byref(loss), None, None)
        assert rc == -3                                                 # no weights yet
        assert lib.eigen_trainer_adam(hdl, ctypes.c_double(1e-3), ctypes.c_double(0.9), ctypes.c_double(0.999), ctypes.c_double(1e-8), None) == -3
    finally:
        lib.eigen_trainer_destroy(hdl)
