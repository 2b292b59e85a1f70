"""The frame gradient d loss / d frames of the trainer (eigen_trainer_loss_grad_frames, forward_backward(frame_grads=...)) and the
gradient refinement of stills (eigen_trainer_still_step, train.refine_stills); DESIGN.md section 13, "Frame gradients".  The
reference is the float64 autograd statement of tests/frame_grad_support.py, which tests/test_frame_grad_host.py pins to
oracle/prednet_train_ref.py; shapes and weight sets are those of tests/train_support.py."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.engine import EngineError
from evolutionary_illusion_generator_amd.train import PredNetTrainer
from oracle import prednet_train_ref as ref
from tests.frame_grad_support import case_inputs, check_frame_grads, fold_tied, run_frames, still_step_ref, target_path, zero_steps
from tests.train_support import (FRAME_CALLS, SHAPES, WSETS, case_frames, case_id, case_kwargs, case_reference, case_weights, cases, check_tensor, frame_sw,
                                 is_all_zero, select)

pytestmark = pytest.mark.gpu

CALLS = FRAME_CALLS      # (B, T, n_fed, requant), tests/train_support.py
WORST = {"ratio": 0.0}
_sw = frame_sw


def _lam(objective, L):
    return [1.0] + [0.1] * (L - 1) if objective == "error" else None


@functools.lru_cache(maxsize=None)
def _gpu_and_ref_of(c):
    """One trainer call of every kind and the float64 reference of the same call, made once."""
    frames, wts = case_frames(c), case_weights(c.w, c.h, c.ch, c.wset)
    kw = case_kwargs(c)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, c.B + c.room[0], c.T + c.room[1]) as tr:
        loss, pred, per = tr.forward_backward(frames, pred=True, frame_grads="frames", **kw)
        loss_t, tied = tr.forward_backward(frames, frame_grads="tied", **kw)
    # with requant both sides read the bytes of the GPU's own float32 predictions, as tests/test_gpu_train_ext.py does
    r = case_reference(c, pred=pred, run=run_frames)
    return frames, (loss, loss_t, pred, per, tied), r, (kw["step_weights"], kw["layer_weights"])


def _case(w, h, ch, wset, objective, call, weighted):
    B, T, n_fed, requant = call
    (c,) = select("frames", w, h, ch, B=B, T=T, wset=wset, objective=objective, n_fed=n_fed, requant=bool(requant), sw=frame_sw(weighted, T))
    return c


def _gpu_and_ref(w, h, ch, wset, objective, call, weighted):
    return _gpu_and_ref_of(_case(w, h, ch, wset, objective, call, weighted))


def _frame_gradients(c):
    frames, (loss, loss_t, pred, per, tied), r, (sw, lam) = _gpu_and_ref_of(c)
    n_fed = c.T if c.n_fed is None else c.n_fed
    assert per.shape == frames.shape and per.dtype == np.float32 and tied.shape == frames[:, 0].shape and tied.dtype == np.float32
    assert np.abs(r.frame_grad).max() > 0
    assert loss == loss_t and abs(loss - r.loss) <= 1e-5 * r.loss, (loss, loss_t, r.loss)
    zero = zero_steps(c.T, n_fed, sw, dead=is_all_zero(c))
    ratio = check_frame_grads(per, r.frame_grad, case_id(c), tied=tied, zero=zero)
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print("frame gradient %s: miss / bound %.4f (worst so far %.4f)" % (case_id(c), ratio, WORST["ratio"]))
    for t in zero:
        assert not per[:, t].any(), t      # no target path and no input path: exactly zero
    # a self-fed step keeps the target path alone
    tp = target_path(frames, pred, c.objective, sw, lam)
    G = float(np.linalg.norm(r.frame_grad.ravel()))
    for t in range(n_fed, c.T):
        if t not in zero:
            check_tensor("target path t=%d" % t, per[:, t], tp[:, t], G, what=case_id(c))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("wset", WSETS)
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_frame_gradients_match_float64_autograd(cuda, w, h, ch, wset, objective, call, weighted):
    """Bound: the project's `_check_grads` rule per step t and for the tied output (tests/frame_grad_support.py
    `check_frame_grads`): in norm 1e-3 of the step's own norm, element-wise E of its largest element, no shared floor.  A step with
    neither path (`zero_steps`) is exactly zero."""
    _frame_gradients(_case(w, h, ch, wset, objective, call, weighted))


@pytest.mark.parametrize("c", cases("frames", wide=True), ids=case_id)
def test_frame_gradients_match_at_the_wide_shapes(cuda, c):
    """tests/train_support.py TILE_PROPERTIES: the dgrad of the tiles real channel counts use ends in the frame gradient"""
    _frame_gradients(c)


@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_neither_path_can_be_dropped_or_flipped_unnoticed(cuda, w, h, ch, objective):
    """The reference gradient with one path removed, or with one sign turned, is far outside the bound the trainer meets."""
    call = (3, 5, 3, 0)
    frames, (_, _, pred, per, tied), r, (sw, lam) = _gpu_and_ref(w, h, tuple(ch), "synthetic", objective, call, False)
    tp = target_path(frames, pred, objective, sw, lam)
    inp = r.frame_grad - tp
    for name, wrong in (("no target path", inp), ("no input path", tp), ("target sign", inp - tp), ("input sign", tp - inp)):
        with pytest.raises(AssertionError):
            check_frame_grads(per, wrong, name, zero=range(5))     # a step the wrong reference leaves at zero must then be zero
    check_frame_grads(per, r.frame_grad, "as it is", tied=tied)


@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("n_fed2", [2, 0])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_a_continued_call_starts_from_a_constant_state(cuda, w, h, ch, n_fed2, objective):
    """Two pieces, the second with reset=False: its frame gradients against the restatement started from the reference's state
    after the first.  The straddling term belongs to no call, so frame 0 of the second piece has no target path; with n_fed = 0
    nothing reads a frame, only target paths remain, and g_0 is exactly zero."""
    B, T = 2, 6
    frames, sets = case_inputs(w, h, tuple(ch), B, T)
    wts, lam = sets["synthetic"], _lam(objective, len(ch))
    a, b = frames[:, :3], frames[:, 3:]
    with PredNetTrainer(wts, ch, w, h, B, T) as tr:
        tr.forward_backward(a, objective=objective, layer_weights=lam)
        loss, pred, per = tr.forward_backward(b, reset=False, n_fed=n_fed2, pred=True, frame_grads="frames", objective=objective, layer_weights=lam)
        tr.forward_backward(a, objective=objective, layer_weights=lam)
        _, tied = tr.forward_backward(b, reset=False, n_fed=n_fed2, frame_grads="tied", objective=objective, layer_weights=lam)
    ra = ref.run(wts, ch, a, objective=objective, layer_weights=lam)
    rb = run_frames(wts, ch, b, state=ra.state, n_fed=n_fed2, objective=objective, layer_weights=lam)
    assert abs(loss - rb.loss) <= 1e-5 * rb.loss
    print("continued %dx%d n_fed=%d %s: miss / bound %.4f" % (w, h, n_fed2, objective, check_frame_grads(per, rb.frame_grad, "continued", tied=tied,
                                                                                                        zero=zero_steps(3, n_fed2))))
    assert np.array_equal(tied, fold_tied(per))
    if n_fed2 == 0:
        assert not per[:, 0].any() and not rb.frame_grad[:, 0].any()
        tp = target_path(b, pred, objective, None, lam)
        assert per[:, 1:].any() and np.abs(per - tp).max() <= 1e-3 * np.abs(tp).max()


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_tied_output_is_the_float32_fold_of_the_per_frame_output(cuda, w, h, ch, objective, call):
    for wset in ("synthetic", "random"):
        _, (_, _, _, per, tied), _, _ = _gpu_and_ref(w, h, tuple(ch), wset, objective, call, True)
        assert np.array_equal(tied, fold_tied(per)), wset


def _raw(tr, d, n_fed, requant, objective, lam, buf, g_b, g_t, loss=None):
    """eigen_trainer_loss_grad_frames called directly on device frames d [B, T, C, H, W] and a device float buffer"""
    B, T = int(d.shape[0]), int(d.shape[1])
    l_arr = None if lam is None else np.ascontiguousarray(lam, np.float64)
    return tr.lib.eigen_trainer_loss_grad_frames(tr._h, ctypes.c_void_p(d.data_ptr()), T * int(np.prod(d.shape[2:])), B, T, n_fed, int(requant), 1, None,
                                                 train.OBJECTIVES[objective], None if l_arr is None else ctypes.c_void_p(l_arr.ctypes.data),
                                                 None if loss is None else ctypes.byref(loss), None, None, None if buf is None else ctypes.c_void_p(buf.data_ptr()),
                                                 g_b, g_t, None)


@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_padded_strides_give_the_same_values_and_leave_the_padding_alone(cuda, w, h, ch, objective):
    call = (3, 5, 3, 1)
    B, T, n_fed, requant = call
    frames, (_, _, _, per, tied), _, (_, lam) = _gpu_and_ref(w, h, tuple(ch), "synthetic", objective, call, False)
    _, sets = case_inputs(w, h, tuple(ch), B, T)
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    SENT = np.float32(-12345.5)
    with PredNetTrainer(sets["synthetic"], ch, w, h, B, T) as tr:
        g_t = n + 7
        g_b = (T - 1) * g_t + n + 13
        buf = torch.full((B * g_b + 5,), float(SENT), dtype=torch.float32, device=cuda)
        assert _raw(tr, d, n_fed, requant, objective, lam, buf, g_b, g_t) == 0
        got = buf.cpu().numpy()
        written = np.zeros(got.shape, bool)
        for b in range(B):
            for t in range(T):
                o = b * g_b + t * g_t
                assert np.array_equal(got[o:o + n].reshape(frames.shape[2:]), per[b, t]), (b, t)
                written[o:o + n] = True
        assert (got[~written] == SENT).all() and (~written).sum() == got.size - B * T * n
        # tied with a padded sample stride: cleared by the call where it writes, nowhere else
        g_b = n + 5
        buf = torch.full((B * g_b,), float(SENT), dtype=torch.float32, device=cuda)
        assert _raw(tr, d, n_fed, requant, objective, lam, buf, g_b, 0) == 0
        got = buf.cpu().numpy().reshape(B, g_b)
        assert np.array_equal(got[:, :n].reshape(tied.shape), tied) and (got[:, n:] == SENT).all()


@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_nothing_else_moves_and_the_gradient_is_reproducible(cuda, w, h, ch, objective):
    B, T = 3, 5
    frames, sets = case_inputs(w, h, tuple(ch), B, T)
    kw = dict(n_fed=3, requant=True, step_weights=[0.5, 1.0, 0.0, 2.0], objective=objective, layer_weights=_lam(objective, len(ch)), pred=True, layer_errors=True)
    with PredNetTrainer(sets["synthetic"], ch, w, h, B, T) as tr:
        runs = []
        for fg in (None, "frames", "tied", "frames"):
            out = tr.forward_backward(frames, frame_grads=fg, **kw)
            assert len(out) == (3 if fg is None else 4)
            runs.append((out, tr.grads(), tr.state_dict()["seq"]))
    (base, g0, s0) = runs[0]
    for out, g, s in runs[1:]:
        assert out[0] == base[0] and np.array_equal(out[1], base[1]) and np.array_equal(out[2], base[2])
        for k in g0:
            assert np.array_equal(g[k], g0[k]), k
        for part in train.SEQ_PARTS:
            for x, y in zip(s[part], s0[part]):
                assert np.array_equal(x, y), part
    assert np.array_equal(runs[1][0][3], runs[3][0][3]) and runs[1][0][3].any()


@pytest.mark.parametrize("step", [2.0, 1.5])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_still_step_is_its_numpy_float32_restatement_bit_for_bit(cuda, w, h, ch, masked, step):
    B, C = 3, ch[0]
    rng = np.random.default_rng(w + int(masked))
    img = rng.integers(0, 256, (B, C, h, w)).astype(np.uint8)
    img[0, :, :2] = 0          # bytes at both ends of the range: the clamp is exercised
    img[0, :, -2:] = 255
    g_b = C * h * w + 3
    grad = np.zeros((B, g_b), np.float32)
    grad[:, :C * h * w] = rng.normal(0, 3e-4, (B, C * h * w)).astype(np.float32)
    grad[1] = 0                # an image whose gradient is all zero stays as it is
    mask = None
    if masked:
        mask = np.ones((h, w), np.uint8)
        mask[:, :w // 4] = 0
        mask[h // 2, :] = 0
    want = still_step_ref(img, grad[:, :C * h * w].reshape(img.shape), step, mask)
    d_img, d_g = torch.from_numpy(img).to(cuda), torch.from_numpy(grad).to(cuda)
    d_m = None if mask is None else torch.from_numpy(mask).to(cuda)
    with PredNetTrainer("synthetic", ch, w, h, B, 2) as tr:
        rc = tr.lib.eigen_trainer_still_step(tr._h, ctypes.c_void_p(d_img.data_ptr()), ctypes.c_void_p(d_g.data_ptr()), g_b,
                                             None if d_m is None else ctypes.c_void_p(d_m.data_ptr()), step, B, None)
        assert rc == 0
    got = d_img.cpu().numpy()
    assert np.array_equal(got, want)
    move = np.abs(got.astype(np.int32) - img)
    assert 1 <= move.max() <= math.ceil(step) and np.array_equal(got[1], img[1]) and (got[0] != img[0]).any()
    if masked:
        assert np.array_equal(got[:, :, mask == 0], img[:, :, mask == 0])


@pytest.mark.parametrize("objective", ["mse", "error"])
@pytest.mark.parametrize("wset", ["synthetic", "random"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_refinement_raises_the_stand_in_loss_and_is_reproducible(cuda, w, h, ch, wset, objective):
    """refine_stills with n_repeat=4, n_ext=2, iters=8, step=2, requant=False and the left quarter kept.  On the float64 reference
    alone every one of the 8 steps raised the loss in all 12 combinations; only the end-to-end rise is asserted."""
    B = 2
    frames, sets = case_inputs(w, h, tuple(ch), B, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    mask = np.ones((h, w), np.uint8)
    mask[:, :w // 4] = 0
    kw = dict(n_repeat=4, n_ext=2, iters=8, step=2, requant=False, objective=objective, layer_weights=_lam(objective, len(ch)), mask=mask)
    with PredNetTrainer(sets[wset], ch, w, h, B, 6) as tr:
        out, hist = train.refine_stills(tr, stills, **kw)
        out2, hist2 = train.refine_stills(tr, torch.from_numpy(stills).to(cuda), **kw)
    print("refine %dx%d %s %s: %s" % (w, h, wset, objective, " ".join("%.4e" % v for v in hist)))
    assert out.dtype == np.uint8 and out.shape == stills.shape and hist.shape == (9,) and hist.dtype == np.float64
    assert hist[-1] > hist[0], hist
    assert np.array_equal(out, out2) and np.array_equal(hist, hist2)
    assert np.array_equal(out[..., :w // 4], stills[..., :w // 4]) and (out != stills).any()
    assert np.abs(out.astype(np.int32) - stills).max() <= 8 * 2


def test_error_returns(cuda):
    w, h, ch = SHAPES[1]
    B, T = 2, 4
    frames, _ = case_inputs(w, h, tuple(ch), B, T)
    n = int(np.prod(frames.shape[2:]))
    d = torch.from_numpy(frames).to(cuda)
    buf = torch.zeros(B * T * n, dtype=torch.float32, device=cuda)
    with PredNetTrainer("synthetic", ch, w, h, B, T) as tr:
        for g_t in (1, n - 1, -n):
            assert _raw(tr, d, T, 0, "mse", None, buf, T * n, g_t) == -1
        assert _raw(tr, d, T, 0, "mse", None, buf, (T - 1) * n + n - 1, n) == -1     # one float short of a sample
        assert _raw(tr, d, T, 0, "mse", None, buf, n - 1, 0) == -1                   # tied: one float short of an image
        assert not buf.any()                                                          # a refused call writes nothing
        assert _raw(tr, d, T, 0, "mse", None, buf, T * n, n) == 0 and buf.any()
        a, b = ctypes.c_double(), ctypes.c_double()
        assert _raw(tr, d, T, 0, "mse", None, None, 0, 0, a) == 0
        assert tr.lib.eigen_trainer_loss_grad_obj(tr._h, ctypes.c_void_p(d.data_ptr()), T * n, B, T, T, 0, 1, None, 0, None, ctypes.byref(b), None, None, None) == 0
        assert a.value == b.value
        img = torch.zeros((B, ch[0], h, w), dtype=torch.uint8, device=cuda)
        step = lambda s, batch=B, g_b=n: tr.lib.eigen_trainer_still_step(tr._h, ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(buf.data_ptr()), g_b, None, s,
                                                                        batch, None)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert step(bad) == -1
        assert step(2.0, g_b=n - 1) == -1 and step(2.0, batch=0) == -1
        assert step(2.0, batch=B + 1) == -4
        assert step(2.0) == 0
        with pytest.raises(ValueError):
            tr.forward_backward(frames, frame_grads="both")
        with pytest.raises(ValueError):
            train.refine_stills(tr, frames[:, 0], n_repeat=3, n_ext=2)
        with pytest.raises(EngineError, match="error -4"):
            train.refine_stills(tr, np.zeros((B + 1, ch[0], h, w), np.uint8), n_repeat=2, n_ext=2)
