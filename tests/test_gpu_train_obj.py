"""Training on the error units, Lotter's L_0 / L_all (eigen_trainer_loss_grad_obj, eigen_trainer_evaluate_err,
train.PredNetTrainer(objective="error")), against the float64 torch-CPU autograd restatement in
oracle/prednet_train_ref.py, run with objective="error": the image layer's error units taken against the true frame, and the
table err[s][l].  Shapes, weight sets and tolerances are those of tests/test_gpu_train.py."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import weights
from evolutionary_illusion_generator_amd.engine import EngineError
from evolutionary_illusion_generator_amd.train import PredNetTrainer, combine_terms
from oracle import prednet_train_ref as ref
from tests.train_support import (N_FED, OBJ_CALLS as CASES, SHAPES, T_SELF as T_OBJ, _check_grads, _drifting, _grads_differ, _loss_grad_ext, _loss_grad_obj_loss,
                                 _same_weights, case_frames, case_id, case_reference, case_weights, cases, lam_of, select)

pytestmark = pytest.mark.gpu


_lam = lam_of


def _rel_close(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool((np.abs(got - ref) <= tol * np.abs(ref)).all())


def _run_case(c):
    """One error-objective call of the trainer and the reference of the same case.  Bounds: `_check_grads` per tensor, 1e-5 relative
    for the loss and every table entry, 1e-5 absolute for the predictions (values in [0, 1], the bound tests/test_gpu_train.py
    puts on them).  A case counts only if the reference gradient of every tensor is non-zero, which `_check_grads` asserts."""
    wts, frames = case_weights(c.w, c.h, c.ch, c.wset), case_frames(c)
    lam, sw = list(c.lam), None if c.sw is None else list(c.sw)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, c.B + c.room[0], c.T + c.room[1]) as tr:
        loss, pred, table = tr.forward_backward(frames, pred=True, n_fed=c.n_fed, requant=c.requant, step_weights=sw, objective="error",
                                                layer_weights=lam, layer_errors=True)
        got = tr.grads()
        c_loss = _loss_grad_obj_loss(tr, frames, c.n_fed, c.requant, sw, lam)
    # with requant both sides read the bytes of the GPU's own float32 predictions (tests/test_gpu_train_ext.py says why)
    r = case_reference(c, pred=pred)
    print("%s: loss %.8f ref %.8f, max |pred diff| %.2e, table max rel err %.2e" % (case_id(c), loss, r.loss, np.abs(pred - r.pred).max(), np.abs(table / r.table - 1).max()))
    assert table.shape == (c.T - 1, len(c.ch)) and table.dtype == np.float64
    assert np.abs(pred - r.pred).max() <= 1e-5, np.abs(pred - r.pred).max()
    assert abs(loss - r.loss) <= 1e-5 * r.loss, (loss, r.loss)
    assert _rel_close(table, r.table), (table, r.table)
    worst = _check_grads(got, r.grads, what=case_id(c))
    print("  error / bound %.4f in norm, %.4f element-wise" % worst)
    # the library's own loss is the documented host formula over the returned table, to the bit
    assert c_loss == loss == combine_terms(table, lam, sw), (c_loss, loss)
    return pred, got


def _l0_differs(c, pred, got):
    """the upper-layer term cannot vanish unnoticed: against the L_0 reference this gradient is far outside the bound"""
    g0 = case_reference(c._replace(lam=tuple(lam_of("l0", len(c.ch)))), pred=pred).grads
    assert _grads_differ(g0, got)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("objective", ["l0", "lall"])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_error_objective_loss_table_predictions_and_every_gradient_match_float64_autograd(cuda, w, h, ch, objective, case):
    n_fed, requant, sw = CASES[case]
    (c,) = select("error_objective", w, h, ch, wset="synthetic", lam=lam_of(objective, len(ch)), n_fed=n_fed, requant=requant, sw=sw)
    assert (c.B, c.T) == (2, T_OBJ)
    pred, got = _run_case(c)
    if objective == "lall":
        _l0_differs(c, pred, got)


@pytest.mark.parametrize("c", cases("error_objective", wide=True), ids=case_id)
def test_l_all_gradients_match_at_the_wide_shapes(cuda, c):
    """tests/train_support.py TILE_PROPERTIES: the tiles real channel counts use, under L_all"""
    pred, got = _run_case(c)
    _l0_differs(c, pred, got)


def test_random_weights_at_the_colour_shape_where_their_gradients_are_not_zero(cuda):
    """The `random` set saturates P0 at the two gray shapes (every L_0 gradient is exactly zero there), so under this objective it is
    used at the colour shape only, where two thirds of P0 sit at the clamp and every tensor still has a gradient
    (tests/train_support.py `is_clamped`): `_check_grads` fails on a tensor whose reference is zero."""
    todo = cases("error_objective_random")
    assert len(todo) == 2 and all((c.w, c.h, list(c.ch)) == SHAPES[1] for c in todo)
    for c in todo:
        _run_case(c)


@pytest.mark.parametrize("sw", [None, [0.0, 1.0, 0.5, 2.0, 1.5]])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_squared_error_through_the_new_entry_is_loss_grad_ext_bit_for_bit(cuda, w, h, ch, sw):
    B = 2
    frames = _drifting(w, B, T_OBJ, ch[0], h, w)
    wts = weights.synthetic_prednet_weights(ch, w, h, seed=1)
    d = torch.from_numpy(frames).to(cuda)
    with PredNetTrainer(wts, ch, w, h, B, T_OBJ) as tr:
        for n_fed, requant in ((T_OBJ, False), (N_FED, True)):
            old_loss, old_g = _loss_grad_ext(tr, d, n_fed, requant, sw)
            assert any(np.any(g) for g in old_g.values())
            plain = tr.forward_backward(frames, n_fed=n_fed, requant=requant, step_weights=sw, objective="mse")
            g_plain = tr.grads()
            # layer weights are checked but not used by the squared error; the table changes nothing either
            with_table, table = tr.forward_backward(frames, n_fed=n_fed, requant=requant, step_weights=sw, objective="mse",
                                                    layer_weights=_lam("lall", len(ch)), layer_errors=True)
            g_table = tr.grads()
            assert plain == old_loss and with_table == old_loss, (plain, with_table, old_loss)
            for k in old_g:
                assert np.array_equal(g_plain[k], old_g[k]), k
                assert np.array_equal(g_table[k], old_g[k]), k
            # and the table is the one the error objective returns for these frames
            _, table_e = tr.forward_backward(frames, n_fed=n_fed, requant=requant, step_weights=sw, objective="error", layer_errors=True)
            assert np.array_equal(table, table_e)


@pytest.mark.parametrize("n_fed,requant", [(None, False), (N_FED, False), (N_FED, True)])
def test_the_image_layer_entry_is_the_mean_of_the_error_pair_of_the_returned_predictions(cuda, n_fed, requant):
    """err[s][0] against the float64 numpy mean of [relu(x - P), relu(P - x)], each formed in float32 from the returned float32
    predictions and the TRUE frames (self-fed steps included): the same numbers in another order of addition, 1e-12 relative."""
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 7
    frames = _drifting(71, B, T, ch[0], h, w)
    x = frames.astype(np.float32) / np.float32(255.0)
    with PredNetTrainer("synthetic:2", ch, w, h, B, T) as tr:
        _, pred, table = tr.forward_backward(frames, pred=True, n_fed=n_fed, requant=requant, objective="error", layer_errors=True)
        _, pred_e, table_e = tr.evaluate(frames, pred=True, n_fed=n_fed, requant=requant, layer_errors=True)
    assert pred.dtype == np.float32 and np.array_equal(pred, pred_e)
    for tab in (table, table_e):
        for s in range(T - 1):
            pair = np.concatenate([np.maximum(x[:, s + 1] - pred[:, s], np.float32(0)), np.maximum(pred[:, s] - x[:, s + 1], np.float32(0))], 1)
            assert pair.dtype == np.float32
            want = pair.astype(np.float64).mean()
            assert want > 0 and abs(tab[s, 0] - want) <= 1e-12 * want, (s, tab[s, 0], want)
            # the pair sums to the float32 |x - P| exactly: the entry is half the mean absolute error
            assert abs(tab[s, 0] - np.abs(x[:, s + 1] - pred[:, s]).astype(np.float64).mean() / 2) <= 1e-12 * want


@pytest.mark.parametrize("requant", [False, True])
def test_one_table_from_evaluate_forward_backward_and_from_pieces(cuda, requant):
    """evaluate and forward_backward return the same table for the same frames, bit for bit -- also when evaluate's sequence is
    longer than the tape and the table is read back in pieces.  A sequence split into two calls gives the rows of one call, bit
    for bit, except the row that straddles the split, which belongs to no call."""
    w, h, ch = 16, 12, [3, 4, 6]
    B, T, n_fed = 2, 11, 6
    frames = _drifting(81, B, T, ch[0], h, w)
    with PredNetTrainer("synthetic:4", ch, w, h, B, T) as tr:
        _, one = tr.forward_backward(frames, n_fed=n_fed, requant=requant, objective="error", layer_weights=_lam("lall", 3), layer_errors=True)
        mse, ev = tr.evaluate(frames, n_fed=n_fed, requant=requant, layer_errors=True)
        assert one.shape == ev.shape == (T - 1, 3) and np.array_equal(one, ev)
        assert np.array_equal(mse, tr.evaluate(frames, n_fed=n_fed, requant=requant))
        assert (one > 0).all()
        # split inside the teacher-forced part: rows 0 .. 2 and 4 .. 9, row 3 straddles
        _, a = tr.forward_backward(frames[:, :4], n_fed=4, requant=requant, objective="error", layer_errors=True)
        _, b = tr.forward_backward(frames[:, 4:], reset=False, n_fed=n_fed - 4, requant=requant, objective="mse", layer_errors=True)
        assert a.shape == (3, 3) and b.shape == (6, 3)
        assert np.array_equal(a, one[0:3]) and np.array_equal(b, one[4:10])
        # split inside the self-fed part: the second piece is self-fed from its first step
        _, a = tr.evaluate(frames[:, :8], n_fed=n_fed, requant=requant, layer_errors=True)
        _, b = tr.evaluate(frames[:, 8:], reset=False, n_fed=0, requant=requant, layer_errors=True)
        assert np.array_equal(a, one[0:7]) and np.array_equal(b, one[8:10])
    # a tape of 4 steps: evaluate reads its table back every 4 rows
    with PredNetTrainer("synthetic:4", ch, w, h, B, 4) as tr:
        mse_small, ev_small = tr.evaluate(frames, n_fed=n_fed, requant=requant, layer_errors=True)
    assert np.array_equal(ev_small, one) and np.array_equal(mse_small, mse)


def test_training_under_l_all_is_reproducible_and_the_objective_is_not_trainer_state(cuda, tmp_path):
    w, h, ch = 16, 12, [3, 4, 6]
    B, T, K = 2, 6, 3
    lall = _lam("lall", len(ch))
    data = [_drifting(90 + i, B, T, ch[0], h, w) for i in range(2 * K)]
    runs = []
    for _ in range(2):
        with PredNetTrainer("synthetic:7", ch, w, h, B, T, alpha=2e-3) as tr:
            for i in range(2 * K):
                tr.step(data[i], objective="error", layer_weights=lall)
            runs.append(tr.weights())
    _same_weights(runs[0], runs[1])
    start = weights.synthetic_prednet_weights(ch, w, h, seed=7)
    assert any(not np.array_equal(runs[0][k], start[k]) for k in start)
    # a run that alternates objectives (and self-fed, weighted steps), resumed from a checkpoint in its middle
    args = [dict(objective="error", layer_weights=lall), dict(), dict(objective="error", n_fed=3, requant=True, step_weights=[0.0, 1.0, 1.0, 2.0, 2.0]),
            dict(objective="mse", n_fed=3), dict(objective="error"), dict(objective="error", layer_weights=[0.0, 1.0, 0.5])]
    with PredNetTrainer("synthetic:7", ch, w, h, B, T, alpha=2e-3) as tr:
        keys = sorted(tr.state_dict())
        for i in range(2 * K):
            tr.step(data[i], **args[i])
        want = tr.weights()
        assert sorted(tr.state_dict()) == keys == ["adam_m", "adam_t", "adam_v", "hyper", "seq"]
    path = str(tmp_path / "ckpt.npz")
    with PredNetTrainer("synthetic:7", ch, w, h, B, T, alpha=2e-3) as tr:
        for i in range(K):
            tr.step(data[i], **args[i])
        tr.save_checkpoint(path)
    with np.load(path) as z:
        assert not [k for k in z.files if k.split("/")[0] not in ("predictor", "adam", "hyper", "seq")]
    with PredNetTrainer("synthetic:8", ch, w, h, B, T) as tr:
        tr.load_checkpoint(path)
        for i in range(K, 2 * K):
            tr.step(data[i], **args[i])
        _same_weights(tr.weights(), want)
    # the objectives really are different runs
    with PredNetTrainer("synthetic:7", ch, w, h, B, T, alpha=2e-3) as tr:
        for i in range(2 * K):
            tr.step(data[i])
        other = tr.weights()
    assert any(not np.array_equal(other[k], want[k]) for k in want)


def test_error_rules_of_the_objective(cuda):
    w, h, ch = 12, 8, [1, 4]
    frames = _drifting(3, 2, 4, 1, h, w)
    d = torch.from_numpy(frames).to(cuda)
    with PredNetTrainer("synthetic", ch, w, h, 2, 4) as tr:
        for objective in ("mse", "error"):
            for lam in ([1.0, -0.1], [0.0, 0.0], [1.0, float("nan")], [float("inf"), 1.0]):
                with pytest.raises(EngineError, match="error -1"):
                    tr.forward_backward(frames, objective=objective, layer_weights=lam)
            for lam in ([1.0], [1.0, 0.1, 0.1]):
                with pytest.raises(ValueError):
                    tr.forward_backward(frames, objective=objective, layer_weights=lam)   # one weight per layer
                with pytest.raises(ValueError):
                    tr.step(frames, objective=objective, layer_weights=lam)
        with pytest.raises(ValueError):
            tr.forward_backward(frames, objective="l1")
        # an objective the library does not know
        loss = ctypes.c_double()
        call = lambda obj: tr.lib.eigen_trainer_loss_grad_obj(tr._h, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(4 * h * w), 2, 4, 4, 0, 1, None, obj, None,
                                                              ctypes.byref(loss), None, None, None)
        assert call(2) == -1 and call(-1) == -1
        assert call(0) == 0 and call(1) == 0
        # every existing rule holds under the new objective
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, objective="error", n_fed=5)
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, objective="error", n_fed=0)
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, objective="error", step_weights=[0.0, 0.0, 0.0])
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, objective="error", step_weights=[1.0, -1.0, 1.0])
        with pytest.raises(EngineError, match="error -4"):
            tr.forward_backward(_drifting(3, 2, 5, 1, h, w), objective="error")
        with pytest.raises(EngineError, match="error -4"):
            tr.evaluate(_drifting(3, 3, 4, 1, h, w), layer_errors=True)
        tr.forward_backward(frames, objective="error")
        with pytest.raises(EngineError, match="error -3"):
            tr.forward_backward(frames[:1], reset=False, objective="error")
        # one step, no term: allowed without a reset, the loss is 0 and the table is empty
        loss1, table1 = tr.forward_backward(frames[:, :1], reset=False, n_fed=0, objective="error", layer_errors=True)
        assert loss1 == 0.0 and table1.shape == (0, 2)
    from evolutionary_illusion_generator_amd import engine
    from evolutionary_illusion_generator_amd.train import TrainerConfig
    lib = engine.load_library()
    cfg = TrainerConfig()
    cfg.device, cfg.width, cfg.height, cfg.n_layers, cfg.max_batch, cfg.max_steps = 0, w, h, 2, 2, 4
    cfg.channels[0], cfg.channels[1] = 1, 4
    hdl = ctypes.c_void_p()
    assert lib.eigen_trainer_create(ctypes.byref(cfg), ctypes.byref(hdl)) == 0
    try:
        out = (ctypes.c_double * 6)()
        assert lib.eigen_trainer_loss_grad_obj(hdl, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(4 * h * w), 2, 4, 4, 0, 1, None, 1, None, None, out, None, None) == -3
        assert lib.eigen_trainer_evaluate_err(hdl, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(4 * h * w), 2, 4, 4, 0, 1, None, out, None, None) == -3   # no weights yet
    finally:
        lib.eigen_trainer_destroy(hdl)


# relative cut of the held-out L_0 error by 200 Adam steps under L_0, measured on MI355X; the test asks
# for half of it
MEASURED_CUT = 0.673


def test_adam_steps_under_l0_cut_the_held_out_l0_error(cuda):
    """200 Adam steps under L_0 at 32x24 gray, 3 layers, batch 4, 6 frames on the drifting patterns (the setting of
    tests/test_gpu_train.py's squared-error training test): the held-out L_0 error, the mean of the image-layer column of
    evaluate's table, must fall by half of what was measured.
    Measured on MI355X: 0.026718 -> 0.008723, 67.3 % lower (the squared error of the same weights falls from 0.004532 to 0.000876);
    the test asks for half of it, 33.65 %."""
    w, h, ch = 32, 24, [1, 8, 16]
    B, T = 4, 6
    held = _drifting(1000, B, T, 1, h, w)
    with PredNetTrainer("synthetic:0", ch, w, h, B, T, alpha=3e-3) as tr:
        mse0, tab0 = tr.evaluate(held, layer_errors=True)
        for i in range(200):
            tr.step(_drifting(i, B, T, 1, h, w), objective="error")
        mse1, tab1 = tr.evaluate(held, layer_errors=True)
    before, after = tab0[:, 0].mean(), tab1[:, 0].mean()
    print("held-out L_0 error %.6f -> %.6f (%.1f %% lower); squared error %.6f -> %.6f" % (before, after, 100 * (1 - after / before), mse0.mean(), mse1.mean()))
    assert after <= (1 - MEASURED_CUT / 2) * before, (before, after)
