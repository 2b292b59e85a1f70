"""Self-fed training steps, step weights, tape-free evaluation and trainer state in and out (eigen_trainer_loss_grad_ext,
eigen_trainer_evaluate, eigen_trainer_get_state / set_state) against the float64 torch-CPU autograd
restatement in oracle/prednet_train_ref.py, run with n_fed, a detached requantisation and step weights.  Shapes, weight sets and
tolerances are those of tests/test_gpu_train.py."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, fitness, weights
from evolutionary_illusion_generator_amd.engine import EngineError
from evolutionary_illusion_generator_amd.train import PredNetTrainer
from oracle import prednet_train_ref as ref
from tests.train_support import (N_FED, SHAPES, STEP_WEIGHTS, T_SELF as T_EXT, WSETS, _check_grads, _drifting, _grads_differ, _same_weights, _weight_sets,
                                 case_frames, case_id, case_reference, case_weights, cases, is_all_zero, select)

pytestmark = pytest.mark.gpu


# term s is prediction s against frame s + 1; steps 3, 4, 5 are self-fed


def _self_fed(c):
    """One self-fed squared-error call against the reference.  Returns what the caller's own checks need."""
    wts, frames = case_weights(c.w, c.h, c.ch, c.wset), case_frames(c)
    sw = None if c.sw is None else list(c.sw)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, c.B + c.room[0], c.T + c.room[1]) as tr:
        loss, pred = tr.forward_backward(frames, pred=True, n_fed=c.n_fed, requant=c.requant, step_weights=sw)
        got = tr.grads()
        loss2, pred2 = tr.forward_backward(frames, pred=True, n_fed=c.n_fed, requant=c.requant, step_weights=sw)
        got2 = tr.grads()
    r = case_reference(c, pred=pred)
    print("%s: loss %.8f ref %.8f, max |pred diff| %.2e" % (case_id(c), loss, r.loss, np.abs(pred - r.pred).max()))
    assert np.abs(pred - r.pred).max() <= 1e-5, (case_id(c), np.abs(pred - r.pred).max())
    assert abs(loss - r.loss) <= 1e-5 * r.loss, (case_id(c), loss, r.loss)
    worst = _check_grads(got, r.grads, zero_allowed=is_all_zero(c), what=case_id(c))
    print("  error / bound %.4f in norm, %.4f element-wise" % worst)
    # the same call twice gives the same bits
    assert loss2 == loss and np.array_equal(pred, pred2)
    assert all(np.array_equal(got[k], got2[k]) for k in got)
    return wts, frames, sw, pred, r


@pytest.mark.parametrize("wkey", list(STEP_WEIGHTS))
@pytest.mark.parametrize("requant", [False, True])
@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_self_fed_loss_predictions_and_every_gradient_match_float64_autograd(cuda, w, h, ch, requant, wkey):
    """A prediction on a byte boundary can quantise differently in float32 and in the float64 restatement, so with requant the
    restatement is fed the bytes of the GPU's own float32 predictions of the previous step: both sides read the same constants,
    and the comparison is of the network and its gradient, not of one rounding."""
    todo = select("self_fed", w, h, ch, requant=requant, sw=STEP_WEIGHTS[wkey])
    assert [c.wset for c in todo] == WSETS and all((c.B, c.T, c.n_fed) == (2, T_EXT, N_FED) for c in todo)
    for c in todo:
        wts, frames, sw, pred, r = _self_fed(c)
        if requant:
            # the error-unit term counts: without it (requant = 0 semantics) the restatement's own gradient is another one
            # (the dead cases aside, where every gradient is exactly zero with either feedback)
            g0 = ref.run(wts, ch, frames, n_fed=N_FED, requant=False, step_weights=sw).grads
            assert is_all_zero(c) == (not any(np.any(g) for g in g0.values()))
            if not is_all_zero(c):
                assert _grads_differ(r.grads, g0), case_id(c)
        else:
            # float feedback: E_0 of a self-fed step is exactly zero, so the prediction of a self-fed step does not depend on its frame
            other = frames.copy()
            other[:, N_FED:] = 255 - other[:, N_FED:]
            with PredNetTrainer(wts, ch, w, h, c.B, T_EXT) as tr:
                _, pred3 = tr.forward_backward(other, pred=True, n_fed=N_FED)
            assert np.array_equal(pred, pred3)


@pytest.mark.parametrize("c", cases("self_fed", wide=True), ids=case_id)
def test_self_fed_gradients_match_at_the_wide_shapes(cuda, c):
    """tests/train_support.py TILE_PROPERTIES: the tiles real channel counts use, under self-fed steps"""
    _self_fed(c)


@pytest.mark.parametrize("w,h,ch", SHAPES)
def test_all_steps_fed_through_the_new_entry_point_is_loss_grad_bit_for_bit(cuda, w, h, ch):
    B, T = 2, 5
    frames = _drifting(w, B, T, ch[0], h, w)
    wts = weights.synthetic_prednet_weights(ch, w, h, seed=1)
    d = torch.from_numpy(frames).to(cuda)
    with PredNetTrainer(wts, ch, w, h, B, T) as tr:
        loss, pred = ctypes.c_double(), torch.empty(frames.shape, dtype=torch.float32, device=cuda)
        rc = tr.lib.eigen_trainer_loss_grad(tr._h, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(T * frames[0, 0].size), B, T, 1, ctypes.byref(loss),
                                            ctypes.c_void_p(pred.data_ptr()), None)
        assert rc == 0
        old = (loss.value, pred.cpu().numpy(), tr.grads())
        new_loss, new_pred = tr.forward_backward(frames, pred=True, n_fed=T, requant=False, step_weights=None)
        new_g = tr.grads()
    assert new_loss == old[0]
    assert np.array_equal(new_pred, old[1])
    for k in new_g:
        assert np.array_equal(new_g[k], old[2][k]), k


@pytest.mark.parametrize("requant", [False, True])
def test_pieces_equal_one_call(cuda, requant):
    """9 steps, 5 of them fed, as one evaluate and as three calls split at step 3 (inside the fed part) and at step 7 (inside
    the self-fed part: n_fed = 0, reset = 0): equal predictions at all 9 steps, equal losses at the 6 terms a piece owns.
    Terms 2 and 6 straddle a split and belong to no piece.  Then the same with the middle piece run by forward_backward:
    evaluate and loss_grad share the one kept state of the handle."""
    w, h, ch = 16, 12, [3, 4, 6]
    B, T, n_fed = 2, 9, 5
    frames = _drifting(21, B, T, ch[0], h, w)
    with PredNetTrainer("synthetic:4", ch, w, h, B, T) as tr:
        one_l, one_p = tr.evaluate(frames, n_fed=n_fed, requant=requant, pred=True)
        assert one_l.shape == (T - 1,) and one_l.dtype == np.float64
        for middle in ("evaluate", "forward_backward"):
            l1, p1 = tr.evaluate(frames[:, :3], reset=True, n_fed=3, requant=requant, pred=True)
            if middle == "evaluate":
                l2, p2 = tr.evaluate(frames[:, 3:7], reset=False, n_fed=2, requant=requant, pred=True)
            else:
                _, p2 = tr.forward_backward(frames[:, 3:7], reset=False, pred=True, n_fed=2, requant=requant)
                l2 = None
            l3, p3 = tr.evaluate(frames[:, 7:], reset=False, n_fed=0, requant=requant, pred=True)
            assert np.array_equal(np.concatenate([p1, p2, p3], 1), one_p), middle
            assert np.array_equal(l1, one_l[0:2]) and np.array_equal(l3, one_l[7:8]), middle
            if l2 is not None:
                assert np.array_equal(l2, one_l[3:6])
        # a self-fed piece really ran on its own predictions: float feedback ignores the frames of self-fed steps
        assert (one_l > 0).all()


def test_evaluate_runs_past_max_steps_and_leaves_the_gradients_alone(cuda):
    w, h, ch = 16, 12, [3, 4, 6]
    B, T, n_fed = 2, 11, 6
    frames = _drifting(31, B, T, ch[0], h, w)
    for label, wts in _weight_sets(ch, w, h):
        with PredNetTrainer(wts, ch, w, h, B, 4) as tr:
            tape = tr.tape_bytes
            tr.forward_backward(frames[:, :4])
            before = tr.grads()
            with pytest.raises(EngineError, match="error -4"):
                tr.forward_backward(frames)                       # the tape holds 4 steps
            got, pred = tr.evaluate(frames, n_fed=n_fed, pred=True)
            got_tf = tr.evaluate(frames)
            after = tr.grads()
            assert tr.tape_bytes == tape
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        r = ref.run(wts, ch, frames, n_fed=n_fed)
        ref_pred, ref_l, ref_tf = r.pred, r.step_mse, ref.run(wts, ch, frames).step_mse
        print(label, "evaluate, 11 frames on a 4-step tape: max rel err", np.abs(got / ref_l - 1).max(), np.abs(got_tf / ref_tf - 1).max())
        assert got.shape == (T - 1,) and got_tf.shape == (T - 1,)
        assert np.abs(pred - ref_pred).max() <= 1e-5
        assert (np.abs(got - ref_l) <= 1e-5 * ref_l).all(), (got, ref_l)
        assert (np.abs(got_tf - ref_tf) <= 1e-5 * ref_tf).all(), (got_tf, ref_tf)


@pytest.mark.parametrize("requant", [False, True])
def test_step_losses_are_the_numbers_loss_grad_reduces(cuda, requant):
    """With step weights the loss is sum_s w_s mse_s / sum_s w_s over evaluate's own mse_s, added in step order in double: the host
    recomputation gives the same bits.  With NULL weights the loss keeps eigen_trainer_loss_grad's arithmetic (one sum over all
    terms in 256 fixed slices, times 1 / n_terms), another order of the same additions: it may differ from the mean of the
    per-step values by rounding.  Each of the ~2^15 double additions is off by at most 2^-53 relative and all terms are positive,
    so a bound of 64 ulps of a double (1.4e-14 relative) is generous; more would be a different set of terms."""
    w, h, ch = 24, 16, [1, 3, 4, 5]
    B, T, n_fed = 2, 6, 3
    frames = _drifting(41, B, T, ch[0], h, w)
    sw = [0.0, 1.0, 0.5, 2.0, 1.5]
    with PredNetTrainer("synthetic:6", ch, w, h, B, T) as tr:
        steps = tr.evaluate(frames, n_fed=n_fed, requant=requant)
        weighted = tr.forward_backward(frames, n_fed=n_fed, requant=requant, step_weights=sw)
        ones = tr.forward_backward(frames, n_fed=n_fed, requant=requant, step_weights=[1.0] * (T - 1))
        plain = tr.forward_backward(frames, n_fed=n_fed, requant=requant)
    acc, tot = 0.0, 0.0
    for s in range(T - 1):
        acc += sw[s] * float(steps[s])
        tot += sw[s]
    assert weighted == acc / tot, (weighted, acc / tot)
    acc = 0.0
    for s in range(T - 1):
        acc += float(steps[s])
    assert ones == acc / (T - 1)
    print("NULL weights against the mean of the step losses: %.3e relative" % abs(plain / ones - 1))
    assert abs(plain - ones) <= 64 * np.finfo(np.float64).eps * ones, (plain, ones)


def test_resume_from_a_checkpoint_is_bit_exact(cuda, tmp_path):
    w, h, ch = 16, 12, [3, 4, 6]
    B, T, K = 2, 6, 3
    kw = dict(alpha=2e-3, beta1=0.85, beta2=0.99, eps=1e-7)
    data = [_drifting(50 + i, B, T, ch[0], h, w) for i in range(2 * K)]
    # odd steps are self-fed, requantised and weighted: the checkpoint must carry whatever those depend on
    args = [dict(n_fed=3, requant=True, step_weights=[0.0, 1.0, 1.0, 2.0, 2.0]) if i % 2 else {} for i in range(2 * K)]
    with PredNetTrainer("synthetic:7", ch, w, h, B, T, **kw) as tr:
        for i in range(2 * K):
            tr.step(data[i], **args[i])
        want = tr.weights()
        want_state = tr.state_dict()
    path = str(tmp_path / "ckpt.npz")
    with PredNetTrainer("synthetic:7", ch, w, h, B, T, **kw) as tr:
        for i in range(K):
            tr.step(data[i], **args[i])
        tr.save_checkpoint(path)
    back = weights.load_chainer_npz(path, ch, w, h)          # the file is still a chainer model file
    with PredNetTrainer("synthetic:8", ch, w, h, B, T) as tr:   # other weights, default hyper-parameters: all come from the file
        tr.load_checkpoint(path)
        _same_weights(tr.weights(), back)
        assert tr.state_dict()["adam_t"] == K and (tr.alpha, tr.beta1, tr.beta2, tr.eps) == (2e-3, 0.85, 0.99, 1e-7)
        for i in range(K, 2 * K):
            tr.step(data[i], **args[i])
        _same_weights(tr.weights(), want)
        got_state = tr.state_dict()
    assert got_state["adam_t"] == want_state["adam_t"] == 2 * K
    _same_weights(got_state["adam_m"], want_state["adam_m"])
    _same_weights(got_state["adam_v"], want_state["adam_v"])
    # without the Adam state the continuation is another run: the test above cannot pass by reloading weights alone
    with PredNetTrainer(back, ch, w, h, B, T, **kw) as tr:
        for i in range(K, 2 * K):
            tr.step(data[i], **args[i])
        other = tr.weights()
    assert any(not np.array_equal(other[k], want[k]) for k in want)


def test_resume_between_two_pieces_of_one_sequence_is_bit_exact(cuda, tmp_path):
    w, h, ch = 16, 12, [3, 4, 6]
    B, T = 2, 8
    frames = _drifting(61, B, T, ch[0], h, w)
    with PredNetTrainer("synthetic:9", ch, w, h, B, T) as tr:
        tr.step(frames[:, :4])
        tr.step(frames[:, 4:], reset=False, n_fed=2)
        want = tr.weights()
    path = str(tmp_path / "mid.npz")
    with PredNetTrainer("synthetic:9", ch, w, h, B, T) as tr:
        tr.step(frames[:, :4])
        tr.save_checkpoint(path)
        seq = tr.state_dict()["seq"]
    assert seq is not None and [a.shape for a in seq["P"]] == [(B, c, h >> l, w >> l) for l, c in enumerate(ch)]
    with PredNetTrainer("synthetic:8", ch, w, h, B, T) as tr:
        tr.load_checkpoint(path)
        loaded = tr.state_dict()["seq"]
        for k in seq:
            for a, b in zip(seq[k], loaded[k]):
                assert np.array_equal(a, b), k
        tr.step(frames[:, 4:], reset=False, n_fed=2)
        _same_weights(tr.weights(), want)


@pytest.mark.parametrize("requant", [False, True])
def test_self_fed_trained_weights_drive_the_inference_engine(cuda, requant):
    """The point of the feature: the trainer's self-fed forward is the inference engine's extension.  Weights after a few Adam
    steps, run by the inference engine (its own kernels, Winograd on layers >= 1) over frames[:, :n_fed] plus n_steps - n_fed
    steps on its own prediction, against uint8(P0 * 255) of evaluate(n_fed, requant).  Shape and bound of
    test_trained_weights_drive_the_inference_engine (48x32 colour, 4 layers; |diff| <= 1 on at most 1e-3 of the bytes).
    Measured on MI355X (B = 2, 5 fed + 3 self-fed steps, 73 728 bytes): teacher-forced, max |diff| 1 on 1.4e-5 of the bytes;
    float feedback, max 1 on 1.4e-5 (no byte off on the self-fed steps); requantised feedback, 1 byte off by 1 in the last fed
    step, then 2, 3 and 3 bytes off in the self-fed steps, max 2, 1.2e-4 of all bytes: see (a) - (c) below.  The trainer run on
    the engine's own fed-back bytes: max 1 on 2.7e-5."""
    w, h, ch = 48, 32, [3, 8, 16, 32]
    B, T, n_fed = 2, 8, 5
    frames = _drifting(11, B, T, ch[0], h, w)
    with PredNetTrainer("synthetic:5", ch, w, h, B, T, alpha=3e-3) as tr:
        for _ in range(5):
            tr.step(frames, n_fed=n_fed, requant=requant)
        _, pred = tr.evaluate(frames, n_fed=n_fed, requant=requant, pred=True)
        _, pred_tf = tr.evaluate(frames, pred=True)
        wts = tr.weights()
    mine = (pred * np.float32(255.0)).astype(np.uint8)
    if requant:
        st = fitness.PredNetStream(wts, ch, w, h, B, requant_feedback=True)
        try:
            theirs = np.concatenate([st.feed(frames[:, :n_fed]), st.extend(T - n_fed)], 1)
        finally:
            st.close()
    else:
        theirs = fitness.prednet_sequence_predictions(frames[:, :n_fed], wts, ch, w, h, n_ext=T - n_fed)
    tf = np.abs((pred_tf * np.float32(255.0)).astype(np.uint8).astype(np.int16) - fitness.prednet_sequence_predictions(frames, wts, ch, w, h).astype(np.int16))
    diff = np.abs(mine.astype(np.int16) - theirs.astype(np.int16))
    print("requant=%d: teacher-forced max |diff| %d, share of bytes off %.2e; %d fed + %d self-fed: max |diff| %d, share off %.2e (self-fed steps alone %.2e)"
          % (requant, tf.max(), (tf > 0).mean(), n_fed, T - n_fed, diff.max(), (diff > 0).mean(), (diff[:, n_fed:] > 0).mean()))
    print("  per step: bytes off", [(int((diff[:, s] > 0).sum()), int(diff[:, s].max())) for s in range(T)])
    assert (diff > 0).mean() <= 1e-3, (diff > 0).mean()
    if not requant:
        assert diff.max() <= 1, diff.max()
        return
    # Requantised feedback.  A step is comparable byte for byte only while both sides were FED the same bytes: once one fed-back
    # byte differs (the same 1e-5 of roundings that flip a byte on teacher-forced steps), the two run on inputs 1/255 apart, and
    # one step of this network sees the whole 48x32 image (3 poolings, 3x3 convolutions at every scale, top-down in the same
    # step).  So: (a) every step up to and including the first one whose emitted bytes differ, per sequence, is within 1;
    same = np.ones(B, bool)
    for s in range(T):
        assert diff[same, s].max(initial=0) <= 1, (s, diff[same, s].max())
        if s >= n_fed - 1:
            same &= ~(diff[:, s] > 0).reshape(B, -1).any(1)
    # (b) the steps after it, which read other inputs, stay within 4: 2 was measured on MI355X (3 bytes of 36 864 in the last two
    # steps), the bound leaves a factor of 2;
    assert diff.max() <= 4, diff.max()
    # (c) and the excess IS the differing input: a requantised self-fed step is a teacher-forced step on the byte emitted before,
    # so the trainer teacher-forced on the engine's own emitted bytes reads exactly what the engine read, and then every step is
    # within 1 on at most 1e-3 of the bytes, as on the teacher-forced case.
    as_fed = frames.copy()
    as_fed[:, n_fed:] = theirs[:, n_fed - 1:T - 1]
    with PredNetTrainer(wts, ch, w, h, B, T) as tr:
        _, pred_c = tr.evaluate(as_fed, pred=True)
    ctl = np.abs((pred_c * np.float32(255.0)).astype(np.uint8).astype(np.int16) - theirs.astype(np.int16))
    print("  trainer on the engine's own fed-back bytes: max |diff| %d, share of bytes off %.2e" % (ctl.max(), (ctl > 0).mean()))
    assert ctl.max() <= 1, ctl.max()
    assert (ctl > 0).mean() <= 1e-3, (ctl > 0).mean()


# relative improvement of the self-fed terms by phase B measured on MI355X; the test asks for half of it
MEASURED_GAIN = 0.204


def test_a_self_fed_phase_cuts_the_held_out_loss_of_the_self_fed_steps(cuda):
    """From one start at 32x24 gray, 3 layers, batch 4, 8 frames: phase A, 200 teacher-forced Adam steps (as
    test_adam_steps_on_drifting_patterns_cut_the_held_out_loss), then phase B, 200 steps with the last 4 frames self-fed.  The
    held-out evaluate losses summed over the self-fed steps (terms 4, 5, 6) must be lower after B than after A.
    Measured on MI355X: 0.10185 at the start, 0.01040 after A, 0.00828 after B, 20.4 % lower than after A (the teacher-forced mean
    rises from 0.00071 to 0.00080: B trades a little of it).  The test asks for half of the 20.4 %."""
    w, h, ch = 32, 24, [1, 8, 16]
    B, T, n_fed = 4, 8, 4
    held = _drifting(1000, B, T, 1, h, w)
    with PredNetTrainer("synthetic:0", ch, w, h, B, T, alpha=3e-3) as tr:
        start = tr.evaluate(held, n_fed=n_fed)
        for i in range(200):
            tr.step(_drifting(i, B, T, 1, h, w))
        after_a, tf_a = tr.evaluate(held, n_fed=n_fed), tr.evaluate(held)
        for i in range(200, 400):
            tr.step(_drifting(i, B, T, 1, h, w), n_fed=n_fed)
        after_b, tf_b = tr.evaluate(held, n_fed=n_fed), tr.evaluate(held)
    a, b = after_a[n_fed:].sum(), after_b[n_fed:].sum()
    print("held-out per-step loss, 4 fed + 4 self-fed: start %s\n  after A %s\n  after B %s" % (start, after_a, after_b))
    print("self-fed terms: start %.6f, after A %.6f, after B %.6f (%.1f %% lower than after A); teacher-forced mean %.6f -> %.6f"
          % (start[n_fed:].sum(), a, b, 100 * (1 - b / a), tf_a.mean(), tf_b.mean()))
    assert b < a, (a, b)
    assert b <= (1 - MEASURED_GAIN / 2) * a, (a, b)


def test_error_rules_of_the_new_calls(cuda):
    w, h, ch = 12, 8, [1, 4]
    frames = _drifting(3, 2, 4, 1, h, w)
    with PredNetTrainer("synthetic", ch, w, h, 2, 4) as tr:
        for call in (tr.forward_backward, tr.evaluate):
            with pytest.raises(EngineError, match="error -1"):
                call(frames, n_fed=5)                                    # n_fed > n_steps
            with pytest.raises(EngineError, match="error -1"):
                call(frames, n_fed=-1)
            with pytest.raises(EngineError, match="error -1"):
                call(frames, n_fed=0)                                    # n_fed = 0 with reset = 1
            with pytest.raises(EngineError, match="error -3"):
                call(frames, reset=False, n_fed=0)                       # no state to continue
            with pytest.raises(EngineError, match="error -4"):
                call(_drifting(3, 3, 4, 1, h, w), n_fed=2)               # batch above the handle's
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, step_weights=[1.0, -0.5, 1.0])  # a negative weight
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, step_weights=[0.0, 0.0, 0.0])   # all zero
        with pytest.raises(EngineError, match="error -1"):
            tr.forward_backward(frames, step_weights=[1.0, float("nan"), 1.0])
        with pytest.raises(ValueError):
            tr.forward_backward(frames, step_weights=[1.0, 1.0])        # T - 1 = 3 weights
        tr.evaluate(frames, n_fed=2)
        for call in (tr.forward_backward, tr.evaluate):
            with pytest.raises(EngineError, match="error -3"):
                call(frames[:1], reset=False, n_fed=0)                   # reset = 0 with another batch
        tr.evaluate(frames, reset=False, n_fed=0)                        # the same batch continues, all steps self-fed
        tr.forward_backward(frames[:, :1], reset=False, n_fed=0)         # one step, no loss term: allowed without a reset

        # set_state: shapes and dtypes are checked on the host, the tensor count by the library
        good = tr.state_dict()
        assert good["seq"] is not None and good["adam_t"] == 0
        bad = dict(good, adam_m=dict(good["adam_m"]))
        bad["adam_m"]["ConvP0/W"] = np.zeros((1, 1, 3, 2), np.float32)
        with pytest.raises(ValueError):
            tr.load_state_dict(bad)
        bad = dict(good, adam_v={k: v for k, v in good["adam_v"].items() if k != "ConvP0/b"})
        with pytest.raises(ValueError):
            tr.load_state_dict(bad)
        bad = dict(good, adam_m={k: v.astype(np.int32) for k, v in good["adam_m"].items()})
        with pytest.raises(ValueError):
            tr.load_state_dict(bad)
        bad = dict(good, seq=dict(good["seq"], P=[a[:, :, :-1] for a in good["seq"]["P"]]))
        with pytest.raises(ValueError):
            tr.load_state_dict(bad)
        bad = dict(good, seq=dict(good["seq"], h=[np.concatenate([a, a], 0) for a in good["seq"]["h"]]))
        with pytest.raises(ValueError):
            tr.load_state_dict(bad)                                      # a state of batch 4 in a trainer of 2
        names = tr._names
        tab = (ctypes.c_void_p * len(names))(*[good["adam_m"][n].ctypes.data for n in names])
        rc = tr.lib.eigen_trainer_set_state(tr._h, tab, tab, len(names) - 1, 0, 0, None, 0)
        assert rc == -1                                                  # a wrong tensor count
        seq = (ctypes.c_void_p * 2)(good["seq"]["h"][0].ctypes.data, good["seq"]["c"][0].ctypes.data)
        assert tr.lib.eigen_trainer_set_state(tr._h, tab, tab, len(names), 0, 2, seq, 2) == -1   # 2 state arrays where 3 * layers are due
        assert tr.lib.eigen_trainer_set_state(tr._h, tab, tab, len(names), 0, 3, None, 0) == -4  # batch above the handle's
        assert tr.lib.eigen_trainer_set_state(tr._h, tab, tab, len(names), -1, 0, None, 0) == -1
        tr.load_state_dict(good)                                         # and the good one loads
        tr.evaluate(frames, reset=False, n_fed=0)
        tr.load_state_dict(dict(good, seq=None))                         # no sequence state: nothing to continue
        with pytest.raises(EngineError, match="error -3"):
            tr.evaluate(frames, reset=False, n_fed=0)
    lib = engine.load_library()
    from evolutionary_illusion_generator_amd.train import TrainerConfig
    cfg = TrainerConfig()
    cfg.device, cfg.width, cfg.height, cfg.n_layers, cfg.max_batch, cfg.max_steps = 0, w, h, 2, 2, 4
    cfg.channels[0], cfg.channels[1] = 1, 4
    hdl = ctypes.c_void_p()
    assert lib.eigen_trainer_create(ctypes.byref(cfg), ctypes.byref(hdl)) == 0
    try:
        d = torch.from_numpy(frames).to(cuda)
        out = (ctypes.c_double * 3)()
        assert lib.eigen_trainer_evaluate(hdl, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(4 * h * w), 2, 4, 4, 0, 1, out, None, None) == -3   # no weights yet
        t, nb = ctypes.c_int32(), ctypes.c_int32()
        assert lib.eigen_trainer_get_state(hdl, None, None, 0, ctypes.byref(t), ctypes.byref(nb), None, 0) == -3
    finally:
        lib.eigen_trainer_destroy(hdl)
