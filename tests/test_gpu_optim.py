"""The optimiser controls of the trainer on the GPU (eigen_trainer_grad_norms, eigen_trainer_adam_ex, eigen_trainer_accumulate and what
train.PredNetTrainer builds on them; DESIGN.md section 13, "Optimiser controls") against the restatements of tests/optim_support.py
and the float64 reference of oracle/prednet_train_ref.py."""
import ctypes

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.engine import EngineError
from evolutionary_illusion_generator_amd.train import PredNetTrainer
from tests import optim_support as osup
from tests.train_support import SHAPES, _check_grads, _drifting, case_weights

pytestmark = pytest.mark.gpu

HYPER = dict(alpha=2e-3, beta1=0.9, beta2=0.999, eps=1e-8)
shape_id = lambda s: "%dx%d-%s" % (s[0], s[1], "_".join(map(str, s[2])))


def _case(shape, wset="live", B=2, T=4, seed=8):
    w, h, ch = shape
    return case_weights(w, h, tuple(ch), wset), _drifting(seed, B, T, ch[0], h, w)


def _moments(tr):
    st = tr.state_dict()
    return st["adam_m"], st["adam_v"], st["adam_t"]


@pytest.mark.parametrize("shape", osup.GPU_SHAPES, ids=shape_id)
def test_norms_match_numpy_within_the_summation_bound(cuda, shape):
    """Per tensor and globally |got - ref| <= n 2^-52 ref, n the element count: both sides add n exact non-negative squares in double
    in some order (relative error at most (n - 1) 2^-53 each) and take one square root."""
    osup.check_shape_properties()
    w, h, ch = shape
    wts, frames = _case(shape, B=3 if shape == osup.WIDE else 2)
    with PredNetTrainer(wts, ch, w, h, frames.shape[0], frames.shape[1]) as tr:
        tr.forward_backward(frames)
        g = tr.grads()
        got, got_per = tr.grad_norms()
        again, again_per = tr.grad_norms()
        assert list(got_per) == tr._names
        only_global, only_per = ctypes.c_double(-1.0), np.full(len(tr._names), -1.0)
        assert tr.lib.eigen_trainer_grad_norms(tr._h, ctypes.byref(only_global), None, len(tr._names), None) == 0
        assert tr.lib.eigen_trainer_grad_norms(tr._h, None, only_per.ctypes.data_as(train._PD), len(tr._names), None) == 0
        assert tr.lib.eigen_trainer_grad_norms(tr._h, None, None, len(tr._names), None) == 0
    ref, ref_per = osup.norm_ref(g)
    counts = osup.tensor_counts(w, h, ch)
    assert ref > 0
    worst = 0.0
    for k in tr._names:
        assert abs(got_per[k] - ref_per[k]) <= counts[k] * 2.0 ** -52 * ref_per[k], (k, got_per[k], ref_per[k])   # (a zero tensor: exactly zero)
        worst = max(worst, abs(got_per[k] - ref_per[k]) / ref_per[k] if ref_per[k] else 0.0)
    print("%s: global norm %.6e, relative error %.2e; worst tensor %.2e" % (shape_id(shape), got, abs(got - ref) / ref, worst))
    assert abs(got - ref) <= sum(counts.values()) * 2.0 ** -52 * ref, (got, ref)
    # the same bits from call to call, and through either output alone
    assert np.float64(got).tobytes() == np.float64(again).tobytes() == np.float64(only_global.value).tobytes()
    assert np.array_equal(np.array([got_per[k] for k in tr._names]).view(np.uint64), np.array([again_per[k] for k in tr._names]).view(np.uint64))
    assert np.array_equal(only_per.view(np.uint64), np.array([got_per[k] for k in tr._names]).view(np.uint64))


def test_the_dead_case_has_norms_of_exactly_zero_and_a_rate_of_one(cuda):
    (w, h, ch), wset = osup.DEAD
    wts, frames = _case(osup.DEAD[0], wset)
    with PredNetTrainer(wts, ch, w, h, 2, 4, clip_norm=1.0, weight_decay=0.0, **HYPER) as tr:
        tr.forward_backward(frames)
        assert all(not g.any() for g in tr.grads().values())
        total, per = tr.grad_norms()
        assert total == 0.0 and all(v == 0.0 for v in per.values()) and len(per) == len(tr._names)
        before = tr.weights()
        tr.adam()   # clipping is on and the norm is 0: the rate is 1, nothing divides, and a zero gradient moves nothing
        assert tr.last_update == {"norm": 0.0, "rate": 1.0, "applied": 1}
        osup.same_bits(before, tr.weights())
        assert tr.state_dict()["adam_t"] == 1


def test_neutral_settings_are_the_plain_entry_bit_for_bit(cuda):
    shape = SHAPES[1]
    w, h, ch = shape
    wts, frames = _case(shape)
    runs = {}
    for how in ("adam", "adam_ex_neutral", "clip_above_the_norm"):
        with PredNetTrainer(wts, ch, w, h, 2, 4, **HYPER) as tr:
            for _ in range(3):
                tr.forward_backward(frames)
                if how == "adam":
                    tr.adam()
                    assert tr.last_update == {"norm": None, "rate": None, "applied": None}
                elif how == "adam_ex_neutral":
                    assert osup.adam_ex_raw(tr) == (0, None)
                else:
                    norm, _ = tr.grad_norms()
                    tr.clip_norm = 2.0 * norm
                    tr.adam()
                    assert tr.last_update == {"norm": norm, "rate": 1.0, "applied": 1}
            runs[how] = (tr.weights(),) + _moments(tr)
    for how in ("adam_ex_neutral", "clip_above_the_norm"):
        for a, b in zip(runs["adam"][:3], runs[how][:3]):
            osup.same_bits(a, b, how)
        assert runs[how][3] == runs["adam"][3] == 3


@pytest.mark.parametrize("clip,decay", [(True, 0.0), (False, 0.01), (True, 0.01)], ids=["clip", "decay", "clip_and_decay"])
@pytest.mark.parametrize("shape,wset", [(SHAPES[0], "live"), (SHAPES[1], "synthetic")], ids=["12x8-live", "16x12-synthetic"])
def test_clipping_and_decay_match_the_float64_restatement(cuda, shape, wset, clip, decay):
    """Three steps; the weights stay within 1e-6 |want| + 1e-9 of the restatement fed with the trainer's own gradients (the bound of
    tests/test_gpu_train.py's Adam test), the reported rate is clip / norm to an ulp and the gradient table is left as it was."""
    w, h, ch = shape
    wts, frames = _case(shape, wset)
    with PredNetTrainer(wts, ch, w, h, 2, 4, weight_decay=decay, **HYPER) as tr:
        p = tr.weights()
        m, v = ({k: np.zeros(a.shape) for k, a in p.items()} for _ in range(2))
        for step in (1, 2, 3):
            tr.forward_backward(frames)
            g = tr.grads()
            norm, _ = tr.grad_norms()
            assert norm > 0
            tr.clip_norm = 0.5 * norm if clip else None
            tr.adam()
            up = tr.last_update
            assert up["applied"] == 1 and up["norm"] == norm
            want_rate = tr.clip_norm / norm if clip else 1.0
            assert abs(up["rate"] - want_rate) <= np.spacing(want_rate), (up["rate"], want_rate)
            osup.same_bits(g, tr.grads(), "the step changed the gradient table")
            want, rate, _ = osup.adam_ex_ref(p, m, v, g, step, clip_norm=tr.clip_norm, weight_decay=decay, **HYPER)
            assert abs(rate - want_rate) <= 1e-12
            got = tr.weights()
            for k in p:
                err = np.abs(got[k] - want[k])
                assert (err <= 1e-6 * np.abs(want[k]) + 1e-9).all(), (k, step, err.max())
            p = got
        assert tr.state_dict()["adam_t"] == 3


# where the NaN goes.  A NaN in ConvP0/b does not reach the loss or the gradient in this build: the ConvP activation is
# fminf(fmaxf(v, 0), 1) (tpact_fwd_kernel), which maps NaN to 0, and every error unit is an fmaxf(., 0) likewise, so the forward
# pass above a NaN is finite and so is every loss.  A NaN in a ConvLSTM bias stays in that layer's gates, and the ConvLSTM backward
# multiplies by the gates (tlstm_bwd_kernel), so every gradient behind it is NaN: that is the non-finite step to leave out.
# Measured on MI355X with the live weights, B = 2, T = 4: NaN in ConvP0/b at 12x8 gray, loss 0.2168 and global norm 0.0 under the squared
# error, 0.2263 and 0.0278 under L_all, no tensor norm non-finite (16x12 colour: 0.1383 / 0.1026, none of 63); NaN in ConvLSTM0/h_i/b,
# loss 0.2168 (finite) and 39 of 40 tensor norms NaN (colour: 62 of 63).  So the norm is NaN and the loss is not: no loss of this build is.
NAN_TENSOR = "ConvLSTM0/h_i/b"


def test_a_step_whose_norm_is_not_finite_is_left_out_on_request(cuda):
    shape = SHAPES[0]
    w, h, ch = shape
    wts, frames = _case(shape)
    with PredNetTrainer(wts, ch, w, h, 2, 4, skip_nonfinite=True, **HYPER) as tr:
        tr.step(frames)
        assert tr.last_update["applied"] == 1 and np.isfinite(tr.last_update["norm"]) and tr.last_update["rate"] == 1.0
        state = tr.state_dict()
        assert state["adam_t"] == 1 and any(a.any() for a in state["adam_m"].values())
        bad = {k: a.copy() for k, a in tr.weights().items()}
        bad[NAN_TENSOR].ravel()[0] = np.nan
        tr.set_weights(bad)          # clears the moments: the saved ones go back in, so that "untouched" is not "still zero"
        tr.load_state_dict(state)
        assert tr.skip_nonfinite is True
        tr.forward_backward(frames)
        norm, per = tr.grad_norms()
        print("NaN in %s: global norm %r, %d of %d tensor norms not finite" % (NAN_TENSOR, norm, sum(not np.isfinite(x) for x in per.values()), len(per)))
        assert np.isnan(norm)
        before = (tr.weights(),) + _moments(tr)
        tr.adam()
        assert tr.last_update["applied"] == 0 and np.isnan(tr.last_update["norm"])
        after = (tr.weights(),) + _moments(tr)
        for a, b in zip(before[:3], after[:3]):
            osup.same_bits(a, b, "a skipped step")
        assert before[3] == after[3] == 1
        # without the request the step is applied, as eigen_trainer_adam applies it
        tr.skip_nonfinite, tr.weight_decay = False, 0.01
        tr.adam()
        assert tr.last_update["applied"] == 1 and np.isnan(tr.last_update["norm"]) and tr.last_update["rate"] == 1.0
        assert tr.state_dict()["adam_t"] == 2
        assert any(np.isnan(a).any() for k, a in tr.weights().items() if k != NAN_TENSOR)


def test_accumulate_clear_add_load(cuda):
    w, h, ch = osup.WIDE
    wts, frames = _case(osup.WIDE, B=3)
    other = _drifting(9, 3, 4, ch[0], h, w)
    with PredNetTrainer(wts, ch, w, h, 3, 4) as tr:
        # nothing accumulated: LOAD is a call-order error, before and after a CLEAR
        assert osup.accumulate_raw(tr, train.ACC_LOAD) == -3
        assert osup.accumulate_raw(tr, train.ACC_CLEAR) == 0 and osup.accumulate_raw(tr, train.ACC_LOAD) == -3
        with pytest.raises(EngineError):
            tr.load_accumulated()
        tr.forward_backward(frames)
        g = tr.grads()
        assert sum(a.any() for a in g.values()) > len(g) // 2
        tr.clear_accumulated()
        tr.accumulate(1.0)
        tr.forward_backward(other)      # overwrites the gradient table; the accumulator keeps the first gradient
        g2 = tr.grads()
        assert any(not np.array_equal(g[k], g2[k]) for k in g)
        tr.load_accumulated()
        back = tr.grads()
        for k in g:
            assert np.array_equal(back[k], g[k]), k      # as values: 0 + (-0) is +0
        tr.load_accumulated()                            # LOAD keeps the accumulator
        osup.same_bits(back, tr.grads())
        # two halves of the same gradient are the gradient, bit for bit away from zeros
        tr.clear_accumulated()
        tr.accumulate(0.5)
        tr.accumulate(0.5)
        tr.forward_backward(other)
        tr.load_accumulated()
        twice = tr.grads()
        for k in g:
            nz = g[k] != 0
            assert np.array_equal(twice[k], g[k]) and np.array_equal(twice[k][nz].view(np.uint32), g[k][nz].view(np.uint32)), k
        # two gradients under two scales: the float32 restatement, bit for bit
        tr.clear_accumulated()
        tr.forward_backward(frames)
        tr.accumulate(0.25)
        tr.forward_backward(other)
        tr.accumulate(0.7)
        tr.load_accumulated()
        mixed = tr.grads()
        for k in g:
            want = osup.axpy_ref(osup.axpy_ref(np.zeros_like(g[k]), g[k], 0.25), g2[k], 0.7)
            assert np.array_equal(mixed[k].view(np.uint32), want.view(np.uint32)), k
        tape = tr.tape_bytes
        # set_weights discards what was accumulated
        tr.set_weights(wts)
        assert osup.accumulate_raw(tr, train.ACC_LOAD) == -3
    with PredNetTrainer(wts, ch, w, h, 3, 4) as fresh:
        assert fresh.tape_bytes == tape      # the accumulator is not counted


def test_refusals_launch_nothing(cuda):
    w, h, ch = SHAPES[0]
    wts, frames = _case(SHAPES[0])
    with PredNetTrainer(wts, ch, w, h, 2, 4, **HYPER) as tr:
        tr.step(frames)
        before = (tr.weights(), tr.grads()) + _moments(tr)
        nan, inf = float("nan"), float("inf")
        assert osup.adam_ex_raw(tr, settings=False)[0] == -1
        for kw in (dict(weight_decay=-1e-3), dict(weight_decay=nan), dict(weight_decay=inf), dict(clip_norm=-1.0), dict(clip_norm=nan), dict(clip_norm=inf),
                   dict(reserved=1), dict(skip_nonfinite=2)):
            assert osup.adam_ex_raw(tr, report=True, **kw)[0] == -1, kw
        for bad in (dict(alpha=0.0), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=0.0)):
            cfg = train.AdamSettings(*[bad.get(k, HYPER[k]) for k in train.HYPER], 0.01, 0.0, 0, 0)
            assert tr.lib.eigen_trainer_adam_ex(tr._h, ctypes.byref(cfg), None, None) == -1, bad
        assert tr.lib.eigen_trainer_adam_ex(None, None, None, None) == -1
        for op, scale in ((3, 1.0), (-1, 1.0), (train.ACC_ADD, nan), (train.ACC_ADD, inf), (train.ACC_CLEAR, nan)):
            assert osup.accumulate_raw(tr, op, scale) == -1, (op, scale)
        assert tr.lib.eigen_trainer_accumulate(None, ctypes.c_int32(0), ctypes.c_double(1.0), None) == -1
        for n in (0, len(tr._names) - 1, len(tr._names) + 1):
            assert tr.lib.eigen_trainer_grad_norms(tr._h, None, None, n, None) == -1
        assert tr.lib.eigen_trainer_grad_norms(None, None, None, len(tr._names), None) == -1
        with pytest.raises(ValueError):
            tr.accumulate(nan)
        for a, b in zip(before[:4], (tr.weights(), tr.grads()) + _moments(tr)[:2]):
            osup.same_bits(a, b)
        assert tr.state_dict()["adam_t"] == before[4] == 1
        assert osup.accumulate_raw(tr, train.ACC_LOAD) == -3    # none of the refused ADDs accumulated anything
        # step()'s own rules, raised before anything runs
        four = _drifting(3, 4, 4, ch[0], h, w)
        for kw in (dict(micro_batches=3), dict(micro_batches=2, reset=False), dict(micro_batches=0), dict(micro_batches=True)):
            with pytest.raises(ValueError):
                tr.step(four, **kw)
        with pytest.raises(ValueError):
            tr.step(np.concatenate([four, four]), micro_batches=2)      # chunks of 4 on a handle of 2
        assert tr.state_dict()["adam_t"] == 1


@pytest.mark.parametrize("objective,lam", [("mse", None), ("error", "lall")], ids=["mse", "error_lall"])
@pytest.mark.parametrize("shape,wset", [(SHAPES[0], "live"), (SHAPES[1], "synthetic")], ids=["12x8-live", "16x12-synthetic"])
def test_micro_batches_give_the_gradient_of_the_whole_batch(cuda, shape, wset, objective, lam):
    """A handle of batch 2 on 4 sequences in two chunks: the accumulated gradient is held to the float64 reference of the batch of 4
    by the rule of a direct call (`_check_grads`), the loss to that file's 1e-5; runs repeat bit for bit."""
    from oracle import prednet_train_ref
    w, h, ch = shape
    wts, frames = _case(shape, wset, B=4, seed=21)
    lam = None if lam is None else [1.0] + [0.1] * (len(ch) - 1)
    kw = dict(objective=objective, layer_weights=lam)
    r = prednet_train_ref.run(wts, ch, frames, **kw)
    with PredNetTrainer(wts, ch, w, h, 2, 4, **HYPER) as tr:
        loss = tr.accumulate_micro_batches(frames, 2, **kw)
        tr.load_accumulated()
        got = tr.grads()
        tr.adam()
        by_hand = tr.weights()
    worst = _check_grads(got, r.grads, what="%s %s micro_batches=2" % (shape_id(shape), objective))
    print("%s %s: loss %.9g against %.9g; gradient error / bound %.4f in norm, %.4f element-wise" % (shape_id(shape), objective, loss, r.loss, worst[0], worst[1]))
    assert abs(loss - r.loss) <= 1e-5 * r.loss, (loss, r.loss)
    runs = []
    for _ in range(2):
        with PredNetTrainer(wts, ch, w, h, 2, 4, **HYPER) as tr:
            assert tr.step(frames, micro_batches=2, **kw) == loss
            runs.append(tr.weights())
            assert tr.state_dict()["adam_t"] == 1
    osup.same_bits(runs[0], runs[1])
    osup.same_bits(runs[0], by_hand)
    assert any(not np.array_equal(runs[0][k], wts[k]) for k in wts)


def test_a_resumed_run_with_settings_gives_the_uninterrupted_bits(cuda, tmp_path):
    shape = SHAPES[1]
    w, h, ch = shape
    wts, _ = _case(shape)
    batches = [_drifting(30 + i, 2, 4, ch[0], h, w) for i in range(6)]
    with PredNetTrainer(wts, ch, w, h, 2, 4) as probe:
        probe.forward_backward(batches[0])
        clip = 0.5 * probe.grad_norms()[0]
    settings = dict(clip_norm=clip, weight_decay=0.01, skip_nonfinite=True, **HYPER)
    with PredNetTrainer(wts, ch, w, h, 2, 4, **settings) as tr:
        rates = []
        for b in batches:
            tr.step(b)
            rates.append(tr.last_update["rate"])
        whole = (tr.weights(),) + _moments(tr)
    assert rates[0] == 0.5 and all(0 < r <= 1 for r in rates)
    path = str(tmp_path / "ckpt.npz")
    with PredNetTrainer(wts, ch, w, h, 2, 4, **settings) as tr:
        for b in batches[:3]:
            tr.step(b)
        tr.save_checkpoint(path)
    with np.load(path) as z:
        assert {"optim/" + k for k in train.OPTIM} <= set(z.files)
    with PredNetTrainer("synthetic", ch, w, h, 2, 4) as tr:     # other weights, default hyper-parameters, neutral controls: all come from the file
        tr.load_checkpoint(path)
        assert (tr.clip_norm, tr.weight_decay, tr.skip_nonfinite) == (clip, 0.01, True)
        for b in batches[3:]:
            tr.step(b)
        resumed = (tr.weights(),) + _moments(tr)
    for a, b in zip(whole[:3], resumed[:3]):
        osup.same_bits(a, b)
    assert whole[3] == resumed[3] == 6
    # a checkpoint of a neutral trainer has no optim entry and loads as neutral, whatever the trainer held
    with PredNetTrainer(wts, ch, w, h, 2, 4) as tr:
        tr.step(batches[0])
        tr.save_checkpoint(path)
    with np.load(path) as z:
        assert not [k for k in z.files if k.startswith("optim/")]
    with PredNetTrainer(wts, ch, w, h, 2, 4, **settings) as tr:
        tr.load_checkpoint(path)
        assert (tr.clip_norm, tr.weight_decay, tr.skip_nonfinite) == (None, 0.0, False)
