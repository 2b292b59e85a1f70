"""CPU: the host side of self-fed training, tape-free evaluation and trainer state -- the register metadata
of their kernels, the kernel list of tests/train_support.py against the header, and the checkpoint npz layout."""
import os
import re

import numpy as np
import pytest

from tests.train_support import GRADIENT_KERNELS, STEP_KERNELS, TEMPLATED, TRAIN_KERNELS, check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_kernel_lists_name_every_global_of_the_header():
    src = open(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc", "train_kernels.h")).read()
    found = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\(", src))
    assert found == set(TRAIN_KERNELS), found ^ set(TRAIN_KERNELS)
    assert len(TRAIN_KERNELS) == len(found) and not set(GRADIENT_KERNELS) & set(STEP_KERNELS) and set(TEMPLATED) <= found


@pytest.mark.parametrize("kernel", STEP_KERNELS)
def test_new_training_kernels_have_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)


def _state(ch, w, h, seed, batch=None):
    from evolutionary_illusion_generator_amd import train, weights
    rng = np.random.default_rng(seed)
    shapes = weights.tensor_shapes(ch, w, h)
    st = {"adam_m": {k: rng.normal(0, 1e-3, s).astype(np.float32) for k, s in shapes.items()},
          "adam_v": {k: rng.uniform(0, 1e-6, s).astype(np.float32) for k, s in shapes.items()},
          "adam_t": 17, "hyper": {"alpha": 2e-3, "beta1": 0.85, "beta2": 0.99, "eps": 1e-7}, "seq": None}
    if batch:
        st["seq"] = {k: [rng.normal(0, 1, s).astype(np.float32) for s in train.seq_state_shapes(ch, w, h, batch)] for k in train.SEQ_PARTS}
    return st


@pytest.mark.parametrize("batch", [None, 3])
def test_checkpoint_npz_round_trips_and_is_still_a_chainer_model_file(tmp_path, batch):
    from evolutionary_illusion_generator_amd import train, weights
    ch, w, h = [3, 4, 6], 16, 12
    wt = weights.synthetic_prednet_weights(ch, w, h, seed=3)
    st = _state(ch, w, h, 5, batch)
    path = str(tmp_path / "ckpt.npz")
    train.write_checkpoint(path, wt, st)
    assert os.path.exists(path)
    with np.load(path) as z:
        want = ["predictor/" + k for k in wt] + ["adam/m/" + k for k in wt] + ["adam/v/" + k for k in wt] + ["adam/t"]
        want += ["hyper/" + k for k in train.HYPER]
        if batch:
            want += ["seq/%s/%d" % (p, l) for p in train.SEQ_PARTS for l in range(len(ch))]
        assert sorted(z.files) == sorted(want)
    back = weights.load_chainer_npz(path, ch, w, h)
    for k in wt:
        assert np.array_equal(back[k], wt[k]), k
    wt2, st2 = train.read_checkpoint(path, ch, w, h)
    for k in wt:
        assert np.array_equal(wt2[k], wt[k]) and wt2[k].dtype == np.float32
        assert np.array_equal(st2["adam_m"][k], st["adam_m"][k]) and st2["adam_m"][k].dtype == np.float32
        assert np.array_equal(st2["adam_v"][k], st["adam_v"][k])
    assert st2["adam_t"] == 17 and st2["hyper"] == st["hyper"]
    if batch:
        for p in train.SEQ_PARTS:
            for a, b in zip(st["seq"][p], st2["seq"][p]):
                assert np.array_equal(a, b) and b.shape[0] == batch
    else:
        assert st2["seq"] is None


def test_checkpoint_shape_and_dtype_errors_are_value_errors(tmp_path):
    from evolutionary_illusion_generator_amd import train, weights
    ch, w, h = [1, 4], 12, 8
    wt = weights.synthetic_prednet_weights(ch, w, h, seed=1)
    good = _state(ch, w, h, 2, 2)
    train.check_state(good, ch, w, h, max_batch=2)
    with pytest.raises(ValueError):
        train.check_state(good, ch, w, h, max_batch=1)                      # the sequence state does not fit
    with pytest.raises(ValueError):
        train.check_state(dict(good, adam_t=-1), ch, w, h)
    bad = dict(good, adam_m=dict(good["adam_m"], **{"ConvP0/b": np.zeros(2, np.float32)}))
    with pytest.raises(ValueError):
        train.check_state(bad, ch, w, h)
    bad = dict(good, adam_v={k: v for k, v in good["adam_v"].items() if k != "ConvP0/b"})
    with pytest.raises(ValueError):
        train.check_state(bad, ch, w, h)
    bad = dict(good, adam_v={k: v.astype(np.int64) for k, v in good["adam_v"].items()})
    with pytest.raises(ValueError):
        train.check_state(bad, ch, w, h)
    bad = dict(good, seq=dict(good["seq"], c=good["seq"]["c"][:1]))
    with pytest.raises(ValueError):
        train.check_state(bad, ch, w, h)
    # a checkpoint of another network is refused when it is read
    path = str(tmp_path / "c.npz")
    train.write_checkpoint(path, wt, good)
    with pytest.raises(ValueError):
        train.read_checkpoint(path, [1, 5], w, h)
    weights.save_chainer_npz(wt, str(tmp_path / "plain.npz"))
    with pytest.raises(KeyError):
        train.read_checkpoint(str(tmp_path / "plain.npz"), ch, w, h)      # a model file without Adam state is no checkpoint
