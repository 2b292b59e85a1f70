"""CPU: the optimiser controls of the trainer ("Optimiser controls") as far as they can be checked without a
GPU: the C ABI's new entries and structs, the kernels' register metadata, the argument rules, the checkpoint layout, the properties of
the float64 restatement the GPU tests compare against, and why 1 / k is the scale of a micro-batch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import engine, train
from tests import optim_support as osup
from tests.train_support import SHAPES, _drifting, _live_weights, check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")


def test_header_exports_and_abi():
    import __graft_entry__ as ge
    ge.build()
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    lib = engine.load_library()
    for name in osup.ENTRIES:
        assert name in declared and name in engine.EXPORTS and hasattr(lib, name), name
    assert engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header and lib.eigen_abi_version() == 4
    assert ctypes.sizeof(train.AdamSettings) == 56 and ctypes.sizeof(train.AdamReport) == 24
    for struct, cls in (("eigen_adam_settings", train.AdamSettings), ("eigen_adam_report", train.AdamReport)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header).group(1)
        fields = re.findall(r"\b(double|int32_t)\s+([^;]+);", body)
        names = [n.strip() for _, group in fields for n in group.split(",")]
        assert names == [n for n, _ in cls._fields_], struct
    assert "EIGEN_ACC_CLEAR = 0, EIGEN_ACC_ADD = 1, EIGEN_ACC_LOAD = 2" in header
    assert (train.ACC_CLEAR, train.ACC_ADD, train.ACC_LOAD) == (0, 1, 2)
    # the header says that a gradient that is not finite is applied unless the caller asks otherwise
    assert "WITHOUT skip_nonfinite A GRADIENT THAT IS NOT FINITE IS APPLIED" in header
    train._bind(lib)
    args = lambda name: [a.strip() for a in re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).replace("\n", " ").split(",")]
    for name in osup.ENTRIES:
        assert len(getattr(lib, name).argtypes) == len(args(name)), name


def test_the_kernels_live_in_their_own_header():
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    text = open(os.path.join(CSRC, "optim_kernels.h")).read()
    assert set(re.findall(pat, text)) == set(osup.OPTIM_KERNELS)
    assert '#include "optim_kernels.h"' in open(os.path.join(CSRC, "prednet_train.hip")).read()
    assert re.search(r"NORM_SLICES\s*=\s*%d\b" % osup.NORM_SLICES, text) and re.search(r"EW_T\s*=\s*%d\b" % osup.NORM_THREADS,
                                                                                      open(os.path.join(CSRC, "train_common.h")).read())
    assert "atomic" not in text.replace("no atomics", "")
    osup.check_shape_properties()


@pytest.mark.parametrize("kernel", osup.OPTIM_KERNELS)
def test_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)


def test_check_optim():
    assert train.check_optim() == (None, 0.0, False) and train.optim_is_neutral(*train.check_optim())
    assert train.check_optim(2, 1, True) == (2.0, 1.0, True)
    assert train.check_optim(clip_norm=np.float32(0.5), weight_decay=np.float64(0.01)) == (0.5, 0.01, False)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), True, "1", [1.0]):
        with pytest.raises(ValueError):
            train.check_optim(clip_norm=bad)
    for bad in (-1e-9, float("nan"), float("inf"), None, False, "0"):
        with pytest.raises(ValueError):
            train.check_optim(weight_decay=bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError):
            train.check_optim(skip_nonfinite=bad)
    for settings in ((1.0, 0.0, False), (None, 1e-4, False), (None, 0.0, True)):
        assert not train.optim_is_neutral(*train.check_optim(*settings))
    # new constructor arguments follow `device`: a positional call means what it meant
    params = list(inspect.signature(train.PredNetTrainer.__init__).parameters)
    assert params[params.index("device"):] == ["device", "clip_norm", "weight_decay", "skip_nonfinite"]
    defaults = inspect.signature(train.PredNetTrainer.__init__).parameters
    assert (defaults["clip_norm"].default, defaults["weight_decay"].default, defaults["skip_nonfinite"].default) == (None, 0.0, False)


def test_micro_batch_rules():
    st = inspect.signature(train.PredNetTrainer.step).parameters
    assert st["micro_batches"].default == 1
    assert train.check_micro_batches(4, 1, 2) == 4      # one chunk: the capacity rule is the library's, as it was
    assert train.check_micro_batches(4, 2, 2) == 2 and train.check_micro_batches(6, 3, 8) == 2 and train.check_micro_batches(4, np.int64(4), 1) == 1
    for n, k, batch in ((5, 2, 8), (4, 3, 8), (8, 2, 3)):
        with pytest.raises(ValueError):
            train.check_micro_batches(n, k, batch)
    for k in (0, -1, 1.5, 2.0, True, None, "2"):
        with pytest.raises(ValueError):
            train.check_micro_batches(4, k, 4)
    with pytest.raises(ValueError):
        train.check_micro_batches(4, 2, 2, reset=False)
    assert train.check_micro_batches(4, 1, 4, reset=False) == 4
    score = train.FlowScore()
    shared = train.FlowObjective(mask=np.ones((8, 12), np.uint8), score=score)
    per_sample = train.FlowObjective(mask=np.ones((4, 8, 12), np.uint8), score=score)
    assert train.check_micro_batches(4, 2, 2, flow=shared) == 2 and train.check_micro_batches(4, 1, 4, flow=per_sample) == 4
    with pytest.raises(ValueError):
        train.check_micro_batches(4, 2, 2, flow=per_sample)


def _state(w, h, ch, seed=0, **extra):
    rng = np.random.default_rng(seed)
    shapes = train.tensor_shapes(ch, w, h)
    tab = lambda: {k: rng.normal(size=s).astype(np.float32) for k, s in shapes.items()}
    return tab(), dict({"adam_m": tab(), "adam_v": tab(), "adam_t": 3, "hyper": {"alpha": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8}, "seq": None}, **extra)


def test_checkpoint_layout(tmp_path):
    w, h, ch = SHAPES[0]
    wts, plain = _state(w, h, ch)
    names = list(wts)
    old_keys = set(["predictor/" + n for n in names] + ["adam/m/" + n for n in names] + ["adam/v/" + n for n in names] + ["adam/t"] + ["hyper/" + k for k in train.HYPER])

    def keys_of(state, name):
        path = str(tmp_path / name)
        train.write_checkpoint(path, wts, state)
        with np.load(path) as z:
            return path, set(z.files)

    # a state without the key (what an earlier trainer wrote), and one whose settings are all neutral: the same file layout
    p_old, k_old = keys_of(plain, "old.npz")
    _, k_neutral = keys_of(dict(plain, optim={"clip_norm": None, "weight_decay": 0.0, "skip_nonfinite": False}), "neutral.npz")
    assert k_old == k_neutral == old_keys
    _, st = train.read_checkpoint(p_old, ch, w, h)
    assert "optim" not in st and sorted(st) == ["adam_m", "adam_t", "adam_v", "hyper", "seq"]
    # settings that are not neutral travel and come back as they were
    for optim in ({"clip_norm": 0.75, "weight_decay": 0.0, "skip_nonfinite": False}, {"clip_norm": None, "weight_decay": 0.01, "skip_nonfinite": False},
                  {"clip_norm": None, "weight_decay": 0.0, "skip_nonfinite": True}, {"clip_norm": 1e-3, "weight_decay": 0.5, "skip_nonfinite": True}):
        path, keys = keys_of(dict(plain, optim=optim), "set.npz")
        assert keys == old_keys | {"optim/" + k for k in train.OPTIM}
        got_w, got = train.read_checkpoint(path, ch, w, h)
        assert got["optim"] == optim and got["hyper"] == plain["hyper"] and got["adam_t"] == 3
        for n in names:
            assert np.array_equal(got_w[n], wts[n]) and np.array_equal(got["adam_m"][n], plain["adam_m"][n]) and np.array_equal(got["adam_v"][n], plain["adam_v"][n])
    for bad in ({"clip_norm": -1.0}, {"weight_decay": float("nan")}, {"skip_nonfinite": 2}, {"momentum": 0.9}):
        with pytest.raises(ValueError):
            train.check_state(dict(plain, optim=bad), ch, w, h)
    assert train.check_state(dict(plain, optim={"weight_decay": 0.1}), ch, w, h)["optim"] == {"clip_norm": None, "weight_decay": 0.1, "skip_nonfinite": False}


def _tables(seed, shapes, scale=1.0):
    rng = np.random.default_rng(seed)
    return {k: (scale * rng.normal(size=s)).astype(np.float32) for k, s in shapes.items()}


def test_restatement_properties():
    w, h, ch = SHAPES[1]
    shapes = train.tensor_shapes(ch, w, h)
    p, g = _tables(1, shapes), _tables(2, shapes, 0.1)
    hyper = (2e-3, 0.9, 0.999, 1e-8)
    n = sum(a.size for a in g.values())
    # neutral settings: the plain rule bit for bit, over three steps
    m0, v0, m1, v1 = ({k: np.zeros(s) for k, s in shapes.items()} for _ in range(4))
    pa, pb = p, p
    for step in (1, 2, 3):
        pa = osup.adam_ref(pa, m0, v0, g, step, *hyper)
        pb, rate, gc = osup.adam_ex_ref(pb, m1, v1, g, step, *hyper)
        assert rate == 1.0
        for k in p:
            assert np.array_equal(pa[k], pb[k]) and np.array_equal(m0[k], m1[k]) and np.array_equal(v0[k], v1[k]) and np.array_equal(gc[k], g[k].astype(np.float64))
    # clip < norm: the clipped table has norm clip
    norm, per = osup.norm_ref(g)
    assert norm > 0 and all(v > 0 for v in per.values())
    for clip in (0.5 * norm, 1e-3 * norm, float(np.nextafter(norm, 0))):
        _, rate, gc = osup.adam_ex_ref(p, {k: np.zeros(s) for k, s in shapes.items()}, {k: np.zeros(s) for k, s in shapes.items()}, g, 1, *hyper, clip_norm=clip)
        assert rate == clip / norm < 1
        got, _ = osup.norm_ref(gc)
        assert abs(got - clip) <= n * 2.0 ** -52 * clip, (got, clip)
    # clip >= norm, no clip, a zero gradient, a norm that is not a number: rate 1, nothing divides
    zero = {k: np.zeros(s, np.float32) for k, s in shapes.items()}
    assert osup.clip_rate(norm, norm) == 1.0 and osup.clip_rate(norm, 2 * norm) == 1.0 and osup.clip_rate(norm, None) == 1.0
    assert osup.clip_rate(0.0, 1.0) == 1.0 and osup.clip_rate(float("nan"), 1.0) == 1.0
    with np.errstate(all="raise"):
        pz, rate, gc = osup.adam_ex_ref(p, {k: np.zeros(s) for k, s in shapes.items()}, {k: np.zeros(s) for k, s in shapes.items()}, zero, 1, *hyper, clip_norm=1.0)
    assert rate == 1.0 and all(not a.any() for a in gc.values()) and all(np.array_equal(pz[k], p[k].astype(np.float64)) for k in p)
    # decay alone: p - wd p on a zero gradient
    pz, _, _ = osup.adam_ex_ref(p, {k: np.zeros(s) for k, s in shapes.items()}, {k: np.zeros(s) for k, s in shapes.items()}, zero, 1, *hyper, weight_decay=0.01)
    assert all(np.array_equal(pz[k], p[k].astype(np.float64) - (0.0 + 0.01 * p[k].astype(np.float64))) for k in p)
    # the accumulator's arithmetic: from zero, 1.0 g is g as values and two halves are g bit for bit away from zeros
    for k in g:
        z = np.zeros_like(g[k])
        assert np.array_equal(osup.axpy_ref(z, g[k], 1.0), g[k])
        assert np.array_equal(osup.axpy_ref(osup.axpy_ref(z, g[k], 0.5), g[k], 0.5).view(np.uint32), g[k].view(np.uint32))


@pytest.mark.parametrize("objective,lam", [("mse", None), ("error", [1.0, 0.1])])
def test_the_mean_of_the_halves_is_the_gradient_of_the_batch(objective, lam):
    """Why step(micro_batches=k) accumulates with scale 1 / k: every objective is a mean over the samples, so the mean of the gradients
    of k equal chunks is the gradient of the whole batch.  The float64 reference alone, B = 4 against 2 + 2: the same terms in
    another order, so equal within 1e-12 of each tensor's norm; the losses likewise."""
    from oracle import prednet_train_ref
    w, h, ch = SHAPES[0]
    B, T = 4, 4
    frames, wts = _drifting(21, B, T, ch[0], h, w), _live_weights(ch, w, h)
    kw = dict(objective=objective, layer_weights=lam)
    full = prednet_train_ref.run(wts, ch, frames, **kw)
    halves = [prednet_train_ref.run(wts, ch, frames[j:j + 2], **kw) for j in (0, 2)]
    assert abs((halves[0].loss + halves[1].loss) / 2 - full.loss) <= 1e-12 * abs(full.loss)
    for k, r in full.grads.items():
        r = np.asarray(r, np.float64)
        mean = (np.asarray(halves[0].grads[k], np.float64) + np.asarray(halves[1].grads[k], np.float64)) / 2
        nr = float(np.linalg.norm(r.ravel()))
        assert nr > 0, k
        assert float(np.linalg.norm((mean - r).ravel())) <= 1e-12 * nr, (k, float(np.linalg.norm((mean - r).ravel())), nr)
