"""Shared by the training tests.  For tests/test_gpu_train*.py and tests/test_train_reference_host.py: shapes, frame and weight
generators, the gradient bound and two raw C-ABI callers (the float64 reference itself is oracle/prednet_train_ref.py).  For
tests/test_train*_host.py: the one list of training kernels and the one check of their register metadata."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import weights
from tests import test_isa_stats as isa

# (w, h, channels): 2, 3 and 4 layers, gray and colour, none square
SHAPES = [(12, 8, [1, 4]), (16, 12, [3, 4, 6]), (24, 16, [1, 3, 4, 5])]


def _drifting(seed, n, T, c, h, w, speed=1):
    """n sequences of T frames: a smooth texture shifted by `speed` pixels per frame, each sequence in its own direction."""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * speed * T, w + 2 * speed * T
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, T, c, h, w), np.uint8)
    for i in range(n):
        tex = np.zeros((c, H, W))
        for ch in range(c):
            for _ in range(3):
                fy, fx, ph = rng.uniform(0.1, 0.6), rng.uniform(0.1, 0.6), rng.uniform(0, 2 * np.pi)
                tex[ch] += np.sin(fy * yy + fx * xx + ph)
        tex = np.clip(128 + 40 * tex, 0, 255)
        dy, dx = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1)][rng.integers(6)]
        for t in range(T):
            y0, x0 = speed * T + dy * speed * t, speed * T + dx * speed * t
            out[i, t] = tex[:, y0:y0 + h, x0:x0 + w].astype(np.uint8)
    return out


def _random_weights(ch, w, h, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for k, shp in weights.tensor_shapes(ch, w, h).items():
        fan = shp[1] * 9 if len(shp) == 4 and "/c_" not in k else 1
        out[k] = (rng.normal(0, 0.8 / np.sqrt(fan), shp) if fan > 1 else rng.normal(0, 0.3, shp)).astype(np.float32)
    return out


def _weight_sets(ch, w, h):
    return [("synthetic", weights.synthetic_prednet_weights(ch, w, h, seed=1)), ("random", _random_weights(ch, w, h, seed=2))]


def _check_grads(got, ref):
    G = np.sqrt(sum(float((r ** 2).sum()) for r in ref.values()))
    for k, r in ref.items():
        err = np.linalg.norm((got[k].astype(np.float64) - r).ravel())
        assert err <= 1e-3 * np.linalg.norm(r.ravel()) + 1e-6 * G, (k, err, np.linalg.norm(r.ravel()), G)


def _grads_differ(a, b):
    """True when b misses a by more than _check_grads allows on at least one tensor"""
    try:
        _check_grads(b, a)
    except AssertionError:
        return True
    return False


def _same_weights(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _q(v):
    """The byte the inference engine emits for a float32 prediction, over 255: the statement of EPI_CONVP / e0_resume_kernel
    (csrc/conv_mfma.h) and of terr_fed_fwd_kernel, `(float)(uint8_t)(int)(v * 255.0f) / 255.0f`, in float32."""
    v = np.asarray(v, np.float32)
    return (v * np.float32(255.0)).astype(np.int32).astype(np.uint8).astype(np.float32) / np.float32(255.0)


def _fed_from(pred):
    """fed[:, t] = q(pred[:, t - 1]): the constants a requantised self-fed step t reads, from float32 predictions"""
    fed = np.zeros_like(pred, dtype=np.float32)
    fed[:, 1:] = _q(pred[:, :-1])
    return fed


def _loss_grad_obj_loss(tr, frames, n_fed, requant, sw, lam):
    """the loss eigen_trainer_loss_grad_obj itself returns under EIGEN_OBJ_ERROR (train.py forms its own from the table)"""
    d = torch.from_numpy(frames).cuda()
    B, T = frames.shape[:2]
    loss = ctypes.c_double()
    w_arr = None if sw is None else np.ascontiguousarray(sw, np.float64)
    l_arr = np.ascontiguousarray(lam, np.float64)
    rc = tr.lib.eigen_trainer_loss_grad_obj(tr._h, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(T * frames[0, 0].size), B, T, T if n_fed is None else n_fed,
                                            int(requant), 1, ctypes.c_void_p(None if w_arr is None else w_arr.ctypes.data), 1,
                                            ctypes.c_void_p(l_arr.ctypes.data), ctypes.byref(loss), None, None, None)
    assert rc == 0
    return loss.value


def _loss_grad_ext(tr, d, n_fed, requant, sw):
    """eigen_trainer_loss_grad_ext called directly: (loss, {name: grad})"""
    B, T = int(d.shape[0]), int(d.shape[1])
    loss = ctypes.c_double()
    w_arr = None if sw is None else np.ascontiguousarray(sw, np.float64)
    rc = tr.lib.eigen_trainer_loss_grad_ext(tr._h, ctypes.c_void_p(d.data_ptr()), ctypes.c_int64(T * int(np.prod(d.shape[2:]))), B, T, n_fed, int(requant), 1,
                                            ctypes.c_void_p(None if w_arr is None else w_arr.ctypes.data), ctypes.byref(loss), None, None)
    assert rc == 0
    return loss.value, tr.grads()


# ---- host side: every __global__ of csrc/train_kernels.h (tests/test_train_ext_host.py checks the list against the header), as the
# kernels one teacher-forced gradient step and Adam launch, then those of self-fed steps and the per-step reductions
GRADIENT_KERNELS = ["tconv3x3_kernel", "twgrad_kernel", "tsum_slabs_kernel", "tbias_grad_kernel", "terr_fwd_kernel", "terr_bwd_kernel",
                    "tlstm_fwd_kernel", "tlstm_bwd_kernel", "tpeep_grad_kernel", "tpact_fwd_kernel", "tpact_bwd_kernel",
                    "tloss_partial_kernel", "tloss_final_kernel", "tadam_kernel"]
STEP_KERNELS = ["terr_fed_fwd_kernel", "tloss_step_partial_kernel", "tloss_step_final_kernel"]
TRAIN_KERNELS = GRADIENT_KERNELS + STEP_KERNELS
# kernel -> the template arguments the library must hold an instantiation of: the seeds of the two backward kernels, the three
# terms of the per-step reduction (squared error, image-layer error units, a plain sum over an E tape)
TEMPLATED = {"tpact_bwd_kernel": (0, 1), "terr_bwd_kernel": (0, 1), "tloss_step_partial_kernel": (0, 1, 2)}


@functools.lru_cache(maxsize=None)
def _kernel_stats():
    """the register metadata of the built library, read once, as tests/test_isa_stats.py reads it"""
    return isa._kernel_stats()


def check_no_scratch_and_no_spills(kernel):
    """every instantiation of `kernel` in the library, those TEMPLATED names among them, has no scratch and no spills"""
    if not os.path.exists(isa.LIB):
        pytest.skip("libeigen_hip.so not built")
    if not os.path.exists(isa.READELF):
        pytest.skip("llvm-readelf not found")
    stats = _kernel_stats()
    names = [n for n in stats if re.match(r"_ZN4eigt\d+%s" % kernel, n)]
    assert names, "%s not in the library" % kernel
    for arg in TEMPLATED.get(kernel, ()):
        assert any(re.match(r"_ZN4eigt\d+%sILi%dEE" % (kernel, arg), n) for n in names), "%s<%d> not in the library: %s" % (kernel, arg, names)
    for n in names:
        for s in stats[n]:
            assert s["private_segment_fixed_size"] == 0, (n, s)
            assert s["vgpr_spill_count"] == 0, (n, s)
            assert s["sgpr_spill_count"] == 0, (n, s)
