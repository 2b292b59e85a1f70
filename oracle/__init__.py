"""CPU ORACLE of EIGen's fitness path -- TEST INFRASTRUCTURE, not product code.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import this
package (as the checker / reported baseline, never as the thing measured or shipped).  The product
package ``evolutionary_illusion_generator_amd`` never imports it.

Stages and what pins them:

============  =========================================  ==========================================
stage         restatement                                pinned by
============  =========================================  ==========================================
grids         ``oracle.grids`` (scalar, per pixel)       reference import -> tests/golden/grids.npz
post-process  ``oracle.cppn.postprocess``                reference import -> tests/golden/postprocess.npz
scorers       ``oracle.scores``                          reference import -> tests/golden/scores.json
orchestration ``oracle.pipeline``                        reference import -> tests/golden/orchestration.json
CPPN eval     ``oracle.cppn`` (PyTorch-NEAT semantics)   PARITY UNPINNED (submodule absent)
PredNet       ``oracle/eig_oracle.c`` + ``prednet_torch`` PARITY UNPINNED (submodule + chainer absent)
LK flow       ``oracle/eig_oracle.c``                    PARITY UNPINNED (submodule + OpenCV absent)
============  =========================================  ==========================================
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

GATES = ("i", "f", "c", "o")


def build(force=False):
    """Compile oracle/eig_oracle.c -> oracle/libeig_oracle.so (gcc, see oracle/Makefile)."""
    so = os.path.join(_HERE, "libeig_oracle.so")
    srcs = [os.path.join(_HERE, f) for f in ("eig_oracle.c", "farneback.c", "Makefile")]
    if force or not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-C", _HERE, "-s", "libeig_oracle.so"])
    return so


class LKParams(ctypes.Structure):
    """Parameters of Optical_Flow_Analyzer.lucas_kanade (OpenCV tutorial values, UPSTREAM-RECALL)."""
    _fields_ = [("max_corners", ctypes.c_int), ("quality_level", ctypes.c_double),
                ("min_distance", ctypes.c_double), ("block_size", ctypes.c_int),
                ("win", ctypes.c_int), ("max_level", ctypes.c_int), ("max_iter", ctypes.c_int),
                ("epsilon", ctypes.c_double), ("min_eig_thr", ctypes.c_double)]

    def __init__(self, max_corners=100, quality_level=0.3, min_distance=7.0, block_size=7, win=15,
                 max_level=2, max_iter=10, epsilon=0.03, min_eig_thr=1e-4):
        super().__init__(max_corners, quality_level, min_distance, block_size, win, max_level, max_iter,
                         epsilon, min_eig_thr)


def lib():
    global _LIB
    if _LIB is None:
        so = os.environ.get("EIG_ORACLE_LIB") or os.path.join(_HERE, "libeig_oracle.so")  # EIG_ORACLE_LIB: A/B builds (scripts/)
        if not os.path.exists(so):
            build()
        _LIB = ctypes.CDLL(so)
        _LIB.eig_oracle_gate_order.restype = ctypes.c_int
        _LIB.eig_oracle_get_threads.restype = ctypes.c_int
        # the C loops run one item per (output channel, row): beyond ~64 threads they only add fork/join cost, and a container's CPU
        # quota (the GPU boxes: 256 CPUs visible, 16 usable) is the real bound
        set_threads(int(os.environ.get("EIG_ORACLE_THREADS", _default_threads())))
        _LIB.eig_oracle_prednet_rollout.restype = ctypes.c_int
        _LIB.eig_oracle_prednet_rollout_order.restype = ctypes.c_int
        _LIB.eig_oracle_prednet_rollout_wino.restype = ctypes.c_int
        _LIB.eig_oracle_prednet_rollout_state.restype = ctypes.c_int
        _LIB.eig_oracle_lucas_kanade.restype = ctypes.c_int
        _LIB.eig_oracle_good_features.restype = ctypes.c_int
        _LIB.eig_oracle_conv_chain.restype = ctypes.c_int
        _LIB.eig_oracle_wino_chain.restype = ctypes.c_int
        _LIB.eig_oracle_wino_chain_m.restype = ctypes.c_int
        _LIB.eig_oracle_wino_form.restype = ctypes.c_int
        for f in ("eig_oracle_farneback", "eig_oracle_fb_vectors", "eig_oracle_fb_levels", "eig_oracle_fb_grid_step"):
            getattr(_LIB, f).restype = ctypes.c_int
    return _LIB


def _default_threads():
    n = min(os.cpu_count() or 1, 64)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except Exception:  # noqa: BLE001
        pass
    return n


def set_threads(n):
    """OpenMP threads of the C oracle's convolution loops (results do not depend on it)."""
    (_LIB or lib()).eig_oracle_set_threads(ctypes.c_int(int(n)))


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def tensor_names(n_layers):
    """Order of the weight-tensor table consumed by eig_oracle.c:bind_tensors (chainer npz key names
    of chainer_prednet with the ``predictor/`` prefix stripped)."""
    names = []
    for l in range(n_layers):
        if l > 0:
            names += ["ConvA%d/W" % l, "ConvA%d/b" % l]
        names += ["ConvP%d/W" % l, "ConvP%d/b" % l]
        for g in GATES:
            names.append("ConvLSTM%d/x_%s0/W" % (l, g))
            if l < n_layers - 1:
                names.append("ConvLSTM%d/x_%s1/W" % (l, g))
            names.append("ConvLSTM%d/h_%s/W" % (l, g))
            names.append("ConvLSTM%d/h_%s/b" % (l, g))
        for g in ("i", "f", "o"):
            names.append("ConvLSTM%d/c_%s/W" % (l, g))
    return names


# EIGEN_WINOGRAD unset: every eligible operator -- bit l ConvLSTM_l, bit 8 + l ConvA_l, bit 16 + l ConvP_l (eig_oracle.c: eig_wino_op; the
# engine's default is the same mask); bit 24: the unpooled source inside the Winograd ConvLSTM's chains (eig_wino_fuse_up); bits 25 / 26 / 27:
# the class bits of the ConvLSTMs / ConvAs / ConvPs -- an operator is a Winograd F(4x4, 3x3) one only with its own bit AND its class bit set (eig_wino_op)
WINO_AUTO = 0x0FFFFFFE


def wino_form(wino_mask, kind, l, channels, w, h):
    """(winograd, fused) of operator `kind` (0 ConvLSTM_l, 1 ConvA_l, 2 ConvP_l) as the roll-out decides it (eig_oracle.c: eig_oracle_wino_form)."""
    ch = (ctypes.c_int * len(channels))(*channels)
    r = lib().eig_oracle_wino_form(ctypes.c_int(int(wino_mask)), ctypes.c_int(kind), ctypes.c_int(l), ctypes.c_int(len(channels)), ch, ctypes.c_int(w), ctypes.c_int(h))
    return bool(r & 1), bool(r & 2)


def wino_mask_default():
    """Which operators run as Winograd F(4x4, 3x3): the engine's switch EIGEN_WINOGRAD (bits as above), so that checker and library
    follow the same setting by default."""
    v = os.environ.get("EIGEN_WINOGRAD")
    m = WINO_AUTO if v is None or v == "" else int(v, 0)
    if os.environ.get("EIGEN_WINO_FUSEUP") == "0":   # (the engine reads the same variable)
        m &= ~(1 << 24)
    return m


STATE_TENSORS = ("R", "c", "P", "E")   # eig_oracle.c: eig_oracle_prednet_rollout_state, `which` 0..3 (the engine's eigen_debug_state numbers them alike)


def prednet_rollout(weights, channels, w, h, img, n_repeat=20, n_ext=2, requant=False, return_float=False, order="canonical", wino_mask=None, state_steps=None):
    """Roll ``img`` (uint8 [C0,H,W]) through PredNet; returns uint8 frames [n_repeat+n_ext, C0, H, W].
    order: "canonical" = the build's arithmetic (what the HIP kernels reproduce bit for bit); "chainer" = the reference's
    element-wise order (eig_oracle.c: lstm_reference_order) -- separate convolution tensors added left to right, plain unpool ->
    9-tap, un-fused gate products, sigmoid = tanh(x/2)/2 + 1/2 on libm.
    state_steps: a list of step counts (1 .. n_repeat + n_ext); the float32 state after that many steps is returned LAST, as
    {count: [per layer {"R": [C_l,H_l,W_l], "c", "P", "E": [2 C_l,H_l,W_l]}]} (E_0: the error units the last executed step consumed)."""
    L = len(channels)
    names = tensor_names(L)
    arrs = [np.ascontiguousarray(weights[n], dtype=np.float32) for n in names]
    tab = (ctypes.POINTER(ctypes.c_float) * len(arrs))(*[_p(a, ctypes.c_float) for a in arrs])
    ch = np.asarray(channels, dtype=np.int32)
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.shape == (channels[0], h, w), img.shape
    T = n_repeat + n_ext
    out = np.zeros((T, channels[0], h, w), dtype=np.uint8)
    p0 = np.zeros((T, channels[0], h, w), dtype=np.float32) if return_float else None
    steps = [] if state_steps is None else [int(s) for s in state_steps]
    if any(s < 1 or s > T for s in steps):
        raise ValueError("state_steps are step counts in 1 .. %d, got %s" % (T, steps))
    states = {s: [{k: np.zeros(((2 if k == "E" else 1) * channels[l], h >> l, w >> l), np.float32) for k in STATE_TENSORS} for l in range(L)] for s in steps}
    st_arr = np.asarray(steps, dtype=np.int32)
    st_tab = (ctypes.POINTER(ctypes.c_float) * max(len(steps) * L * 4, 1))(*[_p(states[s][l][k], ctypes.c_float) for s in steps for l in range(L) for k in STATE_TENSORS])
    rc = lib().eig_oracle_prednet_rollout_state(
        ctypes.c_int(L), _p(ch, ctypes.c_int), ctypes.c_int(w), ctypes.c_int(h), tab, _p(img, ctypes.c_uint8),
        ctypes.c_int(n_repeat), ctypes.c_int(n_ext), ctypes.c_int(int(requant)), _p(out, ctypes.c_uint8),
        _p(p0, ctypes.c_float) if return_float else None, ctypes.c_int({"canonical": 0, "chainer": 1}[order]),
        ctypes.c_int((wino_mask_default() if wino_mask is None else int(wino_mask)) if order == "canonical" else 0),
        ctypes.c_int(len(steps)), _p(st_arr, ctypes.c_int) if steps else None, st_tab if steps else None)
    if rc != 0:
        raise ValueError("eig_oracle_prednet_rollout failed (size must be divisible by 2^(L-1))")
    res = (out, p0) if return_float else (out,)
    if state_steps is not None:
        res += (states,)
    return res if len(res) > 1 else out


class PredNetC:
    """The C roll-out behind the interface of oracle.prednet_torch.PredNetTorch (``rollout(imgs, n_repeat, n_ext)``), so that
    oracle.classify.population_report can take it as the 'other' implementation: order="chainer" is the torch-free statement of
    the reference's element-wise order."""

    def __init__(self, weights, channels, w, h, order="chainer"):
        self.weights, self.channels, self.w, self.h, self.order = weights, list(channels), w, h, order

    def rollout(self, imgs, n_repeat=20, n_ext=2, requant=False):
        fr, fl = zip(*[prednet_rollout(self.weights, self.channels, self.w, self.h, im, n_repeat=n_repeat, n_ext=n_ext, requant=requant,
                                       return_float=True, order=self.order) for im in np.asarray(imgs)])
        return np.stack(fr), np.stack(fl)


def conv_chain(sources, ups, weights, H, W):
    """out[o,y,x] = canonical fmaf chain over the listed sources.  sources[i]: [Cin_i, Hs, Ws] float32,
    ups[i] in {0,1} (1 = source is half resolution, unpooled x2), weights[i]: [Cout, Cin_i, 3, 3]."""
    ns = len(sources)
    srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in sources]
    ws = [np.ascontiguousarray(x, dtype=np.float32) for x in weights]
    cout = ws[0].shape[0]
    st = (ctypes.POINTER(ctypes.c_float) * ns)(*[_p(a, ctypes.c_float) for a in srcs])
    wt = (ctypes.POINTER(ctypes.c_float) * ns)(*[_p(a, ctypes.c_float) for a in ws])
    cin = np.asarray([s.shape[0] for s in srcs], dtype=np.int32)
    up = np.asarray(ups, dtype=np.int32)
    out = np.zeros((cout, H, W), dtype=np.float32)
    lib().eig_oracle_conv_chain(ctypes.c_int(ns), st, _p(cin, ctypes.c_int), _p(up, ctypes.c_int), wt,
                                ctypes.c_int(cout), ctypes.c_int(H), ctypes.c_int(W), _p(out, ctypes.c_float))
    return out


def wino_chain(sources, weights, H, W, m=2):
    """out[o,y,x] = the canonical Winograd F(m x m, 3x3) chain, m = 2 or 4, over the listed full-resolution sources (eig_oracle.c: wino_*)."""
    ns = len(sources)
    srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in sources]
    ws = [np.ascontiguousarray(x, dtype=np.float32) for x in weights]
    cout = ws[0].shape[0]
    st = (ctypes.POINTER(ctypes.c_float) * ns)(*[_p(a, ctypes.c_float) for a in srcs])
    wt = (ctypes.POINTER(ctypes.c_float) * ns)(*[_p(a, ctypes.c_float) for a in ws])
    cin = np.asarray([s.shape[0] for s in srcs], dtype=np.int32)
    out = np.zeros((cout, H, W), dtype=np.float32)
    rc = lib().eig_oracle_wino_chain_m(ctypes.c_int(ns), st, _p(cin, ctypes.c_int), wt, ctypes.c_int(cout), ctypes.c_int(H), ctypes.c_int(W), _p(out, ctypes.c_float), ctypes.c_int(m))
    if rc != 0:
        raise ValueError("wino_chain needs even W (m = 4: W % 4 == 0)")
    return out


def det_math(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    e, s, t = (np.zeros_like(x) for _ in range(3))
    lib().eig_oracle_det_math(_p(x, ctypes.c_float), ctypes.c_int(x.size), _p(e, ctypes.c_float),
                              _p(s, ctypes.c_float), _p(t, ctypes.c_float))
    return e, s, t


def gray(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    c, h, w = img.shape
    out = np.zeros((h, w), dtype=np.uint8)
    lib().eig_oracle_gray(_p(img, ctypes.c_uint8), ctypes.c_int(c), ctypes.c_int(h), ctypes.c_int(w), _p(out, ctypes.c_uint8))
    return out


def pyr_down(g):
    g = np.ascontiguousarray(g, dtype=np.uint8)
    h, w = g.shape
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), dtype=np.uint8)
    lib().eig_oracle_pyr_down(_p(g, ctypes.c_uint8), ctypes.c_int(h), ctypes.c_int(w), _p(out, ctypes.c_uint8))
    return out


def min_eig(g, block=7):
    g = np.ascontiguousarray(g, dtype=np.uint8)
    h, w = g.shape
    out = np.zeros((h, w), dtype=np.float32)
    lib().eig_oracle_min_eig(_p(g, ctypes.c_uint8), ctypes.c_int(h), ctypes.c_int(w), ctypes.c_int(block), _p(out, ctypes.c_float))
    return out


def good_features(g, params=None):
    params = params or LKParams()
    g = np.ascontiguousarray(g, dtype=np.uint8)
    h, w = g.shape
    pts = np.zeros((max(params.max_corners, 1), 2), dtype=np.float32)
    n = lib().eig_oracle_good_features(_p(g, ctypes.c_uint8), ctypes.c_int(h), ctypes.c_int(w), ctypes.byref(params), _p(pts, ctypes.c_float))
    return pts[:n].copy()


def pyr_lk(g0, g1, pts, params=None):
    params = params or LKParams()
    g0 = np.ascontiguousarray(g0, dtype=np.uint8)
    g1 = np.ascontiguousarray(g1, dtype=np.uint8)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    h, w = g0.shape
    n = pts.shape[0]
    nxt = np.zeros((max(n, 1), 2), dtype=np.float32)
    st = np.zeros(max(n, 1), dtype=np.uint8)
    if n:
        lib().eig_oracle_pyr_lk(_p(g0, ctypes.c_uint8), _p(g1, ctypes.c_uint8), ctypes.c_int(h), ctypes.c_int(w),
                                ctypes.byref(params), _p(pts, ctypes.c_float), ctypes.c_int(n), _p(nxt, ctypes.c_float), _p(st, ctypes.c_uint8))
    return nxt[:n], st[:n]


def lucas_kanade(img0, img1, params=None):
    """img0/img1: uint8 [C,H,W].  Returns float32 [n,4] rows [x0, y0, dx, dy] (possibly n == 0)."""
    params = params or LKParams()
    img0 = np.ascontiguousarray(img0, dtype=np.uint8)
    img1 = np.ascontiguousarray(img1, dtype=np.uint8)
    c, h, w = img0.shape
    vec = np.zeros((max(params.max_corners, 1), 4), dtype=np.float32)
    n = lib().eig_oracle_lucas_kanade(_p(img0, ctypes.c_uint8), _p(img1, ctypes.c_uint8), ctypes.c_int(c), ctypes.c_int(h),
                                      ctypes.c_int(w), ctypes.byref(params), _p(vec, ctypes.c_float))
    return vec[:n].copy()


class FBParams(ctypes.Structure):
    """cv::calcOpticalFlowFarneback parameters of OpenCV's dense-flow tutorial + the vector sampling grid (oracle/farneback.c)."""
    _fields_ = [("levels", ctypes.c_int), ("winsize", ctypes.c_int), ("iterations", ctypes.c_int), ("poly_n", ctypes.c_int),
                ("poly_sigma", ctypes.c_double), ("step", ctypes.c_int), ("max_vectors", ctypes.c_int)]

    def __init__(self, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, step=16, max_vectors=100):
        super().__init__(levels, winsize, iterations, poly_n, poly_sigma, step, max_vectors)


def farneback_flow(g0, g1, params=None):
    """g0/g1: uint8 gray [H,W] -> dense flow float32 [H,W,2] (dx, dy)."""
    params = params or FBParams()
    g0 = np.ascontiguousarray(g0, dtype=np.uint8); g1 = np.ascontiguousarray(g1, dtype=np.uint8)
    h, w = g0.shape
    flow = np.zeros((h, w, 2), dtype=np.float32)
    rc = lib().eig_oracle_farneback(_p(g0, ctypes.c_uint8), _p(g1, ctypes.c_uint8), ctypes.c_int(h), ctypes.c_int(w), ctypes.byref(params),
                                    _p(flow, ctypes.c_float))
    if rc != 0:
        raise ValueError("farneback: unsupported size/parameters")
    return flow


def farneback_vectors(flow, params=None):
    """dense flow -> float32 [n,4] rows [x, y, dx, dy] on the sampling grid."""
    params = params or FBParams()
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    h, w, _ = flow.shape
    vec = np.zeros((max(params.max_vectors, 1), 4), dtype=np.float32)
    n = lib().eig_oracle_fb_vectors(_p(flow, ctypes.c_float), ctypes.c_int(h), ctypes.c_int(w), ctypes.byref(params), _p(vec, ctypes.c_float))
    return vec[:n].copy()


def farneback(img0, img1, params=None):
    """img0/img1: uint8 [C,H,W] -> float32 [n,4] vectors (gray conversion as for Lucas-Kanade)."""
    return farneback_vectors(farneback_flow(gray(img0), gray(img1), params), params)
