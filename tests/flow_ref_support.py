"""Shared by tests/test_flow_ref_host.py and tests/test_gpu_flow_ref.py ("The moving reference"):
(a) `flow_ref_grad`, a numpy float64 restatement of csrc/flow_ref_kernels.h on top of the fields of tests/flow_obj_support.py
    `flow_ref`, operation by operation in the order the kernels use;
(b) the folds by which a training call adds the reference path to the frame gradient, in float32;
(c) the case lists and the refinement loop on the float64 reference alone;
(d) the names of the kernels of the new header."""
import functools
from collections import namedtuple

import numpy as np

from tests import flow_obj_support as fs
from tests.flow_obj_support import _gray, window_sum

FLOW_REF_KERNELS = ["tflow_ref_sums_kernel", "tflow_ref_fold_kernel"]

# the field cases of tests/flow_obj_support.py plus one tile and a ragged strip of 2 pixels in both directions
FIELD_CASES = fs.FIELD_CASES + [(18, 18, 1, 1, False, ("energy", "tangent"))]


# ---- (a) the numpy restatement
RefGrad = namedtuple("RefGrad", "grad grad64 u seed")


def _fold_last(g):
    """[..., n + 2] padded positions -1 .. n -> [..., n]: the two ends are added onto the border, ascending, each sum from its first term"""
    n = g.shape[-1] - 2
    out = g[..., 1:n + 1].copy()
    out[..., 0] = g[..., 0] + out[..., 0]
    out[..., n - 1] = out[..., n - 1] + g[..., n + 1]
    return out


def scharr_adjoint(rx, ry):
    """S^T(rx, ry), [B, H, W] -> [B, H, W]: the gather over the padded positions with r zero outside the image, then the padding ring
    folded onto the border: along x first (per padded row), then along y (the order csrc/flow_ref_kernels.h states)"""
    B, H, W = rx.shape
    # padded position (Y, X) is index (Y + 1, X + 1) of G; r(Y + j, X + i) is index (Y + j + 2, X + i + 2) of the twice-padded r
    px, py = np.pad(rx, ((0, 0), (2, 2), (2, 2))), np.pad(ry, ((0, 0), (2, 2), (2, 2)))
    RX = lambda j, i: px[:, 1 + j:1 + j + H + 2, 1 + i:1 + i + W + 2]
    RY = lambda j, i: py[:, 1 + j:1 + j + H + 2, 1 + i:1 + i + W + 2]
    gx = ((3.0 * (RX(-1, -1) - RX(-1, 1)) + 10.0 * (RX(0, -1) - RX(0, 1))) + 3.0 * (RX(1, -1) - RX(1, 1))) / 32.0
    gy = ((3.0 * (RY(-1, -1) - RY(1, -1)) + 10.0 * (RY(-1, 0) - RY(1, 0))) + 3.0 * (RY(-1, 1) - RY(1, 1))) / 32.0
    G = gx + gy
    rows = _fold_last(G)                                                  # [B, H + 2, W]
    return np.swapaxes(_fold_last(np.swapaxes(rows, -1, -2)), -1, -2)     # [B, H, W]


def flow_ref_grad(pred, ref, r, eps, direction=None, mask=None, scale=1.0):
    """scale * d value / d reference of the flow term, by x = (float)byte / 255.0f: pred float32 [B, C, H, W], ref uint8 [B, C, H, W];
    the settings of `flow_ref`.  -> grad float32 [B, C, H, W], the same ahead of its rounding to float, and u and seed of `flow_ref`'s
    own arithmetic (restated here, since the sums need Ix, Iy, It and q)."""
    pred = np.asarray(pred, np.float32)
    B, C, H, W = pred.shape
    x = (np.asarray(ref, np.uint8).astype(np.float32) / np.float32(255.0)).astype(np.float64)
    I0, I1 = _gray(x), _gray(pred.astype(np.float64))
    It = I1 - I0
    ap = np.pad(I0, ((0, 0), (1, 1), (1, 1)), mode="edge")
    a = lambda dy, dx: ap[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    Ix = ((3.0 * (a(-1, 1) - a(-1, -1)) + 10.0 * (a(0, 1) - a(0, -1))) + 3.0 * (a(1, 1) - a(1, -1))) / 32.0
    Iy = ((3.0 * (a(1, -1) - a(-1, -1)) + 10.0 * (a(1, 0) - a(-1, 0))) + 3.0 * (a(1, 1) - a(-1, 1))) / 32.0
    Gxx, Gxy, Gyy = window_sum(Ix * Ix, r), window_sum(Ix * Iy, r), window_sum(Iy * Iy, r)
    bx, by = window_sum(Ix * It, r), window_sum(Iy * It, r)
    aa, cc, bb = Gxx + eps, Gyy + eps, Gxy
    det = aa * cc - bb * bb
    ux, uy = -((cc * bx - bb * by) / det), -((aa * by - bb * bx) / det)
    if direction is None:
        gx, gy = 2.0 * ux, 2.0 * uy
    else:
        d = np.asarray(direction, np.float32).astype(np.float64)
        gx, gy = np.broadcast_to(d[0], ux.shape), np.broadcast_to(d[1], ux.shape)
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    qx = np.where(m, (cc * gx - bb * gy) / det, 0.0)
    qy = np.where(m, (aa * gy - bb * gx) / det, 0.0)
    kappa = float(scale) / float(B * int(m.sum()))
    k = [1.0] if C == 1 else [0.299, 0.587, 0.114]
    # tflow_ref_sums_kernel
    Qx, Qy = window_sum(qx, r), window_sum(qy, r)
    Mxx, Mxy, Myy = window_sum(2.0 * (qx * ux), r), window_sum(qx * uy + qy * ux, r), window_sum(2.0 * (qy * uy), r)
    rx = -(((Qx * It + Mxx * Ix) + Mxy * Iy) * kappa)
    ry = -(((Qy * It + Mxy * Ix) + Myy * Iy) * kappa)
    e = (Ix * Qx + Iy * Qy) * kappa
    # tflow_ref_fold_kernel
    dI0 = e + scharr_adjoint(rx, ry)
    grad64 = np.stack([kc * dI0 for kc in k], 1)
    seed = np.stack([kc * -((Ix * Qx + Iy * Qy) * kappa) for kc in k], 1).astype(np.float32)
    return RefGrad(grad64.astype(np.float32), grad64, np.stack([ux, uy], 1), seed)


# ---- (b) the folds of a training call
def add_reference_paths(per_constant, refs):
    """per-frame mode: g_t = fl(g_t(constant) + ref_{t-1}); refs: {s: float32 [B, C, H, W]}, the reference path of every computed term s
    (weight not zero), which belongs to frame s + 1"""
    out = np.array(per_constant, np.float32)
    for s, g in refs.items():
        out[:, s + 1] = out[:, s + 1] + np.asarray(g, np.float32)
    return out


def fold_tied_moving(per_constant, refs):
    """tied mode: zeros, then for s = T - 1 .. 0 first + ref_s (where term s was computed), then + input_s (the constant-reference frame
    gradient of step s), every addition in float32"""
    per_constant = np.asarray(per_constant, np.float32)
    acc = np.zeros(per_constant.shape[:1] + per_constant.shape[2:], np.float32)
    for s in reversed(range(per_constant.shape[1])):
        if s in refs:
            acc = acc + np.asarray(refs[s], np.float32)
        acc = acc + per_constant[:, s]
    return acc


# ---- (c) the cases
LIVE_CASES = [c for c in fs.FLOW_CASES if c.wset == "live"]
DEAD_CASES = [c for c in fs.FLOW_CASES if fs.is_dead(c)]

# refinement on the reference alone: (w, h, channels), the table of DESIGN.md
REFINE_SHAPES = [(12, 8, (1, 4)), (16, 12, (3, 4, 6)), (24, 16, (1, 4, 8)), (40, 24, (3, 4))]
REFINE = dict(n_repeat=4, n_ext=2, iters=8, step=2)


def refine_mask(w, h):
    """the left quarter is kept"""
    m = np.ones((h, w), np.uint8)
    m[:, :w // 4] = 0
    return m


@functools.lru_cache(maxsize=None)
def refine_reference(w, h, ch, mode, constant_reference=False):
    """refine_stills on the float64 reference alone: `run_flow` with the tied leaf, then tests/frame_grad_support.py `still_step_ref`.
    -> (stills uint8, history float64 [iters + 1])"""
    from tests.frame_grad_support import case_inputs, still_step_ref
    frames, sets = case_inputs(w, h, tuple(ch), 2, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    T = REFINE["n_repeat"] + REFINE["n_ext"]
    weights = [0.0] * (REFINE["n_repeat"] - 1) + [1.0] * REFINE["n_ext"]
    d = fs.direction_of(mode, w, h)
    mask = refine_mask(w, h)
    hist = []
    run = lambda st: fs.run_flow(sets["live"], list(ch), np.ascontiguousarray(np.broadcast_to(st[:, None], (st.shape[0], T) + st.shape[1:])), radius=7, eps=1e-2,
                                 direction=d, mask=None, n_fed=REFINE["n_repeat"], requant=False, step_weights=weights, leaf="tied",
                                 constant_reference=constant_reference)
    for _ in range(REFINE["iters"]):
        res = run(stills)
        hist.append(res.loss)
        stills = still_step_ref(stills, res.frame_grad.astype(np.float32), REFINE["step"], mask)
    hist.append(run(stills).loss)
    return stills, np.array(hist)
