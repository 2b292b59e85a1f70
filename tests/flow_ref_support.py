"""Shared by tests/test_flow_ref_host.py and tests/test_gpu_flow_ref.py ("The moving reference"):
(a) `flow_ref_grad`, the reference gradient (csrc/flow_ref_kernels.h) of tests/flow_obj_support.py `flow_stage_ref`;
(b) the folds by which a training call adds the reference path to the frame gradient, in float32;
(c) the case lists and the refinement loop on the float64 reference alone;
(d) the names of the kernels of the new header."""
import functools
from collections import namedtuple

import numpy as np

from tests import flow_obj_support as fs
from tests.flow_obj_support import scharr_adjoint  # noqa: F401  (tests import it from here)

FLOW_REF_KERNELS = ["tflow_ref_sums_kernel", "tflow_ref_fold_kernel"]

# the field cases of tests/flow_obj_support.py plus one tile and a ragged strip of 2 pixels in both directions
FIELD_CASES = fs.FIELD_CASES + [(18, 18, 1, 1, False, ("energy", "tangent"))]


# ---- (a) the numpy restatement
RefGrad = namedtuple("RefGrad", "grad grad64 u seed")


def flow_ref_grad(pred, ref, r, eps, direction=None, mask=None, scale=1.0):
    """scale * d value / d reference of the flow term, by x = (float)byte / 255.0f: pred float32 [B, C, H, W], ref uint8 [B, C, H, W];
    the settings of `flow_ref`.  -> grad float32 [B, C, H, W], the same ahead of its rounding to float, and u and seed of the same
    statement (`flow_obj_support.flow_stage_ref`)."""
    s = fs.flow_stage_ref(pred, fs.byte_reference(ref), r, eps, direction, mask, scale)
    return RefGrad(s.grad, s.grad64, s.u, s.seed)


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


def refine_loop(run, weights, w, h, ch, mode):
    """refine_stills on a float64 reference alone: run(weights of the network, channels, frames, **settings) with the tied leaf and the
    step weights `weights`, then tests/frame_grad_support.py `still_step_ref`.  -> (stills uint8, history float64 [iters + 1])"""
    from tests.frame_grad_support import case_inputs, still_step_ref
    frames, sets = case_inputs(w, h, tuple(ch), 2, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    T = REFINE["n_repeat"] + REFINE["n_ext"]
    d = fs.direction_of(mode, w, h)
    mask = refine_mask(w, h)
    hist = []
    call = lambda st: run(sets["live"], list(ch), np.ascontiguousarray(np.broadcast_to(st[:, None], (st.shape[0], T) + st.shape[1:])), radius=7, eps=1e-2,
                          direction=d, mask=None, n_fed=REFINE["n_repeat"], requant=False, step_weights=weights, leaf="tied")
    for _ in range(REFINE["iters"]):
        res = call(stills)
        hist.append(res.loss)
        stills = still_step_ref(stills, res.frame_grad.astype(np.float32), REFINE["step"], mask)
    hist.append(call(stills).loss)
    return stills, np.array(hist)


@functools.lru_cache(maxsize=None)
def refine_reference(w, h, ch, mode, constant_reference=False):
    """`refine_loop` under a FlowObjective: `run_flow` and the weights of the extension's terms"""
    weights = [0.0] * (REFINE["n_repeat"] - 1) + [1.0] * REFINE["n_ext"]
    return refine_loop(functools.partial(fs.run_flow, constant_reference=constant_reference), weights, w, h, ch, mode)
