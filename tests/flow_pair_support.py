"""Shared by tests/test_flow_pair_host.py and tests/test_gpu_flow_pair.py ("The prediction pairing"):
(a) `pair_ref`, tests/flow_obj_support.py `flow_stage_ref` on a pair of FLOAT images (csrc/flow_pair_kernels.h in front of the
    kernels of csrc/flow_obj_kernels.h and csrc/flow_ref_kernels.h);
(b) `run_pair`, the float64 torch-CPU autograd statement: tests/flow_obj_support.py `run_flow` with a stateful `term` that remembers
    the previous P0 IN THE GRAPH and starts from the detached start-state P;
(c) the case lists and the refinement loop on the float64 reference alone;
(d) the name of the kernel of the new header.
It imports tests/flow_obj_support.py and tests/flow_ref_support.py and changes neither."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import flow_obj_support as fs
from tests import flow_ref_support as rs
from tests.train_support import _fed_from, _random_weights

FLOW_PAIR_KERNELS = ["tflow_pair_prep_kernel"]


# ---- (a) the numpy restatement
PairRef = namedtuple("PairRef", "value u seed prev_grad prev_grad64 mv bound")


def pair_ref(pred, prev, r, eps, direction=None, mask=None, scale=1.0):
    """pred, prev float32 [B, C, H, W]: the prediction and the reference image; the settings of `flow_ref`.  -> value (exactly summed,
    then divided), u float64 [B, 2, H, W], seed = scale * d value / d pred and prev_grad = scale * d value / d prev as float32
    [B, C, H, W], the latter also ahead of its rounding, mv = m v and the bound of a double-precision sum of the N = B H W summands in
    any order, N 2^-53 sum |m v| / (B N_m)."""
    pred, prev = np.asarray(pred, np.float32), np.asarray(prev, np.float32)
    assert prev.dtype == np.float32 and prev.shape == pred.shape
    s = fs.flow_stage_ref(pred, prev.astype(np.float64), r, eps, direction, mask, scale)
    return PairRef(s.value, s.u, s.seed, s.grad, s.grad64, s.mv, s.bound)


def pair_field_inputs(w, h, C, kind, B=2):
    """(pred, prev) float32 [B, C, h, w]: `flow_obj_support.field_inputs`' prediction, and a float reference that is no byte over 255:
    kind "random" floats in [0, 1] with exact 0 and 1 among them, or the "smooth" frame moved off the byte grid"""
    pred, ref = fs.field_inputs(w, h, C, kind, B)
    rng = np.random.default_rng(7000 * w + h + C + (kind == "smooth"))
    if kind == "random":
        prev = rng.random((B, C, h, w)).astype(np.float32)
        prev[:, :, 1, 1::3] = 0.0
        prev[:, :, -2, ::4] = 1.0
    else:
        prev = np.clip(ref.astype(np.float32) / np.float32(255.0) + (rng.random((B, C, h, w)).astype(np.float32) - np.float32(0.5)) * np.float32(0.01),
                       np.float32(0), np.float32(1)).astype(np.float32)
    return pred, prev


# ---- (b) the autograd statement
class PairTerm:
    """The `term` callback of `run_flow` under the prediction pairing: term s is `torch_flow_term(P0_s, P0_{s-1})` with P0_{s-1} IN THE
    GRAPH, the first reference being `start`, the start state's P of layer 0, detached.  detach_prev: the statement the trainer must
    NOT match, every reference a constant.  The flow term's arithmetic is float64 on the widened images whatever the network runs in."""

    def __init__(self, start, radius, eps, direction, mask, detach_prev=False):
        self.prev, self.args, self.detach_prev = start.detach(), (radius, eps, direction, mask), detach_prev

    def __call__(self, P, xn):
        prev = self.prev.detach() if self.detach_prev else self.prev
        self.prev = P
        return fs.torch_flow_term(P.to(torch.float64), prev.to(torch.float64), *self.args)[:2]


def run_pair(weights, channels, frames, *, radius=7, eps=1e-2, direction=None, mask=None, state=None, dtype=torch.float64, detach_prev=False, **kw):
    """`run_flow` under the prediction pairing.  state: the (h, c, P) lists a previous result left (None: a reset, the first reference
    is zeros); the other keywords are `run_flow`'s."""
    B, _, C, H, W = frames.shape
    start = torch.zeros(B, C, H, W, dtype=dtype) if state is None else state[2][0].to(dtype)
    return fs.run_flow(weights, channels, frames, state=state, dtype=dtype, term=PairTerm(start, radius, eps, direction, mask, detach_prev), **kw)


# ---- (c) the cases
# form: "still" (a still repeated 4 times and 2 self-fed steps on the float prediction, weights [0, 0, 0, 0, 1]: the population term,
# P0 after the last fed frame -> the first extended prediction), "still_requant" (the same through the byte), "drifting" (T = 5,
# teacher-forced, all weights one: term 0 runs with its constant zero reference), "continued" (the drifting call again with reset=False:
# term 0's reference is the kept P)
PairCase = namedtuple("PairCase", "w h ch wset mode r form")
FLOW_SHAPES = list(fs.FLOW_SHAPES)   # 12x8 gray, 16x12 colour, 24x16 gray, 40x24 colour: three tiles across, the last ragged
FORMS = ("still", "still_requant", "drifting", "continued")
MODES = fs.MODES
RADII = fs.RADII
B_CASE = fs.B_CASE
POPULATION_WEIGHTS = [0.0, 0.0, 0.0, 0.0, 1.0]

PAIR_CASES = [PairCase(w, h, tuple(ch), "live", mode, r, form) for w, h, ch in FLOW_SHAPES for mode in MODES for r in RADII for form in FORMS]

# the weight seed of a case's "live" set where `_live_weights`' own (tests/train_support.py) misses the float32 yardstick of
# tests/test_flow_pair_host.py under this pairing: {case id: seed}.  Measured with seed 2: 1.28e-4 (ConvLSTM0/h_f/b), 9.07e-5 (ConvP0/b),
# 2.79e-3 (ConvP0/b), 8.56e-5 (ConvP1/b) and 1.35e-4 (ConvP1/b): bias gradients in which the steps' contributions nearly cancel, as in
# the case that set the yardstick.  With seed 3 the five give 2.1e-6, 4.5e-6, 9.9e-6, 3.0e-5 and 4.2e-6.
PAIR_SEEDS = {"12x8-1_4-energy-r2-drifting": 3, "24x16-1_3_4_5-energy-r7-still_requant": 3, "24x16-1_3_4_5-tangent-r2-still": 3,
              "24x16-1_3_4_5-tangent-r2-still_requant": 3, "24x16-1_3_4_5-tangent-r7-drifting": 3}


def pair_case_id(c):
    return "%dx%d-%s-%s-r%d-%s" % (c.w, c.h, "_".join(map(str, c.ch)), c.mode, c.r, c.form)


def as_flow_case(c):
    """the FlowCase that shares the frames and the settings"""
    return fs.FlowCase(c.w, c.h, c.ch, c.wset, c.mode, c.r, "drifting" if c.form == "continued" else c.form)


def pair_case_frames(c):
    return fs.flow_case_frames(as_flow_case(c))


def pair_case_weights(c):
    from tests.train_support import case_weights
    seed = PAIR_SEEDS.get(pair_case_id(c))
    if seed is None:
        return case_weights(c.w, c.h, c.ch, c.wset)
    wts = _random_weights(list(c.ch), c.w, c.h, seed=seed)
    wts["ConvP0/b"] = np.full_like(wts["ConvP0/b"], 0.5)
    return wts


def pair_case_call(c):
    """the keywords the trainer and run_pair share"""
    if c.form in ("drifting", "continued"):
        return dict(n_fed=None, requant=False, step_weights=None)
    return dict(n_fed=4, requant=c.form == "still_requant", step_weights=list(POPULATION_WEIGHTS))


def pair_case_settings(c):
    return fs.flow_case_settings(as_flow_case(c))


def has_reference_term(c):
    """whether the case has a computed term s >= 1, one whose reference is in the graph (every case of the list has)"""
    w = pair_case_call(c)["step_weights"]
    return w is None or any(v != 0 for v in w[1:])


def pair_case_reference(c, pred=None, dtype=torch.float64, leaf=None, run=None, **kw):
    """The reference of a case.  run: `run_pair` (None) or another statement with its keywords.  pred: the float32 predictions whose
    bytes a requantised case is fed (the GPU's own); None: the run is repeated on its own requantised predictions until every self-fed
    step has read them.  "continued": the call is made twice, the second from the state the first left, and the second is returned."""
    run = run or run_pair
    wts, frames = pair_case_weights(c), pair_case_frames(c)
    args = dict(pair_case_call(c), **pair_case_settings(c), dtype=dtype, leaf=leaf, **kw)
    if c.form == "continued":
        first = run(wts, list(c.ch), frames, **args)
        return run(wts, list(c.ch), frames, state=first.state, **args)
    if not args["requant"]:
        return run(wts, list(c.ch), frames, **args)
    if pred is not None:
        return run(wts, list(c.ch), frames, fed=_fed_from(pred), **args)
    fed = np.zeros(frames.shape, np.float32)
    T, n_fed = frames.shape[1], args["n_fed"]
    for _ in range(T - n_fed + 1):
        r = run(wts, list(c.ch), frames, fed=fed, **args)
        fed = _fed_from(r.pred.astype(np.float32))
    return r


def frame_pairing(weights, channels, frames, *, state=None, detach_prev=False, **kw):
    """the frame-pairing statement of the same call (`run_flow` as it is), with `run_pair`'s signature"""
    return fs.run_flow(weights, channels, frames, state=state, **kw)


# refinement on the reference alone: the shapes and settings of tests/flow_ref_support.py, the population term's weights
REFINE_SHAPES, REFINE = rs.REFINE_SHAPES, rs.REFINE
REFINE_ROWS = [(w, h, ch, mode) for w, h, ch in REFINE_SHAPES for mode in ("tangent", "energy")]
# the rows in which the term rises on the float64 reference alone (tests/test_flow_pair_host.py asserts exactly these and at least
# four); tests/test_gpu_flow_pair.py runs them
RISING_ROWS = list(REFINE_ROWS)


@functools.lru_cache(maxsize=None)
def pair_refine_reference(w, h, ch, mode):
    """refine_stills under a PredictionFlow on the float64 reference alone: tests/flow_ref_support.py `refine_loop` with `run_pair` and the
    weights [0] * n_repeat + [1] * (n_ext - 1).  -> (stills uint8, history [iters + 1])"""
    return rs.refine_loop(run_pair, [0.0] * REFINE["n_repeat"] + [1.0] * (REFINE["n_ext"] - 1), w, h, ch, mode)
