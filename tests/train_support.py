"""Shared by the training tests.  For tests/test_gpu_train*.py, tests/test_gpu_frame_grad.py and the host tests beside them: shapes, frame
and weight generators, the gradient rule (`_check_grads`), the one list of gradient cases (ALL_CASES), the wide shapes with the table of
tile configurations they must reach and a restatement of the launch arithmetic that reaches them, and two raw C-ABI callers (the float64
reference itself is oracle/prednet_train_ref.py).  For
tests/test_train*_host.py: the one list of training kernels and the one check of their register metadata."""
import ctypes
import functools
import os
import re
from collections import namedtuple

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


# The seed of the "live" weight set per (w, h, channels).  The condition is tests/test_train_cases_host.py: G > 0, no tensor with a zero
# gradient, at most half of P0 at the clamp, in every case of the list below.  Seed 2 meets it at every shape (no pixel of P0 at the
# clamp); (24, 8, [1, 4, 12, 20]) takes seed 3, since seed 2 was seen to leave two tensors without a gradient there with other frames.
LIVE_SEEDS = {(24, 8, (1, 4, 12, 20)): 3}


def _live_weights(ch, w, h):
    """The "random" draw with ConvP0/b = 0.5: the prediction starts in the middle of [0, 1] and not at the clamp"""
    wts = _random_weights(ch, w, h, seed=LIVE_SEEDS.get((w, h, tuple(ch)), 2))
    wts["ConvP0/b"] = np.full_like(wts["ConvP0/b"], 0.5)
    return wts


def _weight_sets(ch, w, h):
    """"synthetic": the package's own start.  "random": large weights, seed 2; at the two gray SHAPES they drive every pixel of
    P0 into the clamp, where no gradient passes (the declared all-zero cases of `is_dead`).  "live": `_live_weights`, a
    non-zero gradient in every tensor at every shape."""
    return [("synthetic", weights.synthetic_prednet_weights(ch, w, h, seed=1)), ("random", _random_weights(ch, w, h, seed=2)),
            ("live", _live_weights(ch, w, h))]


# ---- the gradient rule
# E of `_check_grads`: 10 x the worst element-wise deviation of the float32 restatement, 8.07e-5 (see the docstring)
ELEMENT_BOUND = 8.1e-4


def _worst_element(name, a, r):
    """where a is furthest from r: 'name[co, ci, ky, kx]: got ..., reference ...'"""
    i = np.unravel_index(int(np.argmax(np.abs(a - r))), r.shape)
    return "%s[%s]: got %.9g, reference %.9g" % (name, ", ".join(str(int(j)) for j in i), a[i], r[i])


def check_tensor(name, got, r, G, cancel=0.0, what=""):
    """The rule of `_check_grads` for one tensor (frame gradients: one step) with reference r != 0; G only for the report.
    cancel: the cancellation term added to the norm bound.  Returns (norm error / norm bound, element error / element bound)."""
    a, r = np.asarray(got, np.float64), np.asarray(r, np.float64)
    assert a.shape == r.shape, (what, name, a.shape, r.shape)
    nr, mr = float(np.linalg.norm(r.ravel())), float(np.abs(r).max())
    assert nr > 0, (what, name, "the reference is zero")
    err, emax = float(np.linalg.norm((a - r).ravel())), float(np.abs(a - r).max())
    bound = 1e-3 * nr + cancel
    assert err <= bound, "%s %s: |got - ref| = %.3e > %.3e (|ref| = %.3e, G = %.3e); worst element %s" % (what, name, err, bound, nr, G, _worst_element(name, a, r))
    assert emax <= ELEMENT_BOUND * mr, "%s %s: max |got - ref| = %.3e > %.0e max |ref| = %.3e (G = %.3e); worst element %s" % (
        what, name, emax, ELEMENT_BOUND, ELEMENT_BOUND * mr, G, _worst_element(name, a, r))
    return err / bound, emax / (ELEMENT_BOUND * mr)


def check_zero_tensor(name, got, G, what=""):
    """A tensor whose reference is exactly zero in a case declared so: |got| <= 1e-6 G, and exactly zero when G is zero"""
    a = np.asarray(got, np.float64)
    if G == 0:
        assert not a.any(), "%s %s: the reference gradients are all zero, got %s" % (what, name, _worst_element(name, a, np.zeros(a.shape)))
    else:
        assert np.linalg.norm(a.ravel()) <= 1e-6 * G, "%s %s: the reference is zero, |got| = %.3e > 1e-6 G = %.3e" % (what, name, np.linalg.norm(a.ravel()), 1e-6 * G)


def _check_grads(got, ref, zero_allowed=False, what=""):
    """The gradient rule, per tensor k, against the float64 reference r_k (no term is shared between tensors):

      norm          |got_k - r_k|_2   <= 1e-3 |r_k|_2
      element-wise  max |got_k - r_k| <= E max |r_k|,  E = ELEMENT_BOUND = 8.1e-4

    A tensor whose reference is exactly zero fails, unless the case is declared so (zero_allowed: the cases `is_all_zero`
    names); there |got_k|_2 <= 1e-6 G with G the norm of all reference gradients together, and got_k == 0 when G == 0.
    On a failure the message names the tensor, the index of the worst element (conv weights: co, ci, ky, kx) and both values.

    E is 10 x the worst element-wise deviation of a float32 run of the reference itself (oracle/prednet_train_ref.py and
    tests/frame_grad_support.py `run_frames` with dtype=torch.float32: no code of the trainer) from its float64 run, over the full
    list ALL_CASES: 257 cases, the 107 weight-gradient cases of ALL_GRAD_CASES (teacher-forced, self-fed, error objective; SHAPES
    x the three weight sets and the twelve wide cases) and the 150 frame-gradient cases (per step and tied), a requantised case
    with both runs fed the bytes of the float32 run's predictions.  Measured on the CPU: the worst deviation is 8.07e-5, of the
    tensor's largest element and of its norm alike: ConvLSTM0/h_o/b (one element, 5.5e-5 of G) at 12x8 gray, synthetic weights,
    requantised feedback, step weights (0, 0, 0, 1, 1), where the contributions of the steps nearly cancel.  The next worst
    element-wise deviation is 1.8e-5 (ConvLSTM0/c_o/W of the same shape); tensors 1e-10 of G are among them, so float32 needs
    no floor.  E = 10 x 8.07e-5 = 8.1e-4.
    tests/test_train_cases_host.py::test_the_float32_restatement_passes_the_rule keeps a sample of that measurement in the suite.
    The HIP trainer measured on MI355X over the 107 weight-gradient cases: at worst 0.020 of the norm bound (2.0e-5 of a tensor's
    norm) and 0.025 of the element-wise bound (2.0e-5 of its largest element); at the wide shapes 0.0044 and 0.0070.  No tensor
    misses the norm bound, so no tensor has a cancellation term.
    Returns the worst (norm, element) ratios of error to bound."""
    ref = {k: np.asarray(r, np.float64) for k, r in ref.items()}
    assert sorted(got) == sorted(ref), (what, sorted(set(got) ^ set(ref)))
    G = float(np.sqrt(sum(float((r ** 2).sum()) for r in ref.values())))
    worst = (0.0, 0.0)
    for k, r in ref.items():
        if not r.any():
            assert zero_allowed, "%s %s: the reference gradient is exactly zero and the case is not declared all-zero: nothing is compared" % (what, k)
            check_zero_tensor(k, got[k], G, what)
            continue
        ratios = check_tensor(k, got[k], r, G, what=what)
        worst = (max(worst[0], ratios[0]), max(worst[1], ratios[1]))
    return worst


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


# ---- shapes that reach the tiles real channel counts use.  conv() and wgrad() of csrc/prednet_train.hip choose MT = 1, 2 or 4
# output-channel blocks of 16 per wave by cout <= 16 / <= 32 / else and tile cout over gridDim.y; at SHAPES cout <= 24.
# (w, h, channels, B): every gradient comparison also runs at these, in the calls WIDE_CALLS lists.
WIDE_SHAPES = [(12, 20, [3, 12, 20], 3), (16, 8, [1, 20, 36], 2), (24, 8, [1, 4, 12, 20], 3)]
# (T, max_batch - B, max_steps - T) of the calls made at every wide shape: one that fills the handle, one that does not
WIDE_CALLS = [(6, 0, 0), (5, 1, 2)]

# What WIDE_SHAPES x WIDE_CALLS must reach, as predicates over one launch (`launches`): kind is "forward", "dgrad" (the same
# kernel, wmode 1; cout is the channel count it WRITES) or "wgrad"; MT, gy = gridDim.y, and for wgrad gx = gridDim.x over
# K = cin * 9, nsplit, chunk (pixels per split), P = N H W pixels, last = P - (nsplit - 1) chunk.
# tests/test_train_cases_host.py asserts that every row is hit.
# On the rows with N H W % 4 != 0: the dead pixel lanes of the last step lie behind the last sample of the last step, whose deltas
# are zero by construction (prediction T - 1 enters no term), so what those rows check is not the masked lanes' values but the
# decoding of a pixel count that is odd per sample (H W = 15 or 3): quads of 4 pixels straddle rows and samples everywhere, and with
# W = 3 one advance of 4 pixels wraps a row and sometimes two.  (Tried on MI355X: a row wrap that handles one wrap only fails 13 of the 24 wide
# cases; at (24, 16, [1, 3, 4, 5]), the one shape of SHAPES with a 3-wide map, it puts ConvP3/W off by 95 % of its norm, 5e-8 of G,
# which the floor of the earlier rule, 1e-6 G, accepted.)
_partial = lambda q: q["cout"] % (16 * q["MT"]) != 0
TILE_PROPERTIES = [
    ("forward: cout in (32, 64], the one M tile partly empty", lambda q: q["kind"] == "forward" and 32 < q["cout"] <= 64 and _partial(q)),
    ("dgrad:   cout in (32, 64], the one M tile partly empty", lambda q: q["kind"] == "dgrad" and 32 < q["cout"] <= 64 and _partial(q)),
    ("wgrad:   cout in (32, 64], the one M tile partly empty", lambda q: q["kind"] == "wgrad" and 32 < q["cout"] <= 64 and _partial(q)),
    ("forward: gridDim.y = 2, last M tile partial", lambda q: q["kind"] == "forward" and q["gy"] == 2 and _partial(q)),
    ("forward: gridDim.y = 3, last M tile partial", lambda q: q["kind"] == "forward" and q["gy"] == 3 and _partial(q)),
    ("dgrad:   gridDim.y = 2, last M tile partial (2 C_l = 72; no dgrad of these shapes writes more than 128 channels)",
     lambda q: q["kind"] == "dgrad" and q["gy"] == 2 and _partial(q)),
    ("wgrad:   gridDim.y = 2, last M tile partial", lambda q: q["kind"] == "wgrad" and q["gy"] == 2 and _partial(q)),
    ("wgrad:   gridDim.y = 3, last M tile partial", lambda q: q["kind"] == "wgrad" and q["gy"] == 3 and _partial(q)),
    ("dgrad:   MT = 4 reading more than 64 channels of dy", lambda q: q["kind"] == "dgrad" and q["MT"] == 4 and q["cin"] > 64),
    ("wgrad:   K = cin * 9 no multiple of 64 and gridDim.x > 1", lambda q: q["kind"] == "wgrad" and q["K"] % 64 != 0 and q["gx"] > 1),
    ("wgrad:   N H W % 4 != 0 under MT = 4 (dead pixel lanes in the last step)", lambda q: q["kind"] == "wgrad" and q["P"] % 4 != 0 and q["MT"] == 4),
    ("wgrad:   N H W % 4 != 0 in a single split", lambda q: q["kind"] == "wgrad" and q["P"] % 4 != 0 and q["nsplit"] == 1),
    ("wgrad:   nsplit > 1, the last split shorter than chunk, under MT = 4", lambda q: q["kind"] == "wgrad" and q["nsplit"] > 1 and q["last"] < q["chunk"] and q["MT"] == 4),
    ("wgrad:   a split boundary inside an image row, under MT = 4", lambda q: q["kind"] == "wgrad" and q["nsplit"] > 1 and q["chunk"] % q["W"] != 0 and q["MT"] == 4),
    ("forward: an up-sampled source under MT = 4", lambda q: q["kind"] == "forward" and q["up"] and q["MT"] == 4),
    ("wgrad:   an up-sampled source under MT = 4", lambda q: q["kind"] == "wgrad" and q["up"] and q["MT"] == 4),
    ("B = 3", lambda q: q["B"] == 3),
    ("a call with batch < max_batch and T < max_steps", lambda q: q["room"][0] > 0 and q["room"][1] > 0),
]

# the constants of csrc/prednet_train.hip the selection reads
WGRAD_WAVES, SLAB_FLOATS, BIAS_SLICES = 2048, 16 << 20, 64


def _mt(cout):
    return 1 if cout <= 16 else 2 if cout <= 32 else 4


def conv_plan(cout, H, W, N):
    """conv() / launch_conv_mt of csrc/prednet_train.hip: MT and the grid (x over 64 pixels, y over 16 MT channels)"""
    MT = _mt(cout)
    return dict(MT=MT, gx=(N * H * W + 63) // 64, gy=(cout + 16 * MT - 1) // (16 * MT), P=N * H * W)


def slab_floats(ch):
    """plan_layout's split-K slab: the largest weight gradient, at least SLAB_FLOATS"""
    slab = 0
    for l, C in enumerate(ch):
        if l > 0:
            slab = max(slab, C * 2 * ch[l - 1] * 9)
        if l < len(ch) - 1:
            slab = max(slab, 4 * C * ch[l + 1] * 9)
        slab = max(slab, 4 * C * 2 * C * 9, BIAS_SLICES * 4 * C)
    return max(slab, SLAB_FLOATS)


def wgrad_plan(cout, cin, H, W, N, slab):
    """wgrad() of csrc/prednet_train.hip, line by line: MT, grid, nsplit and chunk"""
    P, K = N * H * W, cin * 9
    MT = _mt(cout)
    gx, gy = (K + 63) // 64, (cout + 16 * MT - 1) // (16 * MT)
    ns = WGRAD_WAVES // (gx * gy)
    ns = min(ns, slab // (cout * K))
    ns = min(ns, (P + 255) // 256)
    ns = max(ns, 1)
    chunk = (P + ns - 1) // ns
    chunk = (chunk + 3) & ~3
    ns = (P + chunk - 1) // chunk
    return dict(MT=MT, gx=gx, gy=gy, nsplit=ns, chunk=chunk, P=P, K=K, last=P - (ns - 1) * chunk)


def launches(w, h, ch, B, T, room=(0, 0)):
    """Every conv() and wgrad() launch of one gradient call (forward_step, backward_step, weight_gradients of
    csrc/prednet_train.hip) with its plan: dicts of kind, name, cout, cin, H, W, up and the plan's entries.  A forward or dgrad
    launch covers the B samples of one step; a wgrad covers the tape's T B samples.  The ConvLSTM forward is one launch of three
    sources; its up-sampled source is listed as a launch of its own."""
    L, slab, out = len(ch), slab_floats(ch), []

    def add(kind, name, cout, cin, l, up=0):
        H, W = h >> l, w >> l
        plan = wgrad_plan(cout, cin, H, W, T * B, slab) if kind == "wgrad" else conv_plan(cout, H, W, B)
        out.append(dict(plan, kind=kind, name=name, cout=cout, cin=cin, H=H, W=W, up=up, B=B, T=T, room=room))

    for l, C in enumerate(ch):
        if l > 0:
            add("forward", "ConvA%d" % l, C, 2 * ch[l - 1], l - 1)
            add("dgrad", "ConvA%d" % l, 2 * ch[l - 1], C, l - 1)
            add("wgrad", "ConvA%d" % l, C, 2 * ch[l - 1], l - 1)
        add("forward", "ConvLSTM%d/x0+h" % l, 4 * C, 3 * C, l)
        add("dgrad", "ConvLSTM%d/x0" % l, 2 * C, 4 * C, l)
        add("dgrad", "ConvLSTM%d/h" % l, C, 4 * C, l)
        add("wgrad", "ConvLSTM%d/x0" % l, 4 * C, 2 * C, l)
        add("wgrad", "ConvLSTM%d/h" % l, 4 * C, C, l)
        if l < L - 1:
            add("forward", "ConvLSTM%d/x1" % l, 4 * C, ch[l + 1], l, up=1)
            add("dgrad", "ConvLSTM%d/x1" % l, ch[l + 1], 4 * C, l)
            add("wgrad", "ConvLSTM%d/x1" % l, 4 * C, ch[l + 1], l, up=1)
        add("forward", "ConvP%d" % l, C, C, l)
        add("dgrad", "ConvP%d" % l, C, C, l)
        add("wgrad", "ConvP%d" % l, C, C, l)
    return out


# ---- the one list of gradient cases: tests/test_gpu_train*.py and tests/test_gpu_frame_grad.py parametrize over it, and
# tests/test_train_cases_host.py checks on the CPU, with the reference alone, that every case compares something.
# group: the GPU test that runs it; seed: of `_drifting`; objective "mse" / "error" with lam (None under "mse"); n_fed None: every
# step reads its frame; sw: step weights or None; room: (max_batch - B, max_steps - T) of the handle.
Case = namedtuple("Case", "group w h ch B T seed wset objective lam n_fed requant sw room")

STEP_WEIGHTS = {"ones": None, "leading_zero": [0.0, 1.0, 0.5, 2.0, 1.5], "self_fed_only": [0.0, 0.0, 0.0, 1.0, 1.0]}
T_SELF, N_FED = 6, 3
# (n_fed, requant, step weights) of the error-objective cases: teacher-forced; three self-fed steps, float and requantised; and
# the latter with step weights (term s is prediction s against frame s + 1; the zero exercises a term whose seed is left out)
OBJ_CALLS = {"teacher_forced": (None, False, None), "self_fed": (N_FED, False, None), "self_fed_requant": (N_FED, True, None),
             "self_fed_requant_weighted": (N_FED, True, [0.0, 1.0, 0.5, 2.0, 1.5])}
# frame gradients, (B, T, n_fed, requant): teacher-forced; self-fed, float and requantised; the shortest call.  12x8 gray at B = 2
# is 192 elements, less than one block of the element-wise kernels; 16x12 colour at B = 3 is 1728, 6.75 blocks
FRAME_CALLS = [(2, 5, 5, 0), (3, 5, 3, 0), (3, 5, 3, 1), (2, 2, 2, 0)]
WSETS = ["synthetic", "random", "live"]


def lam_of(name, L):
    return {"l0": [1.0] + [0.0] * (L - 1), "lall": [1.0] + [0.1] * (L - 1)}[name]


def frame_sw(weighted, T):
    """non-uniform step weights with a zero among them (a term whose target path is left out)"""
    return None if not weighted else [2.0] if T == 2 else [0.5, 1.0, 0.0, 2.0, 1.5][:T - 1]


def _cases():
    out = []
    case = lambda group, w, h, ch, B, T, wset, objective="mse", lam=None, n_fed=None, requant=False, sw=None, room=(0, 0), seed=None: out.append(
        Case(group, w, h, tuple(ch), B, T, w + len(ch) if seed is None else seed, wset, objective, None if lam is None else tuple(lam), n_fed, bool(requant),
             None if sw is None else tuple(sw), room))
    for w, h, ch in SHAPES:
        L = len(ch)
        for wset in WSETS:
            case("teacher_forced", w, h, ch, 2, 5, wset)
            for requant in (False, True):
                for wkey in STEP_WEIGHTS:
                    case("self_fed", w, h, ch, 2, T_SELF, wset, n_fed=N_FED, requant=requant, sw=STEP_WEIGHTS[wkey])
        for name in ("l0", "lall"):
            for n_fed, requant, sw in OBJ_CALLS.values():
                case("error_objective", w, h, ch, 2, T_SELF, "synthetic", "error", lam_of(name, L), n_fed, requant, sw)
        for wset in WSETS:
            for objective in ("mse", "error"):
                for B, T, n_fed, requant in FRAME_CALLS:
                    for weighted in (False, True):
                        case("frames", w, h, ch, B, T, wset, objective, [1.0] + [0.1] * (L - 1) if objective == "error" else None, n_fed, requant,
                             frame_sw(weighted, T), seed=w + L + B)
    w, h, ch = SHAPES[1]
    for name in ("l0", "lall"):
        case("error_objective_random", w, h, ch, 2, T_SELF, "random", "error", lam_of(name, len(ch)), *OBJ_CALLS["self_fed_requant"])
    # the wide shapes: not the cross product.  Every shape runs both calls of WIDE_CALLS under every kind of comparison once
    for w, h, ch, B in WIDE_SHAPES:
        L = len(ch)
        (T0, *room0), (T1, *room1) = WIDE_CALLS
        case("teacher_forced", w, h, ch, B, T0, "live", room=tuple(room0))
        case("teacher_forced", w, h, ch, B, T1, "synthetic", room=tuple(room1))
        case("self_fed", w, h, ch, B, T0, "live", n_fed=N_FED, requant=True, sw=STEP_WEIGHTS["leading_zero"], room=tuple(room0))
        case("self_fed", w, h, ch, B, T1, "synthetic", n_fed=N_FED, requant=False, room=tuple(room1))
        case("error_objective", w, h, ch, B, T0, "live", "error", lam_of("lall", L), N_FED, True, STEP_WEIGHTS["leading_zero"], room=tuple(room0))
        case("error_objective", w, h, ch, B, T1, "synthetic", "error", lam_of("lall", L), None, False, None, room=tuple(room1))
        case("frames", w, h, ch, B, T0, "live", "error", lam_of("lall", L), N_FED, True, frame_sw(True, T0), room=tuple(room0), seed=w + L + B)
        case("frames", w, h, ch, B, T1, "synthetic", "mse", None, T1, False, None, room=tuple(room1), seed=w + L + B)
    return out


ALL_CASES = _cases()
ALL_GRAD_CASES = [c for c in ALL_CASES if c.group != "frames"]


def cases(group, wide=None):
    """the cases of one GPU test; wide: None all, False those at SHAPES, True those at WIDE_SHAPES"""
    is_wide = lambda c: (c.w, c.h, list(c.ch)) not in SHAPES
    return [c for c in ALL_CASES if c.group == group and (wide is None or is_wide(c) == wide)]


def select(group, w, h, ch, **fields):
    """the cases of a group at one shape whose fields have the given values"""
    fields = {k: tuple(v) if isinstance(v, list) else v for k, v in fields.items()}
    return [c for c in ALL_CASES if c.group == group and (c.w, c.h, c.ch) == (w, h, tuple(ch)) and all(getattr(c, k) == v for k, v in fields.items())]


def case_id(c):
    return "%dx%d-%s-B%dT%d-%s-%s%s-fed%s%s-%s%s" % (c.w, c.h, "_".join(map(str, c.ch)), c.B, c.T, c.wset, c.objective,
                                                    "" if c.lam is None else ("_l0" if not any(c.lam[1:]) else "_lall"), "all" if c.n_fed is None else c.n_fed,
                                                    "q" if c.requant else "", "ones" if c.sw is None else "w" + "_".join("%g" % v for v in c.sw),
                                                    "" if c.room == (0, 0) else "-room%d_%d" % c.room)


def is_dead(c):
    """The declared dead cases: the "random" set at a gray shape of SHAPES drives every pixel of P0 into the clamp on every step.
    No gradient passes the clamp, so under the squared error and under L_0 every weight gradient is exactly zero (the
    `zero_allowed` cases of `_check_grads`), and a frame gradient keeps its target path alone."""
    return c.wset == "random" and c.ch[0] == 1 and (c.w, c.h, list(c.ch)) in SHAPES


def is_clamped(c):
    """The "random" set at the colour shape of SHAPES: kept as it was, every tensor has a gradient, but more than half of P0 (two
    thirds) sits at the clamp.  It is the one live case that exercises the clamp's mask on a mixed map, and the one exception to
    the cap of one half that tests/test_train_cases_host.py puts on every other live case."""
    return c.wset == "random" and (c.w, c.h, list(c.ch)) == SHAPES[1]


def is_all_zero(c):
    return is_dead(c) and (c.objective == "mse" or not any(c.lam[1:]))


@functools.lru_cache(maxsize=None)
def case_weights(w, h, ch, wset):
    """one weight set of one shape, made once (read-only by convention)"""
    return dict(_weight_sets(list(ch), w, h))[wset]


@functools.lru_cache(maxsize=None)
def case_frames(c):
    return _drifting(c.seed, c.B, c.T, c.ch[0], c.h, c.w)


def case_kwargs(c):
    """the keywords of oracle.prednet_train_ref.run (and of frame_grad_support.run_frames) that state the case"""
    return dict(objective=c.objective, layer_weights=None if c.lam is None else list(c.lam), n_fed=c.n_fed, requant=c.requant,
                step_weights=None if c.sw is None else list(c.sw))


def case_reference(c, pred=None, dtype=torch.float64, run=None):
    """The reference of a case.  pred: the float32 predictions whose bytes a requantised case is fed (the GPU's own; tests/
    test_gpu_train_ext.py says why).  None: the run is repeated on its own requantised predictions until every self-fed step has
    read them (one more step is settled by each run), which is what a host test has."""
    from oracle import prednet_train_ref
    run = run or prednet_train_ref.run
    kw = dict(case_kwargs(c), dtype=dtype)
    wts, frames = case_weights(c.w, c.h, c.ch, c.wset), case_frames(c)
    if not c.requant:
        return run(wts, list(c.ch), frames, **kw)
    if pred is not None:
        return run(wts, list(c.ch), frames, fed=_fed_from(pred), **kw)
    fed = np.zeros(frames.shape, np.float32)
    for _ in range(c.T - c.n_fed + 1):
        r = run(wts, list(c.ch), frames, fed=fed, **kw)
        fed = _fed_from(r.pred.astype(np.float32))
    return r


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
