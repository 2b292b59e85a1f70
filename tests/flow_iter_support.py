"""Shared by tests/test_flow_iter_host.py and tests/test_gpu_flow_iter.py ("The iterated solve's gradient"):
(a) `torch_iter_field`, the float64 torch statement of the pyramidal, iterated solve (include/eigen_engine.h eigen_dense_solve,
    tests/dense_pyr_support.py) with the prediction AND the reference in the graph: `torch.where` for the sampler's two clamps,
    `floor(...).detach()`, index gathers for the taps.  Its forward is `dense_pyr_support.dense_pyr_ref` up to the order of the sums.
    The three cut variants (coarse path detached, sampling position held constant, windows summed in reverse order) are keywords.
(b) `torch_iter_term`, the flow term on that field (the displacement modes of tests/flow_obj_support.py, the scores of
    tests/flow_score_support.py and tests/flow_struct_support.py), and `IterTerm`, which plugs it into `flow_obj_support.run_flow(term=...)`
    the way `flow_pair_support.PairTerm` does.
(c) the stage cases (the shapes of `dense_pyr_support.GPU_CASES`, float images from `shift_case`), their modes and the reference of a
    case, made once.
torch on the CPU only; no GPU."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import dense_pyr_support as dp
from tests import flow_obj_support as fs
from tests import flow_score_support as ss
from tests import flow_struct_support as st

FLOW_ITER_KERNELS = ["tfiter_gray_kernel", "tfiter_fwd_kernel", "tfiter_adj_kernel", "tfiter_umax_kernel", "tfiter_i1_kernel", "tfiter_q_kernel", "tfiter_i0_kernel",
                     "tfiter_down_kernel", "tfiter_pyr_adj_kernel", "tfiter_store_kernel", "tfiter_value_kernel", "tfiter_score_g_kernel"]
EPS = dp.EPS
BOUND = 2.0 ** -23      # of max |ref| per tensor: the single rounding of the float32 store is 2^-24 relative, doubled
REORDER = 2.0 ** -30    # of max |ref|: what summing the reference's windows in reverse order may move it by


# ---- (a) the solve in torch
def _gray(v):
    return v[:, 0] if v.shape[1] == 1 else (0.299 * v[:, 0] + 0.587 * v[:, 1]) + 0.114 * v[:, 2]


def _reduce_last(a):
    n = a.shape[-1]
    c = 2 * np.arange((n + 1) // 2)
    t = [a[..., torch.from_numpy(np.asarray(dp._reflect(c + k, n)))] for k in (-2, -1, 0, 1, 2)]
    return (((t[0] + t[4]) + 4.0 * (t[1] + t[3])) + 6.0 * t[2]) / 16.0


def _pyr_down(a):
    return _reduce_last(_reduce_last(a).transpose(-1, -2)).transpose(-1, -2)


def _scharr(I0):
    H, W = I0.shape[-2:]
    ap = F.pad(I0[:, None], (1, 1, 1, 1), mode="replicate")[:, 0]
    a = lambda dy, dx: ap[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    Ix = ((3.0 * (a(-1, 1) - a(-1, -1)) + 10.0 * (a(0, 1) - a(0, -1))) + 3.0 * (a(1, 1) - a(1, -1))) / 32.0
    Iy = ((3.0 * (a(1, -1) - a(-1, -1)) + 10.0 * (a(1, 0) - a(-1, 0))) + 3.0 * (a(1, 1) - a(-1, 1))) / 32.0
    return Ix, Iy


def _sample(I1, x, y):
    """the sampler S on [B, H, W] planes: the two clamps as torch.where (a clamped coordinate passes no gradient), floor detached,
    x1 = min(x0 + 1, W - 1), the taps as index gathers"""
    B, H, W = I1.shape
    x = torch.where(x > 0.0, x, torch.zeros_like(x))
    x = torch.where(x < W - 1.0, x, torch.full_like(x, W - 1.0))
    y = torch.where(y > 0.0, y, torch.zeros_like(y))
    y = torch.where(y < H - 1.0, y, torch.full_like(y, H - 1.0))
    xf, yf = torch.floor(x).detach(), torch.floor(y).detach()
    x0, y0 = xf.long(), yf.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    fx, fy = x - xf, y - yf
    b = torch.arange(B)[:, None, None]
    v00, v01, v10, v11 = I1[b, y0, x0], I1[b, y0, x1], I1[b, y1, x0], I1[b, y1, x1]
    top = v00 + fx * (v01 - v00)
    bot = v10 + fx * (v11 - v10)
    return top + fy * (bot - top)


def _iterate(I0, I1, Ix, Iy, a, b, c, det, ux, uy, r, hold_position, reverse, clamped):
    B, H, W = I0.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    px, py = (ux.detach(), uy.detach()) if hold_position else (ux, uy)
    offsets = range(r, -r - 1, -1) if reverse else range(-r, r + 1)
    bx = by = None
    for dy in offsets:
        qy = ys + dy
        oky = (qy >= 0) & (qy < H)
        qyc = qy.clamp(0, H - 1)
        rx = ry = None
        for dx in offsets:
            qx = xs + dx
            ok = (oky & (qx >= 0) & (qx < W)).to(I0.dtype)
            qxc = qx.clamp(0, W - 1)
            sx_, sy_ = qxc.to(I0.dtype) + px, qyc.to(I0.dtype) + py
            if clamped is not None:
                out = (sx_ < 0) | (sx_ > W - 1) | (sy_ < 0) | (sy_ > H - 1)     # strictly outside: a clamp replaced the coordinate
                clamped[0] += int((out & (ok > 0)).sum())
            d = _sample(I1, sx_, sy_) - I0[:, qyc, qxc]
            tx, ty = ok * (Ix[:, qyc, qxc] * d), ok * (Iy[:, qyc, qxc] * d)
            rx, ry = (tx, ty) if rx is None else (rx + tx, ry + ty)
        bx, by = (rx, ry) if bx is None else (bx + rx, by + ry)
    return ux + -((c * bx - b * by) / det), uy + -((a * by - b * bx) / det)


def torch_iter_field(P, x, r, eps, levels, iters, cut_coarse=False, hold_position=False, reverse=False, all_levels=False, clamped=None):
    """The field u [B, 2, H, W] of level 0 of prediction P against the reference x, both [B, C, H, W] float64 and in the graph where the
    caller left them there.  cut_coarse: every level starts from the DETACHED field of the level above; hold_position: the sampling
    position is a constant (no path through grad S); reverse: the windows are summed in the opposite order; all_levels: the list of
    the fields of every level, finest first; clamped: a one-element list that receives how many window positions were sampled at a
    coordinate strictly outside the image, which a clamp replaced."""
    I0, I1 = [_gray(x)], [_gray(P)]
    for _ in range(levels - 1):
        I0.append(_pyr_down(I0[-1]))
        I1.append(_pyr_down(I1[-1]))
    ones = torch.ones(1, 1, 2 * r + 1, 2 * r + 1, dtype=P.dtype)
    ws = lambda f: F.conv2d(f[:, None], ones, padding=r)[:, 0]    # zero padding of a sum is truncation
    fields, ux, uy = [], None, None
    for l in range(levels - 1, -1, -1):
        B, H, W = I0[l].shape
        if ux is None:
            ux, uy = torch.zeros(B, H, W, dtype=P.dtype), torch.zeros(B, H, W, dtype=P.dtype)
        else:
            if cut_coarse:
                ux, uy = ux.detach(), uy.detach()
            yy, xx = torch.arange(H)[:, None] >> 1, torch.arange(W)[None, :] >> 1
            ux, uy = 2.0 * ux[:, yy, xx], 2.0 * uy[:, yy, xx]
        Ix, Iy = _scharr(I0[l])
        a, c, b = ws(Ix * Ix) + eps, ws(Iy * Iy) + eps, ws(Ix * Iy)
        det = a * c - b * b
        for _ in range(iters):
            ux, uy = _iterate(I0[l], I1[l], Ix, Iy, a, b, c, det, ux, uy, r, hold_position, reverse, clamped)
        fields.insert(0, torch.stack([ux, uy], 1))
    return fields if all_levels else fields[0]


# ---- (b) the term
def value_of_field(u, direction=None, mask=None, score=None):
    """(f, its un-cancelled scale) of a torch field u [B, 2, H, W]: the displacement modes of `flow_obj_support.torch_flow_term`, or the
    score of a `flow_score_support.Score` / `flow_struct_support.Bands` / `Free`"""
    B, _, H, W = u.shape
    if isinstance(score, ss.Score):
        f = ss.torch_score_of_field(u, mask, score).sum() / float(B)
        return f, float(f.detach().abs())
    if score is not None:
        S, scales = st.torch_struct_of_field(u, mask, score)
        return S.sum() / float(B), float(scales.sum() / B)
    ux, uy = u[:, 0], u[:, 1]
    if direction is None:
        v = ux * ux + uy * uy
    else:
        d = torch.from_numpy(np.asarray(direction, np.float32)).to(u.dtype)
        v = d[0] * ux + d[1] * uy
    m = torch.ones(H, W, dtype=u.dtype) if mask is None else torch.from_numpy((np.asarray(mask) != 0).astype(np.float64)).to(u.dtype)
    div = float(B) * float(m.sum())
    return (m * v).sum() / div, float((m * v.detach().abs()).sum() / div)


def torch_iter_term(P, x, r, eps, levels, iters, direction=None, mask=None, score=None, **variants):
    """The flow term through the iterated solve -> (f, its un-cancelled scale, u)"""
    u = torch_iter_field(P, x, r, eps, levels, iters, **variants)
    f, scale = value_of_field(u, direction, mask, score)
    return f, scale, u


class IterTerm:
    """The `term` callback of `flow_obj_support.run_flow` under an iterated solve.  pairing "prediction": term s runs from P0_{s-1} IN THE
    GRAPH (the first reference is `start`, detached), as `flow_pair_support.PairTerm`; "frame": from frame s + 1, a constant unless
    moving.  detach_prev / a constant frame: the reference out of the graph.  single: the single step's term (the statement the trainer
    must NOT match under a real solve).  step_weights: the call's (None: all one); a term of weight zero is not formed, as the trainer
    does not compute it: it is returned as an exact zero that carries no gradient."""

    def __init__(self, start, radius, eps, levels, iters, direction=None, mask=None, score=None, pairing="prediction", moving=False, detach_prev=False,
                 single=False, step_weights=None):
        self.step_weights, self.s = step_weights, 0
        self.prev = None if start is None else start.detach()
        self.args, self.kw = (radius, eps, levels, iters), dict(direction=direction, mask=mask, score=score)
        self.pairing, self.moving, self.detach_prev, self.single = pairing, moving, detach_prev, single

    def __call__(self, P, xn):
        if self.pairing == "prediction":
            ref = self.prev.detach() if self.detach_prev else self.prev
            self.prev = P
        else:
            ref = xn if self.moving else xn.detach()
        s, self.s = self.s, self.s + 1
        if self.step_weights is not None and self.step_weights[s] == 0:
            return P.sum() * 0.0, 0.0
        P, ref = P.to(torch.float64), ref.to(torch.float64)
        if self.single:
            u = fs.torch_flow_term(P, ref, self.args[0], self.args[1], None, None)[2]
            return value_of_field(u, **self.kw)
        return torch_iter_term(P, ref, *self.args, **self.kw)[:2]


# ---- (c) the stage cases: (name, w, h, C, levels, iters, radius, genome seeds, shifts), one sample per seed
STAGE_CASES = [("8x8", 8, 8, 1, 2, 2, 7, (2,), ((0.7, -0.4),)),                                  # less than a tile, a 4 x 4 coarsest level
               ("20x15r3", 20, 15, 3, 3, 2, 3, (21, 23), ((2.5, 1.5), (-0.6, 0.5))),             # odd sizes, border clamps
               ("20x15r7", 20, 15, 3, 3, 2, 7, (21, 23), ((2.5, 1.5), (-0.6, 0.5))),
               ("48x32", 48, 32, 3, 2, 3, 7, (63, 76, 63), ((2.5, 1.5), (1.25, -0.75), (5.5, -4.5))),   # 3 x 2 tiles, taps and reach beyond the patch
               ("16x12", 16, 12, 1, 1, 5, 7, (76, 13), ((0.25, -0.125), (0.5, 0.75))),
               ("40x24r16", 40, 24, 1, 2, 2, 16, (63,), ((1.25, -0.75),))]                       # the dynamic-LDS attribute
STAGE_NAMES = [c[0] for c in STAGE_CASES]
MODES = ("energy", "horizontal", "circles", "bands", "free")   # "horizontal": a direction field that does not cancel over a uniform shift
# the scores' limits on fields of several pixels: every moving pixel can be a member
SCORE_LIMITS = dict(max_norm=8.0, min_norm=1e-3)


def stage_case(name):
    return next(c for c in STAGE_CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def stage_images(name):
    """(img0, img1 uint8 [B, C, h, w]): the reference and the prediction of a stage case as bytes"""
    _, w, h, C, _, _, _, seeds, shifts = stage_case(name)
    pairs = [dp.shift_case(w, h, C, seed, shift)[:2] for seed, shift in zip(seeds, shifts)]
    img0, img1 = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    return img0, img1


def as_floats(img):
    """the floats the trainer sees of bytes: (float)byte / 255.0f"""
    return img.astype(np.float32) / np.float32(255.0)


def mode_objects(mode, w, h):
    """(direction or None, the trainer's score object or None) of a mode"""
    from evolutionary_illusion_generator_amd import train
    if mode == "energy":
        return None, None
    if mode == "horizontal":
        return train.flow_direction("horizontal", w, h), None
    if mode == "circles":
        return None, train.FlowScore(min_count=4, **SCORE_LIMITS)
    if mode == "bands":
        return None, train.BandsScore(min_count=4, **SCORE_LIMITS)
    return None, train.FreeScore(min_count=4, **SCORE_LIMITS)


def support_score(score, h):
    """the restatements' score object of a trainer score object (`dense_pyr_support.restatement_score` on the object itself)"""
    from evolutionary_illusion_generator_amd import train
    if score is None:
        return None
    if isinstance(score, train.FlowScore):
        return ss.Score(score.max_norm, score.min_norm, 0.0, h / 2.0, score.weights[0], score.weights[1], score.min_count)
    if isinstance(score, train.BandsScore):
        return st.Bands(score.max_norm, score.min_norm, 0.0, (h / 4.0) * 2.0, score.min_count)
    return st.Free(score.max_norm, score.min_norm, score.max_distance, score.min_count, score.weights)


def make_objective(mode, w, h, r, levels, iters, mask=None, members=None):
    """the trainer's FlowObjective of a mode with the solve on it"""
    from evolutionary_illusion_generator_amd import train
    direction, score = mode_objects(mode, w, h)
    return train.FlowObjective(r, EPS, direction, mask, score=score, members=members).solved(levels, iters)


StageRef = namedtuple("StageRef", "value u seed64 ref64")


def stage_grads(pred, ref, r, eps, levels, iters, modes, h, w, mask=None, scale=1.0, **variants):
    """{mode: StageRef} of float images pred, ref [B, C, H, W]: the field's graph is built once and differentiated per mode.  seed64,
    ref64: scale * d value / d pred, d ref, float64 [B, C, H, W]"""
    P = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    x = torch.tensor(np.asarray(ref, np.float64), requires_grad=True)
    u = torch_iter_field(P, x, r, eps, levels, iters, **variants)
    out = {}
    for mode in modes:
        direction, score = mode_objects(mode, w, h)
        f, _ = value_of_field(u, direction, mask, support_score(score, h))
        gP, gx = torch.autograd.grad(f, [P, x], retain_graph=True, allow_unused=True)
        zero = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.numpy() * scale
        out[mode] = StageRef(float(f.detach()), u.detach().numpy(), zero(gP, P), zero(gx, x))
    return out


@functools.lru_cache(maxsize=None)
def stage_reference(name):
    """{mode: StageRef} of a stage case under every mode, made once"""
    _, w, h, C, levels, iters, r, _, _ = stage_case(name)
    img0, img1 = stage_images(name)
    return stage_grads(as_floats(img1), as_floats(img0), r, EPS, levels, iters, MODES, h, w)


def single_step_grads(pred, ref, r, eps):
    """(d f / d pred, d f / d ref) float64 of the single step's energy term with the reference in the graph"""
    P = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    x = torch.tensor(np.asarray(ref, np.float64), requires_grad=True)
    f = fs.torch_flow_term(P, x, r, eps)[0]
    gP, gx = torch.autograd.grad(f, [P, x])
    return gP.numpy(), gx.numpy()


def within(got, ref, bound=BOUND):
    """(max |got - ref|, bound * max |ref|) of one tensor"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()), bound * float(np.abs(ref).max())


# ---- (d) the training cases: prediction pairing, 2 levels x 2 iterations, `live` weights, from `flow_pair_support.FLOW_SHAPES` (all
# four halve once to at least 4 pixels); forms "still" (the population term, weights [0, 0, 0, 0, 1], float and requantised feedback)
# and "drifting"; the energy mode and the Circles score; r 3 and 7.  tests/test_flow_iter_host.py keeps every case under the project's
# float32 yardstick on the reference alone; a case that sits on a kink of the sampler is re-seeded there (TRAIN_SEEDS), not excused.
TRAIN_LEVELS, TRAIN_ITERS = 2, 2
YARDSTICK = 8.07e-5     # network in float32 against float64, worst element of a tensor over its maximum (tests/train_support.py)
# {case id: the seed of its "live" weights} where `flow_pair_support.pair_case_weights`' own leaves the yardstick little room.  The requantised
# Circles case measured 6.23e-5 (ConvLSTM0/h_c/b, a bias gradient in which the steps' contributions nearly cancel) with the default seed:
# under the bound, but float32 CPU convolutions may differ by that much between hosts.  Seeds 3, 4 and 5 give 2.7e-5, 4.1e-6 and 4.8e-4.
TRAIN_SEEDS = {"24x16-1_3_4_5-circles-r3-still_requant": 4}


def _train_cases():
    from tests import flow_pair_support as ps
    rows = ((0, "energy", 3, "still"), (1, "energy", 7, "drifting"), (2, "circles", 3, "still_requant"), (3, "circles", 7, "drifting"),
            (1, "circles", 3, "still"), (2, "energy", 7, "drifting"))
    return [ps.PairCase(ps.FLOW_SHAPES[i][0], ps.FLOW_SHAPES[i][1], tuple(ps.FLOW_SHAPES[i][2]), "live", mode, r, form) for i, mode, r, form in rows]


TRAIN_CASES = _train_cases()


def train_case_id(c):
    from tests import flow_pair_support as ps
    return ps.pair_case_id(c)


def train_case_weights(c):
    from tests import flow_pair_support as ps
    from tests.train_support import _random_weights
    seed = TRAIN_SEEDS.get(train_case_id(c))
    if seed is None:
        return ps.pair_case_weights(ps.PairCase(c.w, c.h, c.ch, c.wset, "energy", c.r, c.form))
    wts = _random_weights(list(c.ch), c.w, c.h, seed=seed)
    wts["ConvP0/b"] = np.full_like(wts["ConvP0/b"], 0.5)
    return wts


def train_case_score(c):
    """the trainer's score object of a training case (None: the energy mode); predictions move by tenths of a pixel to a few pixels"""
    from evolutionary_illusion_generator_amd import train
    return train.FlowScore(max_norm=2.0, min_norm=1e-3, min_count=4) if c.mode == "circles" else None


def train_case_flow(c):
    """the trainer's objective of a training case"""
    from evolutionary_illusion_generator_amd import train
    return train.PredictionFlow(c.r, 1e-2).scored(train_case_score(c)).solved(TRAIN_LEVELS, TRAIN_ITERS)


def train_case_reference(c, fed=None, dtype=torch.float64, leaf="frames", **variant):
    """`run_flow` of a training case under `IterTerm`; fed: the requantised feedback of a "still_requant" case (the GPU's own, or None:
    the run is repeated on its own, as `flow_pair_support.pair_case_reference` does); variant: detach_prev=True or single=True"""
    from tests import flow_pair_support as ps
    from tests.train_support import _fed_from
    frames, wts, call = ps.pair_case_frames(c), train_case_weights(c), ps.pair_case_call(c)
    B, T = frames.shape[:2]

    def run(fed):
        start = torch.zeros(B, c.ch[0], c.h, c.w, dtype=dtype)
        term = IterTerm(start, c.r, 1e-2, TRAIN_LEVELS, TRAIN_ITERS, score=support_score(train_case_score(c), c.h), step_weights=call["step_weights"], **variant)
        return fs.run_flow(wts, list(c.ch), frames, term=term, leaf=leaf, fed=fed, dtype=dtype, **call)

    if not call["requant"] or fed is not None:
        return run(fed)
    fed = np.zeros(frames.shape, np.float32)
    for _ in range(T - call["n_fed"] + 1):
        r = run(fed)
        fed = _fed_from(r.pred.astype(np.float32))
    return r


# ---- (e) refinement through the solve on the reference alone: `flow_ref_support.refine_loop` (n_repeat 4, n_ext 2, 8 steps of 2 bytes, float
# feedback, the left quarter kept) under `DenseFitness.solve_objective()`, the Circles score at 2 levels x 2 iterations, the population term
REFINE_SHAPE = (16, 12, (3, 4, 6))
REFINE_LEVELS, REFINE_ITERS, REFINE_RADIUS = 2, 2, 3     # a 7-pixel window: the autograd statement walks every window offset in Python


def refine_fitness():
    """the DenseFitness whose `solve_objective()` the refinement climbs"""
    from evolutionary_illusion_generator_amd import fitness, train
    return fitness.DenseFitness(train.FlowScore(max_norm=2.0, min_norm=1e-3, min_count=4), radius=REFINE_RADIUS, eps=1e-2, levels=REFINE_LEVELS, iters=REFINE_ITERS)


@functools.lru_cache(maxsize=None)
def refine_reference():
    """-> (stills uint8, history float64 [iters + 1]) of `refine_stills` with `refine_fitness().solve_objective()` on float64 autograd alone"""
    from tests import flow_ref_support as rs
    w, h, ch = REFINE_SHAPE
    score = support_score(refine_fitness().score, h)

    def run(weights, channels, frames, *, radius, eps, direction, mask, **kw):
        B, _, C, H, W = frames.shape
        # `refine_loop` states its own radius; the objective's is the fitness's
        term = IterTerm(torch.zeros(B, C, H, W, dtype=torch.float64), REFINE_RADIUS, eps, REFINE_LEVELS, REFINE_ITERS, score=score, step_weights=kw["step_weights"])
        return fs.run_flow(weights, channels, frames, term=term, **kw)

    return rs.refine_loop(run, [0.0] * rs.REFINE["n_repeat"] + [1.0] * (rs.REFINE["n_ext"] - 1), w, h, ch, "energy")


@functools.lru_cache(maxsize=None)
def refine_genomes_reference():
    """`train.refine_genomes` with `refine_fitness().solve_objective()` at the setting of tests/cppn_grad_support.py `SIM`, simulated with
    the references alone as tests/test_cppn_grad_host.py `simulate_refine` does: the render and its quantisation in numpy, `run_flow`
    under `IterTerm` with the tied leaf for the trainer call (float feedback, the population term's weights), `grads_reverse` for the
    CPPN's parameter gradients and `train.genome_update` itself for the update.  -> (genomes, history float64 [iters + 1])"""
    import copy
    from evolutionary_illusion_generator_amd import fitness, genome, train
    from tests import cppn_grad_support as S
    from tests.train_support import _weight_sets
    SIM = S.SIM
    w, h, ch, n_repeat, n_ext = SIM["w"], SIM["h"], SIM["ch"], SIM["n_repeat"], SIM["n_ext"]
    weights = dict(_weight_sets(list(ch), w, h))["live"]
    cfg, genomes = S.sim_genomes()
    leaves = [np.asarray(p, np.float64).reshape(-1) for p in fitness.leaf_planes(SIM["structure"], w, h, 2)]
    out = [copy.deepcopy(g) for g in genomes]
    maps = [genome.flatten_genome_map(g, cfg) for g in out]
    T, sw = n_repeat + n_ext, [0.0] * n_repeat + [1.0] * (n_ext - 1)
    score = support_score(refine_fitness().score, h)
    history = np.zeros(SIM["iters"] + 1)

    def loss_of():
        flats = [genome.flatten_genome(g, cfg) for g in out]
        img = np.stack([S.quantise(S.forward_np(f, leaves)[0], f, leaves, ch[0]) for f in flats]).reshape(len(out), ch[0], h, w)
        frames = np.ascontiguousarray(np.repeat(img[:, None], T, 1))
        term = IterTerm(torch.zeros(len(out), ch[0], h, w, dtype=torch.float64), REFINE_RADIUS, 1e-2, REFINE_LEVELS, REFINE_ITERS, score=score, step_weights=sw)
        r = fs.run_flow(weights, list(ch), frames, term=term, n_fed=n_repeat, requant=False, step_weights=sw, leaf="tied")
        return r.loss, r.frame_grad.astype(np.float32), flats

    for i in range(SIM["iters"]):
        history[i], grad, flats = loss_of()
        for g, m, f, gi in zip(out, maps, flats, grad):
            g_w, g_bias, g_resp = S.grads_reverse(f, leaves, gi.reshape(ch[0], -1), ch[0])
            train.genome_update(g, m, g_bias, g_resp, g_w, SIM["lr"])
    history[SIM["iters"]] = loss_of()[0]
    return out, history
