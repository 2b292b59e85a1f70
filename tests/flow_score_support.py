"""Shared by tests/test_flow_score_host.py and tests/test_gpu_flow_score.py ("The score mode"):
(a) `score_ref`, the numpy float64 restatement of csrc/flow_score_kernels.h on a field u, with its own exactly summed moments or with a
    given per-sample record, and `score_stage_ref`, the flow stage around it (the planes, the solve, q from the score's gradient, the
    seed and the reference gradient, in the operations and orders of tests/flow_obj_support.py `flow_stage_ref`);
(b) `torch_score_term`, the autograd statement on `flow_obj_support.torch_flow_term`'s u with membership detached, and the `term`
    callbacks of `run_flow` for both pairings;
(c) the cases;
(d) the names of the kernels of the new header.
It imports tests/flow_obj_support.py and tests/flow_pair_support.py and changes neither."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from tests import flow_obj_support as fs
from tests import flow_pair_support as ps

FLOW_SCORE_KERNELS = ["tflow_score_moment_kernel", "tflow_score_final_kernel", "tflow_score_q_kernel"]
REC = 10        # SCORE_REC of csrc/flow_score_kernels.h: N, m_rho, m_tau, m_a, m_n, V_rho, V_tau, V_n, S_b, spare
SLICES = 16     # SCORE_SLICES

Score = namedtuple("Score", "max_norm min_norm r_min r_max w_direction w_strength min_count")


def flow_of(sc, radius, eps=1e-2, mask=None, pairing="frame", reference="constant"):
    """the FlowObjective or PredictionFlow of a Score"""
    from evolutionary_illusion_generator_amd import train
    return train.make_flow(pairing, radius, eps, None, mask, reference=reference, score=as_flow_score(sc))


def as_flow_score(sc):
    """the train.FlowScore of a Score"""
    from evolutionary_illusion_generator_amd import train
    return train.FlowScore(sc.max_norm, sc.min_norm, (sc.r_min, sc.r_max), sc.min_count, (sc.w_direction, sc.w_strength))


# ---- (a) the numpy restatement
Points = namedtuple("Points", "px py dist nrm nx ny rho tau member candidate")


def score_points(u, mask, sc):
    """u float64 [B, 2, H, W] -> the per-pixel quantities of tflow_score_point, [B, H, W] each (zeros where the pixel is no member), and
    `candidate`, the geometric part of membership (mask and ring) alone"""
    B, _, H, W = u.shape
    ux, uy = u[:, 0], u[:, 1]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    px, py = np.broadcast_to(xx - W / 2.0, ux.shape), np.broadcast_to(yy - H / 2.0, ux.shape)
    dist = np.sqrt(px * px + py * py)
    nrm = np.sqrt(ux * ux + uy * uy)
    counted = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    candidate = counted & (dist != 0.0) & (sc.r_min <= dist) & (dist <= sc.r_max)
    member = candidate & (nrm > 0.0) & (sc.min_norm <= nrm) & (nrm <= sc.max_norm)
    sn, sd = np.where(member, nrm, 1.0), np.where(member, dist, 1.0)
    nx, ny = np.where(member, ux / sn, 0.0), np.where(member, uy / sn, 0.0)
    x1, y1 = px + nx, py + ny
    rho = np.where(member, (x1 * px + y1 * py) / sd - dist, 0.0)
    tau = np.where(member, (-x1 * py + y1 * px) / sd, 0.0)
    return Points(px, py, dist, nrm, nx, ny, rho, tau, member, candidate)


def exact_record(u, pts, sc):
    """the per-sample record [B, 10] with every sum formed exactly (math.fsum), then divided: two passes, as np.var"""
    B = u.shape[0]
    rec = np.zeros((B, REC), np.float64)
    for b in range(B):
        m = pts.member[b]
        N = int(m.sum())
        rec[b, 0] = N
        if N == 0:
            continue
        cols = [pts.rho[b][m], pts.tau[b][m], np.abs(u[b, 0][m]), pts.nrm[b][m]]
        for k, v in enumerate(cols):
            rec[b, 1 + k] = math.fsum(v.tolist()) / N
        for k, (v, mean) in enumerate(((cols[0], rec[b, 1]), (cols[1], rec[b, 2]), (cols[3], rec[b, 4]))):
            d = v - mean
            rec[b, 5 + k] = math.fsum((d * d).tolist()) / N
        rec[b, 8] = sample_value(rec[b], sc)
    return rec


def sample_value(r, sc):
    """S_b of one record, tflow_score_value"""
    N, m_a, Vr, Vt, Vn = r[0], r[3], r[5], r[6], r[7]
    if N < sc.min_count:
        return 0.0
    R = ((1.0 - Vr) * (1.0 - Vr) + (1.0 - Vt) * (1.0 - Vt)) / 2.0
    A = m_a / sc.max_norm
    F = 1.0 - (Vn if Vn < 1.0 else 1.0)
    return sc.w_direction * R + sc.w_strength * (A * F)


ScoreRef = namedtuple("ScoreRef", "value S record g points")


def score_ref(u, mask, sc, record=None):
    """The score mode on a field: u float64 [B, 2, H, W].  record None: the restatement's own exactly summed moments; else a [B, 10]
    record whose moments are taken as they are (the device's), S_b and f being formed from them again.  -> f, S [B], the record,
    g = d S_b / d u [B, 2, H, W] in the order csrc/flow_score_kernels.h fixes, and the per-pixel quantities."""
    u = np.asarray(u, np.float64)
    B = u.shape[0]
    pts = score_points(u, mask, sc)
    rec = exact_record(u, pts, sc) if record is None else np.array(record, np.float64)
    S = np.array([sample_value(rec[b], sc) for b in range(B)])
    total = S[0]
    for b in range(1, B):
        total = total + S[b]
    g = np.zeros_like(u)
    for b in range(B):
        N, m_rho, m_tau, m_a, m_n, Vr, Vt, Vn = rec[b, :8]
        if N < sc.min_count:
            continue
        m = pts.member[b]
        px, py, dist, nrm, nx, ny = (a[b][m] for a in (pts.px, pts.py, pts.dist, pts.nrm, pts.nx, pts.ny))
        rho, tau, ux = pts.rho[b][m], pts.tau[b][m], u[b, 0][m]
        c_rho = -(((sc.w_direction * (1.0 - Vr)) * (2.0 * (rho - m_rho))) / N)
        c_tau = -(((sc.w_direction * (1.0 - Vt)) * (2.0 * (tau - m_tau))) / N)
        gmx = (c_rho * px) / dist - (c_tau * py) / dist
        gmy = (c_rho * py) / dist + (c_tau * px) / dist
        d = gmx * nx + gmy * ny
        gx, gy = (gmx - d * nx) / nrm, (gmy - d * ny) / nrm
        A = m_a / sc.max_norm
        F = 1.0 - (Vn if Vn < 1.0 else 1.0)
        gx = gx + ((sc.w_strength * F) * np.sign(ux)) / (N * sc.max_norm)
        if Vn < 1.0:
            c_n = -(((sc.w_strength * A) * (2.0 * (nrm - m_n))) / N)
        else:
            c_n = np.zeros_like(nrm)
        gx = gx + c_n * nx
        gy = gy + c_n * ny
        g[b, 0][m], g[b, 1][m] = gx, gy
    return ScoreRef(total / float(B), S, rec, g, pts)


StageRef = namedtuple("StageRef", "value u seed seed64 grad grad64 score")


def score_stage_ref(pred, ref64, r, eps, mask, sc, scale=1.0, record=None):
    """The flow stage in the score mode: pred float32 [B, C, H, W]; ref64 float64 [B, C, H, W], the reference as the prep kernel widens it
    (`flow_obj_support.byte_reference` of bytes, or floats widened).  The planes, the solve, the seed and the reference gradient are
    `flow_obj_support.flow_stage_ref`'s operations; q comes from `score_ref`'s g and kappa = scale / B."""
    pred = np.asarray(pred, np.float32)
    B, C, H, W = pred.shape
    I0, I1 = fs._gray(ref64), fs._gray(pred.astype(np.float64))
    It = I1 - I0
    ap = np.pad(I0, ((0, 0), (1, 1), (1, 1)), mode="edge")
    a = lambda dy, dx: ap[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    Ix = ((3.0 * (a(-1, 1) - a(-1, -1)) + 10.0 * (a(0, 1) - a(0, -1))) + 3.0 * (a(1, 1) - a(1, -1))) / 32.0
    Iy = ((3.0 * (a(1, -1) - a(-1, -1)) + 10.0 * (a(1, 0) - a(-1, 0))) + 3.0 * (a(1, 1) - a(-1, 1))) / 32.0
    Gxx, Gxy, Gyy = fs.window_sum(Ix * Ix, r), fs.window_sum(Ix * Iy, r), fs.window_sum(Iy * Iy, r)
    bx, by = fs.window_sum(Ix * It, r), fs.window_sum(Iy * It, r)
    aa, cc, bb = Gxx + eps, Gyy + eps, Gxy
    det = aa * cc - bb * bb
    ux, uy = -((cc * bx - bb * by) / det), -((aa * by - bb * bx) / det)
    u = np.stack([ux, uy], 1)
    s = score_ref(u, mask, sc, record)
    gx, gy = s.g[:, 0], s.g[:, 1]
    live = s.points.member & (s.record[:, 0] >= sc.min_count)[:, None, None]
    qx = np.where(live, (cc * gx - bb * gy) / det, 0.0)
    qy = np.where(live, (aa * gy - bb * gx) / det, 0.0)
    kappa = float(scale) / float(B)
    k = [1.0] if C == 1 else [0.299, 0.587, 0.114]
    Qx, Qy = fs.window_sum(qx, r), fs.window_sum(qy, r)
    t = Ix * Qx + Iy * Qy
    seed64 = np.stack([kc * -(t * kappa) for kc in k], 1)
    Mxx, Mxy, Myy = fs.window_sum(2.0 * (qx * ux), r), fs.window_sum(qx * uy + qy * ux, r), fs.window_sum(2.0 * (qy * uy), r)
    rx = -(((Qx * It + Mxx * Ix) + Mxy * Iy) * kappa)
    ry = -(((Qy * It + Mxy * Ix) + Myy * Iy) * kappa)
    dI0 = t * kappa + fs.scharr_adjoint(rx, ry)
    grad64 = np.stack([kc * dI0 for kc in k], 1)
    return StageRef(s.value, u, seed64.astype(np.float32), seed64, grad64.astype(np.float32), grad64, s)


# ---- (b) the autograd statement
def torch_score_of_field(u, mask, sc):
    """S [B] of a torch field u [B, 2, H, W], membership taken from its detached values: the semantics in torch ops"""
    dt = u.dtype
    B, _, H, W = u.shape
    pts = score_points(u.detach().double().numpy(), mask, sc)
    px, py, dist = (torch.from_numpy(np.array(a[0])).to(dt) for a in (pts.px, pts.py, pts.dist))
    out = []
    for b in range(B):
        m = torch.from_numpy(pts.member[b])
        N = int(m.sum())
        if N < sc.min_count:
            out.append(u[b].sum() * 0.0)
            continue
        ux, uy = u[b, 0][m], u[b, 1][m]
        x, y, d = px[m], py[m], dist[m]
        nrm = torch.sqrt(ux * ux + uy * uy)
        nx, ny = ux / nrm, uy / nrm
        x1, y1 = x + nx, y + ny
        rho = (x1 * x + y1 * y) / d - d
        tau = (-x1 * y + y1 * x) / d
        var = lambda v: ((v - v.mean()) ** 2).mean()
        Vr, Vt, Vn = var(rho), var(tau), var(nrm)
        R = ((1.0 - Vr) * (1.0 - Vr) + (1.0 - Vt) * (1.0 - Vt)) / 2.0
        A = ux.abs().mean() / sc.max_norm
        F = 1.0 - torch.clamp(Vn, max=1.0)
        out.append(sc.w_direction * R + sc.w_strength * (A * F))
    return torch.stack(out)


def torch_score_term(P, x, radius, eps, mask, sc):
    """The score term of prediction P [B, C, H, W] against the reference x (in the graph only if the caller left it there), usable as
    `run_flow(term=...)`.  -> (f, its un-cancelled scale: every S_b is a sum of two non-negative products, so that is f itself, u)."""
    u = fs.torch_flow_term(P, x, radius, eps, None, mask)[2]
    S = torch_score_of_field(u, mask, sc)
    f = S.sum() / float(P.shape[0])
    return f, float(f.detach().abs()), u


def frame_term(radius, eps, mask, sc, moving=False, seen=None):
    """`run_flow`'s term under the frame pairing: the frame a constant, or (moving) in the graph.  seen: a list that collects every u"""
    def term(P, xn):
        f, scale, u = torch_score_term(P.to(torch.float64), (xn if moving else xn.detach()).to(torch.float64), radius, eps, mask, sc)
        if seen is not None:
            seen.append(u.detach().numpy())
        return f, scale
    return term


class PairScoreTerm:
    """`run_flow`'s term under the prediction pairing (tests/flow_pair_support.py `PairTerm` with the score): the previous P0 stays in
    the graph, the first reference is `start`, detached"""

    def __init__(self, start, radius, eps, mask, sc, seen=None):
        self.prev, self.args, self.seen = start.detach(), (radius, eps, mask, sc), seen

    def __call__(self, P, xn):
        prev, self.prev = self.prev, P
        f, scale, u = torch_score_term(P.to(torch.float64), prev.to(torch.float64), *self.args)
        if self.seen is not None:
            self.seen.append(u.detach().numpy())
        return f, scale


# ---- (c) the cases
# the stage alone: the shapes and inputs of flow_obj_support.FIELD_CASES, B = 2, limits (0, h / 2), max_norm the median |u| of the case's
# B H W pixels on the CPU restatement, min_norm 1e-3; min_count 4, and 25 (at 12 x 8 that leaves a sample below the count)
STAGE_CASES = [(w, h, C, r, masked) for w, h, C, r, masked, _ in fs.FIELD_CASES]
# (reference kind, input kind): a byte reference on field_inputs' "random" bytes, a float reference on pair_field_inputs' "smooth" floats.
# tests/test_flow_score_host.py asserts the conditions every case must satisfy; the two other combinations miss them (a float "random"
# reference leaves one member in a sample at 12 x 8, r = 7; the "smooth" bytes at 40 x 24 put a norm on the median)
REFS = (("bytes", "random"), ("floats", "smooth"))
MIN_COUNTS = (4, 25)
MIN_NORM = 1e-3
WEIGHTS = (0.7, 0.3)
B_STAGE = 2


def stage_inputs(w, h, C, kind, ref_kind):
    """(pred float32, the reference as given to the trainer, the reference widened to float64)"""
    if ref_kind == "bytes":
        pred, ref = fs.field_inputs(w, h, C, kind, B_STAGE)
        return pred, ref, fs.byte_reference(ref)
    pred, prev = ps.pair_field_inputs(w, h, C, kind, B_STAGE)
    return pred, prev, prev.astype(np.float64)


@functools.lru_cache(maxsize=None)
def stage_case(w, h, C, r, masked, ref_kind, min_count):
    """-> (pred, ref, ref64, mask, Score) of a case, max_norm from the restatement's own field"""
    pred, ref, ref64 = stage_inputs(w, h, C, dict(REFS)[ref_kind], ref_kind)
    mask = fs.field_mask(w, h) if masked else None
    probe = Score(1.0, MIN_NORM, 0.0, h / 2.0, WEIGHTS[0], WEIGHTS[1], min_count)
    st = score_stage_ref(pred, ref64, r, 1e-2, mask, probe)
    max_norm = float(np.median(st.score.points.nrm))
    return pred, ref, ref64, mask, probe._replace(max_norm=max_norm)


# training calls against run_flow(term=...): the shapes of flow_obj_support.FLOW_SHAPES, "live" weights, B = 2, r in {2, 7}, the three forms,
# and the pairing: "moving" is the frame pairing with the frame in the graph (loss, terms and weight gradients are those of the constant
# reference; the frame gradient also holds every term's reference path), "prediction" the prediction pairing.  Under the prediction
# pairing term 0 of a reset call has the zero image as its reference: its field is zero and it has no member, so the drifting form
# weighs the terms [0, 1, 1, 1] there.
ScoreCase = namedtuple("ScoreCase", "w h ch r form pairing")
PAIRINGS = ("moving", "prediction")
TRAIN_MIN_COUNT = 4
TRAIN_CASES = [ScoreCase(w, h, tuple(ch), r, form, pairing) for w, h, ch in fs.FLOW_SHAPES for r in fs.RADII for form in fs.FORMS for pairing in PAIRINGS]


def train_case_id(c):
    return "%dx%d-%s-r%d-%s-%s" % (c.w, c.h, "_".join(map(str, c.ch)), c.r, c.form, c.pairing)


def _flow_case(c):
    return fs.FlowCase(c.w, c.h, c.ch, "live", "energy", c.r, c.form)


def train_case_frames(c):
    return fs.flow_case_frames(_flow_case(c))


def train_case_call(c):
    """the keywords the trainer and run_flow share"""
    call = fs.flow_case_call(_flow_case(c))
    if c.pairing == "prediction":
        call["step_weights"] = [0.0, 1.0, 1.0, 1.0] if c.form == "drifting" else list(ps.POPULATION_WEIGHTS)
    return call


# the weight seed of a case's "live" set where `_live_weights`' own (tests/train_support.py) misses the float32 yardstick of
# tests/test_flow_score_host.py, as tests/flow_pair_support.py PAIR_SEEDS does.  Measured with seed 2: 8.7e-5, 1.04e-4 and 1.05e-4 of a
# tensor's largest element against the yardstick's 8.07e-5.
SCORE_SEEDS = {"24x16-1_3_4_5-r2-still-prediction": 3, "24x16-1_3_4_5-r2-still_requant-prediction": 3, "24x16-1_3_4_5-r2-drifting-prediction": 3}


def train_case_weights(c):
    from tests.train_support import _random_weights, case_weights
    seed = SCORE_SEEDS.get(train_case_id(c))
    if seed is None:
        return case_weights(c.w, c.h, c.ch, "live")
    wts = _random_weights(list(c.ch), c.w, c.h, seed=seed)
    wts["ConvP0/b"] = np.full_like(wts["ConvP0/b"], 0.5)
    return wts


def score_for(h, max_norm):
    """the Score of the training and refinement cases on an image of height h"""
    return Score(float(max_norm), MIN_NORM, 0.0, h / 2.0, WEIGHTS[0], WEIGHTS[1], TRAIN_MIN_COUNT)


def train_case_score(c, max_norm):
    return score_for(c.h, max_norm)


def train_case_reference(c, sc, pred=None, dtype=torch.float64, leaf="frames"):
    """`run_flow` of a case under the score term.  pred: the float32 predictions whose bytes a requantised case is fed (the GPU's own);
    None: the run is repeated on its own requantised predictions.  -> (FlowResult, the fields u of the weighted terms, in step order)"""
    from tests.train_support import _fed_from
    wts, frames, call = train_case_weights(c), train_case_frames(c), train_case_call(c)
    B, T, C, H, W = frames.shape

    def run(fed):
        seen = []
        if c.pairing == "prediction":
            term = PairScoreTerm(torch.zeros(B, C, H, W, dtype=dtype), c.r, 1e-2, None, sc, seen)
        else:
            term = frame_term(c.r, 1e-2, None, sc, moving=True, seen=seen)
        res = fs.run_flow(wts, list(c.ch), frames, term=term, leaf=leaf, dtype=dtype, fed=fed, **call)
        w = call["step_weights"] or [1.0] * (T - 1)
        return res, [u for u, ws in zip(seen, w) if ws != 0]

    if not call["requant"]:
        return run(None)
    if pred is not None:
        return run(_fed_from(pred))
    fed = np.zeros(frames.shape, np.float32)
    for _ in range(T - call["n_fed"] + 1):
        out = run(fed)
        fed = _fed_from(out[0].pred.astype(np.float32))
    return out


def candidate_norms(fields, h):
    """the norms of the geometric candidates of every (field, sample) of a case on an image of height h: a list of 1-d arrays"""
    probe = score_for(h, 1.0)
    out = []
    for u in fields:
        pts = score_points(u, None, probe)
        out += [pts.nrm[b][pts.candidate[b]] for b in range(u.shape[0])]
    return out


def case_max_norm(fields, h):
    """A max_norm for a training case from the float64 reference's fields of its weighted terms, -> (max_norm, half the gap it sits in).
    The (term, sample) whose candidates have the largest median norm is taken; max_norm lies between the 40th and the 80th percentile
    of that sample's norms, so it keeps at least two fifths of its candidates and more of every other sample's: every sample of every
    weighted term has members.  Among all the case's norms in that range the midpoint of the widest gap is taken, so no norm sits
    closer to the limit than half that gap and the float32 network's field cannot move a pixel across it
    (tests/test_flow_score_host.py measures both)."""
    per = candidate_norms(fields, h)
    tv = np.sort(max(per, key=lambda v: float(np.median(v))))
    lo, hi = tv[int(0.4 * (len(tv) - 1))], tv[int(0.8 * (len(tv) - 1))]
    pool = np.sort(np.concatenate(per))
    v = pool[(pool >= lo) & (pool <= hi)]
    gaps = np.diff(v)
    if not gaps.max() > 0:
        # a plateau (a window wider than the image gives many pixels one field): the widest gap above it, the top norm's double included
        v = np.append(pool[pool >= lo], 2.0 * pool[-1])
        gaps = np.diff(v)
    k = int(np.argmax(gaps))
    return 0.5 * (v[k] + v[k + 1]), 0.5 * float(gaps[k])


# refinement on the reference alone: the shapes and settings of tests/flow_ref_support.py under the prediction pairing with the
# population term's weights, as the fitness pairs; max_norm by `case_max_norm` from the field of that term at the unrefined stills
REFINE_SHAPES, REFINE = ps.REFINE_SHAPES, ps.REFINE
# the shapes at which the score term rises over the 8 iterations on the float64 reference alone (tests/test_flow_score_host.py asserts
# exactly these); tests/test_gpu_flow_score.py asserts the rise on the device at these shapes only
RISING_SHAPES = [(16, 12, (3, 4, 6)), (24, 16, (1, 4, 8)), (40, 24, (3, 4))]


def _pair_score_run(sc):
    def run(weights, channels, frames, *, radius, eps, direction, mask, seen=None, **kw):
        B, _, C, H, W = frames.shape
        return fs.run_flow(weights, channels, frames, term=PairScoreTerm(torch.zeros(B, C, H, W, dtype=torch.float64), radius, eps, None, sc, seen), **kw)
    return run


@functools.lru_cache(maxsize=None)
def refine_score(w, h, ch):
    """the Score of a refinement row: one probe call at the unrefined stills gives the field of the weighted term"""
    from tests.frame_grad_support import case_inputs
    frames, sets = case_inputs(w, h, tuple(ch), 2, 5)
    T = REFINE["n_repeat"] + REFINE["n_ext"]
    stills = np.ascontiguousarray(np.broadcast_to(frames[:, :1], (frames.shape[0], T) + frames.shape[2:]))
    seen = []
    weights = [0.0] * REFINE["n_repeat"] + [1.0] * (REFINE["n_ext"] - 1)
    _pair_score_run(score_for(h, 1.0))(sets["live"], list(ch), stills, radius=7, eps=1e-2, direction=None, mask=None, seen=seen, n_fed=REFINE["n_repeat"],
                                        requant=False, step_weights=weights)
    return score_for(h, case_max_norm(seen[-1:], h)[0])


@functools.lru_cache(maxsize=None)
def refine_reference(w, h, ch):
    """refine_stills under PredictionFlow(score=...) on the float64 reference alone -> (stills uint8, history [iters + 1])"""
    from tests import flow_ref_support as rs
    weights = [0.0] * REFINE["n_repeat"] + [1.0] * (REFINE["n_ext"] - 1)
    return rs.refine_loop(_pair_score_run(refine_score(w, h, ch)), weights, w, h, ch, "energy")
