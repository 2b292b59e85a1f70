"""Shared by tests/test_flow_struct_host.py and tests/test_gpu_flow_struct.py ("The structure scores"):
(a) `struct_ref`, the numpy float64 restatement of csrc/flow_struct_kernels.h on a field u, with its own exactly summed moments or with
    a given per-sample record, and `struct_stage_ref`, the flow stage around it (the planes, the solve, q from the score's gradient, the
    seed and the reference gradient, in the operations and orders of tests/flow_score_support.py `score_stage_ref`);
(b) `torch_struct_of_field`, the autograd statement with membership detached, and the `term` callbacks of `run_flow` for both pairings;
(c) the cases;
(d) the names of the kernels of the new header.
It imports tests/flow_obj_support.py, tests/flow_pair_support.py and tests/flow_score_support.py and changes none of them."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from tests import flow_obj_support as fs
from tests import flow_pair_support as ps
from tests import flow_score_support as ss

FLOW_STRUCT_KERNELS = ["tflow_free_prepare_kernel", "tflow_struct_moment_kernel", "tflow_struct_final_kernel", "tflow_free_pair_kernel", "tflow_struct_grad_kernel",
                       "tflow_struct_q_kernel"]
REC = 10        # STRUCT_REC of csrc/flow_struct_kernels.h.  Bands: N, m_x, m_y, V, 0 x 4, S_b, 0.  Free: N, m_a, m_n, V_n, swarm, A F, 0 x 2, S_b, 0
SLICES = 16     # STRUCT_SLICES
PI = 3.141592653589793
BANDS, FREE = 0, 2

Bands = namedtuple("Bands", "max_norm min_norm lim_lo lim_hi min_count")
Free = namedtuple("Free", "max_norm min_norm max_distance min_count w")
is_bands = lambda sc: isinstance(sc, Bands)


def as_score(sc):
    """the train.BandsScore or train.FreeScore of a Bands or a Free"""
    from evolutionary_illusion_generator_amd import train
    if is_bands(sc):
        return train.BandsScore(sc.max_norm, sc.min_norm, (sc.lim_lo, sc.lim_hi), sc.min_count)
    return train.FreeScore(sc.max_norm, sc.min_norm, sc.max_distance, sc.min_count, sc.w)


def flow_of(sc, radius, eps=1e-2, mask=None, pairing="frame", reference="constant"):
    from evolutionary_illusion_generator_amd import train
    return train.make_flow(pairing, radius, eps, None, mask, reference=reference, score=as_score(sc))


def bands_for(h, max_norm, min_count=1):
    """the fitness's own limits on an image of height h: (0, (h / 4) * 2)"""
    return Bands(float(max_norm), 1e-3, 0.0, (h / 4.0) * 2.0, min_count)


# ---- (a) the numpy restatement
Points = namedtuple("Points", "nrm nx ny member candidate upper")


def struct_points(u, mask, sc):
    """u float64 [B, 2, H, W] -> the per-pixel quantities of tflow_struct_point, [B, H, W] each (zeros where the pixel is no member);
    `candidate` is the geometric part of membership (mask and rule) alone, `upper` y < middle (Bands; all False for Free)"""
    B, _, H, W = u.shape
    ux, uy = u[:, 0], u[:, 1]
    yy = np.broadcast_to(np.mgrid[0:H, 0:W][0].astype(np.float64), ux.shape)
    nrm = np.sqrt(ux * ux + uy * uy)
    counted = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    candidate = np.broadcast_to(counted, ux.shape).copy()
    upper = np.zeros(ux.shape, bool)
    if is_bands(sc):
        candidate &= (sc.lim_lo <= yy) & (yy <= sc.lim_hi)
        upper = yy < int(sc.lim_hi / 2.0)
    member = candidate & (nrm > 0.0) & (sc.min_norm <= nrm) & (nrm <= sc.max_norm)
    sn = np.where(member, nrm, 1.0)
    nx, ny = np.where(member, ux / sn, 0.0), np.where(member, uy / sn, 0.0)
    return Points(nrm, nx, ny, member, candidate, upper)


Pairs = namedtuple("Pairs", "theta L rowS colS min_gap min_wrap terms")


def free_pairs(nx, member, DD, theta=None):
    """The pair pass of one sample: nx, member [H, W] -> theta [N], L [N] (each row added in j order, from 0), the integer sign sums as
    row and as column, and the two margins the host test asserts: the smallest |theta_j - opt_ij| over the close pairs and the smallest
    distance of theta_i + f pi from a multiple of 2 (inf with no member), and the matrix of the rows' terms."""
    ys, xs = np.nonzero(member)       # pixel order
    th = np.arccos(nx[member]) if theta is None else np.asarray(theta, np.float64)[member]      # theta: a plane of angles to take in numpy's place (the device's)
    if len(th) == 0:
        z = np.zeros(0)
        return Pairs(th, z, z.astype(np.int64), z.astype(np.int64), np.inf, np.inf, np.zeros((0, 0)))
    dx = (xs[None, :] - xs[:, None]).astype(np.float64)
    dy = (ys[None, :] - ys[:, None]).astype(np.float64)
    f = (dx * dx + dy * dy) / DD
    f = np.where(f > 1.0, 1.0, f)
    close = f < 1.0
    arg = th[:, None] + f * PI
    wrapped = np.fmod(arg, 2.0)
    diff = th[None, :] - wrapped * PI
    terms = np.where(close, np.abs(diff), 0.0)
    L = np.cumsum(terms, axis=1)[:, -1]      # sequential, j ascending; a pair that is not close adds +0
    sg = np.where(close, np.sign(diff), 0.0).astype(np.int64)
    return Pairs(th, L, sg.sum(1), sg.sum(0), float(np.abs(diff)[close].min()), float(np.minimum(wrapped, 2.0 - wrapped)[close].min()), terms)


def sample_value(r, sc):
    """S_b of one record, tflow_struct_value"""
    N = r[0]
    if N < sc.min_count:
        return 0.0
    if is_bands(sc):
        return ((1.0 - r[3]) + abs(r[1]) + (1.0 - abs(r[2]))) / 3.0
    A = r[1] / sc.max_norm
    F = 1.0 - (r[3] if r[3] < 1.0 else 1.0)
    num = (N if N < 15.0 else 15.0) / 15.0
    return (sc.w[0] * r[4] + sc.w[1] * (A * F)) + sc.w[2] * num


def sample_columns(u, pts, sc, b, pairs=None, rec=None):
    """the terms of the sums of sample b: (first-pass columns, second-pass columns given the record's means)"""
    m = pts.member[b]
    if is_bands(sc):
        mx = np.where(pts.upper[b][m], pts.nx[b][m], -pts.nx[b][m])
        my = np.where(pts.upper[b][m], pts.nx[b][m], pts.ny[b][m])
        first = [mx, my]
        second = None if rec is None else [(mx - rec[1]) * (mx - rec[1])]
    else:
        nrm = pts.nrm[b][m]
        first = [np.abs(u[b, 0][m]), nrm]
        second = None if rec is None else [(nrm - rec[2]) * (nrm - rec[2]), (PI - pairs.L / rec[0]) / PI]
    return first, second


def exact_record(u, pts, sc, pairs):
    """the per-sample record [B, 10] with every sum formed exactly (math.fsum), then divided: two passes, as np.var"""
    B = u.shape[0]
    rec = np.zeros((B, REC), np.float64)
    for b in range(B):
        N = int(pts.member[b].sum())
        rec[b, 0] = N
        if N == 0:
            continue
        first, _ = sample_columns(u, pts, sc, b)
        for k, v in enumerate(first):
            rec[b, 1 + k] = math.fsum(v.tolist()) / N
        _, second = sample_columns(u, pts, sc, b, pairs[b] if pairs else None, rec[b])
        for k, v in enumerate(second):
            rec[b, 3 + k] = math.fsum(v.tolist()) / N
        fill_value(rec[b], sc)
    return rec


def fill_value(r, sc):
    """entries 5 (Free: A F) and 8 (S_b) of a record from its moments, as tflow_struct_final_kernel<2> writes them"""
    if not is_bands(sc):
        A = r[1] / sc.max_norm
        F = 1.0 - (r[3] if r[3] < 1.0 else 1.0)
        r[5] = A * F if not r[0] < sc.min_count else 0.0
    r[8] = sample_value(r, sc)


StructRef = namedtuple("StructRef", "value S record g points pairs")


def struct_ref(u, mask, sc, record=None):
    """A structure score on a field: u float64 [B, 2, H, W].  record None: the restatement's own exactly summed moments; else a [B, 10]
    record whose moments are taken as they are (the device's), S_b and f being formed from them again.  -> f, S [B], the record,
    g = d S_b / d u [B, 2, H, W] in the order csrc/flow_struct_kernels.h fixes, the per-pixel quantities and (Free) the pair pass."""
    u = np.asarray(u, np.float64)
    B = u.shape[0]
    pts = struct_points(u, mask, sc)
    pairs = None if is_bands(sc) else [free_pairs(pts.nx[b], pts.member[b], sc.max_distance * sc.max_distance) for b in range(B)]
    rec = exact_record(u, pts, sc, pairs) if record is None else np.array(record, np.float64)
    S = np.array([sample_value(rec[b], sc) for b in range(B)])
    total = S[0]
    for b in range(1, B):
        total = total + S[b]
    g = np.zeros_like(u)
    for b in range(B):
        N = rec[b, 0]
        if N < sc.min_count:
            continue
        m = pts.member[b]
        nrm, nx, ny = pts.nrm[b][m], pts.nx[b][m], pts.ny[b][m]
        if is_bands(sc):
            m_x, m_y = rec[b, 1], rec[b, 2]
            upper = pts.upper[b][m]
            mx = np.where(upper, nx, -nx)
            c_x = (-(2.0 * (mx - m_x)) + np.sign(m_x)) / (3.0 * N)
            c_y = -np.sign(m_y) / (3.0 * N)
            a_x, a_y = np.where(upper, c_x + c_y, -c_x), np.where(upper, 0.0, c_y)
            xy = nx * ny
            gx = (a_x * (ny * ny) - a_y * xy) / nrm
            gy = (a_y * (nx * nx) - a_x * xy) / nrm
        else:
            m_a, m_n, Vn = rec[b, 1], rec[b, 2], rec[b, 3]
            ux = u[b, 0][m]
            c_th = -((sc.w[0] * (pairs[b].colS.astype(np.float64) - PI * pairs[b].rowS.astype(np.float64))) / (PI * (N * N)))
            gx = (c_th * -np.abs(ny)) / nrm
            gy = (c_th * (np.sign(ny) * nx)) / nrm
            A = m_a / sc.max_norm
            F = 1.0 - (Vn if Vn < 1.0 else 1.0)
            gx = gx + ((sc.w[1] * F) * np.sign(ux)) / (N * sc.max_norm)
            c_n = -(((sc.w[1] * A) * (2.0 * (nrm - m_n))) / N) if Vn < 1.0 else np.zeros_like(nrm)
            gx = gx + c_n * nx
            gy = gy + c_n * ny
        g[b, 0][m], g[b, 1][m] = gx, gy
    return StructRef(total / float(B), S, rec, g, pts, pairs)


StageRef = namedtuple("StageRef", "value u seed seed64 grad grad64 score")


def struct_stage_ref(pred, ref64, r, eps, mask, sc, scale=1.0, record=None):
    """The flow stage under a structure score: `flow_score_support.score_stage_ref`'s operations with q from `struct_ref`'s g (which is 0
    off the members and in a sample below min_count) and kappa = scale / B."""
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
    s = struct_ref(u, mask, sc, record)
    gx, gy = s.g[:, 0], s.g[:, 1]
    qx = (cc * gx - bb * gy) / det
    qy = (aa * gy - bb * gx) / det
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


def oracle_value(u_b, member, sc, w, h):
    """the oracle's score of one sample's member vectors, as [x, y, dx, dy] rows in pixel order"""
    from oracle import scores
    yy, xx = np.nonzero(member)
    vec = np.stack([xx.astype(np.float64), yy.astype(np.float64), u_b[0][member], u_b[1][member]], 1)
    if is_bands(sc):
        return float(scores.horizontal_symmetry_score(vec, (sc.lim_lo, sc.lim_hi)))
    assert sc.max_distance == 100.0, "oracle.scores.swarm_score has the distance 100 built in"
    n = len(vec)
    return sc.w[0] * scores.swarm_score(vec) + sc.w[1] * scores.strength_number(vec, sc.max_norm) + sc.w[2] * min(n, 15) / 15


# ---- (b) the autograd statement
def torch_struct_of_field(u, mask, sc):
    """(S [B], its un-cancelled scale [B]) of a torch field u [B, 2, H, W], membership taken from its detached values"""
    dt = u.dtype
    B, _, H, W = u.shape
    pts = struct_points(u.detach().double().numpy(), mask, sc)
    out, scales = [], []
    for b in range(B):
        m = torch.from_numpy(pts.member[b].copy())
        N = int(m.sum())
        if N < sc.min_count:
            out.append(u[b].sum() * 0.0)
            scales.append(0.0)
            continue
        ux, uy = u[b, 0][m], u[b, 1][m]
        nrm = torch.sqrt(ux * ux + uy * uy)
        nx, ny = ux / nrm, uy / nrm
        if is_bands(sc):
            upper = torch.from_numpy(pts.upper[b][pts.member[b]].copy())
            mx, my = torch.where(upper, nx, -nx), torch.where(upper, nx, ny)
            V = ((mx - mx.mean()) ** 2).mean()
            out.append(((1.0 - V) + mx.mean().abs() + (1.0 - my.mean().abs())) / 3.0)
            scales.append(float(out[-1].detach()))      # three non-negative parts
            continue
        ys, xs = (torch.from_numpy(v.astype(np.float64)).to(dt) for v in np.nonzero(pts.member[b]))
        # theta = acos(nx) as atan2(|ny|, nx), the same angle on a unit vector: autograd's 1 / sqrt(1 - nx^2) of acos loses as many digits as
        # 1 - nx^2 cancels (measured: 1.1e-11 of the largest element at 40 x 24), the quotient form does not
        th = torch.atan2(ny.abs(), nx)
        dx, dy = xs[None, :] - xs[:, None], ys[None, :] - ys[:, None]
        f = torch.clamp((dx * dx + dy * dy) / (sc.max_distance * sc.max_distance), max=1.0)
        close = (f < 1.0).to(dt)
        opt = torch.fmod(th[:, None] + f * PI, 2.0) * PI
        L = (close * (th[None, :] - opt).abs()).sum(1)
        swarm = ((PI - L / N) / PI).sum() / N
        strength = (ux.abs().mean() / sc.max_norm) * (1.0 - torch.clamp(((nrm - nrm.mean()) ** 2).mean(), max=1.0))
        rest = sc.w[1] * strength + sc.w[2] * (min(N, 15) / 15.0)
        out.append(sc.w[0] * swarm + rest)
        scales.append(float((sc.w[0] * (1.0 + L.sum() / (PI * N * N)) + rest).detach()))
    return torch.stack(out), np.array(scales)


def torch_struct_term(P, x, radius, eps, mask, sc):
    """The term of prediction P [B, C, H, W] against the reference x (in the graph only if the caller left it there), usable as
    `run_flow(term=...)`.  -> (f, its un-cancelled scale, u)."""
    u = fs.torch_flow_term(P, x, radius, eps, None, mask)[2]
    S, scales = torch_struct_of_field(u, mask, sc)
    return S.sum() / float(P.shape[0]), float(scales.sum() / P.shape[0]), u


def frame_term(radius, eps, mask, sc, moving=False, seen=None):
    """`run_flow`'s term under the frame pairing: the frame a constant, or (moving) in the graph.  seen: a list that collects every u"""
    def term(P, xn):
        f, scale, u = torch_struct_term(P.to(torch.float64), (xn if moving else xn.detach()).to(torch.float64), radius, eps, mask, sc)
        if seen is not None:
            seen.append(u.detach().numpy())
        return f, scale
    return term


class PairStructTerm:
    """`run_flow`'s term under the prediction pairing: the previous P0 stays in the graph, the first reference is `start`, detached"""

    def __init__(self, start, radius, eps, mask, sc, seen=None):
        self.prev, self.args, self.seen = start.detach(), (radius, eps, mask, sc), seen

    def __call__(self, P, xn):
        prev, self.prev = self.prev, P
        f, scale, u = torch_struct_term(P.to(torch.float64), prev.to(torch.float64), *self.args)
        if self.seen is not None:
            self.seen.append(u.detach().numpy())
        return f, scale


# ---- (c) the cases
# The stage alone, B = 2, a byte reference on field_inputs' "random" bytes and a float reference on pair_field_inputs' "smooth" floats
# (flow_score_support.REFS); min_norm 1e-3; max_norm is a quantile of |u| over the case's geometric candidates on the CPU restatement: the
# median for Free, the 0.4 quantile for Bands, which leaves one sample of 12 x 8 under 25 members beside a live one under either reference
# (the median leaves 28 and 32).  A masked Bands case counts the row y == lim_hi, which `flow_obj_support.field_mask` cuts: `bands_mask`.
# Bands: (w, h, C, r, masked) with the fitness's own limits (0, (h / 4) * 2); at 16 x 10, h / 4 is fractional: lim_hi 5.0, middle 2.
BANDS_SHAPES = [(12, 8, 1, 2, False), (16, 10, 3, 3, True), (24, 16, 1, 7, False), (40, 24, 3, 16, True)]
BANDS_MIN_COUNTS = (1, 25)
# Free: (w, h, C, r, masked, max_distance).  16 x 12 with D = 5 has pairs at d2 = 25, so f == 1 exactly, the not-close side; 24 x 16 has 384
# pixels, two LDS tiles with a partial tail, all pairs close; 40 x 24 spans four tiles and four blocks per sample.
FREE_SHAPES = [(16, 12, 1, 3, False, 5.0), (24, 16, 1, 7, False, 100.0), (40, 24, 3, 16, True, 10.0)]
FREE_W = (0.5, 0.1, 0.4)
REFS = ss.REFS
B_STAGE = 2
StageCase = namedtuple("StageCase", "kind w h C r masked ref_kind min_count max_distance empty")
# "empty": sample 1's float reference is its prediction, so its field is exactly zero and it has no member at all
# Input kinds per reference kind that were tried and rejected for a case, with the condition of tests/test_flow_struct_host.py they miss, are
# listed in STAGE_INPUT_KINDS' comment below.
STAGE_CASES = [StageCase("bands", w, h, C, r, masked, rk, mc, 0.0, False) for w, h, C, r, masked in BANDS_SHAPES for rk, _ in REFS for mc in BANDS_MIN_COUNTS]
STAGE_CASES += [StageCase("free", w, h, C, r, masked, rk, 1, D, False) for w, h, C, r, masked, D in FREE_SHAPES for rk, _ in REFS]
STAGE_CASES += [StageCase("free", 16, 12, 1, 3, False, "floats", 1, 5.0, True)]
# {(kind, w, h, ref_kind): input kind} where flow_score_support.REFS' own misses a condition; none needed so far
STAGE_INPUT_KINDS = {}


def bands_mask(w, h):
    """`flow_obj_support.field_mask` with the row h // 2, which is lim_hi at these heights, counted again and row 1 cut in its place"""
    m = fs.field_mask(w, h)
    m[h // 2, w // 4:] = 1
    m[1, :] = 0
    m[1::5, 2::7] = 0
    return m


def stage_id(c):
    return "%s-%dx%dx%d-r%d-%s-min%d%s" % (c.kind, c.w, c.h, c.C, c.r, c.ref_kind, c.min_count, "-empty" if c.empty else "")


@functools.lru_cache(maxsize=None)
def stage_case(c):
    """-> (pred, ref, ref64, mask, Bands or Free) of a case, max_norm from the restatement's own field"""
    kind = STAGE_INPUT_KINDS.get((c.kind, c.w, c.h, c.ref_kind), dict(REFS)[c.ref_kind])
    pred, ref, ref64 = ss.stage_inputs(c.w, c.h, c.C, kind, c.ref_kind)
    if c.empty:
        ref = ref.copy()
        ref[1] = pred[1]
        ref64 = ref.astype(np.float64)
    mask = (bands_mask if c.kind == "bands" else fs.field_mask)(c.w, c.h) if c.masked else None
    probe = bands_for(c.h, 1.0, c.min_count) if c.kind == "bands" else Free(1.0, 1e-3, c.max_distance, c.min_count, FREE_W)
    st = struct_stage_ref(pred, ref64, c.r, 1e-2, mask, probe)
    pts = st.score.points
    live = pts.candidate & (pts.nrm > 0)
    # between two distinct norms, not on one: a window wider than the image gives many pixels one field, and a quantile lands on such a plateau
    v = np.unique(pts.nrm[live])
    k = min(int(np.searchsorted(v, np.quantile(pts.nrm[live], 0.4 if c.kind == "bands" else 0.5), side="right")) - 1, len(v) - 2)
    return pred, ref, ref64, mask, probe._replace(max_norm=float(0.5 * (v[k] + v[k + 1])))


# training calls against run_flow(term=...): the cases of tests/flow_score_support.py (shapes, forms, radii, pairings, weights, frames),
# once per structure; Free with max_distance 10, so that both sides of the comparison occur at every shape
TRAIN_DISTANCE = 10.0
StructCase = namedtuple("StructCase", "kind base")
TRAIN_CASES = [StructCase(kind, c) for kind in ("bands", "free") for c in ss.TRAIN_CASES]


def train_case_id(c):
    return c.kind + "-" + ss.train_case_id(c.base)


def train_case_score(c, max_norm):
    return bands_for(c.base.h, max_norm) if c.kind == "bands" else Free(float(max_norm), 1e-3, TRAIN_DISTANCE, 1, FREE_W)


# the weight seed of a case's "live" set where `flow_score_support.train_case_weights`' own misses the float32 yardstick of
# tests/test_flow_struct_host.py, 8.07e-5, as flow_score_support.SCORE_SEEDS does: bias gradients in which the steps' contributions nearly
# cancel.  Measured with the score mode's weights: 6.07e-4, 3.40e-4, 1.57e-4, 1.21e-4, 1.08e-4, 1.03e-4 and 8.31e-5, in this order.
STRUCT_SEEDS = {"bands-24x16-1_3_4_5-r2-drifting-prediction": 4, "bands-12x8-1_4-r7-still_requant-prediction": 4, "bands-12x8-1_4-r2-still_requant-prediction": 4,
                "bands-12x8-1_4-r7-still_requant-moving": 4, "free-12x8-1_4-r7-drifting-prediction": 4, "free-40x24-3_4-r2-still-prediction": 3,
                "bands-24x16-1_3_4_5-r7-drifting-prediction": 4,
                # Free cases in which `free_pairs_at_risk` finds pairs under the score mode's weights (3, 1, 1, 3, 3, 16 and 4 of them): the float32 trainer
                # landed on the other side of one at 40x24 r = 2 drifting, prediction pairing (ConvLSTM0/c_i/W off by 2e-3 of its largest element)
                "free-24x16-1_3_4_5-r2-drifting-prediction": 4, "free-24x16-1_3_4_5-r7-still_requant-moving": 3, "free-24x16-1_3_4_5-r7-still_requant-prediction": 3,
                "free-40x24-3_4-r2-still_requant-prediction": 3, "free-40x24-3_4-r2-drifting-prediction": 3, "free-40x24-3_4-r7-still_requant-prediction": 5}


def train_case_weights(c):
    from tests.train_support import _random_weights
    seed = STRUCT_SEEDS.get(train_case_id(c))
    if seed is None:
        return ss.train_case_weights(c.base)
    wts = _random_weights(list(c.base.ch), c.base.w, c.base.h, seed=seed)
    wts["ConvP0/b"] = np.full_like(wts["ConvP0/b"], 0.5)
    return wts


def train_case_reference(c, sc, pred=None, dtype=torch.float64, leaf="frames"):
    """`flow_score_support.train_case_reference` under a structure score's term"""
    from tests.train_support import _fed_from
    b = c.base
    wts, frames, call = train_case_weights(c), ss.train_case_frames(b), ss.train_case_call(b)
    B, T, C, H, W = frames.shape

    def run(fed):
        seen = []
        if b.pairing == "prediction":
            term = PairStructTerm(torch.zeros(B, C, H, W, dtype=dtype), b.r, 1e-2, None, sc, seen)
        else:
            term = frame_term(b.r, 1e-2, None, sc, moving=True, seen=seen)
        res = fs.run_flow(wts, list(b.ch), frames, term=term, leaf=leaf, dtype=dtype, fed=fed, **call)
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


def candidate_norms(fields, sc):
    """the norms of the geometric candidates of every (field, sample): a list of 1-d arrays"""
    out = []
    for u in fields:
        pts = struct_points(u, None, sc)
        out += [pts.nrm[b][pts.candidate[b]] for b in range(u.shape[0])]
    return out


def case_max_norm(fields, sc):
    """`flow_score_support.case_max_norm`'s gap construction on this structure's candidates -> (max_norm, half the gap it sits in)"""
    per = candidate_norms(fields, sc)
    tv = np.sort(max(per, key=lambda v: float(np.median(v))))
    lo, hi = tv[int(0.4 * (len(tv) - 1))], tv[int(0.8 * (len(tv) - 1))]
    pool = np.sort(np.concatenate(per))
    v = pool[(pool >= lo) & (pool <= hi)]
    gaps = np.diff(v)
    if not (len(gaps) and gaps.max() > 0):
        v = np.append(pool[pool >= lo], 2.0 * pool[-1])
        gaps = np.diff(v)
    k = int(np.argmax(gaps))
    return 0.5 * (v[k] + v[k + 1]), 0.5 * float(gaps[k])


# refinement on the reference alone: the shapes and settings of tests/flow_score_support.py (8 steps of 2 bytes, the prediction pairing with
# the population term's weights); max_norm by `case_max_norm` from the field of that term at the unrefined stills
REFINE_SHAPES, REFINE = ps.REFINE_SHAPES, ps.REFINE
# the shapes at which the term rises over the 8 iterations on the float64 reference alone (tests/test_flow_struct_host.py asserts exactly
# these); tests/test_gpu_flow_struct.py asserts the rise on the device at these shapes only
RISING_SHAPES = {"bands": [(12, 8, (1, 4)), (16, 12, (3, 4, 6)), (24, 16, (1, 4, 8)), (40, 24, (3, 4))],
                 "free": [(12, 8, (1, 4)), (16, 12, (3, 4, 6)), (40, 24, (3, 4))]}
REFINE_ROWS = [(kind, w, h, tuple(ch)) for kind in ("bands", "free") for w, h, ch in REFINE_SHAPES]


def _pair_struct_run(sc):
    def run(weights, channels, frames, *, radius, eps, direction, mask, seen=None, **kw):
        B, _, C, H, W = frames.shape
        return fs.run_flow(weights, channels, frames, term=PairStructTerm(torch.zeros(B, C, H, W, dtype=torch.float64), radius, eps, None, sc, seen), **kw)
    return run


def refine_probe(kind, h):
    return bands_for(h, 1.0) if kind == "bands" else Free(1.0, 1e-3, TRAIN_DISTANCE, 1, FREE_W)


@functools.lru_cache(maxsize=None)
def refine_score(kind, w, h, ch):
    """the score of a refinement row: one probe call at the unrefined stills gives the field of the weighted term"""
    from tests.frame_grad_support import case_inputs
    frames, sets = case_inputs(w, h, tuple(ch), 2, 5)
    T = REFINE["n_repeat"] + REFINE["n_ext"]
    stills = np.ascontiguousarray(np.broadcast_to(frames[:, :1], (frames.shape[0], T) + frames.shape[2:]))
    seen = []
    weights = [0.0] * REFINE["n_repeat"] + [1.0] * (REFINE["n_ext"] - 1)
    probe = refine_probe(kind, h)
    _pair_struct_run(probe)(sets["live"], list(ch), stills, radius=7, eps=1e-2, direction=None, mask=None, seen=seen, n_fed=REFINE["n_repeat"],
                            requant=False, step_weights=weights)
    return probe._replace(max_norm=case_max_norm(seen[-1:], probe)[0])


@functools.lru_cache(maxsize=None)
def refine_reference(kind, w, h, ch):
    """refine_stills under PredictionFlow(score=...) on the float64 reference alone -> (stills uint8, history [iters + 1])"""
    from tests import flow_ref_support as rs
    weights = [0.0] * REFINE["n_repeat"] + [1.0] * (REFINE["n_ext"] - 1)
    return rs.refine_loop(_pair_struct_run(refine_score(kind, w, h, ch)), weights, w, h, ch, "energy")


def free_pairs_at_risk(u64, u32, mask, sc, safety=4.0):
    """How many close pairs of the Free score on the float64 field u64 could change a sign or a wrap under the float32 network: those whose
    |theta_j - opt_ij| is at most `safety` times what the float32 field u32 moves it by (pi |d theta_i| + |d theta_j|), or whose
    theta_i + f pi is nearer to a multiple of 2 than `safety` |d theta_i|.  The gradient's integers are piecewise constant in theta; a
    case with such a pair has no float32 yardstick."""
    pa, pb = struct_points(u64, mask, sc), struct_points(u32, mask, sc)
    assert np.array_equal(pa.member, pb.member)
    DD = sc.max_distance * sc.max_distance
    risk = 0
    for b in range(u64.shape[0]):
        m = pa.member[b]
        ys, xs = np.nonzero(m)
        th, dth = np.arccos(pa.nx[b][m]), np.abs(np.arccos(pb.nx[b][m]) - np.arccos(pa.nx[b][m]))
        dx, dy = (xs[None, :] - xs[:, None]).astype(np.float64), (ys[None, :] - ys[:, None]).astype(np.float64)
        f = np.minimum((dx * dx + dy * dy) / DD, 1.0)
        close = f < 1.0
        wrapped = np.fmod(th[:, None] + f * PI, 2.0)
        gap = np.abs(th[None, :] - wrapped * PI)
        wrap = np.minimum(wrapped, 2.0 - wrapped)
        risk += int((close & ((gap <= safety * (PI * dth[:, None] + dth[None, :])) | (wrap <= safety * dth[:, None]))).sum())
    return risk
