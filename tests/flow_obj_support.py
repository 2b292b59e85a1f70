"""Shared by tests/test_flow_obj_host.py and tests/test_gpu_flow_obj.py ("The flow objective"):
(a) `flow_stage_ref`, the numpy float64 restatement of the flow stage with its seed and its reference gradient (csrc/flow_obj_kernels.h,
    flow_ref_kernels.h, flow_pair_kernels.h), operation by operation in the order the kernels use, window sums as loops over offsets that add
    shifted arrays, and `flow_ref`, its adapter for a byte reference;
(b) `run_flow`, the float64 torch-CPU autograd statement of PredNet training with the predictions in the graph and the flow term written
    in torch ops on them (the operations of oracle/prednet_train_ref.py `run`, in its order, as tests/frame_grad_support.py `run_frames`);
(c) the case lists;
(d) the names of the kernels of the new header."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import GATES
from oracle.prednet_train_ref import _error_pair, clamp01
from tests.train_support import SHAPES, _drifting, _fed_from, case_weights

FLOW_OBJ_KERNELS = ["tflow_prep_kernel", "tflow_solve_kernel", "tflow_seed_kernel", "tflow_sum_kernel"]
TILE = 16   # FLOW_TILE of csrc/flow_obj_kernels.h


# ---- (a) the numpy restatement
def _gray(v):
    """v float64 [B, C, H, W] -> [B, H, W]"""
    if v.shape[1] == 1:
        return v[:, 0]
    return (0.299 * v[:, 0] + 0.587 * v[:, 1]) + 0.114 * v[:, 2]


def _sum_last(a, r):
    """sum over the offsets d = -r .. r, ascending, of a[..., i + d] where i + d is inside; every sum starts from its first term"""
    n = a.shape[-1]
    acc = np.zeros_like(a)
    started = np.zeros(n, bool)
    for d in range(-r, r + 1):
        lo, hi = max(0, -d), min(n, n - d)
        if lo >= hi:
            continue
        term = a[..., lo + d:hi + d]
        acc[..., lo:hi] = np.where(started[lo:hi], acc[..., lo:hi] + term, term)
        started[lo:hi] = True
    return acc


def window_sum(a, r):
    """the truncated window sum: rows first (along x), then columns (along y) over those row sums"""
    return np.swapaxes(_sum_last(np.swapaxes(_sum_last(a, r), -1, -2), r), -1, -2)


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


StageRef = namedtuple("StageRef", "value u seed mv bound seed64 grad grad64")


def flow_stage_ref(pred, ref64, r, eps, direction=None, mask=None, scale=1.0):
    """The flow stage of one prediction / reference pair, the ONE statement behind `flow_ref`, `flow_ref_support.flow_ref_grad` and
    `flow_pair_support.pair_ref`: pred float32 [B, C, H, W]; ref64 float64 [B, C, H, W], the reference image as the prep kernel widens
    it; direction float32 [2, H, W] or None; mask [H, W] or None.  -> value (exactly summed, then divided), u float64 [B, 2, H, W],
    seed = scale * d value / d pred and grad = scale * d value / d reference as float32 [B, C, H, W], each also ahead of its rounding
    to float (seed64, grad64), mv = m v, and the bound of a double-precision sum of the N = B H W summands in any order,
    N 2^-53 sum |m v| / (B N_m)."""
    pred = np.asarray(pred, np.float32)
    B, C, H, W = pred.shape
    # tflow_prep_kernel / tflow_pair_prep_kernel
    I0, I1 = _gray(ref64), _gray(pred.astype(np.float64))
    It = I1 - I0
    ap = np.pad(I0, ((0, 0), (1, 1), (1, 1)), mode="edge")
    a = lambda dy, dx: ap[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    Ix = ((3.0 * (a(-1, 1) - a(-1, -1)) + 10.0 * (a(0, 1) - a(0, -1))) + 3.0 * (a(1, 1) - a(1, -1))) / 32.0
    Iy = ((3.0 * (a(1, -1) - a(-1, -1)) + 10.0 * (a(1, 0) - a(-1, 0))) + 3.0 * (a(1, 1) - a(-1, 1))) / 32.0
    # tflow_solve_kernel
    Gxx, Gxy, Gyy = window_sum(Ix * Ix, r), window_sum(Ix * Iy, r), window_sum(Iy * Iy, r)
    bx, by = window_sum(Ix * It, r), window_sum(Iy * It, r)
    aa, cc, bb = Gxx + eps, Gyy + eps, Gxy
    det = aa * cc - bb * bb
    ux, uy = -((cc * bx - bb * by) / det), -((aa * by - bb * bx) / det)
    if direction is None:
        gx, gy = 2.0 * ux, 2.0 * uy
        v = ux * ux + uy * uy
    else:
        d = np.asarray(direction, np.float32).astype(np.float64)
        gx, gy = np.broadcast_to(d[0], ux.shape), np.broadcast_to(d[1], ux.shape)
        v = gx * ux + gy * uy
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    n_m = int(m.sum())
    mv = np.where(m, v, 0.0)
    qx = np.where(m, (cc * gx - bb * gy) / det, 0.0)
    qy = np.where(m, (aa * gy - bb * gx) / det, 0.0)
    kappa = float(scale) / float(B * n_m)
    k = [1.0] if C == 1 else [0.299, 0.587, 0.114]
    # tflow_seed_kernel
    Qx, Qy = window_sum(qx, r), window_sum(qy, r)
    t = Ix * Qx + Iy * Qy
    s = -(t * kappa)
    seed64 = np.stack([kc * s for kc in k], 1)
    # tflow_ref_sums_kernel
    Mxx, Mxy, Myy = window_sum(2.0 * (qx * ux), r), window_sum(qx * uy + qy * ux, r), window_sum(2.0 * (qy * uy), r)
    rx = -(((Qx * It + Mxx * Ix) + Mxy * Iy) * kappa)
    ry = -(((Qy * It + Mxy * Ix) + Myy * Iy) * kappa)
    e = t * kappa
    # tflow_ref_fold_kernel
    dI0 = e + scharr_adjoint(rx, ry)
    grad64 = np.stack([kc * dI0 for kc in k], 1)
    value = math.fsum(mv.ravel().tolist()) / float(B * n_m)
    bound = mv.size * 2.0 ** -53 * math.fsum(np.abs(mv).ravel().tolist()) / float(B * n_m)
    return StageRef(value, np.stack([ux, uy], 1), seed64.astype(np.float32), mv, bound, seed64, grad64.astype(np.float32), grad64)


def byte_reference(ref):
    """uint8 -> the float64 image the byte prep kernel forms: (float)byte / 255.0f, widened"""
    return (np.asarray(ref, np.uint8).astype(np.float32) / np.float32(255.0)).astype(np.float64)


FlowRef = namedtuple("FlowRef", "value u seed mv bound seed64")


def flow_ref(pred, ref, r, eps, direction=None, mask=None, scale=1.0):
    """pred float32 [B, C, H, W], ref uint8 [B, C, H, W]; the settings of `flow_stage_ref`.  -> its value, u, seed, mv, bound and seed64."""
    s = flow_stage_ref(pred, byte_reference(ref), r, eps, direction, mask, scale)
    return FlowRef(s.value, s.u, s.seed, s.mv, s.bound, s.seed64)


# ---- (b) the autograd statement
def torch_flow_term(P, x, r, eps, direction=None, mask=None):
    """The flow term of prediction P [B, C, H, W] against the frame x (in the graph only if the caller left it there) in torch ops, in
    P's dtype.  -> (f, sum m |v| / (B N_m): the un-cancelled scale of f, u [B, 2, H, W])."""
    dt = P.dtype
    B, C, H, W = P.shape
    gray = lambda v: v[:, 0] if C == 1 else (0.299 * v[:, 0] + 0.587 * v[:, 1]) + 0.114 * v[:, 2]
    I0, I1 = gray(x), gray(P)
    It = I1 - I0
    ap = F.pad(I0[:, None], (1, 1, 1, 1), mode="replicate")[:, 0]
    a = lambda dy, dx: ap[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    Ix = ((3.0 * (a(-1, 1) - a(-1, -1)) + 10.0 * (a(0, 1) - a(0, -1))) + 3.0 * (a(1, 1) - a(1, -1))) / 32.0
    Iy = ((3.0 * (a(1, -1) - a(-1, -1)) + 10.0 * (a(1, 0) - a(-1, 0))) + 3.0 * (a(1, 1) - a(-1, 1))) / 32.0
    ones = torch.ones(1, 1, 2 * r + 1, 2 * r + 1, dtype=dt)
    ws = lambda f: F.conv2d(f[:, None], ones, padding=r)[:, 0]    # zero padding of a sum is truncation
    aa, cc, bb = ws(Ix * Ix) + eps, ws(Iy * Iy) + eps, ws(Ix * Iy)
    bx, by = ws(Ix * It), ws(Iy * It)
    det = aa * cc - bb * bb
    ux, uy = -((cc * bx - bb * by) / det), -((aa * by - bb * bx) / det)
    if direction is None:
        v = ux * ux + uy * uy
    else:
        d = torch.from_numpy(np.asarray(direction, np.float32)).to(dt)
        v = d[0] * ux + d[1] * uy
    m = torch.ones(H, W, dtype=dt) if mask is None else torch.from_numpy((np.asarray(mask) != 0).astype(np.float64)).to(dt)
    div = float(B) * float(m.sum())
    return (m * v).sum() / div, float((m * v.detach().abs()).sum() / div), torch.stack([ux, uy], 1)


# loss: float; grads: {name: float64 array}; frame_grad: d loss / d frames (None without a leaf); pred: P0 [B, T, C, H, W] float64; terms:
# float64 [T - 1], 0.0 where the weight is zero; scale: sum_s w_s (sum m |v| / (B N_m))_s / sum_s w_s, the un-cancelled scale of the loss;
# term_scales: that of every term
FlowResult = namedtuple("FlowResult", "loss grads frame_grad pred terms scale term_scales state")


def run_flow(weights, channels, frames, *, radius=7, eps=1e-2, direction=None, mask=None, n_fed=None, requant=False, step_weights=None, state=None, fed=None,
             leaf=None, term=None, constant_reference=True, dtype=torch.float64, flow_dtype=torch.float64):
    """`oracle.prednet_train_ref.run` with the loss formed from the predictions by `term`: term s is term(P0_s, x_{s+1}) -> (scalar, its
    un-cancelled scale).  None: the flow term of the settings, with x_{s+1} detached (constant_reference=False leaves it in the graph:
    the reference with a target path, which the trainer must NOT match).  leaf: None, "frames" (d loss / d frames [B, T, C, H, W]) or
    "tied" (the frames are one still per sequence; [B, C, H, W]).  dtype: as `run`'s: the network's arithmetic, float32 for the yardstick.
    flow_dtype: the flow term's arithmetic, on the widened prediction and frame; the semantics make it float64 whatever the network runs
    in (None: the network's dtype, an all-float32 statement)."""
    ch, L = list(channels), len(channels)
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in weights.items()}
    x = torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)).to(dtype)
    lf = None
    if leaf == "frames":
        x = lf = x.requires_grad_(True)
    elif leaf == "tied":
        assert (frames == frames[:, :1]).all(), "tied: every frame of a sequence must be the same still"
        lf = x[:, 0].detach().clone().requires_grad_(True)
        x = lf[:, None].expand(*x.shape)
    if term is None:
        fd = dtype if flow_dtype is None else flow_dtype
        term = lambda P, xn: torch_flow_term(P.to(fd), (xn.detach() if constant_reference else xn).to(fd), radius, eps, direction, mask)[:2]
    B, T = frames.shape[:2]
    H, W = frames.shape[3:]
    n_fed = T if n_fed is None else n_fed
    w_s = [1.0] * (T - 1) if step_weights is None else [float(v) for v in step_weights]
    if state is None:
        z = lambda l: torch.zeros(B, ch[l], H >> l, W >> l, dtype=dtype)
        hs, cs, Ps = [z(l) for l in range(L)], [z(l) for l in range(L)], [z(l) for l in range(L)]
    else:
        hs, cs, Ps = [[v.to(dtype) for v in s] for s in state]
    conv = lambda a, wt, b=None: F.conv2d(a, wt, b, padding=1)
    preds, terms, scales = [], [], []
    for t in range(T):
        if t < n_fed:
            xin = x[:, t]
        elif requant:
            xin = torch.from_numpy(np.asarray(fed[:, t], np.float32)).to(dtype)
        else:
            xin = Ps[0]
        E = [None] * L
        E[0] = _error_pair(xin, Ps[0])
        for l in range(1, L):
            A = F.max_pool2d(F.relu(conv(E[l - 1], p["ConvA%d/W" % l], p["ConvA%d/b" % l])), 2, 2)
            E[l] = _error_pair(A, Ps[l])
        for l in reversed(range(L)):
            stack = lambda s: torch.cat([p["ConvLSTM%d/%s/W" % (l, s % g)] for g in GATES], 0)
            zz = conv(E[l], stack("x_%s0")) + conv(hs[l], stack("h_%s"), torch.cat([p["ConvLSTM%d/h_%s/b" % (l, g)] for g in GATES]))
            if l < L - 1:
                zz = zz + conv(F.interpolate(hs[l + 1], scale_factor=2, mode="nearest"), stack("x_%s1"))
            zi, zf, zc, zo = torch.chunk(zz, 4, 1)
            c = cs[l]
            i = torch.sigmoid(zi + p["ConvLSTM%d/c_i/W" % l] * c)
            f = torch.sigmoid(zf + p["ConvLSTM%d/c_f/W" % l] * c)
            o = torch.sigmoid(zo + p["ConvLSTM%d/c_o/W" % l] * c)
            cs[l] = torch.tanh(zc) * i + f * c
            hs[l] = o * torch.tanh(cs[l])
            v = conv(hs[l], p["ConvP%d/W" % l], p["ConvP%d/b" % l])
            Ps[l] = clamp01(v) if l == 0 else F.relu(v)
        preds.append(Ps[0])
        if t < T - 1:
            f_s, sc = term(Ps[0], x[:, t + 1])
            terms.append(f_s)
            scales.append(sc)
    names = list(p)
    if T >= 2:
        loss = sum(w_s[s] * terms[s] for s in range(T - 1)) / sum(w_s)
        g = torch.autograd.grad(loss, [p[n] for n in names] + ([lf] if lf is not None else []), allow_unused=True)
        loss = float(loss.detach())
        scale = sum(w_s[s] * scales[s] for s in range(T - 1)) / sum(w_s)
    else:
        loss, scale, g = 0.0, 0.0, [None] * (len(names) + (lf is not None))
    grads = {n: (gg.double().numpy() if gg is not None else np.zeros(p[n].shape)) for n, gg in zip(names, g)}
    gx = None
    if lf is not None:
        gx = g[-1].double().numpy() if g[-1] is not None else np.zeros(tuple(lf.shape))
    out_terms = np.array([float(f_s.detach()) if w_s[s] != 0 else 0.0 for s, f_s in enumerate(terms)])
    state = tuple([s.detach() for s in ss] for ss in (hs, cs, Ps))
    return FlowResult(loss, grads, gx, torch.stack(preds, 1).detach().double().numpy(), out_terms, scale, np.array(scales), state)


def squared_error_term(P, xn):
    """the term under which run_flow is oracle.prednet_train_ref.run with objective="mse" """
    return ((P - xn) ** 2).mean(), 0.0


# ---- (c) the cases
# fields, bit for bit: (w, h, C, r, masked, modes).  (40, 24) is three 16-wide tiles, the last ragged (8 columns), and two tile rows, the
# second ragged; r = 16 is FLOW_MAX_R, where one tile's windows reach 48 rows; r = 7 at 12 x 8 is a window wider than the image
FIELD_CASES = [(12, 8, 1, 2, False, ("energy", "tangent")), (12, 8, 1, 7, False, ("energy", "tangent")), (16, 12, 3, 3, True, ("energy", "radial")),
               (24, 16, 1, 7, False, ("energy", "horizontal")), (40, 24, 3, 16, True, ("energy", "tangent"))]


def field_mask(w, h):
    """a mask that cuts windows, rows and tiles: the left quarter, one row and a scatter of single pixels are not counted"""
    m = np.ones((h, w), np.uint8)
    m[:, :w // 4] = 0
    m[h // 2, :] = 0
    m[1::5, 2::7] = 0
    return m


def field_inputs(w, h, C, kind, B=2):
    """(pred float32 [B, C, h, w] in [0, 1] with exact 0 and 1 among them, ref uint8): kind "random" bytes or a "smooth" pattern"""
    rng = np.random.default_rng(1000 * w + h + C + (kind == "smooth"))
    pred = rng.random((B, C, h, w)).astype(np.float32)
    pred[:, :, 0, ::3] = 0.0
    pred[:, :, -1, 1::4] = 1.0
    if kind == "random":
        ref = rng.integers(0, 256, (B, C, h, w)).astype(np.uint8)
    else:
        ref = np.ascontiguousarray(_drifting(w + h, B, 2, C, h, w)[:, 0])
    return pred, ref


def direction_of(mode, w, h):
    from evolutionary_illusion_generator_amd import train
    return None if mode == "energy" else train.flow_direction(mode, w, h)


# training calls against run_flow.  form: "still" (a still repeated 4 times, 2 self-fed steps on the float prediction, weights
# [0, 0, 0, 1, 1]), "still_requant" (the same through the byte), "drifting" (T = 5, teacher-forced, all weights one)
FlowCase = namedtuple("FlowCase", "w h ch wset mode r form")
FLOW_SHAPES = SHAPES + [(40, 24, [3, 4])]
FORMS = ("still", "still_requant", "drifting")
MODES = ("energy", "tangent")
RADII = (2, 7)
B_CASE = 2
STILL_WEIGHTS = [0.0, 0.0, 0.0, 1.0, 1.0]


def _flow_cases():
    out = []
    for w, h, ch in FLOW_SHAPES:
        wsets = ["live"] + (["random"] if (w, h, ch) in SHAPES else [])
        for wset in wsets:
            for mode in MODES:
                for r in RADII:
                    for form in FORMS:
                        out.append(FlowCase(w, h, tuple(ch), wset, mode, r, form))
    return out


FLOW_CASES = _flow_cases()


def flow_case_id(c):
    return "%dx%d-%s-%s-%s-r%d-%s" % (c.w, c.h, "_".join(map(str, c.ch)), c.wset, c.mode, c.r, c.form)


def is_dead(c):
    """"random" weights at the two gray shapes of SHAPES: P0 sits at the clamp everywhere, no gradient passes, the loss is not zero"""
    return c.wset == "random" and c.ch[0] == 1


@functools.lru_cache(maxsize=None)
def flow_case_frames(c):
    T = 6 if c.form != "drifting" else 5
    frames = _drifting(c.w + len(c.ch), B_CASE, T, c.ch[0], c.h, c.w)
    if c.form != "drifting":
        frames = np.ascontiguousarray(np.broadcast_to(frames[:, :1], frames.shape))
    return frames


def flow_case_call(c):
    """the keywords the trainer and run_flow share"""
    if c.form == "drifting":
        return dict(n_fed=None, requant=False, step_weights=None)
    return dict(n_fed=4, requant=c.form == "still_requant", step_weights=list(STILL_WEIGHTS))


def flow_case_settings(c):
    return dict(radius=c.r, eps=1e-2, direction=direction_of(c.mode, c.w, c.h), mask=None)


def flow_case_reference(c, pred=None, dtype=torch.float64, leaf=None, **kw):
    """run_flow of a case.  pred: the float32 predictions whose bytes a requantised case is fed (the GPU's own); None: the run is
    repeated on its own requantised predictions until every self-fed step has read them, as tests/train_support.py case_reference does."""
    wts, frames = case_weights(c.w, c.h, c.ch, c.wset), flow_case_frames(c)
    args = dict(flow_case_call(c), **flow_case_settings(c), dtype=dtype, leaf=leaf, **kw)
    if not args["requant"]:
        return run_flow(wts, list(c.ch), frames, **args)
    if pred is not None:
        return run_flow(wts, list(c.ch), frames, fed=_fed_from(pred), **args)
    fed = np.zeros(frames.shape, np.float32)
    T, n_fed = frames.shape[1], args["n_fed"]
    for _ in range(T - n_fed + 1):
        r = run_flow(wts, list(c.ch), frames, fed=fed, **args)
        fed = _fed_from(r.pred.astype(np.float32))
    return r
