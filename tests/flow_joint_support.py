"""Shared by tests/test_flow_joint_host.py and tests/test_gpu_flow_joint.py ("The joint objective and the valid
pixels"):
(a) the validity planes of moving textures: `valid_ref`, the numpy restatement of csrc/cppn_valid_kernel.h operation for operation,
    `valid_brute`, the same statement pixel by pixel in Python floats, and their cases;
(b) the numpy restatement of csrc/flow_valid_kernels.h on top of tests/flow_target_support.py (the field, the fixed-order reduction),
    so the value compares bit for bit, and the float64 torch statement -- the mean over the samples of every sample's mean squared
    endpoint error over its own counted pixels -- whose autograd gives the seed and the reference gradient;
(c) the training calls: `JointTerm`, which adds mu * mean((P - x)^2) with x in the graph to any `run_flow` term, the four kinds of call
    and their float64 references.
torch on the CPU only; no GPU."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import dense_pyr_support as dp
from tests import flow_iter_support as fi
from tests import flow_obj_support as fs
from tests import flow_target_support as ft
from tests import moving_support as ms

FLOW_VALID_KERNELS = ["tflow_target_valid_kernel", "tflow_valid_count_kernel"]
EPS = ft.EPS


# ---- (a) the validity planes
VALID, OUT_OF_BOUNDS, OCCLUDED = 0, 1, 2      # the classes of `valid_ref`: out of bounds wins where a pixel is both


def valid_ref(desc):
    """(valid uint8 [n, T - 1, h, w], class uint8 likewise) of a case of tests/moving_support.py: csrc/cppn_valid_kernel.h in numpy, every
    product and sum one float64 rounding in the kernel's order"""
    w, h, n, T, L = (desc[k] for k in ("w", "h", "n", "T", "L"))
    px, py = ms.pixel_centres(w, h)
    hx, hy = (w - 1) / 2.0, (h - 1) / 2.0
    valid, cls = np.zeros((n, T - 1, h * w), np.uint8), np.zeros((n, T - 1, h * w), np.uint8)
    for b in range(n):
        for t in range(T - 1):
            u, v = ms.texture_coords(desc["affine"][b, t, 0], px, py)
            vis = np.zeros(h * w, bool)
            if L == 2:
                u1, v1 = ms.texture_coords(desc["affine"][b, t, 1], px, py)
                vis = u1 * u1 + v1 * v1 < 1.0
                u, v = np.where(vis, u1, u), np.where(vis, v1, v)
            inv = desc["affine_inv"][b, t + 1]
            i = [np.where(vis, inv[L - 1][k], inv[0][k]) for k in range(6)]
            qx, qy = (i[0] * u + i[1] * v) + i[2], (i[3] * u + i[4] * v) + i[5]
            inb = (qx >= -hx) & (qx <= hx) & (qy >= -hy) & (qy <= hy)
            occ = np.zeros(h * w, bool)
            if L == 2:
                u1, v1 = ms.texture_coords(desc["affine"][b, t + 1, 1], qx, qy)
                occ = ~vis & (u1 * u1 + v1 * v1 < 1.0)
            valid[b, t] = inb & ~occ
            cls[b, t] = np.where(~inb, OUT_OF_BOUNDS, np.where(occ, OCCLUDED, VALID))
    return valid.reshape(n, T - 1, h, w), cls.reshape(n, T - 1, h, w)


def valid_brute(desc):
    """the planes of `valid_ref` pixel by pixel in Python floats: take the pixel to the texture of the layer it shows, bring that point
    back through the next frame's inverse, and ask whether it lands inside the image and, if it is on layer 0, outside the disc there"""
    w, h, n, T, L = (desc[k] for k in ("w", "h", "n", "T", "L"))
    A, I = desc["affine"].tolist(), desc["affine_inv"].tolist()
    out = np.zeros((n, T - 1, h, w), np.uint8)
    to = lambda a, x, y: ((a[0] * x + a[1] * y) + a[2], (a[3] * x + a[4] * y) + a[5])
    for b in range(n):
        for t in range(T - 1):
            for row in range(h):
                for col in range(w):
                    x, y = col - (w - 1) / 2.0, row - (h - 1) / 2.0
                    layer, (u, v) = 0, to(A[b][t][0], x, y)
                    if L == 2:
                        u1, v1 = to(A[b][t][1], x, y)
                        if u1 * u1 + v1 * v1 < 1.0:
                            layer, u, v = 1, u1, v1
                    qx, qy = to(I[b][t + 1][layer], u, v)
                    seen = -(w - 1) / 2.0 <= qx <= (w - 1) / 2.0 and -(h - 1) / 2.0 <= qy <= (h - 1) / 2.0
                    if seen and L == 2 and layer == 0:
                        u1, v1 = to(A[b][t + 1][1], qx, qy)
                        seen = not u1 * u1 + v1 * v1 < 1.0
                    out[b, t, row, col] = seen
    return out


# "live": 16 x 12, two layers, T 3, two samples: the backgrounds leave the image on one side, the discs move against them and cover what
#   was visible; sample 1 also turns and zooms.  tests/test_flow_joint_host.py asserts at least 4 pixels of every class in some term.
# "33x18": one layer, T 2: N = 594 is no multiple of the block of 128, and only out-of-bounds pixels exist.
# "8x8": two layers, T 2, less than one block.
VALID_CASES = ("live", "33x18", "8x8")


@functools.lru_cache(maxsize=None)
def valid_case(name):
    g = lambda seed: ms._genome(1, seed, 5)     # the planes do not read the genomes: the smallest will do
    if name == "live":
        layers = [ms._layer0(0.2, 0.3, (0.2, 0.1), (1.75, -1.25)), ms._disc(3.1, (-2.03, 1.02), 0.7, (-1.5, 0.75)),
                  ms._layer0(0.2, 1.1, (-0.3, 0.2), (-1.25, 0.5), turn=0.05, zoom=1.03), ms._disc(2.6, (3.02, -1.01), 1.3, (1.0, 1.25), zoom=1.04)]
        return ms.build_case(16, 12, 1, 3, [g(11), g(12), g(13), g(14)], layers, 2)
    if name == "33x18":
        return ms.build_case(33, 18, 1, 2, [g(15)], [ms._layer0(0.1, 0.4, (0.1, -0.2), (1.5, -0.75), turn=0.02)], 1)
    if name == "8x8":
        return ms.build_case(8, 8, 1, 2, [g(16), g(17)], [ms._layer0(0.3, 0.4, (0.1, -0.2), (0.7, -0.4), turn=0.01), ms._disc(2.2, (0.52, -0.51), 0.2, (-1.0, 0.75))], 2)
    raise KeyError(name)


# ---- (b) the stage under validity planes
ValidValue = namedtuple("ValidValue", "value mv gx gy n_mask counts ratios")


def valid_value_ref(u, target, valid, mask=None):
    """csrc/flow_valid_kernels.h on the field u and the target, float64 [B, 2, H, W], under the planes valid [B, H, W] and the shared mask
    [H, W] (None: all): the integer counts c_b, r_b = N_m / c_b (0 where c_b is 0), mv = v r_b and g = ((2 ex) r_b, (2 ey) r_b) where
    the pixel counts, 0 elsewhere; the term through `flow_target_support.device_sum` over B N_m, the target field's own divisor"""
    u, target = np.asarray(u, np.float64), np.asarray(target, np.float64)
    B, _, H, W = u.shape
    ex, ey = u[:, 0] - target[:, 0], u[:, 1] - target[:, 1]
    v = ex * ex + ey * ey
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    n_m = int(m.sum())
    counted = m[None] & (np.asarray(valid) != 0)
    c = counted.reshape(B, -1).sum(1).astype(np.int64)
    r = np.array([float(n_m) / float(k) if k > 0 else 0.0 for k in c])[:, None, None]
    mv = np.where(counted, v * r, 0.0)
    gx, gy = np.where(counted, (2.0 * ex) * r, 0.0), np.where(counted, (2.0 * ey) * r, 0.0)
    return ValidValue(ft.device_sum(mv, float(B * n_m)), mv, gx, gy, n_m, c, r[:, 0, 0])


def valid_stage_ref(name, r, solve, masked, valid):
    """(value, field) of a stage case of `flow_target_support.STAGE_SHAPES` against its truth under the planes"""
    img0, img1, truth = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    mask = ft.stage_mask(w, h) if masked else None
    if tuple(solve) == (1, 1):
        u = ft.solve_planes(fi.as_floats(img1), fs.byte_reference(img0), r, EPS)[-1]
    else:
        u = dp.dense_pyr_ref(img0, img1, r, EPS, solve[0], solve[1])
    return valid_value_ref(u, truth, valid, mask), u


def torch_valid_value(u, target, valid, mask=None):
    """(f, its un-cancelled scale: every summand is >= 0, so f itself) of a torch field u [B, 2, H, W]: the mean over the samples of each
    sample's mean squared endpoint error over the pixels its plane and the mask count; a sample that counts none adds 0"""
    B, _, H, W = u.shape
    tg = torch.from_numpy(np.array(target, dtype=np.float64)).to(u.dtype)
    ex, ey = u[:, 0] - tg[:, 0], u[:, 1] - tg[:, 1]
    v = ex * ex + ey * ey
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    counted = torch.from_numpy((m[None] & (np.asarray(valid) != 0)).astype(np.float64)).to(u.dtype)
    f = u.sum() * 0.0
    for b in range(B):
        c = float(counted[b].sum())
        if c > 0:
            f = f + (counted[b] * v[b]).sum() / c
    f = f / float(B)
    return f, float(f.detach())


def torch_valid_stage(pred, ref, r, eps, solve, target, valid, mask=None, scale=1.0):
    """`flow_target_support.torch_stage` under the planes"""
    P = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    x = torch.tensor(np.asarray(ref, np.float64), requires_grad=True)
    u = ft.torch_field(P, x, r, eps, solve)
    f, _ = torch_valid_value(u, target, valid, mask)
    gP, gx = torch.autograd.grad(f, [P, x])
    return ft.TorchStage(float(f.detach()), u.detach().numpy(), gP.numpy() * scale, gx.numpy() * scale)


STAGE_RADII = (1, 7)
STAGE_CASES = [(s[0], r, solve) for s in ft.STAGE_SHAPES for r in STAGE_RADII for solve in ft.SOLVES]


def stage_valid(w, h):
    """uint8 [2, h, w]: planes that differ per sample and cut windows, rows and tiles: sample 0 loses its right third, one row and a
    lattice of single pixels, sample 1 its two top rows, one column and another lattice"""
    v = np.ones((2, h, w), np.uint8)
    v[0, :, w - w // 3:] = 0
    v[0, h // 3, :] = 0
    v[0, ::4, 1::5] = 0
    v[1, :2, :] = 0
    v[1, :, w // 2] = 0
    v[1, 2::3, ::6] = 0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def stage_reference(name, r, solve, masked):
    """(the numpy restatement (ValidValue, field), the torch statement) of a stage case under `stage_valid`; made once and shared"""
    img0, img1, truth = ft.stage_inputs(name)
    h, w = img0.shape[-2:]
    valid = stage_valid(w, h)
    mask = ft.stage_mask(w, h) if masked else None
    return valid_stage_ref(name, r, solve, masked, valid), torch_valid_stage(fi.as_floats(img1), fi.as_floats(img0), r, EPS, solve, truth, valid, mask)


# ---- (c) the training calls: `flow_target_support.TRAIN_SHAPE`, B 2, T 4, two fed and two self-fed steps
class ValidTargetTerm(ft.TargetTerm):
    """`flow_target_support.TargetTerm` under validity planes [B, T - 1, H, W]"""

    def __init__(self, target, valid, *args, **kw):
        super().__init__(target, *args, **kw)
        self.valid = np.asarray(valid)

    def __call__(self, P, xn):
        if self.pairing == "prediction":
            ref, self.prev = self.prev, P
        else:
            ref = xn if self.moving else xn.detach()
        s, self.s = self.s, self.s + 1
        u = ft.torch_field(P.to(torch.float64), ref.to(torch.float64), *self.args)
        return torch_valid_value(u, self.target[:, s], self.valid[:, s], self.mask)


class JointTerm:
    """`run_flow`'s term of the joint objective: the flow term of `inner` plus mu * mean((P - x)^2), the frame x in the graph (its
    target path reaches the frame gradient).  mu 0: the flow term alone, the statement a joint call must NOT match."""

    def __init__(self, inner, mu):
        self.inner, self.mu = inner, float(mu)

    def __call__(self, P, xn):
        f, scale = self.inner(P, xn)
        if self.mu == 0.0:
            return f, scale
        sq = ((P - xn) ** 2).mean()
        return f + self.mu * sq, scale + self.mu * float(sq.detach())


KINDS = ("target", "valid", "plain", "score")     # (a) .. (d) of the issue
TRAIN_SCORE = dict(min_count=4, **fi.SCORE_LIMITS)


@functools.lru_cache(maxsize=None)
def train_mu(kind, pairing, reference, solve=(1, 1), n=ft.TRAIN_B):
    """The weight of the frame term in a training case, chosen on the float64 references alone: the power of two nearest to the ratio of
    the weight-gradient norms of the flow part and of the squared error, so that neither part drowns the other (the flow parts of the
    cases span four decades).  tests/test_flow_joint_host.py asserts that the two norms then lie within a factor of 10 of each other."""
    flow_part = grad_norm(train_reference(kind, pairing, reference, solve, 0.0, n).grads)
    frame_part = grad_norm(train_reference(kind, pairing, reference, solve, 0.0, n, "mse").grads)
    return float(2.0 ** round(np.log2(flow_part / frame_part)))


@functools.lru_cache(maxsize=None)
def train_desc(n=ft.TRAIN_B):
    """the case `flow_target_support.train_inputs` renders, as a case of tests/moving_support.py (its affines state the validity)"""
    w, h, ch = ft.TRAIN_SHAPE
    seeds, shifts = (ft.TRAIN_SEEDS * n)[:n], (ft.TRAIN_SHIFTS * n)[:n]
    layers = [(complex(0.04, 0.0), complex(0.5, -0.25), complex(1.0, 0.0), complex(*shift)) for shift in shifts]
    return ms.build_case(w, h, ch[0], ft.TRAIN_T, [ms._genome(ch[0], seed) for seed in seeds], layers, 1)


def train_valid(n=ft.TRAIN_B):
    """uint8 [n, T - 1, 12, 16]: the validity planes of the training video on the restatement"""
    return valid_ref(train_desc(n))[0]


def train_flow(kind, pairing, reference, solve=(1, 1)):
    """the trainer's objective of a kind"""
    from evolutionary_illusion_generator_amd import train
    score = train.FlowScore(**TRAIN_SCORE) if kind == "score" else None
    return train.make_flow(pairing, ft.TRAIN_RADIUS, EPS, reference=reference, score=score, levels=solve[0], iters=solve[1])


def train_kwargs(kind, n=ft.TRAIN_B):
    """flow_target / flow_valid of a kind"""
    _, flow, _ = ft.train_inputs(n)
    return {"target": dict(flow_target=flow), "valid": dict(flow_target=flow, flow_valid=train_valid(n)), "plain": {}, "score": {}}[kind]


@functools.lru_cache(maxsize=None)
def train_reference(kind, pairing, reference, solve=(1, 1), mu=None, n=ft.TRAIN_B, part="joint"):
    """`run_flow` of a training call of a kind under `JointTerm`, float64, the frames a leaf; mu None: `train_mu` of the case.  part
    "mse": the squared error alone (`flow_obj_support.squared_error_term`), for the choice of mu"""
    if mu is None and part == "joint":
        mu = train_mu(kind, pairing, reference, solve, n)
    frames, flow, wts = ft.train_inputs(n)
    w, h, ch = ft.TRAIN_SHAPE
    if part == "mse":
        return fs.run_flow(wts, list(ch), frames, term=fs.squared_error_term, leaf="frames", n_fed=ft.TRAIN_FED, requant=False)
    start = torch.zeros(n, ch[0], h, w, dtype=torch.float64) if pairing == "prediction" else None
    moving = reference == "moving"
    if kind == "target":
        inner = ft.TargetTerm(flow, ft.TRAIN_RADIUS, EPS, solve=solve, pairing=pairing, moving=moving, start=start)
    elif kind == "valid":
        inner = ValidTargetTerm(flow, train_valid(n), ft.TRAIN_RADIUS, EPS, solve=solve, pairing=pairing, moving=moving, start=start)
    else:
        from evolutionary_illusion_generator_amd import train
        score = fi.support_score(train.FlowScore(**TRAIN_SCORE), h) if kind == "score" else None
        inner = fi.IterTerm(start, ft.TRAIN_RADIUS, EPS, solve[0], solve[1], score=score, pairing=pairing, moving=moving, single=tuple(solve) == (1, 1))
    return fs.run_flow(wts, list(ch), frames, term=JointTerm(inner, mu), leaf="frames", n_fed=ft.TRAIN_FED, requant=False)


def grad_norm(grads):
    return float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads.values())))
