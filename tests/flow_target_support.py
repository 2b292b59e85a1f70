"""Shared by tests/test_flow_target_host.py and tests/test_gpu_flow_target.py ("The target field"):
(a) the numpy restatement of the value, g and q under a target field (csrc/flow_target_kernels.h, then `tflow_struct_q_kernel`),
    operation for operation, on top of `flow_obj_support.flow_stage_ref` (the single step) and `dense_pyr_support.dense_pyr_ref` (the
    iterated solve), and of the fixed-order reduction `tflow_sum_kernel` -> `tloss_step_final_kernel`, so the value compares bit for bit;
(b) the float64 torch statement whose autograd gives the seed and the reference gradient, on `flow_obj_support.torch_flow_term`'s field
    and `flow_iter_support.torch_iter_field`'s, and `TargetTerm`, which plugs it into `flow_obj_support.run_flow(term=...)`;
(c) the cases.
torch on the CPU only; no GPU."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import dense_pyr_support as dp
from tests import flow_iter_support as fi
from tests import flow_obj_support as fs

FLOW_TARGET_KERNELS = ["tflow_target_kernel"]
EPS = dp.EPS
SUM_BLOCKS, SUM_THREADS = 64, 256      # STEP_LOSS_BLOCKS and EW_T of csrc/train_common.h


# ---- (a) the numpy restatement
def device_sum(v, div):
    """`tflow_sum_kernel` then `tloss_step_final_kernel` on v (any shape, read in memory order): thread t of block k adds its elements
    k 256 + t + j 16384 in ascending j from 0.0, a block folds its 256 sums in the LDS tree (w = 128 .. 1: red[t] += red[t + w]), the
    final kernel adds the 64 partials in order from 0.0 and divides"""
    v = np.asarray(v, np.float64).ravel()
    lanes = SUM_BLOCKS * SUM_THREADS
    acc = np.zeros(lanes)
    for lo in range(0, v.size, lanes):
        part = v[lo:lo + lanes]
        acc[:part.size] = acc[:part.size] + part
    red = acc.reshape(SUM_BLOCKS, SUM_THREADS).copy()
    w = SUM_THREADS // 2
    while w > 0:
        red[:, :w] = red[:, :w] + red[:, w:2 * w]
        w //= 2
    s = 0.0
    for k in range(SUM_BLOCKS):
        s = s + red[k, 0]
    return float(s / float(div))


TargetValue = namedtuple("TargetValue", "value mv gx gy n_mask")


def target_value_ref(u, target, mask=None):
    """`tflow_target_kernel` on the field u and the target, both float64 [B, 2, H, W]; mask [H, W] or None.  -> the term (through
    `device_sum`), mv [B, H, W] and g = (gx, gy), masked"""
    u, target = np.asarray(u, np.float64), np.asarray(target, np.float64)
    B, _, H, W = u.shape
    ex, ey = u[:, 0] - target[:, 0], u[:, 1] - target[:, 1]
    v = ex * ex + ey * ey
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    n_m = int(m.sum())
    mv = np.where(m, v, 0.0)
    gx, gy = np.where(m, 2.0 * ex, 0.0), np.where(m, 2.0 * ey, 0.0)
    return TargetValue(device_sum(mv, float(B * n_m)), mv, gx, gy, n_m)


def solve_planes(pred, ref64, r, eps):
    """(Ix, Iy, a, b, c, det, u) of the single step as `flow_obj_support.flow_stage_ref` forms them (its prep and solve lines, restated:
    that function returns the field alone); u is asserted to be its field bit for bit"""
    pred = np.asarray(pred, np.float32)
    H, W = pred.shape[-2:]
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
    u = np.stack([-((cc * bx - bb * by) / det), -((aa * by - bb * bx) / det)], 1)
    assert np.array_equal(u, fs.flow_stage_ref(pred, ref64, r, eps).u)
    return Ix, Iy, aa, bb, cc, det, u


TargetStage = namedtuple("TargetStage", "value u mv gx gy qx qy")


def target_stage_ref(pred, ref64, r, eps, target, mask=None):
    """The single step's stage under a target: pred float32 and ref64 float64 [B, C, H, W] (`flow_stage_ref`'s arguments), target
    float64 [B, 2, H, W].  q is `tflow_struct_q_kernel`'s, from g over the solve's a, b, c and det in the solve's written formula."""
    Ix, Iy, aa, bb, cc, det, u = solve_planes(pred, ref64, r, eps)
    t = target_value_ref(u, target, mask)
    qx, qy = (cc * t.gx - bb * t.gy) / det, (aa * t.gy - bb * t.gx) / det
    return TargetStage(t.value, u, t.mv, t.gx, t.gy, qx, qy)


def target_iter_ref(img0, img1, r, eps, levels, iters, target, mask=None):
    """The iterated stage under a target on byte images (`dense_pyr_ref`'s arguments): the field, the value and g, which `iter_backward`
    takes as it is (no q is formed)"""
    u = dp.dense_pyr_ref(img0, img1, r, eps, levels, iters)
    t = target_value_ref(u, target, mask)
    return TargetStage(t.value, u, t.mv, t.gx, t.gy, None, None)


# ---- (b) the torch statement
def torch_target_value(u, target, mask=None):
    """(f, its un-cancelled scale: every summand is >= 0, so f itself) of a torch field u [B, 2, H, W] against the target"""
    B, _, H, W = u.shape
    tg = torch.from_numpy(np.array(target, dtype=np.float64)).to(u.dtype)
    ex, ey = u[:, 0] - tg[:, 0], u[:, 1] - tg[:, 1]
    v = ex * ex + ey * ey
    m = torch.ones(H, W, dtype=u.dtype) if mask is None else torch.from_numpy((np.asarray(mask) != 0).astype(np.float64)).to(u.dtype)
    f = (m * v).sum() / (float(B) * float(m.sum()))
    return f, float(f.detach())


def torch_field(P, x, r, eps, solve=(1, 1)):
    """the field of prediction P against the reference x, both in the graph where the caller left them: the single step's
    (`flow_obj_support.torch_flow_term`) or the iterated solve's (`flow_iter_support.torch_iter_field`)"""
    if tuple(solve) == (1, 1):
        return fs.torch_flow_term(P, x, r, eps)[2]
    return fi.torch_iter_field(P, x, r, eps, solve[0], solve[1])


TorchStage = namedtuple("TorchStage", "value u seed64 ref64")


def torch_stage(pred, ref, r, eps, solve, target, mask=None, scale=1.0):
    """float images pred, ref [B, C, H, W] -> the value, the field, and scale * d value / d pred, d ref as float64"""
    P = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    x = torch.tensor(np.asarray(ref, np.float64), requires_grad=True)
    u = torch_field(P, x, r, eps, solve)
    f, _ = torch_target_value(u, target, mask)
    gP, gx = torch.autograd.grad(f, [P, x])
    return TorchStage(float(f.detach()), u.detach().numpy(), gP.numpy() * scale, gx.numpy() * scale)


class TargetTerm:
    """The `term` callback of `flow_obj_support.run_flow` under a target field [B, T - 1, 2, H, W]: term s is the mean squared endpoint
    error of the field against target[:, s].  pairing "prediction": the field runs from P0_{s-1} IN THE GRAPH (the first reference is
    `start`, detached) to P0_s; "frame": from frame s + 1, a constant unless moving."""

    def __init__(self, target, radius, eps, solve=(1, 1), mask=None, pairing="frame", moving=False, start=None):
        self.target, self.args, self.mask = np.asarray(target, np.float64), (radius, eps, tuple(solve)), mask
        self.pairing, self.moving, self.s = pairing, moving, 0
        self.prev = None if start is None else start.detach()

    def __call__(self, P, xn):
        if self.pairing == "prediction":
            ref, self.prev = self.prev, P
        else:
            ref = xn if self.moving else xn.detach()
        s, self.s = self.s, self.s + 1
        u = torch_field(P.to(torch.float64), ref.to(torch.float64), *self.args)
        return torch_target_value(u, self.target[:, s], self.mask)


# ---- (c) the cases
# the stage alone: (name, w, h, C, genome seeds, shifts): less than one tile; ragged tiles and three channels; three tiles across and odd
# pyramid sizes (33 x 18 -> 17 x 9).  Two samples each, whose truths differ.
STAGE_SHAPES = [("8x8", 8, 8, 1, (2, 13), ((0.7, -0.4), (-0.3, 0.2))),
                ("20x15", 20, 15, 3, (21, 23), ((1.5, 0.5), (-0.6, 0.5))),
                ("33x18", 33, 18, 1, (63, 76), ((1.25, -0.75), (0.5, 0.75)))]
RADII = (1, 3, 7)            # every image allows all three: a window is truncated at the border (7 at 8 x 8 is wider than the image)
SOLVES = ((1, 1), (2, 2))    # 2 levels: the coarsest levels are 4 x 4, 10 x 8 and 17 x 9, all at least 4 pixels
STAGE_CASES = [(s[0], r, solve) for s in STAGE_SHAPES for r in RADII for solve in SOLVES]


def stage_case_id(c):
    return "%s-r%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1])


@functools.lru_cache(maxsize=None)
def stage_inputs(name):
    """(img0, img1 uint8 [2, C, h, w], truth float64 [2, 2, h, w]): the reference, the prediction and the exact flow between them"""
    _, w, h, C, seeds, shifts = next(s for s in STAGE_SHAPES if s[0] == name)
    parts = [dp.shift_case(w, h, C, seed, shift) for seed, shift in zip(seeds, shifts)]
    out = tuple(np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def stage_mask(w, h):
    """a shared mask that cuts windows, rows and tiles (`flow_obj_support.field_mask`)"""
    return fs.field_mask(w, h)


@functools.lru_cache(maxsize=None)
def stage_reference(name, r, solve, masked, target="truth"):
    """(the numpy restatement, the torch statement) of a stage case; target "truth" or "zero"; made once and shared"""
    img0, img1, truth = stage_inputs(name)
    h, w = img0.shape[-2:]
    mask = stage_mask(w, h) if masked else None
    tg = truth if target == "truth" else np.zeros_like(truth)
    pred = fi.as_floats(img1)
    if tuple(solve) == (1, 1):
        rest = target_stage_ref(pred, fs.byte_reference(img0), r, EPS, tg, mask)
    else:
        rest = target_iter_ref(img0, img1, r, EPS, solve[0], solve[1], tg, mask)
    return rest, torch_stage(pred, fi.as_floats(img0), r, EPS, solve, tg, mask)


# the host case of the issue: the exact binary shift (0.25, -0.125) at 16 x 12 of tests/moving_support.py, radius 3, eps 1e-4, the pixels
# at least 3 from the border
TRUTH_RADIUS, TRUTH_EPS = 3, 1e-4


def truth_case():
    """(frames uint8 [1, T, C, h, w], flow float64 [1, T - 1, 2, h, w], mask uint8 [h, w]) of the shared exact-shift sample"""
    from tests import moving_support as ms
    name, b = ms.SHIFT_SAMPLE
    c, r = ms.case(name), ms.reference(name)
    mask = np.zeros((c["h"], c["w"]), np.uint8)
    mask[TRUTH_RADIUS:c["h"] - TRUTH_RADIUS, TRUTH_RADIUS:c["w"] - TRUTH_RADIUS] = 1
    return r["frames"][b:b + 1], r["flow"][b:b + 1], mask


# the training call: [1, 8, 16] at 16 x 12 gray, B = 2, T = 4, two fed steps and two self-fed on the float prediction; frames and truth
# from two moving textures (`dense_pyr_support.shift_case`'s layer, four frames)
TRAIN_SHAPE = (16, 12, (1, 8, 16))
TRAIN_B, TRAIN_T, TRAIN_FED, TRAIN_RADIUS = 2, 4, 2, 3
TRAIN_FORMS = (("frame", "constant"), ("prediction", "constant"), ("frame", "moving"))
TRAIN_SEEDS, TRAIN_SHIFTS = (76, 13), ((0.25, -0.125), (0.5, 0.75))


@functools.lru_cache(maxsize=None)
def train_inputs(n=TRAIN_B):
    """(frames uint8 [n, T, 1, 12, 16], flow float64 [n, T - 1, 2, 12, 16], weights): the video, its exact flow, the "live" weights"""
    from tests import moving_support as ms
    from tests.train_support import _weight_sets
    w, h, ch = TRAIN_SHAPE
    seeds, shifts = (TRAIN_SEEDS * n)[:n], (TRAIN_SHIFTS * n)[:n]
    layers = [(complex(0.04, 0.0), complex(0.5, -0.25), complex(1.0, 0.0), complex(*shift)) for shift in shifts]
    ref = ms.moving_ref(ms.build_case(w, h, ch[0], TRAIN_T, [ms._genome(ch[0], seed) for seed in seeds], layers, 1))
    return np.ascontiguousarray(ref["frames"]), np.ascontiguousarray(ref["flow"]), dict(_weight_sets(list(ch), w, h))["live"]


def train_objective(pairing, reference):
    from evolutionary_illusion_generator_amd import train
    return train.PredictionFlow(TRAIN_RADIUS, EPS) if pairing == "prediction" else train.FlowObjective(TRAIN_RADIUS, EPS, reference=reference)


@functools.lru_cache(maxsize=None)
def train_reference(pairing, reference, target="truth", n=TRAIN_B):
    """`run_flow` of the training call under `TargetTerm`, float64, the frames a leaf; target "truth" or "zero" (the plain mean squared
    displacement: the statement the trainer must NOT match under the truth)"""
    frames, flow, wts = train_inputs(n)
    w, h, ch = TRAIN_SHAPE
    tg = flow if target == "truth" else np.zeros_like(flow)
    start = torch.zeros(n, ch[0], h, w, dtype=torch.float64) if pairing == "prediction" else None
    term = TargetTerm(tg, TRAIN_RADIUS, EPS, pairing=pairing, moving=reference == "moving", start=start)
    return fs.run_flow(wts, list(ch), frames, term=term, leaf="frames", n_fed=TRAIN_FED, requant=False)
