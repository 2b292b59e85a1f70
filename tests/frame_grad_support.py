"""Shared by tests/test_frame_grad_host.py and tests/test_gpu_frame_grad.py: the float64 autograd statement of PredNet training with
the FRAMES as a leaf (the operations of oracle/prednet_train_ref.py `run`, in its order, so that its loss and weight gradients are
`run`'s to the bit; DESIGN.md section 13, "Frame gradients"), the analytic target path, and a numpy float32 restatement of
tstill_step_kernel / tstill_absmax_kernel (csrc/frame_grad_kernels.h)."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import GATES
from oracle.prednet_train_ref import _error_pair, clamp01

# loss: float; grads: {name: float64 array}; frame_grad: d loss / d x [B, T, C, H, W] float64 (x = byte / 255 in float32, as a double);
# pred: P0 [B, T, C, H, W] float64; state: the final (h, c, P), lists of detached tensors
FrameResult = namedtuple("FrameResult", "loss grads frame_grad pred state")


def run_frames(weights, channels, frames, *, objective="mse", layer_weights=None, n_fed=None, requant=False, step_weights=None, state=None, fed=None, tied=False, dtype=torch.float64):
    """`oracle.prednet_train_ref.run` with the frames as a leaf of the graph: the same arguments, the same operations.  A step
    t >= n_fed does not read x_t (its input is the previous prediction, or the constant fed[:, t]); every x_{s+1} is the target
    of term s.  tied=True: the T frames of every sequence are one still; the leaf is that still, which every step and every
    target reads, and frame_grad is [B, C, H, W].  dtype: as `run`'s, the float32 yardstick."""
    ch, L = list(channels), len(channels)
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in weights.items()}
    x = leaf = torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)).to(dtype).requires_grad_(True)
    if tied:
        assert (frames == frames[:, :1]).all(), "tied: every frame of a sequence must be the same still"
        leaf = x[:, 0].detach().clone().requires_grad_(True)
        x = leaf[:, None].expand(*x.shape)
    B, T = frames.shape[:2]
    H, W = frames.shape[3:]
    n_fed = T if n_fed is None else n_fed
    w_s = [1.0] * (T - 1) if step_weights is None else [float(v) for v in step_weights]
    lam = [1.0] + [0.0] * (L - 1) if layer_weights is None else [float(v) for v in layer_weights]
    if state is None:
        z = lambda l: torch.zeros(B, ch[l], H >> l, W >> l, dtype=dtype)
        hs, cs, Ps = [z(l) for l in range(L)], [z(l) for l in range(L)], [z(l) for l in range(L)]
    else:
        hs, cs, Ps = [[v.to(dtype) for v in s] for s in state]
    conv = lambda a, wt, b=None: F.conv2d(a, wt, b, padding=1)
    preds, mses = [], []
    err = [[None] * L for _ in range(T - 1)]
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
            if t >= 1:
                err[t - 1][l] = E[l].mean()
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
            err[t][0] = _error_pair(x[:, t + 1], Ps[0]).mean()
            mses.append(((Ps[0] - x[:, t + 1]) ** 2).mean())
    names = list(p)
    if T >= 2:
        terms = mses if objective == "mse" else [sum(lam[l] * row[l] for l in range(L)) for row in err]
        loss = sum(w_s[s] * terms[s] for s in range(T - 1)) / sum(w_s)
        g = torch.autograd.grad(loss, [p[n] for n in names] + [leaf], allow_unused=True)
        loss = float(loss.detach())
    else:
        loss, g = 0.0, [None] * (len(names) + 1)
    grads = {n: (gg.double().numpy() if gg is not None else np.zeros(p[n].shape)) for n, gg in zip(names, g)}
    gx = g[-1].double().numpy() if g[-1] is not None else np.zeros(tuple(leaf.shape))
    state = tuple([s.detach() for s in ss] for ss in (hs, cs, Ps))
    return FrameResult(loss, grads, gx, torch.stack(preds, 1).detach().double().numpy(), state)


def target_path(frames, pred, objective="mse", step_weights=None, layer_weights=None):
    """The target path of d loss / d x_t in float64, from the predictions: for t >= 1, -2 w (P0_{t-1} - x_t) / (sum w B C H W)
    under "mse" and -w lam_0 sign(P0_{t-1} - x_t) / (sum w B 2 C H W) under "error"; zero for t = 0."""
    x = (frames.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    B, T = frames.shape[:2]
    numel = float(B * np.prod(frames.shape[2:]))
    w = np.ones(T - 1) if step_weights is None else np.asarray(step_weights, np.float64)
    lam0 = 1.0 if layer_weights is None else float(layer_weights[0])
    out = np.zeros_like(x)
    for t in range(1, T):
        d = np.asarray(pred[:, t - 1], np.float64) - x[:, t]
        if objective == "mse":
            out[:, t] = -2.0 * w[t - 1] * d / (w.sum() * numel)
        else:
            out[:, t] = -w[t - 1] * lam0 * np.sign(d) / (w.sum() * 2.0 * numel)
    return out


def fold_tied(per_frame):
    """the float32 fold the tied mode is: zeros, then + g_s for s = T - 1 .. 0"""
    per_frame = np.asarray(per_frame, np.float32)
    acc = np.zeros(per_frame.shape[:1] + per_frame.shape[2:], np.float32)
    for s in reversed(range(per_frame.shape[1])):
        acc = acc + per_frame[:, s]
    return acc


def still_step_ref(images, grad, step, mask=None):
    """tstill_absmax_kernel + tstill_step_kernel in numpy float32, operation by operation.  images uint8 [n, C, H, W], grad float32
    [n, C, H, W], mask [H, W] (0 = keep) or None.  Returns the new uint8 images."""
    images = np.asarray(images, np.uint8)
    g = np.asarray(grad, np.float32)
    free = np.ones(images.shape[2:], bool) if mask is None else np.asarray(mask) != 0
    free = np.broadcast_to(free, images.shape)
    k = np.float32(float(step) / 255.0)
    out = images.copy()
    for b in range(images.shape[0]):
        mb = np.float32(np.abs(g[b])[free[b]].max()) if free[b].any() else np.float32(0)
        if not mb > 0:
            continue
        x = images[b].astype(np.float32) / np.float32(255.0)
        xn = np.minimum(np.maximum(x + k * (g[b] / mb), np.float32(0)), np.float32(1))
        new = (xn * np.float32(255.0) + np.float32(0.5)).astype(np.int32).astype(np.uint8)
        out[b] = np.where(free[b], new, images[b])
    return out


def zero_steps(T, n_fed, step_weights=None, dead=False, first_has_target=False):
    """The steps whose frame gradient is exactly zero by construction: no target path (the call's first frame, or a term of weight
    zero) and no input path (a self-fed step; or dead: a case of tests/train_support.py `is_all_zero`, where P0 sits at the clamp everywhere and the
    objective reaches the frames through P0 alone)."""
    n_fed = T if n_fed is None else n_fed
    no_target = lambda t: (t == 0 and not first_has_target) or (t >= 1 and step_weights is not None and step_weights[t - 1] == 0)
    return {t for t in range(T) if no_target(t) and (t >= n_fed or dead)}


def check_frame_grads(got, ref, what="", tied=None, zero=()):
    """The project's gradient rule (tests/train_support.py `_check_grads`, which states where its two bounds come from) per step t
    and for the tied output: |got_t - ref_t|_2 <= 1e-3 |ref_t|_2 and max |got_t - ref_t| <= E max |ref_t|, no term shared between
    steps.  A step whose reference is exactly zero fails unless it is in `zero` (`zero_steps`); there |got_t|_2 <= 1e-6 G, G the
    norm of the whole frame gradient.  got, ref: [B, T, C, H, W]; tied: the tied output [B, C, H, W] (None: the sum of got).
    Returns the worst ratio of a miss to its bound, norm or element-wise."""
    from tests.train_support import check_tensor, check_zero_tensor
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    G = float(np.linalg.norm(ref.ravel()))
    assert G > 0, (what, "the reference frame gradient is zero")
    worst = 0.0
    parts = [(t, got[:, t], ref[:, t]) for t in range(ref.shape[1])] + [("tied", got.sum(1) if tied is None else np.asarray(tied, np.float64), ref.sum(1))]
    for t, a, r in parts:
        name = "frame gradient %s" % ("t=%d" % t if t != "tied" else t)
        if not r.any():
            assert t in zero, "%s %s: the reference is exactly zero and the step is not declared so: nothing is compared" % (what, name)
            check_zero_tensor(name, a, G, str(what))
            continue
        worst = max(worst, *check_tensor(name, a, r, G, what=str(what)))
    return worst


@functools.lru_cache(maxsize=None)
def case_inputs(w, h, ch, B, T):
    """frames and both weight sets of one shape, made once (read-only by convention)"""
    from tests.train_support import _drifting, _weight_sets
    return _drifting(w + len(ch) + B, B, T, ch[0], h, w), dict(_weight_sets(list(ch), w, h))
