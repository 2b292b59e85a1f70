"""The float64 reference of PredNet TRAINING -- TEST INFRASTRUCTURE (see oracle/__init__.py): one torch-CPU autograd restatement
of the network, its two objectives and their gradients (DESIGN.md section 13 states the semantics the HIP trainer and this file
both follow).  tests/test_gpu_train*.py compare the trainer against it; tests/test_train_reference_host.py pins it on the CPU."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from . import GATES

# loss: float; grads: {name: float64 array}; pred: P0 [B, T, C, H, W] float64; step_mse: [T - 1]; table: err[s][l], [T - 1, L];
# state: the final (h, c, P), each a list of detached tensors, one per layer
Result = namedtuple("Result", "loss grads pred step_mse table state")


def clamp01(v):
    """clamp(v, 0, 1) whose gradient passes only where 0 < v < 1 (chainer's clipped_relu)"""
    inside = (v > 0) & (v < 1)
    return torch.where(inside, v, v.detach().clamp(0.0, 1.0))


def _error_pair(a, p):
    return torch.cat((F.relu(a - p), F.relu(p - a)), 1)


def run(weights, channels, frames, *, objective="mse", layer_weights=None, n_fed=None, requant=False, step_weights=None, state=None,
        fed=None, dtype=torch.float64):
    """float64 autograd PredNet over frames uint8 [B, T, C, H, W] from `state` (detached (h, c, P), or zeros).

    Steps t < n_fed read frame t (None: all do); steps t >= n_fed are fed the previous prediction -- itself (requant False: part
    of the graph, E_0 = relu(0)) or the constant fed[:, t] (requant True: float32 [B, T, C, H, W], the requantised prediction
    of step t - 1; quantisation passes no gradient).
    step_mse[s] = mean of (P0_s - x_{s+1})^2.  table[s][0] = mean of [relu(x_{s+1} - P0_s), relu(P0_s - x_{s+1})], against the
    TRUE frame on every step; table[s][l > 0] = mean of E_l of step s + 1.
    objective "mse": loss = sum_s w_s step_mse[s] / sum_s w_s; "error": loss = sum_s w_s sum_l lam_l table[s][l] / sum_s w_s,
    with w = step_weights (None: all one) and lam = layer_weights (None: L_0, [1, 0, ...]).  T = 1 has no term: loss 0, zero
    gradients.
    dtype=torch.float32 runs the same statement in float32 (results are still returned as float64 arrays): the yardstick of what
    float32 arithmetic alone costs, which tests/train_support.py `_check_grads` takes its element-wise bound from."""
    if objective not in ("mse", "error"):
        raise ValueError("objective must be 'mse' or 'error', got %r" % (objective,))
    ch, L = list(channels), len(channels)
    p = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in weights.items()}
    x = torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)).to(dtype)
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
        g = torch.autograd.grad(loss, [p[n] for n in names], allow_unused=True)
        loss = float(loss.detach())
    else:
        loss, g = 0.0, [None] * len(names)
    grads = {n: (gg.double().numpy() if gg is not None else np.zeros(p[n].shape)) for n, gg in zip(names, g)}
    table = np.array([[float(e.detach()) for e in row] for row in err]).reshape(T - 1, L)
    step_mse = np.array([float(m.detach()) for m in mses])
    state = tuple([s.detach() for s in ss] for ss in (hs, cs, Ps))
    return Result(loss, grads, torch.stack(preds, 1).detach().double().numpy(), step_mse, table, state)
