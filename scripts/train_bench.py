"""Time PredNet training steps (train.PredNetTrainer: gradient + Adam) at 160x120 colour, channels [3, 48, 96, 192], batch 16,
10 frames, then -- in a separate process under its own time limit -- torch-ROCm autograd of the same network and loss
(F.conv2d, float32) on the same GPU.  Between the two: a step whose last 5 steps are self-fed (float and requantised feedback) and
the tape-free evaluate of that call.  Prints one JSON line per side and writes profiles/train_bench.json.

    python scripts/train_bench.py [--steps 5] [--warmup 2] [--side trainer|torch|both] [--objective mse|l0|lall]
    python scripts/train_bench.py --frame-grads [--steps 5] [--warmup 2]
    python scripts/train_bench.py --flow-cost [--steps 5] [--warmup 2] [--flow-reference constant|moving] [--flow-pairing frame|prediction]
        [--flow-score [--flow-score-structure circles|bands|free] [--flow-max-norm M]]
    python scripts/train_bench.py [--clip-norm X] [--weight-decay X] [--skip-nonfinite] [--micro-batches K] [--side trainer]
    python scripts/train_bench.py --optim-cost [--clip-norm X] [--weight-decay X] [--skip-nonfinite] [--micro-batches K]
    python scripts/train_bench.py --data textures [--texture-layers 1|2] [--steps 5] [--warmup 2]
    python scripts/train_bench.py --flow-cost --data textures --flow-target truth [--flow-pairing prediction] [--flow-levels 3 --flow-iters 3]

--objective times the trainer step under the error-unit objective instead (L_0, or L_all with the upper layers at 0.1); the torch
side is always the squared error.  --frame-grads times that leg alone: one loss_grad call (no Adam) without frame gradients, with
per-frame and with tied ones, every output left on the device; one JSON line each.  --objective flow is the flow objective (r = 7,
energy, the last two terms weighted); --flow-cost times one loss_grad call (no Adam) under "mse" and under "flow" with the same step
weights, alternated round by round in one process, and prints the ms per call of each with the spread over the rounds.
--flow-reference moving gives the FlowObjective the moving reference; --flow-cost then adds two legs, the "flow" call with tied frame
gradients (left on the device) under the constant and under the moving reference: their difference is what the mode costs.
--flow-pairing prediction makes the flow objective a PredictionFlow (term s from prediction s - 1 to prediction s); --flow-cost then adds
one leg, "flow_prediction", beside "mse" and the frame-pairing "flow": their difference over the two computed terms is what the pairing costs.
--flow-score gives the flow objective a train.FlowScore (the Circles score of the dense field); --flow-cost then adds one leg, "flow_score",
under the pairing and reference asked for, beside the energy-mode legs: their difference over the two computed terms is what the mode costs.
--clip-norm, --weight-decay, --skip-nonfinite give the timed trainer those optimiser controls ("Optimiser controls");
--micro-batches K times step(micro_batches=K) of the same 16 sequences on a handle of batch 16 / K.  --optim-cost times three trainers,
alternated round by round in one process: neutral controls, the controls given (none given: clip_norm at half the first gradient's norm
and weight_decay 0.01) and micro-batches (K, at least 2); one JSON line each with the spread over the rounds.
--data textures (the default, rings, is every run above) times the device frame source train.MovingTextures at this shape: one
batch(k, 16) with one and with two layers (its host part, describe, also alone), the host drifting() call of examples/train_prednet.py
it replaces, and the trainer step fed by batch() of --texture-layers; one JSON line each.
--flow-target truth (with --data textures) reads the frames from train.MovingTextures and makes their exact flow the target of the flow objective
(forward_backward(flow_target=)); --flow-cost then times the "flow" call of the pairing asked for without and with the target
("flow_target"; under a real solve also "flow_iter_target"), alternated like the other legs; without --flow-cost the timed step trains on it.
--frame-weight MU (with --objective flow or --flow-cost) is the joint objective, forward_backward(frame_weight=): --flow-cost then adds the
"flow" call with the frame term ("flow_joint"; with --flow-target truth also "flow_target_joint").  --flow-valid visible (with --data textures
--flow-target truth) passes the video's validity planes, forward_backward(flow_valid=): --flow-cost then adds "flow_target_valid".
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.flow_args import add_flow_arguments, add_flow_joint_arguments, add_flow_target_argument, check_flow_joint, check_flow_target, members_of, score_of  # noqa: E402

W, H, CH, B, T = 160, 120, [3, 48, 96, 192], 16, 10
GATES = ("i", "f", "c", "o")


def conv_flops_per_sample_step(ch, w, h):
    """multiply-adds x 2 of the forward 3x3 convolutions of one sample-step; dgrad and wgrad each repeat them"""
    f, L = 0, len(ch)
    for l, C in enumerate(ch):
        hw = (h >> l) * (w >> l)
        if l > 0:
            f += 2 * C * 2 * ch[l - 1] * 9 * hw * 4
        f += 2 * 4 * C * (2 * C + (ch[l + 1] if l < L - 1 else 0) + C) * 9 * hw
        f += 2 * C * C * 9 * hw
    return f


def frames(seed, n, T, c, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h + 2 * T, 0:w + 2 * T].astype(np.float64)
    out = np.zeros((n, T, c, h, w), np.uint8)
    for i in range(n):
        tex = sum(np.sin(rng.uniform(0.05, 0.3) * yy + rng.uniform(0.05, 0.3) * xx + rng.uniform(0, 6.3)) for _ in range(3))
        tex = np.clip(128 + 40 * tex, 0, 255)
        for t in range(T):
            out[i, t] = tex[None, T + t:T + t + h, T:T + w].astype(np.uint8).repeat(c, 0)
    return out


FLOW_WEIGHTS = [0.0] * (T - 3) + [1.0, 1.0]   # two weighted terms, as a refinement call has them


def objective_args(name, reference="constant", pairing="frame", score=None, members=None, levels=1, iters=1):
    if name == "flow":
        from evolutionary_illusion_generator_amd.train import make_flow
        return dict(objective="flow", flow=make_flow(pairing, radius=7, eps=1e-2, reference=reference, score=score, members=members, levels=levels, iters=iters),
                    step_weights=FLOW_WEIGHTS)
    return {"mse": {}, "l0": dict(objective="error"), "lall": dict(objective="error", layer_weights=[1.0] + [0.1] * (len(CH) - 1))}[name]


def texture_frames():
    """(frames uint8 [B, T, C, H, W], their exact flow float64 [B, T - 1, 2, H, W]) of train.MovingTextures, on the device"""
    from evolutionary_illusion_generator_amd.train import MovingTextures
    with MovingTextures(W, H, CH[0], T) as src:
        return src.batch(0, B, flow=True)[:2]


def texture_valid():
    """the validity planes uint8 [B, T - 1, H, W] of `texture_frames`' video, on the device"""
    from evolutionary_illusion_generator_amd.train import MovingTextures
    with MovingTextures(W, H, CH[0], T) as src:
        return src.batch(0, B, flow=True, valid=True)[3]


def run_flow_cost(steps, warmup, rounds=6, reference="constant", pairing="frame", score=None, members=None, levels=1, iters=1, target=False, frame_weight=None,
                  valid=False):
    """ms per forward_backward call under "mse" and under "flow" (r = 7, the same two weighted terms), alternated round by round; with
    the moving reference also per "flow" call with tied frame gradients, under either reference; with a real solve (levels, iters) also per
    "flow" call of the same settings whose gradient runs through that solve ("flow_iter")"""
    import ctypes
    import torch
    from evolutionary_illusion_generator_amd import weights
    from evolutionary_illusion_generator_amd.train import PredNetTrainer
    d = torch.from_numpy(frames(0, B, T, CH[0], H, W)).cuda()
    calls = {"mse": dict(step_weights=FLOW_WEIGHTS), "flow": objective_args("flow", reference)}
    if reference == "moving":
        calls["flow_tied_constant"] = dict(objective_args("flow"), frame_grads="tied")
        calls["flow_tied_moving"] = dict(objective_args("flow", "moving"), frame_grads="tied")
    if pairing == "prediction":
        calls["flow_prediction"] = objective_args("flow", pairing="prediction")
    if score is not None:
        calls["flow_score"] = objective_args("flow", reference, pairing, score)
    if members is not None:
        calls["flow_score_corners"] = objective_args("flow", reference, pairing, score, members)
    if (levels, iters) != (1, 1):
        calls["flow_iter"] = objective_args("flow", reference, pairing, score, members, levels, iters)
    if target:
        # the frames of the device source and their exact flow: the call of the pairing asked for without and with the target
        d, truth = texture_frames()
        calls = {"mse": calls["mse"], "flow": objective_args("flow", reference, pairing)}
        calls["flow_target"] = dict(calls["flow"], flow_target=truth)
        if (levels, iters) != (1, 1):
            calls["flow_iter"] = objective_args("flow", reference, pairing, levels=levels, iters=iters)
            calls["flow_iter_target"] = dict(calls["flow_iter"], flow_target=truth)
        if valid:
            calls["flow_target_valid"] = dict(calls["flow_target"], flow_valid=texture_valid())
    if frame_weight is not None:
        # the joint objective: the call of the pairing asked for with the frame term beside it
        calls["flow_joint"] = dict(calls["flow_prediction" if pairing == "prediction" and not target else "flow"], frame_weight=frame_weight)
        if target:
            calls["flow_target_joint"] = dict(calls["flow_target"], frame_weight=frame_weight)
    ms = {k: [] for k in calls}
    loss = {}
    with PredNetTrainer(weights.synthetic_prednet_weights(CH, W, H, seed=0), CH, W, H, B, T) as tr:
        def run(kw):
            if "frame_grads" not in kw:
                return tr.forward_backward(d, **kw)
            # the tied gradient stays on the device, as refine_stills leaves it
            kw = dict(kw)
            return tr._loss_grad(d, B, T, T, ctypes.c_int64(T * CH[0] * H * W), True, False, None, False, kw.pop("step_weights"), kw.pop("objective", "mse"), None,
                                 False, kw.pop("frame_grads", None), flow=kw.pop("flow", None))[0]

        for k, kw in calls.items():
            for _ in range(warmup):
                run(kw)
        for _ in range(rounds):
            for k, kw in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    loss[k] = run(kw)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return [dict(side="loss_grad_" + k, call_ms=float(np.median(v)), call_ms_min=min(v), call_ms_max=max(v), rounds=rounds, loss=loss[k]) for k, v in ms.items()]


def run_optim_cost(steps, warmup, rounds=6, clip_norm=None, weight_decay=0.0, skip_nonfinite=False, micro_batches=2):
    """ms per step() of three trainers on the same weights and frames, alternated round by round in one process: "plain" (neutral
    controls: the plain Adam entry), "controls" (the controls given; none given: clip_norm = half the first gradient's norm and
    weight_decay 0.01) and "micro" (a handle of batch B / micro_batches, step(micro_batches=...): the same logical batch)"""
    import torch
    from evolutionary_illusion_generator_amd import weights
    from evolutionary_illusion_generator_amd.train import PredNetTrainer, check_optim, optim_is_neutral
    d = torch.from_numpy(frames(0, B, T, CH[0], H, W)).cuda()
    wts = weights.synthetic_prednet_weights(CH, W, H, seed=0)
    optim = check_optim(clip_norm, weight_decay, skip_nonfinite)
    legs = {"plain": (PredNetTrainer(wts, CH, W, H, B, T), {}), "controls": (PredNetTrainer(wts, CH, W, H, B, T), {}),
            "micro": (PredNetTrainer(wts, CH, W, H, B // micro_batches, T), dict(micro_batches=micro_batches))}
    tr = legs["controls"][0]
    if optim_is_neutral(*optim):
        tr.forward_backward(d)
        optim = (0.5 * tr.grad_norms()[0], 0.01, False)
    tr.clip_norm, tr.weight_decay, tr.skip_nonfinite = optim
    ms, loss = {k: [] for k in legs}, {}
    for k, (t, kw) in legs.items():
        for _ in range(warmup):
            t.step(d, **kw)
    for _ in range(rounds):
        for k, (t, kw) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss[k] = t.step(d, **kw)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    out = [dict(side="step_" + k, step_ms=float(np.median(v)), step_ms_min=min(v), step_ms_max=max(v), rounds=rounds, loss=loss[k], batch=legs[k][0].batch,
                last_update=legs[k][0].last_update, **(dict(zip(("clip_norm", "weight_decay", "skip_nonfinite"), optim)) if k == "controls" else {})) for k, v in ms.items()]
    for t, _ in legs.values():
        t.close()
    return out


def run_data(steps, warmup, layers=1, rounds=6):
    """ms per MovingTextures.batch(k, B) with one and two layers, per describe(k, B) alone, per host drifting() call, and per trainer
    step on batch() of `layers`; every leg a median over the rounds with its spread"""
    import torch
    from evolutionary_illusion_generator_amd import weights
    from evolutionary_illusion_generator_amd.train import MovingTextures, PredNetTrainer
    from examples.train_prednet import drifting
    src = {L: MovingTextures(W, H, CH[0], T, layers=L) for L in (1, 2)}
    tr = PredNetTrainer(weights.synthetic_prednet_weights(CH, W, H, seed=0), CH, W, H, B, T)
    count = [0]

    def k():
        count[0] += 1
        return count[0]
    legs = {"batch_1_layer": lambda: src[1].batch(k(), B), "batch_2_layers": lambda: src[2].batch(k(), B), "describe_1_layer": lambda: src[1].describe(k(), B),
            "describe_2_layers": lambda: src[2].describe(k(), B), "drifting_host": lambda: drifting(k(), B, T, CH[0], H, W),
            "step_on_batch": lambda: tr.step(src[layers].batch(k(), B)), "step_alone": None}
    still = src[layers].batch(0, B)
    legs["step_alone"] = lambda: tr.step(still)
    ms = {name: [] for name in legs}
    for call in legs.values():
        for _ in range(warmup):
            call()
    for _ in range(rounds):
        for name, call in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    tr.close()
    for s in src.values():
        s.close()
    return [dict(side=name, call_ms=float(np.median(v)), call_ms_min=min(v), call_ms_max=max(v), rounds=rounds, **(dict(layers=layers) if name.startswith("step") else {}))
            for name, v in ms.items()]


def run_trainer(steps, warmup, objective="mse", reference="constant", pairing="frame", score=None, members=None, optim=(None, 0.0, False), micro_batches=1, levels=1,
                iters=1, target=False, frame_weight=None, valid=False):
    import torch
    from evolutionary_illusion_generator_amd import weights
    from evolutionary_illusion_generator_amd.train import PredNetTrainer
    d = torch.from_numpy(frames(0, B, T, CH[0], H, W)).cuda()
    kw = objective_args(objective, reference, pairing, score, members, levels, iters) if objective == "flow" else objective_args(objective)
    # the logical batch stays B: with micro-batches the handle, and so the tape, is B / micro_batches
    tr = PredNetTrainer(weights.synthetic_prednet_weights(CH, W, H, seed=0), CH, W, H, B // micro_batches, T, clip_norm=optim[0], weight_decay=optim[1],
                        skip_nonfinite=optim[2])
    kw = dict(kw, micro_batches=micro_batches)
    if target:
        d, truth = texture_frames()
        kw["flow_target"] = truth
        if valid:
            kw["flow_valid"] = texture_valid()
    if frame_weight is not None:
        kw["frame_weight"] = frame_weight
    for _ in range(warmup):
        tr.step(d, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = tr.step(d, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    res = dict(side="trainer", objective=objective, step_ms=ms, sample_steps_per_s=B * T / ms * 1e3, loss=loss, tape_bytes=tr.tape_bytes,
               tape_bytes_per_sample_step=tr.tape_bytes / (tr.batch * T), conv_flops_per_step=3 * conv_flops_per_sample_step(CH, W, H) * B * T)
    if optim != (None, 0.0, False) or micro_batches != 1:
        res.update(clip_norm=optim[0], weight_decay=optim[1], skip_nonfinite=optim[2], micro_batches=micro_batches, last_update=tr.last_update)
    tr.close()
    return res


def run_ext(steps, warmup, n_self=5):
    """a step whose last n_self steps are self-fed (float and requantised feedback), and the tape-free evaluate of the same call"""
    import torch
    from evolutionary_illusion_generator_amd import weights
    from evolutionary_illusion_generator_amd.train import PredNetTrainer
    d = torch.from_numpy(frames(0, B, T, CH[0], H, W)).cuda()
    out = []
    with PredNetTrainer(weights.synthetic_prednet_weights(CH, W, H, seed=0), CH, W, H, B, T) as tr:
        calls = [("trainer_self_fed", lambda: tr.step(d, n_fed=T - n_self)), ("trainer_self_fed_requant", lambda: tr.step(d, n_fed=T - n_self, requant=True)),
                 ("evaluate", lambda: float(tr.evaluate(d, n_fed=T - n_self).mean()))]
        for side, call in calls:
            for _ in range(warmup):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = call()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / steps
            out.append(dict(side=side, n_fed=T - n_self, step_ms=ms, sample_steps_per_s=B * T / ms * 1e3, loss=loss))
    return out


def run_frame_grads(steps, warmup):
    """ms per eigen_trainer_loss_grad_frames call with d_frame_grad NULL (the call eigen_trainer_loss_grad_obj is), with a per-frame
    buffer and with a tied one"""
    import ctypes
    import torch
    from evolutionary_illusion_generator_amd import weights
    from evolutionary_illusion_generator_amd.train import PredNetTrainer
    d = torch.from_numpy(frames(0, B, T, CH[0], H, W)).cuda()
    per = CH[0] * H * W
    out = []
    with PredNetTrainer(weights.synthetic_prednet_weights(CH, W, H, seed=0), CH, W, H, B, T) as tr:
        for side, shape, g_b, g_t in (("loss_grad", None, 0, 0), ("loss_grad_frames", (B, T, per), T * per, per), ("loss_grad_tied", (B, per), per, 0)):
            buf = None if shape is None else torch.zeros(shape, dtype=torch.float32, device="cuda")
            loss = ctypes.c_double()

            def call():
                rc = tr.lib.eigen_trainer_loss_grad_frames(tr._h, ctypes.c_void_p(d.data_ptr()), T * per, B, T, T, 0, 1, None, 0, None, ctypes.byref(loss), None, None,
                                                           None if buf is None else ctypes.c_void_p(buf.data_ptr()), g_b, g_t, None)
                assert rc == 0, rc

            for _ in range(warmup):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / steps
            out.append(dict(side=side, call_ms=ms, loss=loss.value, grad_norm=None if buf is None else float(buf.double().norm())))
    return out


def run_torch(steps, warmup):
    import torch
    import torch.nn.functional as F
    from evolutionary_illusion_generator_amd import weights
    wts = weights.synthetic_prednet_weights(CH, W, H, seed=0)
    p = {k: torch.tensor(v, device="cuda", requires_grad=True) for k, v in wts.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    x = torch.from_numpy(frames(0, B, T, CH[0], H, W)).cuda().float() / 255.0
    L = len(CH)

    def loss_fn():
        z = lambda l: torch.zeros(B, CH[l], H >> l, W >> l, device="cuda")
        hs, cs, Ps = [z(l) for l in range(L)], [z(l) for l in range(L)], [z(l) for l in range(L)]
        loss = 0.0
        for t in range(T):
            E = [torch.cat((F.relu(x[:, t] - Ps[0]), F.relu(Ps[0] - x[:, t])), 1)]
            for l in range(1, L):
                A = F.max_pool2d(F.relu(F.conv2d(E[l - 1], p["ConvA%d/W" % l], p["ConvA%d/b" % l], padding=1)), 2, 2)
                E.append(torch.cat((F.relu(A - Ps[l]), F.relu(Ps[l] - A)), 1))
            for l in reversed(range(L)):
                st = lambda s: torch.cat([p["ConvLSTM%d/%s/W" % (l, s % g)] for g in GATES], 0)
                zz = F.conv2d(E[l], st("x_%s0"), padding=1) + F.conv2d(hs[l], st("h_%s"), torch.cat([p["ConvLSTM%d/h_%s/b" % (l, g)] for g in GATES]), padding=1)
                if l < L - 1:
                    zz = zz + F.conv2d(F.interpolate(hs[l + 1], scale_factor=2, mode="nearest"), st("x_%s1"), padding=1)
                zi, zf, zc, zo = torch.chunk(zz, 4, 1)
                c = cs[l]
                i = torch.sigmoid(zi + p["ConvLSTM%d/c_i/W" % l] * c)
                f = torch.sigmoid(zf + p["ConvLSTM%d/c_f/W" % l] * c)
                o = torch.sigmoid(zo + p["ConvLSTM%d/c_o/W" % l] * c)
                cs[l] = torch.tanh(zc) * i + f * c
                hs[l] = o * torch.tanh(cs[l])
                v = F.conv2d(hs[l], p["ConvP%d/W" % l], p["ConvP%d/b" % l], padding=1)
                Ps[l] = v.clamp(0, 1) if l == 0 else F.relu(v)
            if t < T - 1:
                loss = loss + ((Ps[0] - x[:, t + 1]) ** 2).mean()
        return loss / (T - 1)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn()
        loss.backward()
        opt.step()
        return float(loss)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(side="torch", step_ms=ms, sample_steps_per_s=B * T / ms * 1e3, loss=loss, max_memory_allocated=torch.cuda.max_memory_allocated())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--side", default="both", choices=["trainer", "torch", "both"])
    ap.add_argument("--objective", default="mse", choices=["mse", "l0", "lall", "flow"], help="the trainer side's objective")
    ap.add_argument("--flow-cost", action="store_true", help="time one loss_grad call under mse and under flow, alternated, and exit")
    add_flow_arguments(ap, ("reference", "pairing", "score", "score-structure", "max-norm", "members", "corner-quality", "corner-distance", "levels", "iters"), **{"score-structure": dict(choices=["circles", "bands", "free"])}, reference=dict(help="the flow objective's reference frame: a constant of the graph, or part of it"),
                       pairing=dict(help="the flow objective's pairing: prediction s against frame s + 1, or against prediction s - 1 (train.PredictionFlow)"))
    add_flow_target_argument(ap)
    add_flow_joint_arguments(ap)
    ap.add_argument("--frame-grads", action="store_true", help="time one loss_grad call without, with per-frame and with tied frame gradients, and exit")
    ap.add_argument("--clip-norm", type=float, default=None, help="the trainer's clip_norm (default: no clipping)")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="the trainer's weight_decay")
    ap.add_argument("--skip-nonfinite", action="store_true", help="the trainer's skip_nonfinite")
    ap.add_argument("--micro-batches", type=int, default=1, help="step(micro_batches=K) on a handle of batch 16 / K")
    ap.add_argument("--optim-cost", action="store_true", help="time step() plain, under the controls and in micro-batches, alternated, and exit")
    ap.add_argument("--data", default="rings", choices=["rings", "textures"], help="textures: time the device frame source train.MovingTextures and the step it feeds, and exit")
    ap.add_argument("--texture-layers", type=int, default=1, choices=[1, 2], help="--data textures: the layers of the batches the timed step reads")
    ap.add_argument("--torch-timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_bench.json"))
    a = ap.parse_args()
    check_flow_target(ap, a)
    target = a.flow_target == "truth"
    if target and not a.flow_cost and a.objective != "flow":
        ap.error("--flow-target truth is a mode of --objective flow (or of --flow-cost)")
    if target and (a.flow_score or a.flow_members != "all"):
        ap.error("--flow-target truth takes no --flow-score and no --flow-members")
    if a.flow_cost and a.frame_weight is not None:
        a.objective = "flow"        # --flow-cost times the flow calls whatever --objective says
    check_flow_joint(ap, a)
    if a.flow_pairing == "prediction" and a.flow_reference == "moving":
        ap.error("--flow-pairing prediction has no frame as a reference: it does not take --flow-reference moving")
    score = score_of(a)
    try:
        members = members_of(a)
    except ValueError as e:
        ap.error(str(e))
    if a.side == "torch":
        print(json.dumps(run_torch(a.steps, a.warmup)))
        return
    if a.data == "textures" and not target:
        for r in run_data(a.steps, a.warmup, a.texture_layers):
            print(json.dumps(r), flush=True)
        return
    if a.frame_grads:
        for r in run_frame_grads(a.steps, a.warmup):
            print(json.dumps(r), flush=True)
        return
    if a.flow_cost:
        for r in run_flow_cost(a.steps, a.warmup, reference=a.flow_reference, pairing=a.flow_pairing, score=score, members=members, levels=a.flow_levels, iters=a.flow_iters,
                               target=target, frame_weight=a.frame_weight, valid=a.flow_valid == "visible"):
            print(json.dumps(r), flush=True)
        return
    from evolutionary_illusion_generator_amd.train import check_micro_batches, check_optim
    try:
        optim = check_optim(a.clip_norm, a.weight_decay, a.skip_nonfinite)
        check_micro_batches(B, a.micro_batches, B)
    except ValueError as e:
        ap.error(str(e))
    if a.optim_cost:
        for r in run_optim_cost(a.steps, a.warmup, clip_norm=optim[0], weight_decay=optim[1], skip_nonfinite=optim[2], micro_batches=max(a.micro_batches, 2)):
            print(json.dumps(r), flush=True)
        return
    res = [run_trainer(a.steps, a.warmup, a.objective, a.flow_reference, a.flow_pairing, score, members, optim, a.micro_batches, a.flow_levels, a.flow_iters, target, a.frame_weight,
                       a.flow_valid == "visible")]
    print(json.dumps(res[0]), flush=True)
    ext = run_ext(a.steps, a.warmup)
    for r in ext:
        print(json.dumps(r), flush=True)
    if a.side == "both":
        # torch in a fresh process of its own: its allocator and MIOpen caches do not share the trainer's process
        cmd = ["timeout", "-k", "10", str(a.torch_timeout), sys.executable, os.path.abspath(__file__), "--side", "torch",
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            res.append(dict(side="torch", error=p.returncode))
        else:
            res.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(res[1]))
    res += ext
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(shape=dict(w=W, h=H, channels=CH, batch=B, steps=T), results=res), f, indent=1)
    sys.exit(0 if all("error" not in r for r in res) else 1)


if __name__ == "__main__":
    main()
