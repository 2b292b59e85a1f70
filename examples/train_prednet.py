#!/usr/bin/env python3
"""Train PredNet on the MI355X (next-frame MSE or PredNet's own error-unit objective, backprop through time, Adam) and use the
result in the fitness path.

    python examples/train_prednet.py -o trained.npz [-i frames_dir] [--size 160x120] [-c 3] [--steps 200] [--seq 10] [--batch 8]
                                     [--data rings|textures [--texture-layers 1|2]] [--loss mse|l0|lall]
                                     [--objective flow [--flow-pairing prediction] [--flow-radius 7] ... [--flow-target truth [--flow-valid visible]]
                                      [--frame-weight MU]]
                                     [--clip-norm X] [--weight-decay X] [--skip-nonfinite] [--micro-batches K]
                                     [--ext-steps 200 --ext-frames 4 [--requant]] [--checkpoint ckpt.npz [--every 50]] [--resume ckpt.npz]

Input: the PNG files of a folder, in name order, centre-cropped to --size, cut into windows of --seq frames; without -i, seeded
drifting patterns (rings moving in a different direction per sequence), or with --data textures moving CPPN textures rendered on
the device (train.MovingTextures: a seeded texture per sequence under its own shift, turn and zoom; --texture-layers 2 puts a
second, disc-shaped texture with a motion of its own in front).  The last window (or a held-out seed) is kept out of
training.  Phase 1 is teacher-forced: every step reads its frame.  --ext-steps adds a second, self-fed fine-tuning phase: the last
--ext-frames steps of every sequence read the network's own prediction (through the emitted byte with --requant), the regime the
fitness path scores; its loss weights only the self-fed predictions.  --checkpoint writes weights, Adam state and step counter as
one npz every --every steps and at the end; --resume continues such a run bit for bit.  --loss picks the objective of both phases:
mse, the squared error of the prediction; l0, the mean of the image layer's error units (Lotter's L_0, an L1 next-frame error);
lall, L_0 plus the error units of the upper layers at weight 0.1 (L_all).  Prints the held-out per-step squared errors and the
mean error units of every layer (tape-free `evaluate`) before and after, writes the weights as a chainer npz (-o), then evaluates one synthetic population's
fitness with them.
--objective flow trains on the dense motion objective of the --flow-* options in place of --loss (train.make_flow; examples/flow_args.py
lists them).  With --data textures --flow-target truth every term is the squared endpoint error of the solved field against the exact flow
of the video (``forward_backward(flow_target=)``): under --flow-pairing prediction "the flow between consecutive predictions shall be the
true flow", on the self-fed steps too.  --flow-valid visible then counts a pixel only where its surface can be seen in the next frame
(``flow_valid=``, the validity planes of ``MovingTextures.batch(valid=True)``), and --frame-weight MU adds MU times the squared error of the
predictions to the flow objective's loss in the same backward pass (``frame_weight=``; the two parts are printed with the loss).  The per-term values of the printed steps are printed with the loss.  With --data textures the
held-out mean squared endpoint error between consecutive predictions (train.flow_epe) is printed before and after, whatever the objective,
over all pixels and over the valid ones.
--clip-norm, --weight-decay and --skip-nonfinite are the trainer's optimiser controls (gradient clipping at a global norm, chainer's weight
decay, leaving out a step whose gradient is not finite); --micro-batches K keeps --batch as the logical batch of a step and runs it as K
chunks on a handle of --batch / K, so the tape is K times smaller.  At the steps whose loss is printed the global gradient norm is printed
too, with the names of the tensors whose gradient is exactly zero.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from evolutionary_illusion_generator_amd import fitness, grids, synth, weights
from evolutionary_illusion_generator_amd.train import MovingTextures, PredictionFlow, PredNetTrainer, check_micro_batches, check_optim, flow_epe
from examples.flow_args import add_flow_arguments, add_flow_joint_arguments, add_flow_target_argument, check_flow_joint, check_flow_target, flow_of


def read_windows(folder, c_dim, w, h, seq):
    names = sorted(f for f in os.listdir(folder) if f.lower().endswith(".png"))
    if len(names) < 2 * seq:
        raise SystemExit("need at least %d PNG files in %s (two windows of --seq frames)" % (2 * seq, folder))
    frames = np.stack([fitness._read_image_chw(os.path.join(folder, f), c_dim, w, h) for f in names])
    return np.stack([frames[i:i + seq] for i in range(0, len(frames) - seq + 1, seq)])


def drifting(seed, n, seq, c_dim, w, h):
    """n sequences of rings drifting by up to 1.5 pixels per frame, each in its own seeded direction."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, seq, c_dim, h, w), np.uint8)
    for i in range(n):
        vx, vy, cx, cy, k = rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 5)
        for t in range(seq):
            v = 127.5 + 127.5 * np.sin(np.hypot(xx - cx - vx * t, yy - cy - vy * t) / k)
            out[i, t] = np.repeat(v[None], c_dim, 0).astype(np.uint8)
    return out


def held_out_epe(tr, frames, truth, radius, eps, n_fed, requant, valid=None):
    """float64 [T - 2]: the mean squared endpoint error of the flow from prediction s - 1 to prediction s against the video's own flow
    from frame s to frame s + 1, for s = 1 .. T - 2 (term 0 has no previous prediction), on the device (train.flow_epe); valid: the
    video's validity planes [n, T - 1, H, W], the mean then runs over every sample's valid pixels"""
    import torch
    pred = torch.from_numpy(tr.evaluate(frames, n_fed=n_fed, requant=requant, pred=True)[1])
    flow = PredictionFlow(radius, eps)
    return np.array([flow_epe(tr, pred[:, s], pred[:, s - 1], flow, truth[:, s], None if valid is None else valid[:, s]) for s in range(1, pred.shape[1] - 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", "-i", default=None, help="folder of PNG frames (default: seeded drifting patterns)")
    ap.add_argument("--output", "-o", default="trained.npz")
    ap.add_argument("--model", "-m", default="synthetic", help="starting weights: chainer npz or synthetic[:seed]")
    ap.add_argument("--size", default="160x120", help="WxH")
    ap.add_argument("--color_space", "-c", type=int, default=3)
    ap.add_argument("--channels", "-ch", default=None, help="PredNet channels (default: c,48,96,192)")
    ap.add_argument("--data", default="rings", choices=["rings", "textures"], help="the seeded source without -i: drifting rings (host) or moving CPPN textures (device)")
    ap.add_argument("--texture-layers", type=int, default=1, choices=[1, 2], help="--data textures: 2 adds a disc with a motion of its own (an occlusion boundary)")
    ap.add_argument("--steps", type=int, default=200, help="Adam steps")
    ap.add_argument("--seq", type=int, default=10, help="frames per sequence")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=1e-3)
    ap.add_argument("--loss", default="mse", choices=["mse", "l0", "lall"], help="objective: squared error, or the error units (L_0 / L_all)")
    ap.add_argument("--objective", default="loss", choices=["loss", "flow"], help="loss: the objective of --loss; flow: the dense motion objective of the --flow-* options")
    add_flow_arguments(ap)
    add_flow_target_argument(ap)
    add_flow_joint_arguments(ap)
    ap.add_argument("--ext-steps", type=int, default=0, help="Adam steps of a second phase whose last --ext-frames steps are self-fed")
    ap.add_argument("--ext-frames", type=int, default=4, help="self-fed steps at the end of every sequence in the second phase")
    ap.add_argument("--requant", action="store_true", help="feed predictions back through the emitted byte (cfg.requant_feedback)")
    ap.add_argument("--checkpoint", default=None, help="write weights + Adam state + step counter here (one npz)")
    ap.add_argument("--every", type=int, default=50, help="checkpoint period in steps")
    ap.add_argument("--resume", default=None, help="continue the run a --checkpoint file holds")
    ap.add_argument("--clip-norm", type=float, default=None, help="scale a step's gradient down to this global L2 norm (default: no clipping)")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="chainer's AdamRule weight_decay_rate")
    ap.add_argument("--skip-nonfinite", action="store_true", help="leave out a step whose gradient norm is not finite")
    ap.add_argument("--micro-batches", type=int, default=1, help="run a step's --batch sequences as K chunks on a handle of --batch / K")
    args = ap.parse_args()
    check_flow_target(ap, args)
    if args.flow_target == "truth" and args.objective != "flow":
        ap.error("--flow-target truth is a mode of --objective flow")
    check_flow_joint(ap, args)
    w, h = (int(v) for v in args.size.lower().split("x"))
    channels = [int(c) for c in args.channels.split(",")] if args.channels else [args.color_space, 48, 96, 192]
    c_dim = channels[0]
    if args.input and args.data != "rings":
        ap.error("--data %s is a source of its own: it does not go with --input" % args.data)
    if args.input:
        windows = read_windows(args.input, c_dim, w, h, args.seq)
        held, train = windows[-1:], windows[:-1]
        batch_of = lambda k: train[np.arange(k * args.batch, (k + 1) * args.batch) % len(train)]
    elif args.data == "textures":
        try:
            source = MovingTextures(w, h, c_dim, args.seq, layers=args.texture_layers)
        except ValueError as e:
            ap.error(str(e))
        held = source.batch(10 ** 6, args.batch)      # uint8 on the device: the trainer reads it where it is
        batch_of = lambda k: source.batch(k, args.batch)
    else:
        held = drifting(10 ** 6, args.batch, args.seq, c_dim, w, h)
        batch_of = lambda k: drifting(k, args.batch, args.seq, c_dim, w, h)

    n_fed = args.seq - args.ext_frames if args.ext_steps else args.seq
    if not 1 <= n_fed <= args.seq or (args.ext_steps and args.seq - n_fed < 1):
        raise SystemExit("--ext-frames must be in [1, --seq - 1]")
    # the self-fed phase weights the predictions made by self-fed steps only (term s: prediction s against frame s + 1)
    ext_w = [0.0] * n_fed + [1.0] * (args.seq - 1 - n_fed)
    total = args.steps + args.ext_steps
    fmt = lambda v: " ".join("%.5f" % x for x in v)
    obj = {"mse": {}, "l0": dict(objective="error"), "lall": dict(objective="error", layer_weights=[1.0] + [0.1] * (len(channels) - 1))}[args.loss]
    try:
        flow = flow_of(args, w, h)
    except ValueError as e:
        ap.error(str(e))
    if flow is not None:
        obj = dict(objective="flow", flow=flow)
        if args.frame_weight is not None:
            obj["frame_weight"] = args.frame_weight
    name = "flow" if flow is not None else args.loss
    truth = args.flow_target == "truth"

    def step_inputs(k):
        """the frames of step k and, under --flow-target truth, their exact flow as the step's target"""
        if not truth:
            return batch_of(k), {}
        if args.flow_valid == "visible":
            frames, fl, _, visible = source.batch(k, args.batch, flow=True, valid=True)
            return frames, dict(flow_target=fl, flow_valid=visible)
        frames, fl, _ = source.batch(k, args.batch, flow=True)
        return frames, dict(flow_target=fl)

    try:
        optim = check_optim(args.clip_norm, args.weight_decay, args.skip_nonfinite)
        chunk = check_micro_batches(args.batch, args.micro_batches, args.batch)
    except ValueError as e:
        ap.error(str(e))
    obj["micro_batches"] = args.micro_batches

    with PredNetTrainer(args.model, channels, w, h, chunk, args.seq, alpha=args.alpha, clip_norm=optim[0], weight_decay=optim[1], skip_nonfinite=optim[2]) as tr:
        first = 0
        if args.resume:
            tr.load_checkpoint(args.resume)    # the checkpoint's optimiser controls replace the command line's, as its hyper-parameters do
            first = tr.state_dict()["adam_t"]
            print("resumed %s at step %d (clip_norm %s, weight_decay %g, skip_nonfinite %s)" % (args.resume, first, tr.clip_norm, tr.weight_decay, tr.skip_nonfinite))
        before, err_before = tr.evaluate(held[:chunk], n_fed=n_fed, requant=args.requant, layer_errors=True)
        print("held-out loss per step (%d fed, %d self-fed) before: %s" % (n_fed, args.seq - n_fed, fmt(before)))
        print("held-out error units per layer (mean over the steps; layer 0 is the L_0 error) before: %s" % fmt(err_before.mean(0)))
        if args.data == "textures" and not args.input:
            held_flow = source.batch(10 ** 6, args.batch, flow=True)[1]
            epe = lambda: held_out_epe(tr, held[:chunk], held_flow[:chunk], args.flow_radius, args.flow_eps, n_fed, args.requant)
            epe_before = epe()
            print("held-out squared endpoint error between consecutive predictions (terms 1 .. %d) before: %s" % (args.seq - 2, fmt(epe_before)))
            held_valid = source.batch(10 ** 6, args.batch, flow=True, valid=True)[3]
            epe_valid = lambda: held_out_epe(tr, held[:chunk], held_flow[:chunk], args.flow_radius, args.flow_eps, n_fed, args.requant, held_valid[:chunk])
            valid_before = epe_valid()
            print("  over the valid pixels (%.1f %% of all) before: %s" % (100 * float(held_valid[:chunk, 1:].float().mean()), fmt(valid_before)))
        for k in range(first, total):
            frames, extra = step_inputs(k)
            if k < args.steps:
                loss = tr.step(frames, **extra, **obj)
            else:
                loss = tr.step(frames, n_fed=n_fed, requant=args.requant, step_weights=ext_w if any(ext_w) else None, **extra, **obj)
            if k % 50 == 0 or k == total - 1 or k == args.steps:
                print("step %4d  %s train loss (%s) %.6f" % (k, "teacher-forced" if k < args.steps else "self-fed      ", name, loss))
                if flow is not None and args.frame_weight is not None:
                    print("           flow part %.6f, squared-error part %.6f (weight %g)%s"
                          % (tr.last_loss_parts + (args.frame_weight, " (last micro-batch)" if args.micro_batches > 1 else "")))
                if flow is not None:     # the terms the library returned (h_terms); with micro-batches those of the step's last chunk
                    print("           flow terms%s: %s" % (" (last micro-batch)" if args.micro_batches > 1 else "", " ".join("%.6f" % v for v in tr.last_flow_terms)))
                # the gradient this step applied (with micro-batches: the accumulated one), before clipping
                norm, per = tr.grad_norms()
                dead = [n for n, v in per.items() if v == 0.0]
                skipped = "  (step left out: the norm is not finite)" if tr.last_update["applied"] == 0 else ""
                print("           gradient norm %.6e%s; %d of %d tensors exactly zero%s" % (norm, skipped, len(dead), len(per), ": " + " ".join(dead) if dead else ""))
            if args.checkpoint and ((k + 1) % args.every == 0 or k == total - 1):
                tr.save_checkpoint(args.checkpoint)
        after, err_after = tr.evaluate(held[:chunk], n_fed=n_fed, requant=args.requant, layer_errors=True)
        if args.data == "textures" and not args.input:
            epe_after = epe()
            print("held-out squared endpoint error between consecutive predictions after:  %s" % fmt(epe_after))
            print("held-out squared endpoint error, mean over the terms: %.6f before, %.6f after (%.1f %% lower)"
                  % (epe_before.mean(), epe_after.mean(), 100 * (1 - epe_after.mean() / epe_before.mean())))
            valid_after = epe_valid()
            print("  over the valid pixels: %.6f before, %.6f after (%.1f %% lower)" % (valid_before.mean(), valid_after.mean(), 100 * (1 - valid_after.mean() / valid_before.mean())))
        trained = tr.weights()
    print("held-out loss per step after:  %s" % fmt(after))
    print("held-out error units per layer after:  %s" % fmt(err_after.mean(0)))
    print("held-out loss, mean over the steps: %.6f before, %.6f after (%.1f %% lower)" % (before.mean(), after.mean(), 100 * (1 - after.mean() / before.mean())))
    if n_fed < args.seq - 1:
        b, a = before[n_fed:].sum(), after[n_fed:].sum()
        print("  self-fed steps alone: %.6f before, %.6f after (%.1f %% lower)" % (b, a, 100 * (1 - a / b)))
    weights.save_chainer_npz(trained, args.output)
    print("weights written to %s" % args.output)

    cfg = synth.make_config(2, c_dim)
    pop = synth.make_population(8, cfg, seed=1)
    fitness.get_fitnesses_neat(int(grids.StructureType.Free), pop, args.output, cfg, w, h, channels, c_dim=c_dim, best_dir=None)
    print("fitness of a synthetic population with the trained weights:", [round(g.fitness, 4) for _, g in pop])


if __name__ == "__main__":
    main()
