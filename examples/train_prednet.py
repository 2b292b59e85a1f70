#!/usr/bin/env python3
"""Train PredNet on the MI355X (next-frame MSE, backprop through time, Adam) and use the result in the fitness path.

    python examples/train_prednet.py -o trained.npz [-i frames_dir] [--size 160x120] [-c 3] [--steps 200] [--seq 10] [--batch 8]

Input: the PNG files of a folder, in name order, centre-cropped to --size, cut into windows of --seq frames; without -i, seeded
drifting patterns (rings moving in a different direction per sequence).  The last window (or a held-out seed) is kept out of
training.  Prints the held-out loss before and after, writes the weights as a chainer npz (-o), then evaluates one synthetic
population's fitness with them.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from evolutionary_illusion_generator_amd import fitness, grids, synth, weights
from evolutionary_illusion_generator_amd.train import PredNetTrainer


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", "-i", default=None, help="folder of PNG frames (default: seeded drifting patterns)")
    ap.add_argument("--output", "-o", default="trained.npz")
    ap.add_argument("--model", "-m", default="synthetic", help="starting weights: chainer npz or synthetic[:seed]")
    ap.add_argument("--size", default="160x120", help="WxH")
    ap.add_argument("--color_space", "-c", type=int, default=3)
    ap.add_argument("--channels", "-ch", default=None, help="PredNet channels (default: c,48,96,192)")
    ap.add_argument("--steps", type=int, default=200, help="Adam steps")
    ap.add_argument("--seq", type=int, default=10, help="frames per sequence")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=1e-3)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    channels = [int(c) for c in args.channels.split(",")] if args.channels else [args.color_space, 48, 96, 192]
    c_dim = channels[0]
    if args.input:
        windows = read_windows(args.input, c_dim, w, h, args.seq)
        held, train = windows[-1:], windows[:-1]
        batch_of = lambda k: train[np.arange(k * args.batch, (k + 1) * args.batch) % len(train)]
    else:
        held = drifting(10 ** 6, args.batch, args.seq, c_dim, w, h)
        batch_of = lambda k: drifting(k, args.batch, args.seq, c_dim, w, h)

    with PredNetTrainer(args.model, channels, w, h, args.batch, args.seq, alpha=args.alpha) as tr:
        before = tr.forward_backward(held)
        for k in range(args.steps):
            loss = tr.step(batch_of(k))
            if k % 50 == 0 or k == args.steps - 1:
                print("step %4d  train loss %.6f" % (k, loss))
        after = tr.forward_backward(held)
        trained = tr.weights()
    print("held-out loss: %.6f before, %.6f after (%.1f %% lower)" % (before, after, 100 * (1 - after / before)))
    weights.save_chainer_npz(trained, args.output)
    print("weights written to %s" % args.output)

    cfg = synth.make_config(2, c_dim)
    pop = synth.make_population(8, cfg, seed=1)
    fitness.get_fitnesses_neat(int(grids.StructureType.Free), pop, args.output, cfg, w, h, channels, c_dim=c_dim, best_dir=None)
    print("fitness of a synthetic population with the trained weights:", [round(g.fitness, 4) for _, g in pop])


if __name__ == "__main__":
    main()
