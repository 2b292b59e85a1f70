#!/usr/bin/env python3
"""Refine images by gradient ascent through PredNet, then score them with the real fitness.

The fitness scores the Lucas-Kanade flow between a still and PredNet's extended prediction of it, which is not differentiable.
`train.refine_stills` climbs a differentiable stand-in, how far the extended prediction leaves the still, with the frame
gradients of the trainer.  This script takes a seeded CPPN population rendered by the engine (or one PNG), refines the best k
images inside the structure (its background, where the grid is -1, is kept) and prints the stand-in loss and the fitness of
every image before and after.  Whether the fitness follows the stand-in is an observation to make, not a property.

    python examples/refine_illusion.py [-m model.npz] [--size small|N] [-s 1] [-c 3] [--pop 16] [-k 4] [--iters 10] [--step 2]
    python examples/refine_illusion.py --png image.png -o refined
    python examples/refine_illusion.py --objective flow --flow-direction tangent [--flow-radius 7] [--flow-eps 1e-2] [--flow-reference constant|moving]
        [--flow-pairing frame|prediction]   (prediction: the flow between consecutive predictions, the pairing of the fitness printed here)
        [--flow-score --flow-members corners [--flow-corner-quality Q] [--flow-corner-distance D]]   (the members of the score are the corners the fitness itself
        would pick on every term's reference: train.CornerMembers)
        [--flow-score [--flow-score-structure circles|bands|free|auto] [--flow-max-norm M]]   (climb the fitness's own score of that structure on the
        dense field: train.FlowScore, BandsScore or FreeScore; auto follows --structure; no --flow-direction)
        (climb the displacement a dense Lucas-Kanade solve finds between the still and the prediction, inside the structure)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from evolutionary_illusion_generator_amd import fitness, synth, train
from evolutionary_illusion_generator_amd.engine import PAIR_POPULATION
from examples.flow_args import add_flow_arguments, flow_of


def score(images, model, structure, w, h, channels):
    """(fitness [n], number of flow vectors [n]) of uint8 [n, C, H, W] images, as the population is scored"""
    eng = fitness.get_engine(model, w, h, channels, max_batch=len(images))
    fit, vecs = eng.eval_images(torch.from_numpy(np.ascontiguousarray(images)).cuda(), len(images), structure, pairing=PAIR_POPULATION)
    return fit, np.array([len(v) for v in vecs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", "-m", default="synthetic", help="chainer npz weights, or synthetic[:seed]")
    ap.add_argument("--structure", "-s", type=int, default=1, help="0 Bands, 1 Circles, 2 Free, 3 CirclesFree")
    ap.add_argument("--size", "-wh", default="small", help="small (160x120) or N for NxN")
    ap.add_argument("--color_space", "-c", type=int, default=3)
    ap.add_argument("--channels", "-ch", default=None, help="default: C,48,96,192")
    ap.add_argument("--pop", type=int, default=16, help="size of the seeded CPPN population")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--top", "-k", type=int, default=4, help="how many of the best images are refined")
    ap.add_argument("--png", default=None, help="refine this image instead of a population")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", type=float, default=2.0, help="largest move of a byte per iteration")
    ap.add_argument("--objective", default="mse", choices=["mse", "error", "flow"])
    add_flow_arguments(ap)
    ap.add_argument("--n_repeat", type=int, default=20)
    ap.add_argument("--n_ext", type=int, default=2)
    ap.add_argument("--output_dir", "-o", default=None, help="write before_<i>.png / after_<i>.png here")
    a = ap.parse_args()
    w, h = (160, 120) if a.size == "small" else (int(a.size), int(a.size))
    c_dim = a.color_space
    channels = [int(c) for c in a.channels.split(",")] if a.channels else [c_dim, 48, 96, 192]
    if a.png:
        images = fitness._read_image_chw(a.png, c_dim, w, h)[None]
    else:
        config = synth.make_config(2, c_dim)
        genomes = [g for _, g in synth.make_population(a.pop, config, seed=a.seed)]
        images = fitness.render_images(a.structure, genomes, a.model, config, w, h, channels, c_dim=c_dim)
    fit, _ = score(images, a.model, a.structure, w, h, channels)
    best = np.argsort(-fit, kind="stable")[:a.top]
    stills = np.ascontiguousarray(images[best])
    mask = (fitness.leaf_planes(a.structure, w, h)[0] != -1).astype(np.uint8)   # 0 on the structure's background
    with train.PredNetTrainer(a.model, channels, w, h, len(stills), a.n_repeat + a.n_ext) as tr:
        refined, history = train.refine_stills(tr, stills, n_repeat=a.n_repeat, n_ext=a.n_ext, iters=a.iters, step=a.step, objective=a.objective, mask=mask,
                                                flow=flow_of(a, w, h, mask))
    fit0, n0 = score(stills, a.model, a.structure, w, h, channels)
    fit1, n1 = score(refined, a.model, a.structure, w, h, channels)
    print("stand-in loss (mean over the %d images) per iteration: %s" % (len(stills), " ".join("%.6e" % v for v in history)))
    print("free pixels: %d of %d; bytes changed: %d, largest move %d" % (int(mask.sum()), mask.size, int((refined != stills).sum()),
                                                                         int(np.abs(refined.astype(np.int32) - stills).max())))
    for i, b in enumerate(best):
        print("image %d: fitness %.6f -> %.6f, flow vectors %d -> %d" % (b, fit0[i], fit1[i], n0[i], n1[i]))
    print("mean fitness %.6f -> %.6f" % (fit0.mean(), fit1.mean()))
    if a.output_dir:
        from PIL import Image
        os.makedirs(a.output_dir, exist_ok=True)
        to_pil = lambda img: Image.fromarray(img.transpose(1, 2, 0) if c_dim == 3 else img[0], "RGB" if c_dim == 3 else "L")
        for i, b in enumerate(best):
            to_pil(stills[i]).save(os.path.join(a.output_dir, "before_%d.png" % b))
            to_pil(refined[i]).save(os.path.join(a.output_dir, "after_%d.png" % b))


if __name__ == "__main__":
    main()
