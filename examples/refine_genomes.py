#!/usr/bin/env python3
"""Refine genomes by gradient ascent through PredNet and the CPPN render, then score them with the real fitness.

`train.refine_stills` climbs its stand-in loss in pixel space and returns bytes; `train.refine_genomes` climbs the same loss by the
connection weights, biases and responses of the genomes themselves (the gradient passes through the CPPN render, straight through its
uint8 quantisation), so what comes back is still a genome: it can go back into the population, be mutated and crossed, and be
rendered at any size.  This script takes a seeded CPPN population, refines the best k genomes and prints the stand-in loss and the
fitness of each before and after.  Whether the fitness follows the stand-in is an observation to make, not a property.

    python examples/refine_genomes.py [-m model.npz] [--size small|N] [-s 1] [-c 3] [--pop 16] [-k 4] [--iters 10] [--lr 0.02]
    python examples/refine_genomes.py --objective flow --flow-direction tangent [--flow-radius 7] [--flow-eps 1e-2] [--flow-reference constant|moving]
        [--flow-pairing frame|prediction]   (prediction: the flow between consecutive predictions, the pairing of the fitness printed here)
        [--flow-score --flow-members corners [--flow-corner-quality Q] [--flow-corner-distance D]]   (the members of the score are the corners the fitness itself
        would pick on every term's reference: train.CornerMembers)
        [--flow-score [--flow-score-structure circles|bands|free|auto] [--flow-max-norm M]]   (climb the fitness's own score of that structure on the
        dense field: train.FlowScore, BandsScore or FreeScore; auto follows --structure; no --flow-direction)
    python examples/refine_genomes.py -o refined      (PNGs, and best.png / enhanced.png ... of the best refined genome)
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
    ap.add_argument("--top", "-k", type=int, default=4, help="how many of the best genomes are refined")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.02, help="largest move of a parameter per iteration")
    ap.add_argument("--params", default="weight,bias,response", help="which kinds of parameters move")
    ap.add_argument("--objective", default="mse", choices=["mse", "error", "flow"])
    add_flow_arguments(ap)
    ap.add_argument("--n_repeat", type=int, default=20)
    ap.add_argument("--n_ext", type=int, default=2)
    ap.add_argument("--output_dir", "-o", default=None, help="write before_<i>.png / after_<i>.png and the artefacts of the best refined genome here")
    a = ap.parse_args()
    w, h = (160, 120) if a.size == "small" else (int(a.size), int(a.size))
    c_dim = a.color_space
    channels = [int(c) for c in a.channels.split(",")] if a.channels else [c_dim, 48, 96, 192]
    config = synth.make_config(2, c_dim)
    genomes = [g for _, g in synth.make_population(a.pop, config, seed=a.seed)]
    images = fitness.render_images(a.structure, genomes, a.model, config, w, h, channels, c_dim=c_dim)
    fit, _ = score(images, a.model, a.structure, w, h, channels)
    best = np.argsort(-fit, kind="stable")[:a.top]
    chosen, stills = [genomes[b] for b in best], np.ascontiguousarray(images[best])
    with train.PredNetTrainer(a.model, channels, w, h, len(chosen), a.n_repeat + a.n_ext) as tr:
        refined, history, after = train.refine_genomes(tr, chosen, config, a.structure, n_repeat=a.n_repeat, n_ext=a.n_ext, iters=a.iters, lr=a.lr,
                                                       objective=a.objective, params=tuple(a.params.split(",")),
                                                       flow=flow_of(a, w, h, (fitness.leaf_planes(a.structure, w, h)[0] != -1).astype(np.uint8)))
    fit0, n0 = score(stills, a.model, a.structure, w, h, channels)
    fit1, n1 = score(after, a.model, a.structure, w, h, channels)
    print("stand-in loss (mean over the %d genomes) per iteration: %s" % (len(chosen), " ".join("%.6e" % v for v in history)))
    print("bytes changed: %d of %d, largest move %d" % (int((after != stills).sum()), stills.size, int(np.abs(after.astype(np.int32) - stills).max())))
    for i, b in enumerate(best):
        print("genome %d: fitness %.6f -> %.6f, flow vectors %d -> %d" % (genomes[b].key, fit0[i], fit1[i], n0[i], n1[i]))
    print("mean fitness %.6f -> %.6f" % (fit0.mean(), fit1.mean()))
    if a.output_dir:
        from PIL import Image
        os.makedirs(a.output_dir, exist_ok=True)
        to_pil = lambda img: Image.fromarray(img.transpose(1, 2, 0) if c_dim == 3 else img[0], "RGB" if c_dim == 3 else "L")
        for i, b in enumerate(best):
            to_pil(stills[i]).save(os.path.join(a.output_dir, "before_%d.png" % genomes[b].key))
            to_pil(after[i]).save(os.path.join(a.output_dir, "after_%d.png" % genomes[b].key))
        top = int(np.argmax(fit1))   # a genome, not a still: it renders at 800 x 800 like any other (enhanced.png)
        fitness.save_best_artifacts(a.structure, refined[top], a.model, config, w, h, channels, c_dim, a.output_dir, 1)


if __name__ == "__main__":
    main()
