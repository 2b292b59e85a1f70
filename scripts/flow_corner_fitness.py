#!/usr/bin/env python3
"""The rows of profiles/flow_score_fitness.txt and profiles/flow_struct_fitness.txt under corner members, and what the membership stage costs.

Every row is the recipe those files state (weights synthetic, UNTRAINED; 160x120 colour, [3, 48, 96, 192]; population 16 of the seed, the
best 4 refined; 20 + 2 frames; steps of 2 bytes inside the structure; radius 7, eps 1e-2; the flow mask = the structure; the structure's
own score with its defaults) with members=train.CornerMembers() (the fitness's own goodFeaturesToTrack settings).  One refine_stills
iteration at a time; before each, one forward_backward call gives the loss, its terms and, from the last weighted term's records, the
members per image; the fitness is the population path's, with the number of flow vectors it tracked.

    python scripts/flow_corner_fitness.py [--rows score,struct] [--timing] > profiles/flow_corner_fitness.txt
    python scripts/flow_corner_fitness.py --rows score --structures 1 --pairings prediction --dense-fitness > profiles/dense_float_refine.txt

--dense-fitness appends to every line the dense fitness of the same stills under the objective's own settings (the structure's score, radius 7, eps 1e-2, the
structure as the mask, CornerMembers()), on the emitted bytes and on the float predictions (fitness.DenseFitness(frames="float"); DESIGN.md section 14,
"Float frames"): whether the quantity that selects follows the loss that refinement climbs.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from evolutionary_illusion_generator_amd import fitness, synth, train
from evolutionary_illusion_generator_amd.engine import PAIR_POPULATION

W, H, C_DIM, CH, N_REPEAT, N_EXT, POP, TOP = 160, 120, 3, [3, 48, 96, 192], 20, 2, 16, 4
NAMES = {0: "Bands", 1: "Circles", 2: "Free", 3: "CirclesFree"}
# (structure, seed, iterations) of the two files' populations; each runs under both pairings and both feedbacks
ROWS = {"score": [(1, 0, 10), (3, 1, 20)], "struct": [(0, 0, 10), (2, 1, 10)]}
MODEL = "synthetic"


def score(images, structure):
    eng = fitness.get_engine(MODEL, W, H, CH, max_batch=len(images))
    fit, vecs = eng.eval_images(torch.from_numpy(np.ascontiguousarray(images)).cuda(), len(images), structure, pairing=PAIR_POPULATION)
    return fit, [len(v) for v in vecs]


def dense_scores(images, structure, mask):
    """(byte, float): the dense fitness of the stills under corner members, on the emitted bytes and on the float predictions"""
    eng = fitness.get_engine(MODEL, W, H, CH, max_batch=len(images))
    d = torch.from_numpy(np.ascontiguousarray(images)).cuda()
    out = []
    for frames in ("byte", "float"):
        dense = fitness.DenseFitness(train.structure_score(structure), radius=7, eps=1e-2, mask=mask, members=train.CornerMembers(), frames=frames)
        out.append(eng.eval_images(d, len(images), structure, pairing=PAIR_POPULATION, dense=dense)[0])
    return out


def stills_of(structure, seed):
    config = synth.make_config(2, C_DIM)
    genomes = [g for _, g in synth.make_population(POP, config, seed=seed)]
    images = fitness.render_images(structure, genomes, MODEL, config, W, H, CH, c_dim=C_DIM)
    fit, _ = score(images, structure)
    best = np.argsort(-fit, kind="stable")[:TOP]
    return np.ascontiguousarray(images[best]), best.tolist()


def flow_of(structure, pairing, mask, members):
    return train.make_flow(pairing, 7, 1e-2, None, mask, reference="moving" if pairing == "frame" else "constant", score=train.structure_score(structure),
                           members=members)


def run_row(structure, seed, iters, pairing, requant, dense_fitness=False):
    stills, best = stills_of(structure, seed)
    mask = (fitness.leaf_planes(structure, W, H)[0] != -1).astype(np.uint8)
    flow = flow_of(structure, pairing, mask, train.CornerMembers())
    T = N_REPEAT + N_EXT
    weights = train._still_weights(None, N_REPEAT, N_EXT, flow)
    last = max(s for s, w in enumerate(weights) if w != 0)
    print("# %s seed %d, %d iterations, --flow-score --flow-score-structure auto --flow-members corners, pairing %s, %s feedback; images %s" % (
        NAMES[structure], seed, iters, "frame + moving reference" if pairing == "frame" else "prediction", "byte" if requant else "float", best), flush=True)
    with train.PredNetTrainer(MODEL, CH, W, H, len(stills), T) as tr:
        img = stills
        for i in range(iters + 1):
            frames = np.ascontiguousarray(np.broadcast_to(img[:, None], (len(img), T) + img.shape[1:]))
            loss, terms = tr.forward_backward(frames, n_fed=N_REPEAT, requant=requant, step_weights=weights, objective="flow", flow=flow, flow_terms=True)
            rec = tr.last_flow_stats[last]
            fit, nvec = score(img, structure)
            print("iter %2d loss %.6e terms %s | members %s | S_b %s | fitness %s mean %.6f | flow vectors %s" % (
                i, loss, " ".join("%.6e" % v for v in terms[N_REPEAT - 1:]), rec[:, 0].astype(int).tolist(), " ".join("%.4f" % v for v in rec[:, 8]),
                " ".join("%.6f" % v for v in fit), float(np.mean(fit)), nvec) + ("" if not dense_fitness else " | dense fitness byte %s mean %.6f | float %s mean %.6f" % tuple(
                    x for f in dense_scores(img, structure, mask) for x in (" ".join("%.6f" % v for v in f), float(np.mean(f))))), flush=True)
            if i < iters:
                img, _ = train.refine_stills(tr, img, n_repeat=N_REPEAT, n_ext=N_EXT, iters=1, step=2.0, requant=requant, objective="flow", mask=mask, flow=flow)


def timing(rounds=3, short=1, long=5):
    """ms of one refine_stills iteration (one loss-and-gradient call and one still step) at 160x120 colour, n = 4, under FlowScore with
    all pixels and with corner members, alternated: (time of `long` iterations - time of `short`) / (long - short), the median of the rounds"""
    stills, _ = stills_of(1, 0)
    mask = (fitness.leaf_planes(1, W, H)[0] != -1).astype(np.uint8)
    ms = {}
    with train.PredNetTrainer(MODEL, CH, W, H, len(stills), N_REPEAT + N_EXT) as tr:
        for pairing in ("frame", "prediction"):
            flows = {"all pixels": flow_of(1, pairing, mask, None), "corner members": flow_of(1, pairing, mask, train.CornerMembers())}

            def run(flow, iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train.refine_stills(tr, stills, n_repeat=N_REPEAT, n_ext=N_EXT, iters=iters, objective="flow", mask=mask, flow=flow)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            for flow in flows.values():
                run(flow, 1)
            for _ in range(rounds):
                for k, flow in flows.items():
                    ms.setdefault((pairing, k), []).append((run(flow, long) - run(flow, short)) / (long - short))
    for (pairing, k), v in ms.items():
        print("# one refine_stills iteration, 160x120 colour, n = 4, FlowScore, pairing %s, %s: %.2f ms (median of %d; %s)" % (
            pairing, k, float(np.median(v)), len(v), " ".join("%.2f" % x for x in v)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="score,struct", help="which files' rows: score, struct, both, or none")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--structures", default="0,1,2,3", help="the rows of these structures only")
    ap.add_argument("--pairings", default="frame,prediction")
    ap.add_argument("--dense-fitness", action="store_true", help="append the byte and the float dense fitness (corner members) of the stills to every line")
    a = ap.parse_args()
    structures, pairings = [int(v) for v in a.structures.split(",")], a.pairings.split(",")
    for name in [n for n in a.rows.split(",") if n in ROWS]:
        for requant in (True, False):
            for structure, seed, iters in ROWS[name]:
                for pairing in ("frame", "prediction"):
                    if structure in structures and pairing in pairings:
                        run_row(structure, seed, iters, pairing, requant, a.dense_fitness)
    if a.timing:
        timing()


if __name__ == "__main__":
    main()
