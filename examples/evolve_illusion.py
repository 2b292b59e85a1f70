#!/usr/bin/env python3
"""Evolve illusions end to end on the MI355X engine: the flow of the reference's neat_illusion()
(/root/reference/generate_illusion.py:676-711) with neat_lite standing in for neat-python.

    python examples/evolve_illusion.py -o results -g 5 [-m model.npz] [--size small|big|256] [-s 1] [-c 3]
    python -m torch.distributed.run --nproc-per-node 8 examples/evolve_illusion.py ...   (population sharded over GPUs)
    python examples/evolve_illusion.py -g 5 --refine 4 --refine_iters 5    (Lamarckian step: after every generation the parameters of
        the 4 best genomes are replaced by those `train.refine_genomes` climbs to, before reproduction; gradient = 1 renders only;
        --objective flow --flow-direction tangent climbs the flow objective instead of the squared error;
        --flow-pairing prediction pairs consecutive predictions, as the fitness that selects does;
        [--flow-score --flow-members corners [--flow-corner-quality Q] [--flow-corner-distance D]]   (the members of the score are the corners the fitness itself
        would pick on every term's reference: train.CornerMembers)
        --flow-score [--flow-score-structure circles|bands|free|auto] [--flow-max-norm M] climbs the fitness's own score of that structure on the
        dense field: train.FlowScore, BandsScore or FreeScore; auto follows --structure)
    python examples/evolve_illusion.py -g 5 --fitness dense [--flow-radius R] [--flow-eps E] [--flow-score [--flow-max-norm M]]   (selection by the dense
        motion score of --structure, fitness.DenseFitness, in place of the corner tracks; with --refine K --objective flow --flow-score
        --flow-pairing prediction selection and refinement use one score with the same settings)
    python examples/evolve_illusion.py -g 5 --fitness dense --dense-members corners [--dense-corner-quality X --dense-corner-distance X]   (the dense score
        over the corners the corner fitness would track, not over every pixel; --refine --refine-solve fitness then refines under the same members)
    python examples/evolve_illusion.py -g 5 --fitness dense --dense-frames float   (the dense score on PredNet's float predictions, not on their bytes:
        selection then sees the sub-byte differences refinement moves)
    python examples/evolve_illusion.py -g 5 --fitness dense --dense-levels 3 --dense-iters 3   (the dense score on the field of a pyramidal, iterated
        Lucas-Kanade solve, which follows motions of a pixel and more where the single step shrinks them; --refine-solve fitness makes --refine climb that
        score through that solve, --flow-levels L --flow-iters K give the objective of the --flow-* options a solve of its own)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from evolutionary_illusion_generator_amd import fitness, neat_lite as neat
from examples.flow_args import add_flow_arguments, dense_fitness_of, flow_of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", "-m", default="synthetic", help="chainer npz weights, or synthetic[:seed]")
    ap.add_argument("--output_dir", "-o", default="results")
    ap.add_argument("--structure", "-s", type=int, default=1, help="0 Bands, 1 Circles, 2 Free, 3 CirclesFree")
    ap.add_argument("--config", "-cfg", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "circles_neat.cfg"))
    ap.add_argument("--size", "-wh", default="small", help="small (160x120), big (640x480) or N for NxN")
    ap.add_argument("--color_space", "-c", type=int, default=3)
    ap.add_argument("--channels", "-ch", default="3,48,96,192")
    ap.add_argument("--gradient", "-g1", type=int, default=1)
    ap.add_argument("--generations", "-g", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--refine", type=int, default=0, help="refine the parameters of this many of the best genomes after every generation (0: off)")
    ap.add_argument("--refine_iters", type=int, default=5, help="ascent steps of train.refine_genomes per generation")
    ap.add_argument("--objective", default="mse", choices=["mse", "error", "flow"], help="what --refine climbs")
    ap.add_argument("--fitness", default="corners", choices=["corners", "dense"],
                    help="what selects: the reference's score of the tracked corners, or the dense motion score of --structure (fitness.DenseFitness)")
    ap.add_argument("--dense-levels", type=int, default=1, help="--fitness dense: pyramid levels of the solve (1 .. 6; 1 with --dense-iters 1 is the single step)")
    ap.add_argument("--dense-iters", type=int, default=1, help="--fitness dense: iterations per pyramid level (1 .. 32)")
    ap.add_argument("--dense-members", default="all", choices=["all", "corners"],
                    help="--fitness dense: who is counted: every pixel, or the corners the corner fitness would track (train.CornerMembers); "
                         "--refine-solve fitness then refines under the same members")
    ap.add_argument("--dense-frames", default="byte", choices=["byte", "float"],
                    help="--fitness dense: the images the score reads: the frames the roll-out emits, or PredNet's float predictions before the byte, "
                         "the images --objective flow itself is evaluated on (fitness.DenseFitness(frames=))")
    ap.add_argument("--dense-corner-quality", type=float, default=None, help="--dense-members corners: goodFeaturesToTrack's quality level, in (0, 1] (default: CornerMembers')")
    ap.add_argument("--dense-corner-distance", type=float, default=None, help="--dense-members corners: the least distance between two corners, in pixels (default: CornerMembers')")
    ap.add_argument("--refine-solve", default="single", choices=["single", "fitness"],
                    help="--refine under --fitness dense: single climbs the objective of the --flow-* options (by default the single regularised step), fitness "
                         "climbs DenseFitness.solve_objective(), the score of the field the fitness itself scores, through --dense-levels and --dense-iters")
    add_flow_arguments(ap, direction=dict(choices=["tangent", "radial", "horizontal", "vertical"], help="objective flow: the field (default: the mean square)"),
                       radius=dict(help=None), eps=dict(help=None),
                       reference=dict(choices=["constant", "moving"], help="objective flow: moving also follows how the term moves with the still as its reference frame"),
                       pairing=dict(choices=["frame", "prediction"],
                                    help="objective flow: frame pairs the still with the extended predictions, prediction pairs consecutive predictions as the population fitness does"))
    a = ap.parse_args()
    w, h = {"small": (160, 120), "big": (640, 480)}.get(a.size) or (int(a.size), int(a.size))
    channels = [int(c) for c in a.channels.split(",")]
    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
        torch.distributed.init_process_group("nccl")
    config = neat.Config(neat.DefaultGenome, neat.DefaultReproduction, neat.DefaultSpeciesSet, neat.DefaultStagnation, a.config)

    inside = (fitness.leaf_planes(a.structure, w, h)[0] != -1).astype("uint8")   # the pixels of the structure's grid: the members' mask
    try:
        dense = dense_fitness_of(a, a.structure, inside)
    except ValueError as e:
        raise SystemExit("--fitness dense: %s" % e)
    if dense is not None:
        try:
            dense.solve_on(w, h)
        except ValueError as e:
            raise SystemExit("--fitness dense: %s" % e)
        fitness.FITNESS_SCORE = dense    # get_fitnesses_neat keeps the reference's signature: the module switch carries the choice

    def eval_genomes(genomes, config):
        fitness.get_fitnesses_neat(a.structure, genomes, a.model, config, w, h, channels, c_dim=a.color_space,
                                   best_dir=a.output_dir, gradient=a.gradient)
        if a.refine > 0 and a.refine_iters > 0:
            refine_best(genomes, config)

    trainer = []

    def refine_best(genomes, config):
        """The Lamarckian step: the a.refine best of the generation keep key, structure and fitness and take the refined parameters.
        Every rank refines the same genomes with the same deterministic calls, so the populations stay identical."""
        from evolutionary_illusion_generator_amd import train
        if a.gradient != 1:
            raise SystemExit("--refine needs the gradient = 1 render (the palette and the rounded gray are not differentiable)")
        best = sorted((g for _, g in genomes), key=lambda g: -g.fitness)[:a.refine]
        if not trainer:
            trainer.append(train.PredNetTrainer(a.model, channels, w, h, a.refine, 22))
        if a.refine_solve == "fitness":
            if dense is None:
                raise SystemExit("--refine-solve fitness needs --fitness dense: it climbs that fitness's own score through its own solve")
            flow, objective = dense.solve_objective(), "flow"
        else:
            flow, objective = flow_of(a, w, h, inside), a.objective
        refined, history, _ = train.refine_genomes(trainer[0], best, config, a.structure, iters=a.refine_iters, objective=objective, flow=flow)
        for g, r in zip(best, refined):
            for k, n in r.nodes.items():
                g.nodes[k].bias, g.nodes[k].response = n.bias, n.response
            for k, c in r.connections.items():
                g.connections[k].weight = c.weight
        print("refined %d genomes: stand-in loss %.6e -> %.6e" % (len(best), history[0], history[-1]))

    p = neat.Population(config, seed=a.seed)  # identical on every rank: same seed, same all-gathered fitness
    p.add_reporter(neat.StdOutReporter(True))
    p.add_reporter(neat.StatisticsReporter())
    winner = p.run(eval_genomes, a.generations)
    print("winner", winner.key, winner.fitness, winner.size())


if __name__ == "__main__":
    main()
