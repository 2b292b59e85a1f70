#!/usr/bin/env python3
"""What the dense motion fitness costs on the population path, against the corner fitness of the same run.

    python scripts/dense_fitness_bench.py [--rounds 6] [--shapes headline,ref160] [--out profiles/dense_fitness_cost.txt]
    python scripts/dense_fitness_bench.py --dense-levels 3 --dense-iters 3 --structures 0,1 --out OTHER.txt
    python scripts/dense_fitness_bench.py --dense-members corners [--out profiles/dense_members_cost.txt]

Per shape of bench.py (headline: 256 x 256 colour, pop 256; ref160: 160 x 120 colour, pop 50) and per structure,
`fitness.population_fitness` is timed under score="corners" and score="dense" in alternation, one generation each per round, after
one warm-up generation of each: the median (min .. max) of the rounds in genome evaluations per second, the ratio of the medians, and
the device time of the stage that follows the roll-out (Lucas-Kanade + score, or the dense stage) against the roll-out's, from the
engine's own HIP events.  A (shape, structure) whose dense generation takes longer than --slow seconds is timed for two rounds only, and
the line says so.  For the headline genomes the agreement of the two fitnesses is recorded: Spearman's rank correlation (ties share
their mean rank) and the share of genomes scoring exactly 0 under each.

With --dense-levels or --dense-iters above 1 the comparison is another one: the dense fitness's single step ("corners" in the columns'
place) against its pyramidal, iterated solve (fitness.DenseFitness(levels=L, iters=K), in "dense"'s place), alternated in the same
way; the header line says so and the lines name the two.

With --dense-members corners three fitnesses are alternated: the corner fitness, the dense fitness on every pixel ("dense all") and the
dense fitness whose members are the corner fitness's own corners ("dense corners", fitness.DenseFitness(members=train.CornerMembers());
DESIGN.md section 14, "Members"), one line each, the two dense ones against the corner fitness.  The output goes to
profiles/dense_members_cost.txt unless --out says otherwise.

With --dense-frames float the comparison is the dense fitness on the emitted bytes ("byte") against the same fitness on PredNet's float
predictions ("float", fitness.DenseFitness(frames="float"); DESIGN.md section 14, "Float frames"), alternated in the same way, under the
members --dense-members names and the solve --dense-levels / --dense-iters name; the roll-out, which holds the float call's two gray
snapshots, is reported for each of the two.  The output goes to profiles/dense_float_cost.txt unless --out says otherwise.

The output file has two parts: what this script measures, which a run replaces, and everything from the line NOTES_MARK on, which a run
keeps as it finds it: the records of other commands of the same visit (the default path against the parent commit, the example), written by
hand."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRUCTURES = {0: "Bands", 1: "Circles", 2: "Free"}
NOTES_MARK = "---- records of other commands of the same visit (kept by scripts/dense_fitness_bench.py, not written by it) ----"


def ranks(v):
    """ranks from 1, ties share their mean rank"""
    v = np.asarray(v, np.float64)
    order = np.argsort(v, kind="stable")
    r = np.empty(len(v))
    i = 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and v[order[j + 1]] == v[order[i]]:
            j += 1
        r[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return r


def spearman(a, b):
    ra, rb = ranks(a), ranks(b)
    if ra.std() == 0 or rb.std() == 0:
        return float("nan")
    return float(np.corrcoef(ra, rb)[0, 1])


def spread(v):
    return "%.1f (%.1f .. %.1f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--shapes", default="headline,ref160")
    ap.add_argument("--slow", type=float, default=4.0, help="a dense generation slower than this many seconds is timed for two rounds only")
    ap.add_argument("--structures", default="0,1,2", help="0 Bands, 1 Circles, 2 Free")
    ap.add_argument("--dense-levels", type=int, default=1, help="with --dense-iters: time the single step against this solve")
    ap.add_argument("--dense-iters", type=int, default=1)
    ap.add_argument("--dense-members", default="all", choices=["all", "corners"],
                    help="corners: also time the dense fitness under the corner fitness's own corners as members, beside the corner fitness and the all-pixel dense one")
    ap.add_argument("--dense-frames", default="byte", choices=["byte", "float"],
                    help="float: time the dense fitness on the emitted bytes against the same fitness on the float predictions")
    ap.add_argument("--append", action="store_true", help="add this run to the output file's measured part in place of replacing it")
    ap.add_argument("--out", default=None, help="default: profiles/dense_fitness_cost.txt, dense_members_cost.txt with --dense-members corners, dense_float_cost.txt with --dense-frames float")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "dense_float_cost.txt" if a.dense_frames == "float" else
                                  "dense_members_cost.txt" if a.dense_members == "corners" else "dense_fitness_cost.txt")
    import torch
    import bench
    from evolutionary_illusion_generator_amd import fitness
    solve = (a.dense_levels, a.dense_iters)
    third = None      # --dense-members corners (byte frames): the label of the third fitness, scores["members"]
    # the two alternated fitnesses sit under the keys "corners" and "dense" whatever they are: first / second name them in the output
    by_frames = a.dense_frames == "float"
    if by_frames:
        from evolutionary_illusion_generator_amd import train
        members = train.CornerMembers() if a.dense_members == "corners" else None
        first, second = "byte", "float"
        scores = {"corners": fitness.DenseFitness(levels=solve[0], iters=solve[1], members=members),
                  "dense": fitness.DenseFitness(levels=solve[0], iters=solve[1], members=members, frames="float")}
        head = ("dense motion fitness on the emitted bytes against the float predictions, members %s, solve %d x %d" % ((a.dense_members,) + solve)
                + ", %s, %d rounds, the two alternated per round")
    elif a.dense_members == "corners":
        from evolutionary_illusion_generator_amd import train
        first, second, third = "corners", "dense all", "dense corners"
        scores = {"corners": "corners", "dense": fitness.DenseFitness(levels=solve[0], iters=solve[1]),
                  "members": fitness.DenseFitness(levels=solve[0], iters=solve[1], members=train.CornerMembers())}
        head = ("dense motion fitness on every pixel and on the corner fitness's corners against the corner fitness" + ("" if solve == (1, 1) else ", solve %d x %d" % solve)
                + ", %s, %d rounds, the three alternated per round")
    elif solve == (1, 1):
        first, second, scores = "corners", "dense", {"corners": "corners", "dense": "dense"}
        head = "dense motion fitness against the corner fitness, %s, %d rounds, corners and dense alternated per round"
    else:
        first, second = "single", "%dx%d" % solve
        scores = {"corners": fitness.DenseFitness(), "dense": fitness.DenseFitness(levels=solve[0], iters=solve[1])}
        head = "dense motion fitness, the single step against " + "%d levels x %d iterations" % solve + ", %s, %d rounds, the two alternated per round"
    lines = [head % (torch.cuda.get_device_name(0), a.rounds), "build %s" % bench.kernel_sources_sha(), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for shape in a.shapes.split(","):
        W, H, CHANNELS, C_DIM, _, _, _, pop, label = bench.SHAPES[shape]
        cfg, population, wts = bench.make_workload(shape, pop)
        genomes = [g for _, g in population]
        max_batch = min(pop, 256)
        eng = fitness.get_engine(wts, W, H, CHANNELS, max_batch=max_batch)
        say("%s: %dx%d, PredNet %s, pop %d, device batch %d" % (shape, W, H, ",".join(map(str, CHANNELS)), pop, max_batch))
        for structure, name in ((s, STRUCTURES[s]) for s in map(int, a.structures.split(","))):
            def generation(score):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fit = fitness.population_fitness(structure, genomes, wts, cfg, W, H, CHANNELS, c_dim=C_DIM, gradient=1, max_batch=max_batch, score=scores[score])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                t = eng.timings()
                return fit, dt, t["prednet_ms"], t["flow_ms"] + t["score_ms"]

            keys = ("corners", "dense") + (("members",) if third else ())
            warm = {s: generation(s) for s in keys}
            rounds = a.rounds if warm["dense"][1] <= a.slow else min(a.rounds, 2)
            rate, stage, roll, roll_of = {s: [] for s in keys}, {s: [] for s in keys}, [], {s: [] for s in keys}
            for _ in range(rounds):
                for s in keys:
                    fit, dt, roll_ms, stage_ms = generation(s)
                    assert fit.tobytes() == warm[s][0].tobytes(), "the fitness of a generation changed between rounds"
                    rate[s].append(pop / dt)
                    stage[s].append(stage_ms)
                    roll.append(roll_ms)
                    roll_of[s].append(roll_ms)
            fc, fd = warm["corners"][0], warm["dense"][0]
            say("  %-7s %s %s evals/s, %s %s evals/s, %s / %s %.3f%s" % (
                name, first, spread(rate["corners"]), second, spread(rate["dense"]), second, first, np.median(rate["dense"]) / np.median(rate["corners"]),
                "" if rounds == a.rounds else "  [%d rounds: a dense generation takes %.1f s]" % (rounds, warm["dense"][1])))
            if by_frames:     # the two gray snapshots of a float call run inside its roll-out: the roll-out of each of the two, to hundredths
                fine = lambda v: "%.2f (%.2f .. %.2f)" % (float(np.median(v)), min(v), max(v))
                say("          device ms per generation: roll-out byte %s, float %s (two gray snapshots inside), difference of the medians %.3f; dense stage byte %s, float %s" % (
                    spread(roll_of["corners"]), spread(roll_of["dense"]), np.median(roll_of["dense"]) - np.median(roll_of["corners"]), fine(stage["corners"]), fine(stage["dense"])))
            else:
                say("          device ms per generation: roll-out %s; %s %s; %s %s = %.1f %% of the roll-out" % (
                    spread(roll), "flow + score" if solve == (1, 1) else "dense stage, single step", spread(stage["corners"]),
                    "dense stage" if solve == (1, 1) else "dense stage, " + second, spread(stage["dense"]), 100.0 * np.median(stage["dense"]) / np.median(roll)))
            say("          agreement over the %d genomes: Spearman %.3f; scoring 0: %s %.1f %%, %s %.1f %%" % (
                pop, spearman(fc, fd), first, 100.0 * float((fc == 0).mean()), second, 100.0 * float((fd == 0).mean())))
            if third:
                fm = warm["members"][0]
                say("  %-7s %s %s evals/s, %s / %s %.3f, %s / %s %.3f" % ("", third, spread(rate["members"]), third, first, np.median(rate["members"]) / np.median(rate["corners"]),
                                                                      third, second, np.median(rate["members"]) / np.median(rate["dense"])))
                say("          device ms per generation: %s stage %s = %.1f %% of the roll-out, %.2f of flow + score" % (
                    third, spread(stage["members"]), 100.0 * np.median(stage["members"]) / np.median(roll), np.median(stage["members"]) / np.median(stage["corners"])))
                say("          agreement of %s with %s over the %d genomes: Spearman %.3f; scoring 0: %.1f %%" % (third, first, pop, spearman(fc, fm), 100.0 * float((fm == 0).mean())))
        fitness.clear_engines()
        say("")
    kept = ""
    if os.path.exists(a.out):
        old = open(a.out).read()
        if NOTES_MARK in old:
            kept = old[old.index(NOTES_MARK):]
        if a.append:
            lines = (old[:old.index(NOTES_MARK)] if NOTES_MARK in old else old).rstrip("\n").split("\n") + [""] + lines
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
