#!/usr/bin/env python3
"""What scoring the float predictions changes in the dense fitness ("Float frames").  Facts, not pass conditions.

    python scripts/dense_float_fitness.py [--shapes headline,ref160] [--out profiles/dense_float_fitness.txt]

Per shape of bench.py and per structure, on the shape's genomes under the population pairing: Spearman's rank correlation of the float
dense fitness against the byte dense fitness and against the corner fitness, under members all and corners; the share of genomes scoring
exactly 0 under each; and the share of pixels whose byte It = I1 - I0 (the gray of the two emitted frames the byte fitness compares) is
exactly 0.

With --torch the byte-flip conditioning is counted: the same images go through the oracle's reference-order torch implementation
(oracle/prednet_torch.py, order="chainer", im2col + matmul on the GPU: another fp32 summation order inside every convolution), whose two
emitted frames and two float predictions are scored by the same dense stage (Engine.dense_score, Engine.dense_score_float).  Per structure and
members: how many genomes keep their byte dense fitness within 1e-4 relative between that implementation and the HIP path, and how many keep
their float dense fitness (|a - b| / |b|, both zero counts as within, as oracle/classify.py); beside them the share of emitted bytes that
differ between the two implementations."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STRUCTURES = {0: "Bands", 1: "Circles", 2: "Free"}


def gray(v):
    """tflow_gray of uint8 [n, C, H, W]"""
    f = (v.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    return f[:, 0] if f.shape[1] == 1 else (0.299 * f[:, 0] + 0.587 * f[:, 1]) + 0.114 * f[:, 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,ref160")
    ap.add_argument("--structures", default="0,1,2")
    ap.add_argument("--torch", action="store_true", help="also count the genomes within 1e-4 relative of the oracle's reference-order torch implementation")
    ap.add_argument("--torch-batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_float_fitness.txt"))
    a = ap.parse_args()
    import torch
    import bench
    from dense_fitness_bench import spearman
    from evolutionary_illusion_generator_amd import fitness, genome, train
    lines = ["float dense fitness against byte dense fitness and corner fitness, population pairing, %s" % torch.cuda.get_device_name(0),
             "build %s" % bench.kernel_sources_sha(), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for shape in a.shapes.split(","):
        W, H, CHANNELS, C_DIM, _, _, _, pop, label = bench.SHAPES[shape]
        cfg, population, wts = bench.make_workload(shape, pop)
        genomes = [g for _, g in population]
        max_batch = min(pop, 256)
        say("%s: %dx%d, PredNet %s, pop %d" % (shape, W, H, ",".join(map(str, CHANNELS)), pop))
        for structure in map(int, a.structures.split(",")):
            kw = dict(c_dim=C_DIM, gradient=1, max_batch=max_batch)
            run = lambda score: fitness.population_fitness(structure, genomes, wts, cfg, W, H, CHANNELS, score=score, **kw)
            corner = run("corners")
            # the two emitted frames of the pair, from the same engine: the share of pixels the byte fitness sees no change at
            eng = fitness.get_engine(wts, W, H, CHANNELS, max_batch=max_batch)
            gb = genome.GenomeBatch(genomes, cfg, C_DIM, n_leaves=len(cfg.genome_config.input_keys))
            d_img = torch.zeros((pop, C_DIM, H, W), dtype=torch.uint8, device="cuda")
            d_fr = torch.zeros((pop, 2, C_DIM, H, W), dtype=torch.uint8, device="cuda")
            nr = eng.cfg.n_repeat
            eng.render_cppn(gb, d_img, bg=1, gradient=1)
            eng.prednet_rollout(d_img, pop, nr + 1, nr - 1, d_fr)
            fr = d_fr.cpu().numpy()
            still = float((gray(fr[:, 1]) - gray(fr[:, 0]) == 0).mean())
            say("  %-7s pixels whose byte It is exactly 0: %.1f %%; corner fitness scoring 0: %.1f %%" % (STRUCTURES[structure], 100.0 * still, 100.0 * float((corner == 0).mean())))
            other = None
            if a.torch:
                from oracle.prednet_torch import PredNetTorch
                torch.backends.cuda.matmul.allow_tf32 = False
                torch.backends.cudnn.allow_tf32 = False
                net = PredNetTorch(wts, CHANNELS, W, H, device="cuda", conv="matmul", order="chainer")
                imgs, tb, tf = d_img.cpu().numpy(), [], []
                for i in range(0, pop, a.torch_batch):
                    fb, fl = net.rollout(imgs[i:i + a.torch_batch], n_repeat=nr, n_ext=1, requant=bool(eng.cfg.requant_feedback))
                    tb.append(fb[:, nr - 1:nr + 1])
                    tf.append(fl[:, nr - 1:nr + 1])
                del net
                other = (np.ascontiguousarray(np.concatenate(tb)), np.ascontiguousarray(np.concatenate(tf)))
                say("          reference-order torch implementation: %.3f %% of the emitted bytes of the pair differ from the HIP path's" % (100.0 * float((other[0] != fr).mean())))
            for name, members in (("all", None), ("corners", train.CornerMembers())):
                byte, flt = run(fitness.DenseFitness(members=members)), run(fitness.DenseFitness(members=members, frames="float"))
                if other is not None:
                    per = C_DIM * H * W
                    dense = fitness.DenseFitness(members=members).resolved(structure)
                    t8, t32 = torch.from_numpy(other[0]).cuda(), torch.from_numpy(other[1]).cuda()
                    ob = eng.dense_score(t8, 2 * per, t8.view(-1)[per:], 2 * per, pop, dense)
                    of = eng.dense_score_float(t32, 2 * per, t32.view(-1)[per:], 2 * per, pop, dense)

                    def within(mine, theirs):
                        rel = np.where(theirs != 0, np.abs(mine - theirs) / np.where(theirs != 0, np.abs(theirs), 1.0), np.where(mine != 0, np.inf, 0.0))
                        return int((rel <= 1e-4).sum()), float(np.median(rel)), float(rel.max())

                    (nb, mb, xb), (nf, mf, xf) = within(byte, ob), within(flt, of)
                    say("          members %-7s within 1e-4 relative of the torch implementation: byte %d of %d (median rel %.2e, max %.2e), float %d of %d (median rel %.2e, max %.2e)" % (
                        name, nb, pop, mb, xb, nf, pop, mf, xf))
                say("          members %-7s Spearman float / byte %.3f, float / corner fitness %.3f, byte / corner fitness %.3f; scoring 0: float %.1f %%, byte %.1f %%" % (
                    name, spearman(flt, byte), spearman(flt, corner), spearman(byte, corner), 100.0 * float((flt == 0).mean()), 100.0 * float((byte == 0).mean())))
        fitness.clear_engines()
        say("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
