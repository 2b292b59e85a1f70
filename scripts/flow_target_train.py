"""Train on moving textures under the flow objective's target field and under the squared error, and report the held-out mean squared
endpoint error between consecutive predictions before and after ("The target field"; profiles/flow_target_train.txt).

    python scripts/flow_target_train.py [--steps 200] [--size 32x24] [--channels 1,8,16] [--batch 4] [--seq 6] [--fed 3] [--alpha 3e-3]
                                        [--radius 3] [--eps 1e-2]

Both runs start from the same synthetic weights and read the same batches of one-layer train.MovingTextures (seed 0; held-out batch
10**6); the last --seq - --fed steps of every sequence are self-fed.  "target": objective="flow" with a PredictionFlow and the video's
exact flow as flow_target, the terms 1 .. T - 2 weighted one (term 0 runs from the reset state's zero image and has no gradient);
"mse": the default objective on the same call.  The metric of both is train.flow_epe on the tape-free predictions, per term and as the
mean over the terms 1 .. T - 2; the held-out squared error of the predictions is printed beside it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.train_prednet import held_out_epe  # noqa: E402


def run(kind, a, w, h, ch):
    from evolutionary_illusion_generator_amd.train import MovingTextures, PredictionFlow, PredNetTrainer
    flow = PredictionFlow(a.radius, a.eps)
    weights = [0.0] + [1.0] * (a.seq - 2)
    with MovingTextures(w, h, ch[0], a.seq, seed=0, layers=1) as src, PredNetTrainer("synthetic:0", ch, w, h, a.batch, a.seq, alpha=a.alpha) as tr:
        held, truth, _ = src.batch(10 ** 6, a.batch, flow=True)
        measure = lambda: (held_out_epe(tr, held, truth, a.radius, a.eps, a.fed, False), tr.evaluate(held, n_fed=a.fed))
        before, losses = measure(), []
        for k in range(a.steps):
            frames, fl, _ = src.batch(k, a.batch, flow=True)
            if kind == "target":
                losses.append(tr.step(frames, n_fed=a.fed, step_weights=weights, objective="flow", flow=flow, flow_target=fl))
            else:
                losses.append(tr.step(frames, n_fed=a.fed))
        after = measure()
    fmt = lambda v: " ".join("%.6f" % x for x in v)
    print("%-6s train loss: first %.6f, last %.6f" % (kind, losses[0], losses[-1]))
    for name, k in (("squared endpoint error per term 1 .. T - 2", 0), ("squared error per term 0 .. T - 2", 1)):
        print("%-6s held-out %s: before %s | after %s" % (kind, name, fmt(before[k]), fmt(after[k])))
        b, c = float(before[k].mean()), float(after[k].mean())
        print("%-6s   mean: %.6f -> %.6f (%.1f %% lower)" % (kind, b, c, 100 * (1 - c / b)))
    return before[0].mean(), after[0].mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--size", default="32x24")
    ap.add_argument("--channels", default="1,8,16")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=6)
    ap.add_argument("--fed", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=3e-3)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--eps", type=float, default=1e-2)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.lower().split("x"))
    ch = [int(c) for c in a.channels.split(",")]
    print("%dx%d %s, B = %d, T = %d (%d fed + %d self-fed), %d Adam steps at alpha %g, PredictionFlow(radius %d, eps %g), one-layer textures"
          % (w, h, ch, a.batch, a.seq, a.fed, a.seq - a.fed, a.steps, a.alpha, a.radius, a.eps))
    for kind in ("target", "mse"):
        run(kind, a, w, h, ch)


if __name__ == "__main__":
    main()
