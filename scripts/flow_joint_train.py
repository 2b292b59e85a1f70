"""Train on moving textures under the joint objective and under the valid pixels, and record the held-out mean squared endpoint error
between consecutive predictions (over all pixels and over the valid ones) and the held-out squared error, before and after (DESIGN.md
section 13, "The joint objective and the valid pixels"; profiles/flow_joint_train.txt).

    python scripts/flow_joint_train.py [--steps 200] [--size 32x24] [--channels 1,8,16] [--batch 4] [--seq 6] [--fed 3] [--alpha 3e-3]
                                       [--radius 3] [--eps 1e-2] [--weights 1,4,16,64] [--out profiles/flow_joint_train.txt]

The setting is scripts/flow_target_train.py's: every leg starts from the same synthetic weights and reads the same batches of
train.MovingTextures (seed 0; held-out batch 10**6); the last --seq - --fed steps of every sequence are self-fed; objective="flow" runs
under a PredictionFlow with the video's exact flow as flow_target and the terms 1 .. T - 2 weighted one.  The legs:
  target, mse            one-layer textures: the two legs of profiles/flow_target_train.txt, which they reproduce
  joint mu               one-layer textures: the target leg with frame_weight = mu, for every mu of --weights
  target/2, valid/2      two-layer textures: the target leg without and with flow_valid, the renderer's validity planes
The metrics are train.flow_epe on the tape-free predictions (terms 1 .. T - 2; `valid`: the mean over every sample's valid pixels) and
the squared error `evaluate` returns (terms 0 .. T - 2), as means over the terms."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.train_prednet import held_out_epe  # noqa: E402


def run(name, a, w, h, ch, layers=1, objective="flow", frame_weight=None, valid=False):
    """one leg -> {metric: (before, after)}, the means over the terms"""
    from evolutionary_illusion_generator_amd.train import MovingTextures, PredictionFlow, PredNetTrainer
    flow = PredictionFlow(a.radius, a.eps)
    weights = [0.0] + [1.0] * (a.seq - 2)
    with MovingTextures(w, h, ch[0], a.seq, seed=0, layers=layers) as src, PredNetTrainer("synthetic:0", ch, w, h, a.batch, a.seq, alpha=a.alpha) as tr:
        held, truth, _, visible = src.batch(10 ** 6, a.batch, flow=True, valid=True)
        measure = lambda: dict(epe=held_out_epe(tr, held, truth, a.radius, a.eps, a.fed, False).mean(),
                               epe_valid=held_out_epe(tr, held, truth, a.radius, a.eps, a.fed, False, visible).mean(), mse=tr.evaluate(held, n_fed=a.fed).mean())
        before, losses = measure(), []
        for k in range(a.steps):
            frames, fl, _, vis = src.batch(k, a.batch, flow=True, valid=True)
            if objective == "mse":
                losses.append(tr.step(frames, n_fed=a.fed))
                continue
            extra = dict(frame_weight=frame_weight) if frame_weight is not None else {}
            if valid:
                extra["flow_valid"] = vis
            losses.append(tr.step(frames, n_fed=a.fed, step_weights=weights, objective="flow", flow=flow, flow_target=fl, **extra))
        after = measure()
        share = float(visible[:, 1:].float().mean())
    out = {k: (float(before[k]), float(after[k])) for k in before}
    lines = ["%-10s train loss: first %.6f, last %.6f; valid pixels of the held-out terms: %.1f %%" % (name, losses[0], losses[-1], 100 * share)]
    for key, label in (("epe", "squared endpoint error, all pixels"), ("epe_valid", "squared endpoint error, valid pixels"), ("mse", "squared error")):
        b, c = out[key]
        lines.append("%-10s   held-out %-36s %.6f -> %.6f (%+.1f %%)" % (name, label + ":", b, c, 100 * (c / b - 1)))
    return out, lines


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
    ap.add_argument("--weights", default="1,4,16,64", help="the frame weights of the joint legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_joint_train.txt"))
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.lower().split("x"))
    ch = [int(c) for c in a.channels.split(",")]
    mus = [float(v) for v in a.weights.split(",")]
    text = ["%dx%d %s, B = %d, T = %d (%d fed + %d self-fed), %d Adam steps at alpha %g, PredictionFlow(radius %d, eps %g)"
            % (w, h, ch, a.batch, a.seq, a.fed, a.seq - a.fed, a.steps, a.alpha, a.radius, a.eps)]
    legs = [("target", {}), ("mse", dict(objective="mse"))] + [("joint %g" % mu, dict(frame_weight=mu)) for mu in mus] \
        + [("target/2", dict(layers=2)), ("valid/2", dict(layers=2, valid=True))]
    results = {}
    for name, kw in legs:
        results[name], lines = run(name, a, w, h, ch, **kw)
        text += lines
        print("\n".join(lines), flush=True)
    both = [name for name, _ in legs if name.startswith("joint") and all(results[name][k][1] < results[name][k][0] for k in ("epe", "mse"))]
    text.append("joint legs that lower both the endpoint error (all pixels) and the squared error: %s" % (", ".join(both) if both else "none"))
    print(text[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
