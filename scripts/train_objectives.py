"""Train PredNet from ONE start on the same data for the same number of Adam steps under three objectives -- next-frame squared
error, Lotter's L_0 (the image layer's error units, an L1 next-frame error) and L_all (upper layers at 0.1) -- and compare what
each leaves behind on held-out data: the squared error, the L_0 error, and the number of Lucas-Kanade vectors the fitness path
(`fitness.get_vectors`: 20 repeats of a still, 2 self-fed steps, corners above quality 0.3) finds on held-out stills.
Prints one JSON line per objective and writes profiles/train_objectives.json.

    python scripts/train_objectives.py [--steps 300] [--size 64x48] [--channels 1,16,32] [--batch 8] [--seq 8] [--stills 16]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OBJECTIVES = {"mse": dict(objective="mse"), "l0": dict(objective="error"), "lall": dict(objective="error", layer_weights="lall")}


def drifting(seed, n, seq, c_dim, w, h):
    """n sequences of a blob-and-ring texture drifting by up to 1.5 pixels per frame, each in its own seeded direction"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, seq, c_dim, h, w), np.uint8)
    for i in range(n):
        vx, vy = rng.uniform(-1.5, 1.5, 2)
        blobs = [(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 6), rng.uniform(-1, 1)) for _ in range(6)]
        cx, cy, k = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 5)
        for t in range(seq):
            v = 0.5 * np.sin(np.hypot(xx - cx - vx * t, yy - cy - vy * t) / k)
            for bx, by, r, a in blobs:
                v += a * np.exp(-((xx - bx - vx * t) ** 2 + (yy - by - vy * t) ** 2) / (2 * r * r))
            out[i, t] = np.repeat(np.clip(127.5 + 100 * v, 0, 255)[None], c_dim, 0).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--size", default="64x48", help="WxH")
    ap.add_argument("--channels", default="1,16,32")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=8)
    ap.add_argument("--stills", type=int, default=16, help="held-out stills given to the fitness path")
    ap.add_argument("--alpha", type=float, default=3e-3)
    ap.add_argument("--model", default="synthetic:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_objectives.json"))
    a = ap.parse_args()
    from evolutionary_illusion_generator_amd import fitness
    from evolutionary_illusion_generator_amd.train import PredNetTrainer
    w, h = (int(v) for v in a.size.lower().split("x"))
    ch = [int(c) for c in a.channels.split(",")]
    held = drifting(10 ** 6, a.batch, a.seq, ch[0], w, h)
    stills = drifting(10 ** 6 + 1, a.stills, 1, ch[0], w, h)[:, 0]

    def held_out(tr):
        mse, table = tr.evaluate(held, layer_errors=True)
        wts = tr.weights()
        counts = []
        for img in stills:
            v = fitness.get_vectors(np.ascontiguousarray(img.transpose(1, 2, 0)), wts, ch, w, h)
            counts.append(0 if (len(v) and v[0] is None) else len(v))
        fitness.clear_engines()
        return dict(mse=float(mse.mean()), l0=float(table[:, 0].mean()), layer_errors=[float(x) for x in table.mean(0)],
                    lk_vectors_mean=float(np.mean(counts)), lk_vectors=counts)

    results = []
    for name, kw in OBJECTIVES.items():
        kw = dict(kw)
        if kw.get("layer_weights") == "lall":
            kw["layer_weights"] = [1.0] + [0.1] * (len(ch) - 1)
        with PredNetTrainer(a.model, ch, w, h, a.batch, a.seq, alpha=a.alpha) as tr:
            before = held_out(tr) if not results else results[0]["before"]
            for k in range(a.steps):
                tr.step(drifting(k, a.batch, a.seq, ch[0], w, h), **kw)
            after = held_out(tr)
        results.append(dict(objective=name, steps=a.steps, before=before, after=after))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(shape=dict(w=w, h=h, channels=ch, batch=a.batch, seq=a.seq, alpha=a.alpha, model=a.model, stills=a.stills), results=results), f, indent=1)


if __name__ == "__main__":
    main()
