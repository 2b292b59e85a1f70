"""How far the two flow paths are from the true motion, on moving CPPN textures whose flow is known exactly (train.MovingTextures,
Engine.render_moving_cppn; DESIGN.md section 13, "Moving textures").  160 x 120 colour, two frames per sequence.

    python scripts/flow_truth.py [--samples 16] [--dense-levels L --dense-iters K] [--out profiles/flow_truth.txt]

Cases: one layer under a pure shift of 0.01, 0.03, 0.1, 0.3 and 1.0 pixels (a seeded direction per sample), and one two-layer case
under the source's default motion (shift <= 1.5 px, turn <= 0.02 rad, zoom within 1 %, a disc with a motion of its own in front).
Paths: the dense solve (eigen_dense_score's field, radius 7, eps 1e-2, over the pixels at least 7 from the border) and the fitness
path's sparse Lucas-Kanade vectors (Engine.flow) at their own corners, each against the true vector of its pixel.  Per case: the mean
and median endpoint error, the same of the zero field (the size of the motion), and of the true vectors under 0.3 px (what the
fitness keeps) the share each path also places under 0.3 px.  Samples whose first frame has fewer than 16 distinct byte values (a
flat texture: no flow can be found) are left out and counted.  With --dense-levels or --dense-iters above 1 every case gets a third
row, the dense stage's pyramidal, iterated solve (fitness.DenseFitness(levels=L, iters=K)) on the same frames and pixels.  These are
facts for DESIGN.md, not pass conditions."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, C, RADIUS, EPS, KEPT = 160, 120, 3, 7, 1e-2, 0.3
SHIFTS = (0.01, 0.03, 0.1, 0.3, 1.0)


def shift_case(src, shift, k, n):
    """describe(k, n) of a one-layer source with every motion replaced by a pure shift of `shift` pixels in the drawn direction"""
    from evolutionary_illusion_generator_amd.train import similarity_affines
    d = src.describe(k, n)
    rng = np.random.default_rng((src.seed, k, 1))
    for b in range(n):
        a0 = d["affine"][b, 0, 0]
        ang = rng.uniform(0.0, 2 * np.pi)
        d["affine"][b, :, 0], d["affine_inv"][b, :, 0] = similarity_affines(complex(a0[0], a0[3]), complex(a0[2], a0[5]), 1.0,
                                                                            shift * complex(np.cos(ang), np.sin(ang)), d["T"])
    return d


def measure(e, d, dense, iterated=None):
    import torch
    n, per = d["n"], C * H * W
    frames, flow, layer = e.render_moving_cppn(d["gb"], d["affine"], d["affine_inv"], flow=True, layer=True)
    torch.cuda.synchronize()
    truth = flow[:, 0].cpu().numpy()
    host = frames.cpu().numpy()
    live = np.array([len(np.unique(host[b, 0])) >= 16 for b in range(n)])
    p0 = int(frames.data_ptr())
    _, u = e.dense_score(p0, 2 * per, p0 + per, 2 * per, n, dense, flow=True)
    ui = None if iterated is None else e.dense_score(p0, 2 * per, p0 + per, 2 * per, n, iterated, flow=True)[1]
    vec = torch.zeros((n, e.K, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    e.flow(p0, 2 * per, p0 + per, 2 * per, n, vec, cnt)
    torch.cuda.synchronize()
    vec, cnt = vec.cpu().numpy().astype(np.float64), cnt.cpu().numpy()
    inner = (slice(None), slice(RADIUS, H - RADIUS), slice(RADIUS, W - RADIUS))
    de, dz, dt, du = [], [], [], []          # dense: error, zero-field error, true norm, solved norm
    ie, iu = [], []                          # the iterated solve, on the dense pixels
    se, sz, st, su = [], [], [], []          # sparse, at the corners
    for b in np.nonzero(live)[0]:
        de.append(np.hypot(*(u[b] - truth[b])[inner]).ravel())
        dt.append(np.hypot(*truth[b][inner]).ravel())
        du.append(np.hypot(*u[b][inner]).ravel())
        if ui is not None:
            ie.append(np.hypot(*(ui[b] - truth[b])[inner]).ravel())
            iu.append(np.hypot(*ui[b][inner]).ravel())
        v = vec[b, :cnt[b]]
        col, row = np.clip(np.rint(v[:, 0]).astype(int), 0, W - 1), np.clip(np.rint(v[:, 1]).astype(int), 0, H - 1)
        t = truth[b][:, row, col].T
        se.append(np.hypot(*(v[:, 2:] - t).T))
        st.append(np.hypot(*t.T))
        su.append(np.hypot(*v[:, 2:].T))
    cat = lambda x: np.concatenate(x) if x else np.zeros(0)
    de, dt, du, se, st, su = cat(de), cat(dt), cat(du), cat(se), cat(st), cat(su)

    def stats(err, true, got):
        if not err.size:
            return "no vectors"
        small = true < KEPT
        share = "%5.1f %%" % (100.0 * (got[small] < KEPT).mean()) if small.any() else "   -   "
        return "EPE mean %.4f median %.4f (zero field %.4f / %.4f); true < 0.3 px: %5.1f %%, of them also < 0.3 px: %s; %d vectors" % (
            err.mean(), np.median(err), true.mean(), np.median(true), 100.0 * small.mean(), share, err.size)
    return int(live.sum()), stats(de, dt, du), stats(se, st, su), float(layer.float().mean()), None if ui is None else stats(cat(ie), dt, cat(iu))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--dense-levels", type=int, default=1, help="pyramid levels of the third row's solve")
    ap.add_argument("--dense-iters", type=int, default=1, help="iterations per level of the third row's solve")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_truth.txt"))
    a = ap.parse_args()
    import torch
    from evolutionary_illusion_generator_amd import fitness, train
    from evolutionary_illusion_generator_amd.engine import Engine
    n = a.samples
    e = Engine(W, H, [C], n)
    dense = fitness.DenseFitness(train.FlowScore(), radius=RADIUS, eps=EPS)
    iterated = None
    if (a.dense_levels, a.dense_iters) != (1, 1):
        iterated = fitness.DenseFitness(train.FlowScore(), radius=RADIUS, eps=EPS, levels=a.dense_levels, iters=a.dense_iters)
        iterated.solve_on(W, H)
    one, two = train.MovingTextures(W, H, C, 2, layers=1, engine=e), train.MovingTextures(W, H, C, 2, layers=2, engine=e)
    lines = ["flow paths against the true flow of moving CPPN textures, %s, %d x %d colour, %d samples per case" % (torch.cuda.get_device_name(0), W, H, n),
             "dense: eigen_dense_score's field, radius %d, eps %g, pixels >= %d from the border; sparse: Engine.flow at its own corners (K = %d)" % (RADIUS, EPS, RADIUS, e.K)]
    if iterated is not None:
        lines.append("dense %d x %d: the same stage with %d pyramid levels and %d iterations per level (eigen_dense_score_iter), same frames, same pixels" % (
            a.dense_levels, a.dense_iters, a.dense_levels, a.dense_iters))
    lines.append("")
    cases = [("1 layer, shift %.2f px" % s, shift_case(one, s, 0, n)) for s in SHIFTS] + [("2 layers, default motion", two.describe(0, n))]
    for name, d in cases:
        live, dense_line, sparse_line, cover, iter_line = measure(e, d, dense, iterated)
        lines += ["%s (%d of %d samples are not flat%s)" % (name, live, n, "; layer 1 covers %.1f %% of the pixels" % (100 * cover) if d["L"] == 2 else ""),
                  "  dense   " + dense_line, "  sparse  " + sparse_line]
        if iter_line is not None:
            lines.append("  dense %d x %d  " % (a.dense_levels, a.dense_iters) + iter_line)
    e.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
