"""Shared by tests/test_dense_pyr_host.py and tests/test_gpu_dense_pyr.py ("The pyramidal, iterated solve"):
``dense_pyr_ref``, the numpy restatement of the dense stage's opt-in solve (include/eigen_engine.h eigen_dense_solve,
csrc/dense_pyr_kernels.h), operation for operation, and the cases of the two files.  numpy only, no GPU.

The semantics, restated:
  gray planes   I0, I1 of level 0 are what tdense_prep_kernel reads: tflow_gray of (float)byte / 255.0f, float64
  pyramid       level l + 1 is ((W_l + 1) / 2, (H_l + 1) / 2); 5 taps (1, 4, 6, 4, 1) / 16 centred on source index 2 i, reflect-101
                borders, along x first (at the source's height), then along y; one tap set is
                (((a + e) + 4.0 (b + d)) + 6.0 c) / 16.0; both images are reduced
  per level     Ix, Iy the normalised Scharr pair of the level's I0 (indices clamped); Gxx, Gxy, Gyy the truncated window sums of their
                products (rows first, then columns, offsets ascending, every sum started from its first term); a = Gxx + eps,
                c = Gyy + eps, b = Gxy, det = a c - b b: fixed over the iterations
  start         the coarsest level starts from the zero field (held as -0.0, so that the first step added to it is the step itself, bit
                for bit, a step of -0.0 included); else u_l(y, x) = 2.0 u_{l+1}(y >> 1, x >> 1)
  iteration     at pixel p with its own u = (ux, uy), over every q of the truncated window of p: d(q) = S(I1, qx + ux, qy + uy) - I0(q),
                bx = sum Ix(q) d(q), by = sum Iy(q) d(q) (per window row ascending in x from its first term, then the rows ascending in
                y from the first row), ux += -((c bx - b by) / det), uy += -((a by - b bx) / det)
  sampler S     x = x > 0 ? x : 0, x = x < W - 1 ? x : W - 1, likewise y; x0 = floor(x), x1 = min(x0 + 1, W - 1), fx = x - x0;
                top = v00 + fx (v01 - v00), bot = v10 + fx (v11 - v10), S = top + fy (bot - top)
At levels = 1, iters = 1 the field is today's single step bit for bit (`flow_obj_support.flow_stage_ref`)."""
import functools

import numpy as np

from tests import flow_obj_support as fs

PYR_KERNELS = ["tdense_gray_kernel", "tdense_pyrdown_kernel", "tdense_iter_kernel"]
MAX_LEVELS, MAX_ITERS, MIN_COARSE = 6, 32, 4
EPS = 1e-2


def gray_planes(img):
    """uint8 [B, C, H, W] -> float64 [B, H, W]: tflow_gray of (float)byte / 255.0f"""
    return fs._gray(fs.byte_reference(img))


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels - 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _reduce_last(a):
    """[..., n] -> [..., (n + 1) / 2]: the five taps about source index 2 i"""
    n = a.shape[-1]
    c = 2 * np.arange((n + 1) // 2)
    t = [a[..., _reflect(c + k, n)] for k in (-2, -1, 0, 1, 2)]
    return (((t[0] + t[4]) + 4.0 * (t[1] + t[3])) + 6.0 * t[2]) / 16.0


def pyr_down(a):
    """[B, H, W] -> [B, (H + 1) / 2, (W + 1) / 2]: along x first, then along y"""
    return np.swapaxes(_reduce_last(np.swapaxes(_reduce_last(a), -1, -2)), -1, -2)


def scharr(I0):
    H, W = I0.shape[-2:]
    ap = np.pad(I0, ((0, 0), (1, 1), (1, 1)), mode="edge")
    a = lambda dy, dx: ap[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    Ix = ((3.0 * (a(-1, 1) - a(-1, -1)) + 10.0 * (a(0, 1) - a(0, -1))) + 3.0 * (a(1, 1) - a(1, -1))) / 32.0
    Iy = ((3.0 * (a(1, -1) - a(-1, -1)) + 10.0 * (a(1, 0) - a(-1, 0))) + 3.0 * (a(1, 1) - a(-1, 1))) / 32.0
    return Ix, Iy


def sample(I1, x, y):
    """the sampler S on [B, H, W] planes at float64 coordinates [B, H, W]"""
    B, H, W = I1.shape
    x = np.where(x > 0.0, x, 0.0)
    x = np.where(x < W - 1.0, x, W - 1.0)
    y = np.where(y > 0.0, y, 0.0)
    y = np.where(y < H - 1.0, y, H - 1.0)
    xf, yf = np.floor(x), np.floor(y)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - xf, y - yf
    b = np.arange(B)[:, None, None]
    v00, v01, v10, v11 = I1[b, y0, x0], I1[b, y0, x1], I1[b, y1, x0], I1[b, y1, x1]
    top = v00 + fx * (v01 - v00)
    bot = v10 + fx * (v11 - v10)
    return top + fy * (bot - top)


def _iterate(I0, I1, Ix, Iy, a, b, c, det, ux, uy, r):
    """one iteration of every pixel: the window of p sampled at q + u(p)"""
    B, H, W = I0.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    bx = by = None
    rows_started = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        qy = ys + dy
        oky = (qy >= 0) & (qy < H)
        qyc = np.clip(qy, 0, H - 1)
        rx = ry = None
        started = np.zeros((H, W), bool)
        for dx in range(-r, r + 1):
            qx = xs + dx
            ok = oky & (qx >= 0) & (qx < W)
            qxc = np.clip(qx, 0, W - 1)
            d = sample(I1, qxc.astype(np.float64) + ux, qyc.astype(np.float64) + uy) - I0[:, qyc, qxc]
            tx, ty = Ix[:, qyc, qxc] * d, Iy[:, qyc, qxc] * d
            if rx is None:
                rx, ry = np.where(ok, tx, 0.0), np.where(ok, ty, 0.0)
            else:
                rx = np.where(ok, np.where(started, rx + tx, tx), rx)
                ry = np.where(ok, np.where(started, ry + ty, ty), ry)
            started = started | ok
        if bx is None:
            bx, by = np.where(started, rx, 0.0), np.where(started, ry, 0.0)
        else:
            bx = np.where(started, np.where(rows_started, bx + rx, rx), bx)
            by = np.where(started, np.where(rows_started, by + ry, ry), by)
        rows_started = rows_started | started
    return ux + -((c * bx - b * by) / det), uy + -((a * by - b * bx) / det)


def dense_pyr_ref(img0, img1, r, eps, levels=1, iters=1, all_levels=False):
    """uint8 [B, C, H, W] twice -> the field u of level 0 after its last iteration, float64 [B, 2, H, W] (all_levels: the list of the
    fields of every level, finest first)"""
    I0, I1 = [gray_planes(img0)], [gray_planes(img1)]
    for _ in range(levels - 1):
        I0.append(pyr_down(I0[-1]))
        I1.append(pyr_down(I1[-1]))
    fields, ux, uy = [], None, None
    for l in range(levels - 1, -1, -1):
        B, H, W = I0[l].shape
        if ux is None:
            ux, uy = np.full((B, H, W), -0.0), np.full((B, H, W), -0.0)
        else:
            yy, xx = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
            ux, uy = 2.0 * ux[:, yy, xx], 2.0 * uy[:, yy, xx]
        Ix, Iy = scharr(I0[l])
        Gxx, Gxy, Gyy = fs.window_sum(Ix * Ix, r), fs.window_sum(Ix * Iy, r), fs.window_sum(Iy * Iy, r)
        a, c, b = Gxx + eps, Gyy + eps, Gxy
        det = a * c - b * b
        for _ in range(iters):
            ux, uy = _iterate(I0[l], I1[l], Ix, Iy, a, b, c, det, ux, uy, r)
        fields.insert(0, np.stack([ux, uy], 1))
    return fields if all_levels else fields[0]


# ---- the accuracy cases (the issue's): one layer under the whole image, a pure shift
ACC_W, ACC_H, ACC_R, ACC_BORDER = 48, 32, 7, 7
ACC_SEEDS = (63, 76)
ACC_SHIFTS = ((0.5, -0.25), (1.25, -0.75), (2.5, 1.5))
ACC_CASES = [(seed, shift) for seed in ACC_SEEDS for shift in ACC_SHIFTS]
ACC_LEVELS, ACC_ITERS, ACC_BOUND = 2, 3, 0.5


@functools.lru_cache(maxsize=None)
def shift_case(w, h, c_dim, seed, shift):
    """(img0, img1 uint8 [1, C, h, w], the exact flow float64 [1, 2, h, w]) of one moving texture: `moving_support` builds and renders it"""
    from tests import moving_support as ms
    layer = (complex(0.04, 0.0), complex(0.5, -0.25), complex(1.0, 0.0), complex(*shift))
    desc = ms.build_case(w, h, c_dim, 2, [ms._genome(c_dim, seed)], [layer], 1)
    ref = ms.moving_ref(desc)
    return ref["frames"][:, 0], ref["frames"][:, 1], ref["flow"][:, 0]


def epe(u, truth, border=0):
    """the mean endpoint error over the pixels at least `border` from the image's edge"""
    d = u - truth
    e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    H, W = e.shape[-2:]
    return float(e[:, border:H - border, border:W - border].mean())


# ---- the GPU cases: (name, w, h, C, levels, iters, radius, genome seeds, shifts), one sample per seed.  The third sample of "48x32"
# moves by more than PYR_MARGIN pixels, so that level 0 reads taps beyond the staged patch (`taps_beyond_patch`).
TILE, PYR_MARGIN = 16, 4    # FLOW_TILE of csrc/flow_obj_kernels.h, PYR_MARGIN of csrc/dense_pyr_kernels.h
GPU_CASES = [("8x8", 8, 8, 1, 2, 2, 7, (2,), ((0.7, -0.4),)),
             ("20x15", 20, 15, 3, 3, 2, 7, (21, 23), ((2.5, 1.5), (-0.6, 0.5))),
             ("48x32", 48, 32, 3, 3, 3, 7, (63, 76, 63), ((2.5, 1.5), (1.25, -0.75), (5.5, -4.5))),
             ("16x12", 16, 12, 1, 1, 5, 7, (76, 13), ((0.25, -0.125), (0.5, 0.75))),
             ("40x24r16", 40, 24, 1, 2, 2, 16, (63,), ((1.25, -0.75),))]      # the largest radius: 100 KB of dynamic LDS, the launch's attribute


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """(img0, img1 uint8 [B, C, h, w], levels, iters, r, the restatement's field) of a GPU case, made once"""
    _, w, h, C, levels, iters, r, seeds, shifts = next(c for c in GPU_CASES if c[0] == name)
    pairs = [shift_case(w, h, C, seed, shift)[:2] for seed, shift in zip(seeds, shifts)]
    img0, img1 = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    want = dense_pyr_ref(img0, img1, r, EPS, levels, iters)
    want.setflags(write=False)
    return img0, img1, levels, iters, r, want


def taps_beyond_patch(u, r):
    """how many pixels of a level with the field u [B, 2, H, W] sample their window's far column or row inside the image but beyond
    the I1 patch of their tile (the tile's windows and PYR_MARGIN pixels around them): those taps come from global memory"""
    B, _, H, W = u.shape
    ys, xs = np.mgrid[0:H, 0:W]
    n = 0
    for coord, pos, size, t0 in ((u[:, 0], xs, W, xs // TILE * TILE), (u[:, 1], ys, H, ys // TILE * TILE)):
        far_hi = np.minimum(pos + r, size - 1) + coord          # the window's last column / row, displaced
        far_lo = np.maximum(pos - r, 0) + coord
        hi_edge, lo_edge = t0 + TILE - 1 + r + PYR_MARGIN, t0 - r - PYR_MARGIN
        n += int(((np.floor(far_hi) + 1 > hi_edge) & (far_hi < size - 1)).sum()) + int(((np.floor(far_lo) < lo_edge) & (far_lo > 0)).sum())
    return n


# ---- the scores of the GPU cases
LIMITS = dict(min_norm=1e-3, min_count=4)


def dense_for(structure, r, max_norm, levels, iters):
    from evolutionary_illusion_generator_amd import fitness
    return fitness.DenseFitness.for_structure(structure, radius=r, eps=EPS, max_norm=max_norm, levels=levels, iters=iters, **LIMITS)


def restatement_score(dense, h):
    """the Score / Bands / Free of tests/flow_score_support.py and tests/flow_struct_support.py of a DenseFitness"""
    from evolutionary_illusion_generator_amd import train
    from tests import flow_score_support as ss, flow_struct_support as st
    d = dense.score
    if isinstance(d, train.FlowScore):
        return ss.Score(d.max_norm, d.min_norm, 0.0, h / 2.0, d.weights[0], d.weights[1], d.min_count)
    if isinstance(d, train.BandsScore):
        return st.Bands(d.max_norm, d.min_norm, 0.0, (h / 4.0) * 2.0, d.min_count)
    return st.Free(d.max_norm, d.min_norm, d.max_distance, d.min_count, d.weights)


class Want:
    """what tests/test_gpu_dense_fitness.py's check_records reads of a restatement: the field and the score on it"""

    def __init__(self, u, sc, mask=None):
        from tests import flow_score_support as ss, flow_struct_support as st
        self.u = u
        self.score = ss.score_ref(u, mask, sc) if isinstance(sc, ss.Score) else st.struct_ref(u, mask, sc)


# ---- end to end: 48 x 32 colour, the genomes, weights and limits of tests/dense_fitness_support.py at 2 levels x 3 iterations.  max_norm
# per pairing: consecutive predictions move by tenths of a pixel, so the fitness's own 0.3 decides membership there; the input image
# against the second extension frame moves by several pixels once the solve follows the motion (median norms of 1 .. 20 on the oracle's
# frames), where 0.3 leaves no sample with min_count members and 3.0 leaves at least five of seven (tests/test_dense_pyr_host.py asserts it)
E2E_LEVELS, E2E_ITERS = 2, 3
E2E_MAX_NORM = {0: 0.3, 1: 3.0}     # dense_fitness_support.PAIR_POPULATION, PAIR_SINGLE


def e2e_dense(structure, pairing):
    from evolutionary_illusion_generator_amd import fitness
    from tests import dense_fitness_support as ds
    limits = dict(ds.E2E_LIMITS, max_norm=E2E_MAX_NORM[pairing])
    return fitness.DenseFitness.for_structure(structure, radius=ds.E2E_RADIUS, eps=EPS, levels=E2E_LEVELS, iters=E2E_ITERS, **limits)
