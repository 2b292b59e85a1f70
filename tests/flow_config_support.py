"""Shared by the flow-configuration and score-edge tests (tests/test_flow_config_host.py, tests/test_gpu_flow_config.py,
tests/test_gpu_score_edges.py): ONE table of the Lucas-Kanade and Farneback settings that `eigen_create` accepts, the settings just
outside every bound, the image generators of the flow tests, and the hand-built vector sets of the score kernels' edge cases.

Why a table: the flow configuration is public and validated ("Flow parameters"), and before this file only the defaults
had ever run.  The kernels are not indifferent to the numbers -- `lk_track_kernel` spreads win^2 taps over 64 lanes in up to four slots,
`mineig_kernel` sizes its LDS tile for block <= 9 and anchors even blocks at block / 2, `corner_select_kernel` has a path of its own for
min_distance < 1, the Farneback halos are sized for winsize 33 / poly_n 7 / a 39-tap blur.  tests/test_flow_config_host.py keeps the table
honest with the oracle alone (every entry changes the oracle's answer); tests/test_gpu_flow_config.py compares the kernels bit for bit.
Numpy only."""
import numpy as np

# ------------------------------------------------------------------------------------------------ image generators


def textured_pairs(rng, B, c, h, w):
    """Smooth random textures and a sub-pixel-shifted, slightly perturbed copy (uint8 planar)."""
    from numpy.fft import irfft2, rfft2
    a = rng.normal(0, 1, (B, c, h, w))
    fy, fx = np.meshgrid(np.fft.fftfreq(h), np.fft.rfftfreq(w), indexing="ij")
    filt = np.exp(-(fy ** 2 + fx ** 2) * 60.0)
    base = irfft2(rfft2(a) * filt, s=(h, w))
    sh = irfft2(rfft2(a) * filt * np.exp(-2j * np.pi * (fy * 0.12 + fx * -0.17)), s=(h, w))
    def q(v):
        v = (v - v.min()) / (v.max() - v.min())
        return (v * 255).astype(np.uint8)
    return q(base), q(sh)


def blocky_pairs(rng, B, c, h, w):
    """Blocky textures (4 x 4 pixel blocks, lightly smoothed: strong corners) and a copy moved by 0..5 px -- every fourth image by 0 / 13 /
    26 px -- with no, light or heavy noise (uint8 planar): multi-pixel motion (iteration cap, lost tracks), noise (the oscillation damping
    branch), corners hugging the border."""
    i0 = np.zeros((B, c, h, w), np.uint8)
    i1 = np.zeros((B, c, h, w), np.uint8)
    for b in range(B):
        base = rng.integers(0, 256, (c, h // 4 + 12, w // 4 + 12)).astype(np.float64)
        big = np.kron(base, np.ones((1, 4, 4)))[:, :h + 40, :w + 40]                    # blocky texture: strong corners
        big = (big + np.roll(big, 1, 1) + np.roll(big, 1, 2)) / 3.0
        sy, sx = rng.integers(0, 6, 2) if b % 4 else rng.integers(0, 3, 2) * 13                # 0..5 px, sometimes 13/26 px
        a = big[:, 30:30 + h, 30:30 + w]
        bimg = big[:, 30 - sy:30 - sy + h, 30 - sx:30 - sx + w]
        noise = rng.normal(0, [0, 3, 12][b % 3], a.shape)
        i0[b] = np.clip(a, 0, 255)
        i1[b] = np.clip(bimg + noise, 0, 255)
    return i0, i1


def faint_pairs(rng, B, c, h, w):
    """textured_pairs squeezed into 128 +- 4 grey levels: windows so weak that their smaller eigenvalue lies around the default min_eig_thr."""
    a, b = textured_pairs(rng, B, c, h, w)
    def f(v):
        return (128 + (v.astype(np.float64) - 128) * 4 / 128).round().astype(np.uint8)
    return f(a), f(b)


GENERATORS = {"blocky": blocky_pairs, "textured": textured_pairs, "faint": faint_pairs}


def entry_images(entry):
    """The image pairs of a table entry, uint8 [B, c, h, w] twice; the LAST image of the first frame is flat (no corner, no flow)."""
    w, h, c = entry["shape"]
    rng = np.random.default_rng(entry.get("seed", 77))
    i0, i1 = GENERATORS[entry.get("images", "blocky")](rng, entry["batch"], c, h, w)
    if entry["batch"] > 1:
        i0[-1] = 128
    return i0, i1


# ------------------------------------------------------------------------------------------------ Lucas-Kanade settings
LK_DEFAULTS = dict(max_corners=100, quality_level=0.3, min_distance=7.0, block_size=7, win=15, max_level=2, max_iter=10, epsilon=0.03,
                   min_eig_thr=1e-4)
LK_BOUNDS = dict(max_corners=(1, 128), win=(3, 16), block_size=(1, 9), max_level=(0, 3))
GRAY, COLOUR = (96, 72, 1), (44, 36, 3)   # the smallest shapes with three pyramid levels under the default window / with border windows everywhere
DENSE = dict(quality_level=0.01, min_distance=1.0)   # a stage on which more than 100 corners exist at 96 x 72


def lk_levels(w, h, win, max_level):
    """The pyramid levels that exist (buildOpticalFlowPyramid: a level exists only while both sizes stay above the window), as [(w, h), ...]."""
    lv = [(w, h)]
    for _ in range(max_level):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            break
        lv.append((w, h))
    return lv


def _lk(name, kw, path, shape=GRAY, batch=5, **flags):
    e = dict(name=name, kw=kw, shape=shape, batch=batch if shape == GRAY else 4, path=path, images="blocky", base={}, empty=False,
             clamp_twin=None, same_pyramid=False)
    e.update(flags)
    return e


# name, keywords (Engine(**kw) and LKParams(**kw)), the code path the entry reaches.  Flags: `base` the keywords of `kw` that only set the
# stage (the entry must differ from the defaults AND from its base), `empty` "corners" / "vectors" (exactly none), `clamp_twin` the
# keywords the host clamps the entry to (identical output), `same_pyramid` the entry's max_level builds the pyramid it would have
# without it (identical output to kw without max_level; exempt from differing there), `role` a census condition of the host test.
LK_CASES = [
    _lk("win3", dict(win=3), "9 taps: 55 idle lanes in slot 0, slots 1-3 empty; half = 1"),
    _lk("win4", dict(win=4), "16 taps, even window: half = 1.5, the window origin sits on half pixels", role="win"),
    _lk("win8", dict(win=8), "64 taps: exactly one per lane, slot 1 empty", role="win"),
    _lk("win9", dict(win=9), "81 taps: slot 1 holds 17", role="win"),
    _lk("win14", dict(win=14), "196 taps: the fourth slot starts (4 taps in it)", role="win"),
    _lk("win16", dict(win=16), "256 taps: every lane of every slot; level 2 is 24 x 18, just above the window", role="win"),
    _lk("block1", dict(block_size=1), "mineig: a 16 x 16 tile without halo, the box sum is one product"),
    _lk("block2", dict(block_size=2), "mineig: even block, anchor 1: window [-1, 0]"),
    _lk("block4", dict(block_size=4), "mineig: even block, anchor 2: window [-2, 1]"),
    _lk("block8", dict(block_size=8), "mineig: even block, anchor 4; 23 x 23 tile"),
    _lk("block9", dict(block_size=9), "mineig: EIG_MAXB, the 24 x 24 tile the LDS arrays are sized for"),
    _lk("level0", dict(max_level=0), "no pyramid: the 13 / 26 px motions are out of the window's reach"),
    _lk("level1", dict(max_level=1), "two levels"),
    _lk("level3_win5", dict(max_level=3, win=5), "FLOW_MAX_LEVELS - 1: level 3 of 96 x 72 is 12 x 9", base=dict(win=5)),
    _lk("corners1", dict(max_corners=1), "K = 1: one block of lk_track, compact_vectors with one live thread"),
    _lk("corners2", dict(max_corners=2), "K = 2"),
    _lk("corners64", dict(max_corners=64, **DENSE), "the greedy selection stops at max_corners with candidates left", base=DENSE),
    _lk("corners127", dict(max_corners=127, **DENSE), "K = 127: thread 126 of compact_vectors is the last with data", base=DENSE),
    _lk("corners128", dict(max_corners=128, **DENSE), "K = 128 = SCORE_T, all filled: thread 127 of compact_vectors carries data", base=DENSE, role="fill128"),
    _lk("mindist0", dict(min_distance=0.0), "corner_select: the min_distance < 1 path (the winner alone is removed)"),
    _lk("mindist0.5", dict(min_distance=0.5), "corner_select: the min_distance < 1 path with a non-zero value"),
    _lk("mindist1", dict(min_distance=1.0), "corner_select: the distance path at its lower edge (md^2 = 1 removes the winner alone)"),
    _lk("mindist7.5", dict(min_distance=7.5), "corner_select: a fractional md^2 = 56.25 between the integer distances 53 and 58"),
    _lk("mindist25", dict(min_distance=25.0), "corner_select: a handful of corners per image"),
    _lk("quality0.01", dict(quality_level=0.01), "nearly every local maximum is a candidate"),
    _lk("quality0.9", dict(quality_level=0.9), "a few candidates"),
    _lk("quality1", dict(quality_level=1.0), "nothing exceeds the threshold: no candidate, win == 0 on the first round", empty="corners"),
    _lk("iter0", dict(max_iter=0), "the iteration loop never runs: next = the initial guess at every level"),
    _lk("iter1", dict(max_iter=1), "one iteration: the j > 0 damping branch is unreachable"),
    _lk("iter2", dict(max_iter=2), "two iterations: the damping branch can fire only at j = 1"),
    _lk("iter30", dict(max_iter=30), "iterations 11 .. 30"),
    _lk("iter150", dict(max_iter=150), "the host clamps to 100", clamp_twin=dict(max_iter=100)),
    _lk("eps0", dict(epsilon=0.0), "only an exactly zero step ends the iteration early"),
    _lk("eps0.001", dict(epsilon=0.001), "a small epsilon: the iteration cap and the damping branch end most tracks"),
    _lk("eps0.3", dict(epsilon=0.3), "a large epsilon: most tracks stop after one or two steps"),
    _lk("eps20", dict(epsilon=20.0), "the host clamps to 10: every track stops after its first step", clamp_twin=dict(epsilon=10.0)),
    _lk("eigthr0", dict(min_eig_thr=0.0), "faint textures: no track is refused for a weak window (the default threshold refuses a sixth of them)", images="faint"),
    _lk("eigthr0.5", dict(min_eig_thr=0.5), "some tracks are lost at level 0, some survive", role="lose_some"),
    _lk("eigthr2", dict(min_eig_thr=2.0), "every track is lost: corners but no vector", empty="vectors"),
    _lk("combo_small", dict(win=5, block_size=3, max_level=3, max_iter=20), "small window, small block, four levels"),
    _lk("combo_even", dict(win=12, block_size=8, max_level=1, min_distance=0.5), "even window in three slots, even block, two levels, the < 1 path"),
    _lk("combo_full", dict(win=16, block_size=2, max_level=0, quality_level=0.05, max_corners=128), "all 256 taps on one level, even block, K = 128"),
    # the window and level entries once more at 44 x 36 colour: every window reaches over a border, gray conversion in front
    _lk("c_win3", dict(win=3), "44 x 36 colour: 9 taps", shape=COLOUR),
    _lk("c_win4", dict(win=4), "44 x 36 colour: even window", shape=COLOUR, role="win"),
    _lk("c_win8", dict(win=8), "44 x 36 colour: one tap per lane", shape=COLOUR, role="win"),
    _lk("c_win9", dict(win=9), "44 x 36 colour: second slot; level 2 (11 x 9) is refused by the height alone", shape=COLOUR, role="win"),
    _lk("c_win14", dict(win=14), "44 x 36 colour: fourth slot", shape=COLOUR, role="win"),
    _lk("c_win16", dict(win=16), "44 x 36 colour: 256 taps; level 1 is 22 x 18, the pyramid refuses level 2", shape=COLOUR, role="win"),
    _lk("c_level0", dict(max_level=0), "44 x 36 colour: no pyramid", shape=COLOUR),
    _lk("c_level1", dict(max_level=1), "44 x 36 colour: two levels -- what the default builds here too (level 2 would be 11 x 9)", shape=COLOUR, same_pyramid=True),
    _lk("c_level3_win5", dict(max_level=3, win=5), "44 x 36 colour: levels 22 x 18 and 11 x 9; 6 x 5 is refused by its height -- the pyramid of max_level 2", shape=COLOUR, same_pyramid=True),
]


def lk_params_kw(kw):
    """The keywords of oracle.LKParams for an entry's Engine keywords (the same names)."""
    return dict(kw)


# ------------------------------------------------------------------------------------------------ Farneback settings
FB_DEFAULTS = dict(fb_levels=3, fb_winsize=15, fb_iterations=3, fb_poly_n=5, fb_poly_sigma=1.2, fb_step=16, max_corners=100)


def _fb(name, kw, path, shape=(64, 64, 1), batch=2, **flags):
    e = dict(name=name, kw=kw, shape=shape, batch=batch, path=path, images="textured", seed=11)
    e.update(flags)
    return e


FB_CASES = [
    _fb("winsize1", dict(fb_winsize=1), "m = 0: the box sums are the pixel itself, no halo"),
    _fb("winsize3", dict(fb_winsize=3), "m = 1"),
    _fb("winsize33", dict(fb_winsize=33), "m = 16 = FB_MAX_WIN_R: the halo fb_box_h_solve_kernel's LDS rows are sized for; wider than half the 32-pixel level"),
    _fb("poly1", dict(fb_poly_n=1), "3-tap polynomial expansion"),
    _fb("poly2", dict(fb_poly_n=2), "5-tap polynomial expansion"),
    _fb("poly7", dict(fb_poly_n=7), "FB_MAX_POLY_N: the 46-column tile fb_polyexp_kernel's LDS is sized for"),
    _fb("sigma0", dict(fb_poly_sigma=0.0), "sigma < FLT_EPSILON: the n * 0.3 path of FarnebackPrepareGaussian"),
    _fb("sigma1.5", dict(fb_poly_sigma=1.5), "another applicability Gaussian"),
    _fb("fb_iter1", dict(fb_iterations=1), "no second update of the matrices"),
    _fb("fb_iter5", dict(fb_iterations=5), "five blur / solve rounds per level"),
    _fb("levels0", dict(fb_levels=0), "no pyramid: the 3-tap blur of level 0 only", shape=(64, 64, 3)),
    _fb("step8_k128", dict(fb_step=8, max_corners=128), "64 grid points in one round of fb_sample_kernel, K = 128"),
    _fb("step5_k7", dict(fb_step=5, max_corners=7), "the grid step grows 5 -> 25 until the vectors fit: 4 points"),
    _fb("levels4_512", dict(fb_levels=4), "512 x 512: pyramid level 4 is 32 x 32 under the 39-tap blur (FB_MAX_BLUR_R)", shape=(512, 512, 1), batch=1),
    _fb("levels4_520x264", dict(fb_levels=4, fb_winsize=21), "520 x 264: three levels are used, the coarsest 65 x 33 -- odd in both dimensions", shape=(520, 264, 1), batch=1),
]


def fb_params_kw(kw, K):
    """The keywords of oracle.FBParams for an entry's Engine keywords: the fb_ prefix dropped, max_corners -> max_vectors."""
    out = {k[3:]: v for k, v in kw.items() if k.startswith("fb_")}
    out["max_vectors"] = K
    return out


# ------------------------------------------------------------------------------------------------ settings eigen_create refuses
# (flow, keywords, (w, h, channels), the fragment of the message, the setting just inside that is accepted)
REFUSALS = [
    ("lk", dict(win=2), (32, 32, [1, 4]), "lk_win must be in 3..16", dict(win=3)),
    ("lk", dict(win=17), (32, 32, [1, 4]), "lk_win must be in 3..16", dict(win=16)),
    ("lk", dict(block_size=0), (32, 32, [1, 4]), "lk_block_size must be in 1..9", dict(block_size=1)),
    ("lk", dict(block_size=10), (32, 32, [1, 4]), "lk_block_size must be in 1..9", dict(block_size=9)),
    ("lk", dict(max_level=-1), (32, 32, [1, 4]), "lk_max_level must be in 0..3", dict(max_level=0)),
    ("lk", dict(max_level=4), (32, 32, [1, 4]), "lk_max_level must be in 0..3", dict(max_level=3)),
    ("lk", dict(max_corners=0), (32, 32, [1, 4]), "lk_max_corners must be in 1..128", dict(max_corners=1)),
    ("lk", dict(max_corners=129), (32, 32, [1, 4]), "lk_max_corners must be in 1..128", dict(max_corners=128)),
    ("farneback", dict(fb_winsize=0), (64, 64, [1, 4]), "fb_winsize must be odd and <= 33", dict(fb_winsize=1)),
    ("farneback", dict(fb_winsize=4), (64, 64, [1, 4]), "fb_winsize must be odd and <= 33", dict(fb_winsize=5)),
    ("farneback", dict(fb_winsize=35), (64, 64, [1, 4]), "fb_winsize must be odd and <= 33", dict(fb_winsize=33)),
    ("farneback", dict(fb_poly_n=0), (64, 64, [1, 4]), "fb_poly_n must be in 1..7", dict(fb_poly_n=1)),
    ("farneback", dict(fb_poly_n=8), (64, 64, [1, 4]), "fb_poly_n must be in 1..7", dict(fb_poly_n=7)),
    ("farneback", dict(fb_levels=-1), (64, 64, [1, 4]), "fb_levels must be in 0..4", dict(fb_levels=0)),
    ("farneback", dict(fb_levels=5), (64, 64, [1, 4]), "fb_levels must be in 0..4", dict(fb_levels=4)),
    ("farneback", dict(fb_iterations=0), (64, 64, [1, 4]), "fb_iterations >= 1 and fb_step >= 1 required", dict(fb_iterations=1)),
    ("farneback", dict(fb_step=0), (64, 64, [1, 4]), "fb_iterations >= 1 and fb_step >= 1 required", dict(fb_step=1)),
    # 130 x 130 with two levels allowed: 65 and 32.5 are both >= 32, so two levels are used and 4 must divide the size; with one level 2 does
    ("farneback", dict(fb_levels=2), (130, 130, [1, 4]), "2 pyramid levels needs an image divisible by 4", dict(fb_levels=1)),
]


def fb_levels_used(w, h, levels):
    """calcOpticalFlowFarneback: no pyramid level below 32 pixels."""
    k, scale = 0, 1.0
    while k < levels:
        scale *= 0.5
        if w * scale < 32 or h * scale < 32:
            break
        k += 1
    return k


# ------------------------------------------------------------------------------------------------ score edge cases
# Vector sets built by hand for the score kernels (csrc/score_kernels.h) -- each hits a branch by construction -- at the geometries
# (w, h, K) of SCORE_GEOMETRIES.  Non-finite input vectors stay out of contract and are not here.
SCORE_GEOMETRIES = [(160, 120, 100), (64, 64, 128), (100, 90, 100), (44, 36, 1)]
F32 = np.float32


def below(x):
    """the largest float32 below the float64 x"""
    f = F32(x)
    return f if float(f) < x else np.nextafter(f, F32(-np.inf))


def above(x):
    """the smallest float32 above the float64 x"""
    f = F32(x)
    return f if float(f) > x else np.nextafter(f, F32(np.inf))


def _ring(n, w, h, radius, dx, dy, phase=0.0):
    """n vectors on a circle of `radius` around the image centre (positions rounded to whole pixels inside the image), displacement (dx, dy)
    rotated with the position (a rotating field) -- float32 [n, 4]."""
    v = np.zeros((n, 4), F32)
    for i in range(n):
        a = phase + 2 * np.pi * i / n
        x = min(max(round(w / 2 + radius * np.cos(a)), 0), w - 1)
        y = min(max(round(h / 2 + radius * np.sin(a)), 0), h - 1)
        v[i] = (x, y, dx * np.cos(a) - dy * np.sin(a), dx * np.sin(a) + dy * np.cos(a))
    return v


def _grid(n, w, h, dx, dy, jitter=0.0):
    """n vectors on a regular grid over the image, displacement (dx, dy) with a deterministic per-vector change of `jitter`."""
    v = np.zeros((n, 4), F32)
    cols = max(1, int(np.ceil(np.sqrt(n * w / h))))
    rows = int(np.ceil(n / cols))
    for i in range(n):
        r, c = divmod(i, cols)
        v[i] = (int((c + 0.5) * w / cols), int((r + 0.5) * h / rows), dx + jitter * ((i * 7) % 5 - 2), dy + jitter * ((i * 3) % 7 - 3))
    return v


def score_cases(w, h, K):
    """[(name, vectors float32 [n, 4], count, branches it is built for)] for one geometry.  count may exceed K (the kernels clamp it); n <= K.
    The branch names are checked against the ORACLE's intermediate counts by `score_census` -- not against the kernel."""
    cases = []

    def add(name, v, count=None):
        v = np.asarray(v, F32).reshape(-1, 4)[:K]
        cases.append((name, v, len(v) if count is None else count))

    big = K >= 32
    add("empty", np.zeros((0, 4)))                                           # the sentinel [[0, 0, -1000, 0]]: every structure 0
    add("one", [[w // 3, h // 3, 0.05, -0.02]])                              # K = 1 runs this one and `empty`, the zero vector and the limits
    add("zero_vector_only", [[w // 4, h // 4, 0.0, 0.0]])                    # an exactly zero displacement: 0 / 0 in every normalisation
    # norm exactly at the limit: a float32 cannot equal 0.15 / 0.3 / 0.4, so the largest float32 below and the smallest above are used
    for lim in (0.15, 0.3, 0.4):
        add("norm_below_%g" % lim, [[w // 2 - 3, h // 5, below(lim), 0.0]])
        add("norm_above_%g" % lim, [[w // 2 - 3, h // 5, above(lim), 0.0]])
    if K < 2:
        return cases
    # Bands: y == lim1 = (h / 4) * 2 is kept, y == middle = int(lim1 / 2) is the first row of the lower half; h / 4 need not be an integer
    lim1 = (h / 4) * 2
    mid = int(lim1 / 2)
    rows = [0, mid - 1, mid, mid + 1, int(lim1), min(int(lim1) + 1, h - 1), h - 1]
    add("bands_rows", [[5 + 3 * i, y, 0.04 + 0.01 * i, 0.02 - 0.01 * i] for i, y in enumerate(rows)])
    add("bands_all_below_lim1", [[7, min(int(lim1) + 1, h - 1), 0.05, 0.05], [9, h - 1, -0.05, 0.02]])   # every vector outside [0, lim1]: 0
    # a zero displacement among ordinary vectors: inside the Circles radius and outside it (the corner of the image is farther than h / 2 from the centre)
    ordinary = _grid(min(K - 1, 30), w, h, 0.06, 0.03, jitter=0.01)
    add("zero_inside_radius", np.concatenate([ordinary, [[w // 2 + 2, h // 2 + 1, 0.0, 0.0]]]))
    add("zero_outside_radius", np.concatenate([ordinary, [[0, 0, 0.0, 0.0]]]))
    # Free: 14 / 15 / 16 kept vectors (min(len, 15) / 15)
    for n in (14, 15, 16):
        if n <= K:
            add("free_%d" % n, _grid(n, w, h, 0.1, -0.05, jitter=0.02))
    # Free: pairs nearer and farther than 100 px (f clamps to 1, `close` drops to 0) and exactly 100 px apart where the width allows it
    far = [[0, 2, 0.1, 0.02], [3, 1, -0.05, 0.1], [w - 1, h - 1, 0.02, -0.1], [w - 2, 4, 0.08, 0.08]]
    if w > 101:
        far += [[100, 2, 0.05, 0.01], [103, 1, 0.03, 0.05]]                  # (0, 2) -> (100, 2): exactly 100 px; (3, 1) -> (103, 1) too
    add("free_near_far", far)
    if not big:
        return cases
    # Circles: m == 24 vs 25 AFTER the plausibility filter: 30 vectors of which 6 / 5 have a norm above 0.3
    ring = _ring(30, w, h, h / 4, 0.0, 0.1)
    for kept in (24, 25):
        v = ring.copy()
        v[:30 - kept, 2:] = (above(0.3), 0.0)
        add("circles_kept_%d" % kept, v)
    # Circles: fewer than two vectors inside the radius (cnt < 2: rotation term 0, strength still counted): all but cnt in the far corners
    for cnt in (0, 1, 2):
        corners = [[(i % 2) * (w - 1), ((i // 2) % 2) * (h - 1), 0.1 + 0.005 * i, 0.05] for i in range(26)]
        inside = [[w // 2 + 3 + i, h // 2 - 2, 0.1, -0.1] for i in range(cnt)]
        add("circles_inside_%d" % cnt, corners + inside)
    # Circles: a point exactly at the image centre (dist == 0 is dropped)
    add("circles_centre_point", np.concatenate([_ring(27, w, h, h / 5, 0.02, 0.12), [[w / 2, h / 2, 0.1, 0.1]]]))
    # Circles: a point exactly ON the radius (dist == h / 2 is kept)
    add("circles_on_radius", np.concatenate([_ring(27, w, h, h / 6, 0.0, 0.15, phase=0.3), [[w / 2, 0, 0.1, 0.0], [w / 2 - h / 2, h / 2, 0.0, 0.1]]]))
    # counts[b] > K: the kernel clamps to K; a full K (every thread of score_kernel with data)
    full = _grid(K, w, h, 0.05, 0.08, jitter=0.01)
    add("full_K", full)
    add("count_above_K", full, count=K + 7)
    add("rotating_field", _ring(min(K, 60), w, h, h / 3, 0.0, 0.12))
    add("mixed_norms", _grid(min(K, 48), w, h, 0.09, 0.0, jitter=0.06))       # norms on both sides of all three limits
    return cases


def io_cases(w, h, K):
    """Vector sets for structure 4 (inside_outside_kernel): the general ones of score_cases (no filter there, so the filter-specific ones are
    left out), plus vectors at x = w - 1, on multiples of the cell step w / 5 (fractional when 5 does not divide w) and on both of its sides."""
    cases = [c for c in score_cases(w, h, K) if not c[0].startswith(("norm_", "circles_kept", "bands_all"))]
    step = w / 5
    border = []
    for k in range(1, 5):
        x = k * step
        for xx in (np.floor(x), np.ceil(x), below(x), above(x)):
            border.append([xx, min(np.floor(k * step), h - 1), 0.1 * k, -0.07 * k])
    border += [[w - 1, h - 1, 0.2, 0.1], [w - 1, 0, -0.1, 0.1], [0, h - 1, 0.1, 0.3]]
    cases.append(("io_cell_borders", np.asarray(border, F32)[:K], min(len(border), K)))
    cases.append(("io_one_cell", np.asarray([[1, 1, 0.3, 0.1], [2, 1, -0.2, 0.1], [1, 2, 0.1, 0.1]], F32)[:K], min(3, K)))
    cases.append(("io_opposed_neighbours", np.asarray([[1, 1, 1.0, 0.0], [int(step) + 1, 1, -1.0, 0.0], [1, int(step) + 1, 1.0, 0.1],
                                                      [int(step) + 1, int(step) + 1, -1.0, 0.2]], F32)[:K], min(4, K)))
    return cases


def score_census(structure, v, w, h):
    """The branches a vector set takes, decided from the ORACLE's intermediate counts (oracle/scores.py restated count by count): a set of names."""
    taken = set()
    v = np.asarray(v, np.float64).reshape(-1, 4)
    if len(v) == 0:
        taken.add("sentinel")
        v = np.array([[0.0, 0.0, -1000.0, 0.0]])
    limit = {0: 0.15, 1: 0.3, 2: 0.4, 3: 0.3}[structure]
    norm = np.sqrt(v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3])
    good = v[~(norm > limit)]
    gnorm = norm[~(norm > limit)]
    m = len(good)
    if m < len(v):
        taken.add("filtered_some")
    if m == 0:
        taken.add("filtered_all")
        return taken
    zero = gnorm == 0
    if zero.any():
        taken.add("zero_vector_kept")
    if structure in (1, 3):
        taken.add("m_eq_24" if m == 24 else "m_eq_25" if m == 25 else "m_le_24" if m < 24 else "m_gt_25")
        if m > 24:
            cx, cy = good[:, 0] - w / 2, good[:, 1] - h / 2
            dist = np.sqrt(cx * cx + cy * cy)
            keep = ~((dist > h / 2) | (dist == 0))
            taken.add("inside_%s" % ("0" if keep.sum() == 0 else "1" if keep.sum() == 1 else "ge2"))
            if (dist == 0).any():
                taken.add("dist_eq_0")
            if (dist == h / 2).any():
                taken.add("dist_eq_radius")
            if (zero & keep).any():
                taken.add("zero_inside_radius")
            if (zero & ~keep).any() and not (zero & keep).any():
                taken.add("zero_outside_radius")
    elif structure == 2:
        taken.add("free_m_%s" % ("lt15" if m < 15 else "eq15" if m == 15 else "gt15"))
        if m == 14:
            taken.add("free_m_eq14")
        if m == 16:
            taken.add("free_m_eq16")
        d2 = (good[:, None, 0] - good[None, :, 0]) ** 2 + (good[:, None, 1] - good[None, :, 1]) ** 2
        off = ~np.eye(m, dtype=bool)
        if (d2[off] < 1e4).any():
            taken.add("pair_near")
        if (d2[off] > 1e4).any():
            taken.add("pair_far")
        if (d2[off] == 1e4).any():
            taken.add("pair_eq_100")
    else:
        lim1 = (h / 4) * 2
        mid = int(lim1 / 2)
        if h % 4:
            taken.add("h4_fractional")
        y = good[:, 1]
        keep = ~((y < 0) | (y > lim1))
        if keep.sum() == 0:
            taken.add("bands_none_in_range")
        if (y == lim1).any():
            taken.add("y_eq_lim1")
        if (y == mid).any():
            taken.add("y_eq_middle")
        if (y > lim1).any():
            taken.add("y_gt_lim1")
    return taken


# every branch the file of score tests must have taken, per structure family (union over geometries and cases)
SCORE_BRANCHES = {
    0: {"sentinel", "filtered_some", "filtered_all", "zero_vector_kept", "h4_fractional", "bands_none_in_range", "y_eq_lim1", "y_eq_middle", "y_gt_lim1"},
    1: {"sentinel", "filtered_some", "filtered_all", "m_eq_24", "m_eq_25", "m_le_24", "m_gt_25", "inside_0", "inside_1", "inside_ge2", "dist_eq_0",
        "dist_eq_radius", "zero_inside_radius", "zero_outside_radius"},
    2: {"sentinel", "filtered_some", "filtered_all", "zero_vector_kept", "free_m_eq14", "free_m_eq15", "free_m_eq16", "pair_near", "pair_far", "pair_eq_100"},
}
SCORE_BRANCHES[3] = SCORE_BRANCHES[1]


def score_table():
    """[(geometry, structure, name, vectors, count, oracle score, branches)] over every geometry, structure 0..3 and case"""
    from oracle import scores
    rows = []
    for (w, h, K) in SCORE_GEOMETRIES:
        for name, v, cnt in score_cases(w, h, K):
            for s in (0, 1, 2, 3):
                used = v[:min(cnt, K)].astype(np.float64)
                rows.append(((w, h, K), s, name, v, cnt, scores.fitness_from_vectors(s, used, w, h), score_census(s, used, w, h)))
    return rows


def check_score_census(rows):
    """the conditions on the whole file of score cases: every listed branch taken, >= 3 NaN, >= 3 exactly 0, at least half finite and non-zero"""
    for s in (0, 1, 2, 3):
        taken = set().union(*[r[6] for r in rows if r[1] == s])
        assert SCORE_BRANCHES[s] <= taken, "structure %d: branches never taken: %s" % (s, sorted(SCORE_BRANCHES[s] - taken))
    ref = np.array([r[5] for r in rows])
    n_nan, n_zero, n_live = int(np.isnan(ref).sum()), int((ref == 0).sum()), int((np.isfinite(ref) & (ref != 0)).sum())
    assert n_nan >= 3 and n_zero >= 3 and 2 * n_live >= len(ref), (n_nan, n_zero, n_live, len(ref))
    return n_nan, n_zero, n_live
