"""Shared by tests/test_cppn_edge_host.py and tests/test_gpu_cppn_edges.py: the edge cases of the CPPN stage (csrc/cppn_kernel.h, its raw
float64 mode 3, csrc/cppn_grad_kernel.h; DESIGN.md section 4 and section 13, "CPPN parameter gradients").  numpy and torch only, no GPU.

  A. ``probe()``: one float64 plane that reaches every branch of csrc/det_math64.h (subnormal results of ldexp, the +-746 / 710 clamps,
     overflow, the 0.625 switch and the 40 cap of tanh, the eight octants of the sine reduction up to the 1.073741824e9 cut, +-inf, NaN),
     ``activation_genome()``: seven output nodes, one per activation, each reading the plane alone, and ``act_reference``: cppn_act
     spelled with oracle.detmath64.  ``long_double_figures`` measures oracle.detmath64 against np.longdouble.
  B. ``extreme_planes()``: three 24 x 16 planes sprinkled with non-finite and huge values and the two sides of every wrap point of the
     uint8 quantisation, with the h, s, v renderer's own edges in plane 0, and two genomes that copy / scale them.
  C. ``big_genome(name)``: synth genomes whose [node][thread] columns need 64 KB ... 160 KiB of LDS, and one above; ``cppn_lds`` restates
     the host's sizing (csrc/eigen_engine.hip) and ``BANDS`` pins where each lands.
  D. ``derivative_genome()`` / ``derivative_planes()``: abs and relu at a pre-activation of exactly +-0, sigmoid, tanh and gauss saturated
     to exactly 1, +-1 and 0, sin at |z| ~ 1e3."""
import functools

import numpy as np

from evolutionary_illusion_generator_amd import synth
from evolutionary_illusion_generator_amd.genome import flatten_genome
from oracle import detmath64 as dm
from tests import cppn_grad_support as G

ACTIVATIONS = ("sigmoid", "tanh", "abs", "gauss", "identity", "sin", "relu")   # genome.ACT_IDS order: cppn_act's cases 0..6
SIN_CUT = 1.073741824e9
PI4 = np.pi / 4


# =========================================================================================== A. the activation probe
def _around(values, ulps=3):
    """every value with its ``ulps`` np.nextafter neighbours on both sides"""
    out = []
    for v in np.asarray(values, np.float64).ravel():
        lo = hi = v
        out.append(v)
        for _ in range(ulps):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            out += [lo, hi]
    return np.asarray(out, np.float64)


def _preimages(t):
    """t and the leaf values that reach it behind the factors cppn_act applies first: 5 x (sigmoid; its exp sees -5 x), 2.5 x (tanh)
    and -5 x^2 (gauss)"""
    t = float(t)
    out = [t, -t, t / 5.0, -t / 5.0, t / 2.5, -t / 2.5]
    r = np.sqrt(abs(t) / 5.0)
    return out + [r, -r]


# the thresholds of csrc/det_math64.h: the switch and the cap of tanh (and the 20 whose double is the 40), the first subnormal result,
# the last non-zero result, the first overflow, the clamps of exp, the cut of sin
THRESHOLDS = (0.625, 40.0, 20.0, -745.14, -745.1332191019411, -708.4, -708.3964185322641, 709.78, 709.782712893384, 710.0, 746.0, SIN_CUT)
SPECIALS = (0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308,
            np.inf, -np.inf, np.nan)
N_PROBE = 128 * 1100 + 1       # 140 801: 1100 full render blocks and one with a single live lane; probe(N_PROBE - 1) is its first 1100 blocks


@functools.lru_cache(maxsize=None)
def _probe_full():
    rng = np.random.default_rng(20240607)
    parts = [np.asarray(SPECIALS, np.float64)]
    thr = [p for t in THRESHOLDS for p in _preimages(t)]
    parts.append(_around(thr, 4))                                   # the factors round, so a few neighbours on each side
    # multiples of pi / 4: every small one, powers of two and their neighbours, and 600 drawn log-uniformly up to the cut
    m = np.concatenate([np.arange(0, 65), [2 ** k + d for k in range(7, 31) for d in (-1, 0, 1)],
                        np.floor(np.exp(rng.uniform(np.log(64.0), np.log(SIN_CUT / PI4), 600)))]).astype(np.float64)
    m = m[m * PI4 <= SIN_CUT * 1.0000001]
    mult = _around(m * PI4, 2)
    parts += [mult, -mult]
    # the dense ranges: the (int) conversion of det_sin sees every y mod 16 = 0 .. 15 from them, below and above 1e6
    parts.append(rng.normal(0.0, 1.0, 8192))
    parts.append(rng.uniform(-760.0, 720.0, 16384))
    for lo, hi in ((0.0, 8.0), (8.0, 1e3), (1e3, 1e6), (1e6, SIN_CUT)):
        u = rng.uniform(lo, hi, 2 * 12288)
        parts.append(np.where(np.arange(u.size) % 2 == 0, u, -u))
    have = sum(p.size for p in parts)
    assert have < N_PROBE - 4096, have
    parts.append(rng.normal(0.0, 3.0, N_PROBE - have))              # filled up with ordinary values: the last lane is one of them
    x = np.concatenate(parts)
    assert x.shape == (N_PROBE,) and np.isfinite(x[-1]) and abs(x[-1]) < 100
    x.setflags(write=False)
    return x


def probe(n=N_PROBE):
    """the first n values of the probe plane (read-only); every special value and threshold lies in its first few thousand"""
    assert 8192 <= n <= N_PROBE
    return _probe_full()[:n]


PROBE_LENGTHS = (N_PROBE - 1, N_PROBE)     # a multiple of 128; a ragged last block with one live lane


def activation_genome(key=300):
    """Output k applies activation k of cppn_act to leaf x alone: weight 1, response 1, bias -0.0, so that pre + bias is x bit for bit
    (x + -0.0 == x for every x, -0.0 included)."""
    nodes = {k: (a, -0.0, 1.0) for k, a in enumerate(ACTIVATIONS)}
    return G.build_genome(key, nodes, [(-1, k, 1.0, True) for k in range(len(ACTIVATIONS))])


def activation_config():
    return synth.make_config(2, len(ACTIVATIONS))


def act_reference(x):
    """[7][N]: cppn_act(k, x) as csrc/cppn_kernel.h spells it, over oracle.detmath64"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([dm.det_sigmoid(5.0 * x), dm.det_tanh(2.5 * x), np.abs(x), dm.det_exp(-5.0 * (x * x)), x, dm.det_sin(x),
                         np.where((x > 0.0) | np.isnan(x), x, 0.0)])


def sin_octant(x):
    """det_sin's reduction restated: (j = y mod 16 & 7 before the bump, whether the bump ran, j after it) for finite |x| <= the cut"""
    ax = np.abs(np.asarray(x, np.float64))
    y = np.floor(ax * dm.FOPI)
    z = y - np.ldexp(np.floor(np.ldexp(y, -4)), 4)
    j = z.astype(np.int32)
    odd = (j & 1) == 1
    return j & 7, odd, np.where(odd, j + 1, j) & 7


# ---- oracle.detmath64 against np.longdouble (the x87 80-bit format: 64 bits of significand, libm's expl / tanhl / sinl behind it).
# The four figures below are what tests/test_cppn_edge_host.py::test_detmath64_is_within_twice_its_measured_distance_from_long_double
# prints for probe() (``long_double_figures(probe())``), rounded up to two digits; the test asserts TWICE each, the room for the last-ulp
# variation of the platform's long-double libm.  exp and tanh in ulps of the float64 result, sin absolute, sigmoid relative.
MEASURED_EXP_ULP = 0.84       # exp on -708 < x < 709.7 (normal results)
MEASURED_TANH_ULP = 1.25      # tanh on finite x != 0
MEASURED_SIN_ABS = 1.7e-16       # sin on |x| <= 1.073741824e9
MEASURED_SIGMOID_REL = 2.1e-16   # 1 / (1 + exp(-z)) on -700 < z < 40
LONG_DOUBLE_SLACK = 2.0


def _ulps(got, ref):
    r64 = ref.astype(np.float64)
    return np.abs(got.astype(np.longdouble) - ref) / np.spacing(np.abs(r64)).astype(np.longdouble)


def long_double_figures(x):
    """dict(exp_ulp, tanh_ulp, sin_abs, sigmoid_rel) of oracle.detmath64 over the finite part of x, each on the domain named above"""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not wider than float64 on this platform"
    x = np.asarray(x, np.float64)
    x = x[np.isfinite(x)]
    L = lambda a: a.astype(np.longdouble)
    xe = x[(x > -708.0) & (x < 709.7)]
    xt = x[x != 0.0]
    xs = x[np.abs(x) <= SIN_CUT]
    xg = x[(x > -700.0) & (x < 40.0)]
    with np.errstate(all="ignore"):
        sig_ref = 1.0 / (1.0 + np.exp(-L(xg)))
        return dict(exp_ulp=float(_ulps(dm.det_exp(xe), np.exp(L(xe))).max()), tanh_ulp=float(_ulps(dm.det_tanh(xt), np.tanh(L(xt))).max()),
                    sin_abs=float(np.abs(L(dm.det_sin(xs)) - np.sin(L(xs))).max()),
                    sigmoid_rel=float((np.abs(L(dm.det_sigmoid(xg)) - sig_ref) / sig_ref).max()))


# =========================================================================================== B. extreme values through every renderer
EXT_W, EXT_H = 24, 16
T31 = 2147483648.0
WRAP_POINTS = (T31 / 255.0, -T31 / 255.0, T31 / 4.0, -T31 / 4.0, 256.0 / 255.0, -1.0 / 255.0)      # v * 255 or v * 4 at +-2^31, 256, -1
GENERAL = (np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, -0.0)
ROUNDED = (0.5, 1.5, 2.5, -0.5, 0.4999999999999999, 8421504.25, 8421505.25, -8421504.25, -8421505.25)   # rint: ties to even, +-2^31 / 255 after it
SEXTANTS = tuple(range(-7, 8))
T53 = 9007199254740992.0


def _general_values():
    return np.concatenate([np.asarray(GENERAL, np.float64), _around(WRAP_POINTS, 2), np.asarray(ROUNDED, np.float64)])


def _hue_values():
    """h with trunc(6 h) = -7 .. 7 (0 from both sides), 6 h on both sides of +-2^53"""
    six = [(k + (0.3 if k >= 0 else -0.3)) / 6.0 for k in SEXTANTS] + [-0.05]
    big = _around([T53 / 6.0], 3)
    return np.concatenate([np.asarray(six, np.float64), big, -big])


@functools.lru_cache(maxsize=None)
def extreme_planes():
    """(planes [3][384], regions): plane 0 is x (and h), plane 1 y (and s), plane 2 the third leaf (and v).  regions: name -> slice of
    pixels.  "p0" / "p1" / "p2": that plane holds the general values, the other two ordinary ones; "hue": plane 0 holds the hue values;
    "s0": s is exactly 0 under ordinary and special h; "bg": plane 0 is -1, the others hold the general values; every other pixel
    ("rest") is ordinary: uniform on [-0.2, 1.2], with 1.0 and its two neighbours among them."""
    rng = np.random.default_rng(77)
    n = EXT_W * EXT_H
    planes = rng.uniform(-0.2, 1.2, (3, n))
    planes[1] = rng.uniform(0.05, 1.0, n)            # s: ordinary and not zero
    planes[2] = rng.uniform(0.05, 1.2, n)            # v
    gen, hue = _general_values(), _hue_values()
    regions, at = {}, 0

    def take(name, count):
        nonlocal at
        regions[name] = slice(at, at + count)
        at += count
        return regions[name]

    for c in range(3):
        planes[c, take("p%d" % c, gen.size)] = gen
    planes[0, take("hue", hue.size)] = hue
    s0 = take("s0", 8)
    planes[1, s0] = 0.0
    planes[0, s0] = [0.3, -0.4, np.nan, np.inf, 1e300, 1.9, -1.2, 0.0]
    bg = take("bg", 24)
    planes[0, bg] = -1.0
    planes[1, bg] = np.resize(gen, 24)
    planes[2, bg] = np.resize(gen[::-1], 24)
    rest = take("rest", n - at)
    assert rest.stop - rest.start >= 100
    planes[:, rest.start:rest.start + 3] = np.asarray([1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)])
    assert not (planes[0, :bg.start] == -1.0).any() and not (planes[0, bg.stop:] == -1.0).any()
    planes.setflags(write=False)
    return planes, regions


def extreme_config():
    return synth.make_config(3, 3)


def copy_genome(key=310):
    """three identity outputs that copy the three planes bit for bit: weight 1, response 1, bias -0.0"""
    return G.build_genome(key, {k: ("identity", -0.0, 1.0) for k in range(3)}, [(-1 - k, k, 1.0, True) for k in range(3)])


def scale_genome(key=311):
    """identity outputs whose responses and biases carry ordinary planes to the wrap points: 2^31 / 255 times plane 0 (its 1.0 and the
    two neighbours straddle 2^31 after the * 255), 2 * 2^31 / 255 times plane 1 through a weight of 0.5 and a response of 4 * 2^31 / 255
    (plane 1 is uniform on [0.05, 1]: 2^31 is crossed at 0.5), and 256 / 255 - plane 2 (bias and a negative weight)"""
    nodes = {0: ("identity", -0.0, T31 / 255.0), 1: ("identity", 0.0, 4.0 * T31 / 255.0), 2: ("identity", 256.0 / 255.0, 1.0)}
    return G.build_genome(key, nodes, [(-1, 0, 1.0, True), (-2, 1, 0.5, True), (-3, 2, -1.0, True)])


# (c_dim, gradient): colour and gray, the palette, the rounded gray, h,s,v; each at bg 0 and 1
RENDERERS = ((3, 1), (1, 1), (3, 0), (1, 0), (3, 2))
RENDER_CASES = tuple((c, g, bg) for (c, g) in RENDERERS for bg in (0, 1))


def extreme_reference(genome, c_dim, gradient, bg):
    """oracle.cppn.render of `genome` over extreme_planes(): uint8 [c_dim][H][W]"""
    from oracle import cppn
    planes, _ = extreme_planes()
    with np.errstate(all="ignore"):
        img = cppn.render({"x_mat": planes[0], "y_mat": planes[1]}, genome, extreme_config(), c_dim, EXT_W, EXT_H, bg=bg, gradient=gradient,
                          extra_leaves=(planes[2],))
    return np.ascontiguousarray(img.transpose(2, 0, 1) if img.ndim == 3 else img[None])


# =========================================================================================== C. genomes from 64 KB to 160 KiB of LDS
RENDER_THREADS, GRAD_THREADS = 128, 64     # csrc/cppn_kernel.h: CPPN_THREADS; csrc/cppn_grad_kernel.h: CPPN_GRAD_THREADS
LDS_CAP = 160 * 1024                       # csrc/eigen_engine.hip: stage_genomes


def cppn_lds(n_nodes, n_edges, columns_per_node=RENDER_THREADS):
    """csrc/eigen_engine.hip: cppn_lds.  The render keeps 128 float64 per node, the gradient 2 x 64: the same figure."""
    return n_nodes * columns_per_node * 8 + n_nodes * 16 + n_edges * 8 + (n_nodes + 1) * 4 + n_edges * 4 + n_nodes + 64


# name -> (num_hidden, seed) of synth.make_genome(seed + 1, cfg, seed, num_hidden=...), and BANDS: name -> (nodes, edges, band)
BIG = {"n22": (20, 3), "n59": (60, 3), "n68a": (70, 3), "n68b": (70, 4), "n142": (150, 3), "n144": (150, 4), "n150": (160, 3)}
BANDS = {"n22": (22, 79, "small"), "n59": (59, 236, "under 64 KB"), "n68a": (68, 266, "over 64 KB"), "n68b": (68, 272, "over 64 KB"),
         "n142": (142, 581, "under 160 KiB"), "n144": (144, 577, "under 160 KiB"), "n150": (150, 610, "refused")}
OVER_64K = ("n68a", "n68b", "n142", "n144")
MIXED = ("n22", "n59") + OVER_64K          # the batch of the GPU test: the four genomes above 64 KB beside a 22-node and the 59-node one
REFUSED = "n150"
BIG_SHAPES = ((24, 16), (20, 15))          # 3 render blocks / 6 gradient blocks; ragged for both block sizes


def band_of(lds):
    if lds > LDS_CAP:
        return "refused"
    if lds > 150 * 1024:
        return "under 160 KiB"
    if lds > 64 * 1024:
        return "over 64 KB"
    return "under 64 KB" if lds > 60 * 1024 else "small"


def big_config():
    return synth.make_config(2, 3)


@functools.lru_cache(maxsize=None)
def big_genome(name):
    nh, seed = BIG[name]
    return synth.make_genome(seed + 1, big_config(), seed, num_hidden=nh)


@functools.lru_cache(maxsize=None)
def big_flat(name):
    """flatten_genome of big_genome(name), checked against BANDS: a change of synth cannot move a case out of its band unnoticed"""
    flat = flatten_genome(big_genome(name), big_config())
    nn, ne = len(flat["act"]), len(flat["edge_w"])
    lds = cppn_lds(nn, ne)
    assert lds == cppn_lds(nn, ne, 2 * GRAD_THREADS)
    assert (nn, ne, band_of(lds)) == BANDS[name], (name, nn, ne, lds, band_of(lds))
    return flat


@functools.lru_cache(maxsize=None)
def big_reference(name, w, h):
    """dict(flat, leaves, gimg [3][N], image uint8 [3][h][w] of oracle.cppn.render, nodes float64 [3][N] of oracle.cppn.render_planes,
    grads = (g_w, g_bias, g_resp) of statement (a), outs = statement (a)'s output values); made once per shape, read-only"""
    from oracle import cppn
    flat, cfg, g = big_flat(name), big_config(), big_genome(name)
    leaves = G.plain_grid(w, h)
    gimg = G.image_grad(4000 + sorted(BIG).index(name), 1, 3, w * h)[0]
    image = cppn.render({"x_mat": leaves[0], "y_mat": leaves[1]}, g, cfg, 3, w, h).transpose(2, 0, 1)
    nodes = np.stack([np.asarray(p, np.float64) for p in cppn.render_planes(g, cfg, leaves)])
    grads, outs = G.grads_autograd(flat, leaves, gimg, 3)
    return dict(flat=flat, leaves=leaves, gimg=gimg, image=np.ascontiguousarray(image), nodes=nodes, grads=grads, outs=outs)


def mask_margin(outs, leaves):
    """the distance of 255 v from -1 and from 256 over the live pixels: a pixel within 1e-6 could flip between the masks of the statements"""
    live = leaves[0] != -1.0
    return float(min(np.abs(outs[:, live] * 255.0 + 1.0).min(), np.abs(outs[:, live] * 255.0 - 256.0).min()))


# =========================================================================================== D. derivatives at the activations' edges
DER_W, DER_H = 20, 15
DER_NODES = dict(abs=3, relu=4, sigmoid=5, tanh=6, gauss=7, sin=8, sat_sigmoid=9, sat_tanh_p=10, sat_tanh_n=11, sat_gauss=12)
SATURATED = ("sat_sigmoid", "sat_tanh_p", "sat_tanh_n", "sat_gauss")      # read leaf y alone, which is large on every live pixel


def derivative_genome(key=320):
    """Nodes 3 .. 8 read leaf x with weight 1 and bias 0 (abs and relu: -0.0, which keeps the sign of a zero sum; sin with weight 80:
    |z| ~ 1e3 where |x| ~ 12.5 .. 13.5); nodes 9 .. 12 read leaf y, 13 <= y <= 30 on every live pixel, so they are saturated everywhere
    and the gradients of their parameters are exactly zero.
    The three identity outputs mix them with small weights: every output stays inside (0, 1), so every live pixel is seeded."""
    x, y, n = -1, -2, DER_NODES
    nodes = {0: ("identity", 0.2, 1.0), 1: ("identity", 0.45, 1.0), 2: ("identity", 0.3, 1.0),
             n["abs"]: ("abs", -0.0, 1.0), n["relu"]: ("relu", -0.0, 1.0), n["sigmoid"]: ("sigmoid", 0.0, 1.0), n["tanh"]: ("tanh", 0.0, 1.0),
             n["gauss"]: ("gauss", 0.0, 1.0), n["sin"]: ("sin", 0.0, 1.0), n["sat_sigmoid"]: ("sigmoid", 0.0, 1.0),
             n["sat_tanh_p"]: ("tanh", 0.0, 1.0), n["sat_tanh_n"]: ("tanh", 0.0, 1.0), n["sat_gauss"]: ("gauss", 0.0, 1.0)}
    conns = [(x, n["abs"], 1.0, True), (x, n["relu"], 1.0, True), (x, n["sigmoid"], 1.0, True), (x, n["tanh"], 1.0, True), (x, n["gauss"], 1.0, True),
             (x, n["sin"], 80.0, True), (y, n["sat_sigmoid"], 1.0, True), (y, n["sat_tanh_p"], 1.0, True), (y, n["sat_tanh_n"], -1.0, True),
             (y, n["sat_gauss"], 1.0, True),
             (n["abs"], 0, 0.02, True), (n["sigmoid"], 0, 0.3, True), (n["sat_sigmoid"], 0, 0.1, True), (n["sin"], 0, 0.1, True),
             (n["relu"], 1, 0.02, True), (n["tanh"], 1, 0.2, True), (n["sat_tanh_p"], 1, 0.1, True), (n["sat_tanh_n"], 1, 0.1, True),
             (n["gauss"], 2, 0.3, True), (n["sat_gauss"], 2, 0.2, True), (n["sin"], 2, 0.1, True), (n["abs"], 2, 0.01, True)]
    return G.build_genome(key, nodes, conns)


@functools.lru_cache(maxsize=None)
def derivative_planes():
    """[x, y] for 20 x 15: x cycles through exact +0.0, -0.0, small values and +-[12.5, 13.5]; y is uniform on [13, 30]; the first 12
    pixels are background (both planes -1)"""
    rng = np.random.default_rng(5)
    n = DER_W * DER_H
    big = rng.uniform(12.5, 13.5, n)
    small = rng.uniform(-0.9, 0.9, n)
    k = np.arange(n) % 6
    x = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [0.0, -0.0, small, big, -big], small)
    x = np.where(k == 1, -0.0, x)            # (np.select keeps the sign, this says so)
    y = rng.uniform(13.0, 30.0, n)
    x[:12], y[:12] = -1.0, -1.0
    assert not (x[12:] == -1.0).any()
    x.setflags(write=False), y.setflags(write=False)
    return [x, y]


@functools.lru_cache(maxsize=None)
def derivative_case():
    """dict(flat, fmap, leaves, gimg, grads, outs) as big_reference; fmap: genome.flatten_genome_map (which flat node is which)"""
    from evolutionary_illusion_generator_amd.genome import flatten_genome_map
    cfg = synth.make_config(2, 3)
    fmap = flatten_genome_map(derivative_genome(), cfg)
    flat = {k: v for k, v in fmap.items() if k not in ("node_key", "edge_key")}
    leaves = derivative_planes()
    gimg = G.image_grad(4100, 1, 3, DER_W * DER_H)[0]
    grads, outs = G.grads_autograd(flat, [p.copy() for p in leaves], gimg, 3)      # (torch wraps the arrays it is given: writable copies)
    return dict(flat=flat, fmap=fmap, leaves=leaves, gimg=gimg, grads=grads, outs=outs)
