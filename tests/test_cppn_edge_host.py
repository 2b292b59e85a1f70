"""CPU: the conditions the CPPN edge cases of tests/cppn_edge_support.py must meet, asserted on the oracle alone, and oracle.detmath64
against np.longdouble.  tests/test_gpu_cppn_edges.py runs the same cases on the device.

  A. the probe plane reaches every branch of csrc/det_math64.h; the flattener keeps the seven activation nodes as written;
     oracle.detmath64 is within twice its measured distance from long double, and is not numpy's libm;
  B. the oracle's images over the extreme planes contain what every branch of quant_u8 and of the h,s,v renderer produces;
  C. every large genome lands in its LDS band, and the two statements of the gradient agree on it within E / 100;
  D. the derivative genome meets its conditions in the forward values, and the two statements agree on it within E / 100."""
import numpy as np
import pytest

from evolutionary_illusion_generator_amd.genome import flatten_genome
from oracle import cppn
from oracle import detmath64 as dm
from tests import cppn_edge_support as S
from tests import cppn_grad_support as G

TINY = np.finfo(np.float64).tiny


# =========================================================================================== A
def _straddled(args, t, ulps=32):
    """values of args on both sides of t, within `ulps` of it"""
    d = ulps * np.spacing(abs(t))
    return bool(((args < t) & (args >= t - d)).any() and ((args >= t) & (args <= t + d)).any())


def _exp_arguments(x):
    """what det_exp sees behind the three activations that call it: -(5 x), 2 min(|2.5 x|, 40) where tanh's upper branch runs, -5 x^2"""
    with np.errstate(all="ignore"):
        t = np.abs(2.5 * x)
        return -(5.0 * x), 2.0 * np.minimum(t[t >= 0.625], 40.0), -5.0 * (x * x)


@pytest.mark.parametrize("n", S.PROBE_LENGTHS)
def test_the_probe_reaches_every_branch_of_the_transcendentals(n):
    x = S.probe(n)
    assert x.shape == (n,) and n < 2e5 and (n % 128 == 0) == (n == S.PROBE_LENGTHS[0]) and S.PROBE_LENGTHS[1] % 128 == 1
    for v in S.SPECIALS:                                              # every special value, bit for bit
        assert (x.view(np.uint64) == np.float64(v).view(np.uint64)).any(), v
    with np.errstate(all="ignore"):
        # ---- exp
        sig_arg, tanh_arg, gauss_arg = _exp_arguments(x)
        args = np.concatenate([sig_arg, tanh_arg, gauss_arg])
        e = dm.det_exp(args)
        census = dict(subnormal=int(((e > 0) & (e < TINY)).sum()), zero=int((e == 0).sum()), inf=int(np.isinf(e).sum()), nan=int(np.isnan(e).sum()),
                      smallest=int((e == 5e-324).sum()))
        print("det_exp over the probe:", census)
        assert census["subnormal"] > 100 and census["zero"] >= 1 and census["inf"] >= 1 and census["nan"] >= 1 and census["smallest"] >= 1
        assert (args < -746.0).any() and (args > 710.0).any() and (args == -np.inf).any() and (args == np.inf).any()     # both clamps
        for t in (-745.1332191019411, -708.3964185322641, 709.782712893384, 710.0, -746.0):
            assert _straddled(args, t), t
        fin = args[np.isfinite(args)]
        k = np.rint(np.clip(fin, -746.0, 710.0) * dm.INV_LN2)
        assert k.min() <= -1075 and k.max() == 1024                 # ldexp below the subnormals and at the overflow
        # ---- tanh
        t = 2.5 * x
        at = np.abs(t[np.isfinite(t)])
        assert (at < 0.625).sum() > 1000 and ((at >= 0.625) & (at <= 40.0)).sum() > 1000 and (at > 40.0).sum() > 1000
        for thr in (0.625, -0.625, 40.0, -40.0):
            assert _straddled(t, thr), thr
        # ---- sin
        fx = x[np.isfinite(x)]
        inside = fx[np.abs(fx) <= S.SIN_CUT]
        j0, bumped, j = S.sin_octant(inside)
        for lo, hi in ((0.0, 1e6), (1e6, np.inf)):
            m = (np.abs(inside) >= lo) & (np.abs(inside) < hi)
            counts = [int(((j0 == o) & m).sum()) for o in range(8)]
            print("det_sin octants on [%g, %g):" % (lo, hi), counts)
            assert min(counts) >= 1000, (lo, counts)
        assert bumped.any() and not bumped.all() and set(np.unique(j)) == {0, 2, 4, 6}
        assert (np.abs(fx) > S.SIN_CUT).any() and _straddled(x, S.SIN_CUT) and _straddled(x, -S.SIN_CUT)
        assert np.isinf(x).sum() == 2 and np.isnan(dm.det_sin(x[np.isinf(x)])).all()
        assert (dm.det_sin(fx[np.abs(fx) > S.SIN_CUT]) == 0.0).all()
        m = np.rint(np.abs(inside) / S.PI4)                          # multiples of pi / 4 up to the cut, a few ulps away on both sides
        near = np.abs(np.abs(inside) - m * S.PI4) <= 4 * np.spacing(np.abs(inside))
        assert (near & (np.abs(inside) > 1e9)).sum() >= 5 and (near & (np.abs(inside) > 1e6)).sum() >= 500 and (near & (np.abs(inside) < 64)).sum() >= 500
        # ---- gauss, relu
        assert np.isinf(x[np.isfinite(x)] ** 2).any() and (gauss_arg == -np.inf).any()
        assert np.isnan(x).any() and (np.signbit(x) & (x == 0.0)).any()
    ref = S.act_reference(x)
    assert ref.shape == (7, n) and ref.dtype == np.float64
    assert np.isnan(ref[:, np.isnan(x)]).all()                      # NaN goes through every activation


def test_the_flattener_keeps_the_seven_activation_nodes_as_written():
    flat = flatten_genome(S.activation_genome(), S.activation_config())
    assert list(flat["act"]) == list(range(7)) and list(flat["out_node"]) == list(range(7))
    assert list(flat["edge_off"]) == list(range(8)) and list(flat["edge_src"]) == [-1] * 7        # one edge each, from leaf x: nothing folded
    assert (flat["edge_w"] == 1.0).all() and (flat["resp"] == 1.0).all()
    assert (flat["bias"] == 0.0).all() and np.signbit(flat["bias"]).all()                         # -0.0
    x = S.probe()
    with np.errstate(all="ignore"):
        pre = 1.0 * (1.0 * x) + flat["bias"][0]
    assert np.array_equal(pre.view(np.uint64)[~np.isnan(x)], x.view(np.uint64)[~np.isnan(x)])      # bit for bit, -0.0 included
    # the two references of the GPU test are the same numbers (render_planes starts its sum at Python's 0, so x = -0.0 enters as +0.0:
    # equal under ==, which is what array_equal compares)
    planes = cppn.render_planes(S.activation_genome(), S.activation_config(), [x, np.zeros_like(x)])
    assert all(p.dtype == np.float64 for p in planes)
    assert np.array_equal(np.stack(planes), S.act_reference(x), equal_nan=True)


def test_detmath64_is_within_twice_its_measured_distance_from_long_double():
    fig = S.long_double_figures(S.probe())
    print("oracle.detmath64 against np.longdouble over probe(): exp %.4g ulp, tanh %.4g ulp, sin %.4g absolute, sigmoid %.4g relative"
          % (fig["exp_ulp"], fig["tanh_ulp"], fig["sin_abs"], fig["sigmoid_rel"]))
    k = S.LONG_DOUBLE_SLACK
    assert k == 2.0
    assert fig["exp_ulp"] <= k * S.MEASURED_EXP_ULP and fig["tanh_ulp"] <= k * S.MEASURED_TANH_ULP, fig
    assert fig["sin_abs"] <= k * S.MEASURED_SIN_ABS and fig["sigmoid_rel"] <= k * S.MEASURED_SIGMOID_REL, fig
    # the constants are measurements, not allowances: none is more than twice what is measured here
    for name, const in (("exp_ulp", S.MEASURED_EXP_ULP), ("tanh_ulp", S.MEASURED_TANH_ULP), ("sin_abs", S.MEASURED_SIN_ABS), ("sigmoid_rel", S.MEASURED_SIGMOID_REL)):
        assert 0 < const <= 4.0 and const <= 2.0 * fig[name], (name, const, fig[name])


def test_detmath64_is_not_numpys_libm():
    """a swapped transcendental changes bits in at least 1 % of the finite probe: the GPU comparison would notice it"""
    x = S.probe()
    x = x[np.isfinite(x)]
    with np.errstate(all="ignore"):
        for name, det, lib in (("exp", dm.det_exp, np.exp), ("tanh", dm.det_tanh, np.tanh), ("sin", dm.det_sin, np.sin)):
            frac = float((det(x) != lib(x)).mean())
            print("%s: oracle.detmath64 differs from numpy in %.2f %% of %d finite probe values" % (name, 100 * frac, x.size))
            assert frac >= 0.01, (name, frac)


# =========================================================================================== B
def _gen_index():
    """where the values of _general_values() sit: general[k], wrap[i] = the five values around wrap point i (v, -1, +1, -2, +2 ulp), rounded[k]"""
    g, w = len(S.GENERAL), len(S.WRAP_POINTS)
    return dict(general=list(range(g)), wrap=[list(range(g + 5 * i, g + 5 * i + 5)) for i in range(w)], rounded=list(range(g + 5 * w, g + 5 * w + len(S.ROUNDED))))


def test_the_extreme_planes_hold_what_they_promise():
    planes, reg = S.extreme_planes()
    n = S.EXT_W * S.EXT_H
    assert planes.shape == (3, n) and (S.EXT_W, S.EXT_H) == (24, 16)
    gen = S._general_values()
    for c in range(3):
        assert np.array_equal(planes[c, reg["p%d" % c]].view(np.uint64), gen.view(np.uint64))
        for v in S.GENERAL:
            assert (planes[c].view(np.uint64) == np.float64(v).view(np.uint64)).any(), (c, v)
    assert (planes[0] == -1.0).sum() == 24 and (planes[0, reg["bg"]] == -1.0).all()
    rest = reg["rest"]
    assert np.isfinite(planes[:, rest]).all() and np.abs(planes[:, rest]).max() <= 1.2 and rest.stop - rest.start >= 100
    assert (planes[1, reg["s0"]] == 0.0).all() and not np.isfinite(planes[0, reg["s0"]]).all()
    with np.errstate(all="ignore"):
        h6 = planes[0] * 6.0
        fin = np.isfinite(h6)
        sext = np.trunc(h6[fin])
        assert set(S.SEXTANTS) <= set(sext[np.abs(sext) < 100].astype(int)), "every sextant -7 .. 7"
        assert (np.signbit(sext) & (sext == 0)).any()                                         # trunc(6 h) = -0.0
        near = np.abs(np.abs(sext) - S.T53) <= 64
        assert (np.abs(sext[near]) < S.T53).any() and (np.abs(sext[near]) >= S.T53).any() and (sext[near] < 0).any()    # 6 h on both sides of +-2^53
        assert ((~fin) & (planes[1] != 0.0) & (planes[0] != -1.0)).sum() >= 3                   # non-finite h with s != 0
        assert ((planes[0] < 0) & (planes[0] != -1.0) & (planes[1] != 0.0)).any()
        # the values only the `fabs(t) < 2^31` form of quant_u8 gets right: trunc(255 v) and 4 v of exactly +2^31
        assert (np.trunc(planes[0] * 255.0) == S.T31).any() and (planes[0] * 4.0 == S.T31).any()


def test_the_oracles_images_contain_every_branch_of_the_quantiser():
    planes, reg = S.extreme_planes()
    ix = _gen_index()
    g = S.copy_genome()
    col = S.extreme_reference(g, 3, 1, 1).reshape(3, -1)
    for c in range(3):
        v = planes[c, reg["p%d" % c]]
        b = col[c, reg["p%d" % c]]
        with np.errstate(all="ignore"):
            t = np.trunc(v * 255.0)
        huge = ~(np.abs(t) < S.T31)
        assert huge.sum() >= 8 and (b[huge] == 0).all(), c                                     # NaN, +-inf, +-1e300, |t| >= 2^31: byte 0
        for i in (0, 1, 4, 5):                                                                 # the wrap points of v * 255
            k = ix["wrap"][i]
            assert b[k[3]] != b[k[4]] and len(set(b[k])) == 2, (c, S.WRAP_POINTS[i], b[k])
        assert b[ix["wrap"][0][3]] == 255 and b[ix["wrap"][0][4]] == 0                         # ... 0x7FFFFFFF below 2^31, the branch above
        assert b[ix["wrap"][1][4]] == 1 and b[ix["wrap"][1][3]] == 0                           # ... 0x80000001 above -2^31
        assert b[ix["wrap"][4][3]] == 255 and b[ix["wrap"][4][4]] == 0                         # 255.99 | 256
        assert b[ix["wrap"][5][3]] == 255 and b[ix["wrap"][5][4]] == 0                         # -1 | -0.99
    # background: plane 0 == -1 fills every channel whatever the other planes hold
    for bg in (0, 1):
        img = S.extreme_reference(g, 3, 1, bg).reshape(3, -1)
        assert (img[:, reg["bg"]] == 255 * bg).all()
    # palette: v * 4 on both sides of +-2^31
    pal = S.extreme_reference(g, 3, 0, 1).reshape(3, -1)[:, reg["p0"]]
    for i in (2, 3):
        k = ix["wrap"][i]
        assert tuple(pal[:, k[3]]) != tuple(pal[:, k[4]]), S.WRAP_POINTS[i]
    assert tuple(pal[:, ix["wrap"][2][3]]) == (0, 0, 0) and tuple(pal[:, ix["wrap"][2][0]]) == (255, 255, 255)     # code 255 | the 2^31 branch: code 0
    assert {tuple(p) for p in pal.T} >= {(0, 0, 0), (255, 255, 255), (255, 0, 0)}
    # rounded gray: half to even, then the quantiser
    gray = S.extreme_reference(g, 1, 0, 1).reshape(-1)[reg["p0"]]
    r = dict(zip(S.ROUNDED, gray[ix["rounded"]]))
    assert (r[0.5], r[1.5], r[2.5], r[-0.5]) == (0, 254, 254, 0) and r[8421504.25] == 128 and r[8421505.25] == 0 and r[-8421505.25] == 0
    # h, s, v
    for bg in (0, 1):
        hsv = S.extreme_reference(g, 3, 2, bg).reshape(3, -1)
        assert (hsv[0, reg["bg"]] == 255 * bg).all() and (hsv[1:, reg["bg"]] == 0).all()      # the fill is h = s = v = bg: red for bg = 1
        assert len(np.unique(hsv[:, reg["hue"]])) > 20
    # the second genome carries ordinary planes to the same branches by its responses and biases
    s = S.scale_genome()
    with np.errstate(all="ignore"):
        vals = np.stack(cppn.render_planes(s, S.extreme_config(), [planes[0], planes[1], planes[2]]))
        t = np.trunc(vals * 255.0)[:, reg["rest"]]
    assert vals.dtype == np.float64
    for c in (0, 1):
        assert (np.abs(t[c]) >= S.T31).any() and ((np.abs(t[c]) < S.T31) & (np.abs(t[c]) > S.T31 / 2)).any(), c
    assert ((t[2] >= 256) | (t[2] < 0)).any() and ((t[2] >= 0) & (t[2] < 256)).any()
    assert (t[0, 0] == S.T31 or t[0, 2] == S.T31) and t[0, 1] < S.T31                           # 1.0 and its neighbours straddle 2^31
    assert not np.array_equal(S.extreme_reference(s, 3, 1, 1), S.extreme_reference(g, 3, 1, 1))


# =========================================================================================== C
def test_every_large_genome_lands_in_its_band():
    assert S.cppn_lds(59, 236) == 64555 and S.cppn_lds(68, 266) == 74320 and S.cppn_lds(142, 581) == 155430 and S.cppn_lds(150, 610) == 164138
    for name in S.BIG:
        flat = S.big_flat(name)                                          # asserts nodes, edges and band
        lds = S.cppn_lds(len(flat["act"]), len(flat["edge_w"]))
        print("%s: %d nodes, %d edges, %d B of LDS: %s" % (name, len(flat["act"]), len(flat["edge_w"]), lds, S.band_of(lds)))
        assert (lds > 64 * 1024) == (name in S.OVER_64K or name == S.REFUSED) and (lds > S.LDS_CAP) == (name == S.REFUSED)
    assert set(S.MIXED) | {S.REFUSED} == set(S.BIG) and len({S.BIG[n][1] for n in ("n68a", "n68b")}) == 2 and len({S.BIG[n][1] for n in ("n142", "n144")}) == 2
    assert [(-(-w * h // S.RENDER_THREADS), -(-w * h // S.GRAD_THREADS), (w * h) % S.RENDER_THREADS, (w * h) % S.GRAD_THREADS) for w, h in S.BIG_SHAPES] == [(3, 6, 0, 0), (3, 5, 44, 44)]


@pytest.mark.parametrize("shape", S.BIG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_two_statements_agree_on_the_large_genomes(shape):
    """the condition of every gradient case (tests/test_cppn_grad_host.py): statement (b) within E / 100 of statement (a), and no pixel at
    the edge of the mask"""
    for name in S.MIXED:
        r = S.big_reference(name, *shape)
        n, e = G.deviation(G.grads_reverse(r["flat"], r["leaves"], r["gimg"], 3), r["grads"])
        print("%s at %dx%d: (b) from (a): %.3g in norm, %.3g element-wise (E / 100 = %.3g); mask margin %.3g" % ((name,) + shape + (n, e, G.E / 100, S.mask_margin(r["outs"], r["leaves"]))))
        assert n <= G.E / 100 and e <= G.E / 100, (name, n, e)
        assert S.mask_margin(r["outs"], r["leaves"]) > 1e-6, name
        vals = G.forward_np(r["flat"], r["leaves"])[0]
        assert np.array_equal(vals[r["flat"]["out_node"]], r["nodes"])                    # the oracle's planes are statement (b)'s forward
        assert np.array_equal(G.quantise(vals, r["flat"], r["leaves"], 3), r["image"].reshape(3, -1))


# =========================================================================================== D
def test_the_derivative_genome_meets_its_conditions():
    c = S.derivative_case()
    flat, fmap, leaves = c["flat"], c["fmap"], c["leaves"]
    at = {name: fmap["node_key"].index(key) for name, key in S.DER_NODES.items()}
    assert None not in fmap["node_key"] and None not in fmap["edge_key"]
    vals, sums, zs = G.forward_np(flat, leaves)
    live = leaves[0] != -1.0
    assert live.sum() == S.DER_W * S.DER_H - 12
    for name in ("abs", "relu"):
        z = zs[at[name]][live]
        assert ((z == 0.0) & ~np.signbit(z)).sum() >= 40 and ((z == 0.0) & np.signbit(z)).sum() >= 40, name     # exactly +0.0 and -0.0
    assert (vals[at["sigmoid"]][live] == 1.0).sum() >= 40 and (vals[at["sigmoid"]][live] == 0.5).sum() >= 80
    assert (vals[at["tanh"]][live] == 1.0).sum() >= 40 and (vals[at["tanh"]][live] == -1.0).sum() >= 40
    assert (vals[at["gauss"]][live] == 0.0).sum() >= 80 and (vals[at["gauss"]][live] == 1.0).sum() >= 80
    zsin = np.abs(zs[at["sin"]][live])
    assert ((zsin >= 1000.0) & (zsin <= 1080.0)).sum() >= 80
    assert (vals[at["sat_sigmoid"]][live] == 1.0).all() and (vals[at["sat_tanh_p"]][live] == 1.0).all()
    assert (vals[at["sat_tanh_n"]][live] == -1.0).all() and (vals[at["sat_gauss"]][live] == 0.0).all()
    outs = vals[flat["out_node"]][:, live]
    assert outs.min() > 0.01 and outs.max() < 0.99                                        # every live pixel is seeded
    assert S.mask_margin(c["outs"], leaves) > 1.0
    # the reference: exactly zero for the parameters of the saturated nodes, not zero altogether
    g_w, g_bias, g_resp = c["grads"]
    for name in S.SATURATED:
        n = at[name]
        k = int(flat["edge_off"][n])
        assert flat["edge_off"][n + 1] == k + 1 and g_w[k] == 0.0 and g_bias[n] == 0.0 and g_resp[n] == 0.0, name
    zeros, total = sum(int((x == 0.0).sum()) for x in c["grads"]), sum(x.size for x in c["grads"])
    assert 3 * len(S.SATURATED) <= zeros <= 3 * len(S.SATURATED) + 1 and total == 22 + 2 * 13      # (+ 1: the weight behind the gauss node that is 0 everywhere)
    rev = G.grads_reverse(flat, leaves, c["gimg"], 3)
    n, e = G.deviation(rev, c["grads"])
    print("derivative genome: (b) from (a): %.3g in norm, %.3g element-wise (E / 100 = %.3g)" % (n, e, G.E / 100))
    assert n <= G.E / 100 and e <= G.E / 100, (n, e)
    for a, b in zip(rev, c["grads"]):
        assert (a[b == 0.0] == 0.0).all()
