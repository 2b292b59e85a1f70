"""Host tests of the flow-configuration table and the score edge cases (tests/flow_config_support.py), the CPU oracle alone: they keep
tests/test_gpu_flow_config.py and tests/test_gpu_score_edges.py from being vacuous.  Every table entry must CHANGE the oracle's answer on
its own images (an engine that ignored the parameter would otherwise pass), clamped settings must equal their twin, "empty" entries must be
empty and the others alive, and the hand-built vector sets must take the branches they are built for."""
import functools

import numpy as np
import pytest

from tests import flow_config_support as fc


@functools.lru_cache(maxsize=None)
def _lk_out(images, frozen_kw, shape, batch, seed):
    """oracle output of one setting on an entry's images: per image (corners, next, status, vectors)"""
    import oracle
    i0, i1 = fc.entry_images(dict(shape=shape, batch=batch, seed=seed, images=images))
    p = oracle.LKParams(**dict(frozen_kw))
    out = []
    for b in range(batch):
        g0, g1 = oracle.gray(i0[b]), oracle.gray(i1[b])
        pts = oracle.good_features(g0, p)
        nxt, st = oracle.pyr_lk(g0, g1, pts, p)
        out.append((pts, nxt, st, oracle.lucas_kanade(i0[b], i1[b], p)))
    return out


def _lk(entry, kw):
    return _lk_out(entry["images"], tuple(sorted(kw.items())), entry["shape"], entry["batch"], entry.get("seed", 77))


def _same(a, b):
    return all(len(x[3]) == len(y[3]) and np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])
               and np.array_equal(x[1][x[2] == 1], y[1][y[2] == 1]) for x, y in zip(a, b))


def test_tables_hold_every_listed_setting():
    """the settings the table has to hold, by value (96 x 72 gray unless said), and the bounds of include/eigen_engine.h"""
    gray = [e["kw"] for e in fc.LK_CASES if e["shape"] == fc.GRAY]
    col = [e["kw"] for e in fc.LK_CASES if e["shape"] == fc.COLOUR]

    def has(pool, **kw):
        return any(all(k.get(a) == b for a, b in kw.items()) for k in pool)

    for win in (3, 4, 8, 9, 14, 16):
        assert has(gray, win=win) and has(col, win=win)
    for blk in (1, 2, 4, 8, 9):
        assert has(gray, block_size=blk)
    for pool in (gray, col):
        assert has(pool, max_level=0) and has(pool, max_level=1) and has(pool, max_level=3, win=5)
    for k in (1, 2, 64, 127):
        assert has(gray, max_corners=k)
    assert has(gray, max_corners=128, quality_level=0.01, min_distance=1.0)
    for md in (0.0, 0.5, 1.0, 7.5, 25.0):
        assert has(gray, min_distance=md)
    for q in (0.01, 0.9, 1.0):
        assert has(gray, quality_level=q)
    for it in (0, 1, 2, 30, 150):
        assert has(gray, max_iter=it)
    for eps in (0.0, 0.001, 0.3, 20.0):
        assert has(gray, epsilon=eps)
    assert has(gray, min_eig_thr=0.0) and sum(e.get("role") == "lose_some" for e in fc.LK_CASES) == 1 and sum(e["empty"] == "vectors" for e in fc.LK_CASES) == 1
    assert sum(len(set(k) & {"win", "block_size", "max_level"}) == 3 for k in gray) >= 3
    assert all(4 <= e["batch"] <= 6 for e in fc.LK_CASES)
    fb = {(e["shape"][:2], e["batch"]): [] for e in fc.FB_CASES}
    for e in fc.FB_CASES:
        fb[(e["shape"][:2], e["batch"])].append(e["kw"])
    small = fb[((64, 64), 2)]
    for kw in [dict(fb_winsize=1), dict(fb_winsize=3), dict(fb_winsize=33), dict(fb_poly_n=1), dict(fb_poly_n=2), dict(fb_poly_n=7), dict(fb_poly_sigma=0.0),
               dict(fb_poly_sigma=1.5), dict(fb_iterations=1), dict(fb_iterations=5), dict(fb_levels=0), dict(fb_step=8, max_corners=128), dict(fb_step=5, max_corners=7)]:
        assert has(small, **kw), kw
    assert fb[((512, 512), 1)] == [dict(fb_levels=4)] and fb[((520, 264), 1)] == [dict(fb_levels=4, fb_winsize=21)]
    assert fc.fb_levels_used(512, 512, 4) == 4 and fc.fb_levels_used(520, 264, 4) == 3 and (520 >> 3, 264 >> 3) == (65, 33)
    assert fc.lk_levels(96, 72, 5, 3)[-1] == (12, 9) and len(fc.lk_levels(44, 36, 16, 2)) == 2 and len(fc.lk_levels(96, 72, 15, 2)) == 3
    names = [e["name"] for e in fc.LK_CASES] + [e["name"] for e in fc.FB_CASES]
    assert len(set(names)) == len(names) and all(e["path"] for e in fc.LK_CASES + fc.FB_CASES)
    # every key inside its accepted range
    for e in fc.LK_CASES:
        for k, (lo, hi) in fc.LK_BOUNDS.items():
            assert lo <= e["kw"].get(k, fc.LK_DEFAULTS[k]) <= hi
        assert set(e["kw"]) <= set(fc.LK_DEFAULTS) and set(e["base"]) <= set(e["kw"])


def test_defaults_are_the_oracles():
    import oracle
    p = oracle.LKParams()
    assert {k: getattr(p, k) for k in fc.LK_DEFAULTS} == fc.LK_DEFAULTS
    f = oracle.FBParams()
    assert {("fb_" + k if k != "max_vectors" else "max_corners"): getattr(f, k) for k, _ in f._fields_} == fc.FB_DEFAULTS


@pytest.mark.parametrize("entry", fc.LK_CASES, ids=lambda e: e["name"])
def test_lk_entry_is_live(oracle_lib, entry):
    """the entry changes the oracle's answer (against the defaults and against its stage), is empty exactly where declared, equals its clamped twin"""
    out, dflt = _lk(entry, entry["kw"]), _lk(entry, {})
    B = entry["batch"]
    assert len(out[-1][0]) == 0, "the last image is flat: no corner"
    if entry["same_pyramid"]:
        w, h, _ = entry["shape"]
        kw = {k: v for k, v in entry["kw"].items() if k != "max_level"}
        win = entry["kw"].get("win", fc.LK_DEFAULTS["win"])
        assert fc.lk_levels(w, h, win, entry["kw"]["max_level"]) == fc.lk_levels(w, h, win, fc.LK_DEFAULTS["max_level"])   # the declaration is true
        assert _same(out, _lk(entry, kw))
        if kw:
            assert not _same(out, dflt)
    else:
        assert not _same(out, dflt), "the oracle answers as under the defaults: an engine ignoring %s would pass" % (entry["kw"],)
        if entry["base"]:
            assert not _same(out, _lk(entry, entry["base"])), "the oracle answers as under %s alone" % (entry["base"],)
        if "max_level" in entry["kw"] and len(entry["kw"]) > 1:   # the level must matter beside the other keywords
            assert not _same(out, _lk(entry, {k: v for k, v in entry["kw"].items() if k != "max_level"}))
    if entry["clamp_twin"]:
        assert _same(out, _lk(entry, entry["clamp_twin"]))
        if "max_iter" in entry["clamp_twin"]:   # some track is still moving at the cap, so iterating past it would show
            assert not _same(out, _lk(entry, dict(max_iter=entry["clamp_twin"]["max_iter"] - 1)))
    for b in range(B - 1):
        pts, nxt, st, vec = out[b]
        if entry["empty"] == "corners":
            assert len(pts) == 0 and len(vec) == 0
        elif entry["empty"] == "vectors":
            assert len(pts) > 0 and len(vec) == 0 and not st.any()
        else:
            assert len(vec) >= 1, "image %d: no vector" % b
    if entry.get("role") == "lose_some":
        lost = sum(int((o[2] == 0).sum()) for o in out) / max(1, sum(len(o[2]) for o in out))
        base_lost = sum(int((o[2] == 0).sum()) for o in dflt) / max(1, sum(len(o[2]) for o in dflt))
        assert 0.1 <= lost <= 0.9 and lost > base_lost, (lost, base_lost)
    if entry.get("role") == "fill128":
        assert all(len(out[b][0]) == 128 for b in range(B - 1)), [len(o[0]) for o in out]


def test_lk_win_entries_lose_a_track(oracle_lib):
    lost = sum(int((o[2] == 0).sum()) for e in fc.LK_CASES if "win" in e["kw"] and e.get("role") == "win" for o in _lk(e, e["kw"]))
    assert lost > 0, "no track was lost over the window entries: the status == 0 paths were not exercised"


@functools.lru_cache(maxsize=None)
def _fb_out(frozen_kw, shape, batch, seed):
    import oracle
    i0, i1 = fc.entry_images(dict(shape=shape, batch=batch, seed=seed, images="textured"))
    kw = dict(frozen_kw)
    p = oracle.FBParams(**fc.fb_params_kw(kw, kw.get("max_corners", 100)))
    out = []
    for b in range(batch):
        fl = oracle.farneback_flow(oracle.gray(i0[b]), oracle.gray(i1[b]), p)
        out.append((fl, oracle.farneback_vectors(fl, p)))
    return out


@pytest.mark.parametrize("entry", fc.FB_CASES, ids=lambda e: e["name"])
def test_farneback_entry_is_live(oracle_lib, entry):
    out = _fb_out(tuple(sorted(entry["kw"].items())), entry["shape"], entry["batch"], entry["seed"])
    dflt = _fb_out((), entry["shape"], entry["batch"], entry["seed"])
    assert all(np.isfinite(fl).all() for fl, _ in out)
    assert max(float(np.abs(fl).max()) for fl, _ in out) > 0.05
    same = all(np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and np.array_equal(a[1], b[1]) for a, b in zip(out, dflt))
    assert not same, "the oracle answers as under the defaults"
    if set(entry["kw"]) & {"fb_step", "max_corners"}:   # the sampling entries change the vectors, not the field
        assert all(not (len(a[1]) == len(b[1]) and np.array_equal(a[1], b[1])) for a, b in zip(out[:1], dflt[:1]))
    live = out if entry["batch"] == 1 else out[:-1]   # (the last first frame of a batch is flat; its field still moves towards the second frame, so nothing is claimed of it)
    assert all(len(v) >= 1 for _, v in live)


def test_refusal_list_is_just_outside_the_bounds():
    """each refused setting is one step outside its bound and its accepted neighbour one step inside (the GPU test runs them through eigen_create)"""
    seen = set()
    for flow, kw, (w, h, ch), frag, inside in fc.REFUSALS:
        assert flow in ("lk", "farneback") and len(kw) == 1 and set(kw) == set(inside) and frag
        (k, v), = kw.items()
        seen.add((k, v))
        if k in fc.LK_BOUNDS:
            lo, hi = fc.LK_BOUNDS[k]
            assert (v == lo - 1 and inside[k] == lo) or (v == hi + 1 and inside[k] == hi)
        assert w % (1 << (len(ch) - 1)) == 0 and h % (1 << (len(ch) - 1)) == 0   # the PredNet size check is not what refuses
    for want in [("win", 2), ("win", 17), ("block_size", 0), ("block_size", 10), ("max_level", -1), ("max_level", 4), ("max_corners", 0), ("max_corners", 129),
                 ("fb_winsize", 0), ("fb_winsize", 4), ("fb_winsize", 35), ("fb_poly_n", 0), ("fb_poly_n", 8), ("fb_levels", -1), ("fb_levels", 5),
                 ("fb_iterations", 0), ("fb_step", 0)]:
        assert want in seen, want
    flow, kw, (w, h, ch), frag, inside = fc.REFUSALS[-1]
    lv = fc.fb_levels_used(w, h, kw["fb_levels"])
    assert (w % (1 << lv) or h % (1 << lv)) and "divisible" in frag
    lv = fc.fb_levels_used(w, h, inside["fb_levels"])
    assert not (w % (1 << lv) or h % (1 << lv))


# ------------------------------------------------------------------------------------------------ score edge cases: the census, oracle alone
def test_score_cases_take_every_listed_branch():
    rows = fc.score_table()
    fc.check_score_census(rows)
    by = {(r[0], r[1], r[2]): r[5] for r in rows}
    g = (160, 120, 100)
    # the zero vector: NaN for Bands and Free, finite for Circles when it lies outside the radius, NaN inside
    assert np.isnan(by[(g, 0, "zero_outside_radius")]) and np.isnan(by[(g, 2, "zero_outside_radius")])
    assert np.isfinite(by[(g, 1, "zero_outside_radius")]) and by[(g, 1, "zero_outside_radius")] != 0 and np.isnan(by[(g, 1, "zero_inside_radius")])
    # 24 kept vectors score 0, 25 do not; fewer than two inside the radius keep the strength term alone
    assert by[(g, 1, "circles_kept_24")] == 0 and by[(g, 1, "circles_kept_25")] != 0
    assert 0 < by[(g, 1, "circles_inside_1")] < 0.3 and by[(g, 1, "circles_inside_2")] != by[(g, 1, "circles_inside_1")]
    # the float32 neighbours of the limits fall on their two sides
    for s, lim in ((0, 0.15), (1, 0.3), (2, 0.4)):
        assert float(fc.below(lim)) < lim < float(fc.above(lim)) and np.nextafter(fc.below(lim), np.float32(1)) == fc.above(lim)
    assert by[(g, 0, "norm_below_0.15")] != 0 and by[(g, 0, "norm_above_0.15")] == 0
    assert by[(g, 2, "norm_below_0.4")] != 0 and by[(g, 2, "norm_above_0.4")] == 0
    assert by[(g, 2, "count_above_K")] == by[(g, 2, "full_K")]
    assert all(len(v) <= K for (w, h, K) in fc.SCORE_GEOMETRIES for _, v, _ in fc.score_cases(w, h, K) + fc.io_cases(w, h, K))
    # every position lies inside its image
    for (w, h, K) in fc.SCORE_GEOMETRIES:
        for name, v, _ in fc.score_cases(w, h, K) + fc.io_cases(w, h, K):
            assert np.isfinite(v).all() and (v[:, 0] >= 0).all() and (v[:, 0] <= w - 1).all() and (v[:, 1] >= 0).all() and (v[:, 1] <= h - 1).all(), (w, h, name)


def test_inside_outside_cases_hit_the_cell_borders():
    """structure 4: vectors on both sides of every cell border, a fractional step where 5 does not divide the width, all finite"""
    from oracle import scores
    fractional = 0
    for (w, h, K) in fc.SCORE_GEOMETRIES:
        step = w / 5
        fractional += step != int(step)
        cases = fc.io_cases(w, h, K)
        assert any(n == "io_cell_borders" for n, _, _ in cases)
        for name, v, cnt in cases:
            r = scores.inside_outside_score(v[:cnt].astype(np.float64), w, h) if cnt else None
            assert r is None or np.isfinite(r), (w, h, name)
            if name == "io_cell_borders" and K > 16:
                cells = {int(x / step) for x in v[:, 0].astype(np.float64)}
                assert cells == {0, 1, 2, 3, 4} and (v[:, 0] == w - 1).any()
                assert any(float(x) / step == int(float(x) / step) and x > 0 for x in v[:, 0]) or step != int(step)
    assert fractional >= 2   # 64 / 5 and 44 / 5
