"""GPU tests of the flow configuration: every setting of the table in tests/flow_config_support.py through the HIP flow kernels against the
CPU oracle, BIT FOR BIT (DESIGN.md sections 3.5 and 4) -- corner list, corner count, status, next points and vectors for Lucas-Kanade, the
dense field and the sampled vectors for Farneback -- the settings just outside every bound of `eigen_create`, and one end-to-end evaluation
under a non-default configuration.  tests/test_flow_config_host.py shows with the oracle alone that every entry changes the answer."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from evolutionary_illusion_generator_amd import synth, weights
from evolutionary_illusion_generator_amd.engine import PAIR_SINGLE, Engine, EngineError
from tests import flow_config_support as fc

EIGEN_ERR_INVALID = -1   # include/eigen_engine.h


def _first_diff(got, ref):
    """index of the first row in which two arrays of features differ"""
    n = min(len(got), len(ref))
    if n == 0:
        return 0
    bad = np.nonzero((got[:n] != ref[:n]).reshape(n, -1).any(axis=1))[0]
    return int(bad[0]) if len(bad) else n


def _flow(e, i0, i1, cuda):
    import torch
    B, c, h, w = i0.shape
    d0, d1 = torch.from_numpy(i0).to(cuda), torch.from_numpy(i1).to(cuda)
    dv = torch.zeros((B, e.K, 4), dtype=torch.float32, device=cuda)
    dc = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    e.flow(d0, c * h * w, d1, c * h * w, B, dv, dc)
    torch.cuda.synchronize()
    return dv.cpu().numpy(), dc.cpu().numpy()


@pytest.mark.parametrize("entry", fc.LK_CASES, ids=lambda e: e["name"])
def test_lk_setting_bit_exact(cuda, oracle_lib, entry):
    w, h, c = entry["shape"]
    B = entry["batch"]
    i0, i1 = fc.entry_images(entry)
    params = oracle_lib.LKParams(**fc.lk_params_kw(entry["kw"]))
    e = Engine(w, h, [c, 4], B, **entry["kw"])
    try:
        assert e.K == params.max_corners
        v, n = _flow(e, i0, i1, cuda)
        corners, ncorn, nxt, st = e.debug_corners(B)
    finally:
        e.close()
    for b in range(B):
        where = "entry %s (%s), image %d" % (entry["name"], entry["kw"], b)
        g0, g1 = oracle_lib.gray(i0[b]), oracle_lib.gray(i1[b])
        pts = oracle_lib.good_features(g0, params)
        k = _first_diff(corners[b, :ncorn[b]], pts)
        assert ncorn[b] == len(pts) and k == len(pts), "%s: corner %d differs (%d corners, oracle %d): %s vs %s" % (
            where, k, ncorn[b], len(pts), corners[b, k:k + 1], pts[k:k + 1])
        rn, rs = oracle_lib.pyr_lk(g0, g1, pts, params)
        k = _first_diff(st[b, :len(pts)], rs)
        assert k == len(pts), "%s: status of feature %d at %s is %d, oracle %d" % (where, k, pts[k], st[b, k], rs[k])
        live = rs == 1
        k = _first_diff(nxt[b, :len(pts)][live], rn[live])
        assert k == int(live.sum()), "%s: next point of tracked feature %d differs: %s vs %s" % (where, k, nxt[b, :len(pts)][live][k], rn[live][k])
        ref = oracle_lib.lucas_kanade(i0[b], i1[b], params)
        k = _first_diff(v[b, :max(n[b], 0)], ref)
        assert n[b] == len(ref) and k == len(ref), "%s: vector %d differs (%d vectors, oracle %d)" % (where, k, n[b], len(ref))


@pytest.mark.parametrize("entry", fc.FB_CASES, ids=lambda e: e["name"])
def test_farneback_setting_bit_exact(cuda, oracle_lib, entry):
    w, h, c = entry["shape"]
    B = entry["batch"]
    i0, i1 = fc.entry_images(entry)
    e = Engine(w, h, [c, 4], B, flow="farneback", **entry["kw"])
    try:
        v, n = _flow(e, i0, i1, cuda)
        dense = e.debug_dense_flow(B)
        params = oracle_lib.FBParams(**fc.fb_params_kw(entry["kw"], e.K))
    finally:
        e.close()
    for b in range(B):
        where = "entry %s (%s), image %d" % (entry["name"], entry["kw"], b)
        ref = oracle_lib.farneback_flow(oracle_lib.gray(i0[b]), oracle_lib.gray(i1[b]), params)
        got = dense[b].transpose(1, 2, 0)
        if not np.array_equal(got, ref):
            y, x = np.argwhere((got != ref).any(axis=2))[0]
            raise AssertionError("%s: the dense field differs first at (x %d, y %d): %s vs %s; %d pixels differ, max abs %g" % (
                where, x, y, got[y, x], ref[y, x], int((got != ref).any(axis=2).sum()), float(np.abs(got - ref).max())))
        rv = oracle_lib.farneback_vectors(ref, params)
        k = _first_diff(v[b, :max(n[b], 0)], rv)
        assert n[b] == len(rv) and k == len(rv), "%s: sampled vector %d differs (%d vectors, oracle %d)" % (where, k, n[b], len(rv))


def _create(flow, kw, w, h, ch):
    """eigen_create with the keywords applied to the default configuration -> (return code, handle, message, library)"""
    from evolutionary_illusion_generator_amd.engine import FLOW_METHODS, EigenConfig, load_library
    lib = load_library()
    cfg = EigenConfig()
    lib.eigen_config_defaults(ctypes.byref(cfg))
    cfg.width, cfg.height, cfg.n_layers, cfg.max_batch, cfg.flow_method = w, h, len(ch), 1, FLOW_METHODS[flow]
    for i, c in enumerate(ch):
        cfg.channels[i] = c
    for k, v in kw.items():
        setattr(cfg, k if k.startswith("fb_") else "lk_" + k, v)
    handle = ctypes.c_void_p(0xDEAD)
    rc = lib.eigen_create(ctypes.byref(cfg), ctypes.byref(handle))
    return rc, handle, lib.eigen_last_error().decode(), lib


def test_settings_outside_the_bounds_are_refused(cuda):
    """every setting one step outside a bound: EIGEN_ERR_INVALID with its message and a NULL handle -- nothing was allocated, so nothing can
    be launched (the checks of eigen_create precede its first HIP call) -- and through Engine an EngineError; the setting just inside is accepted"""
    for flow, kw, (w, h, ch), frag, inside in fc.REFUSALS:
        rc, handle, msg, lib = _create(flow, kw, w, h, ch)
        assert rc == EIGEN_ERR_INVALID and not handle.value and frag in msg, (flow, kw, rc, handle.value, msg)
        with pytest.raises(EngineError) as err:
            Engine(w, h, ch, 1, flow=flow, **kw)
        assert "error %d" % EIGEN_ERR_INVALID in str(err.value) and frag in str(err.value), (kw, str(err.value))
        rc, handle, msg, lib = _create(flow, inside, w, h, ch)
        assert rc == 0 and handle.value, (flow, inside, rc, msg)
        assert lib.eigen_destroy(handle) == 0


def test_configuration_reaches_the_whole_path(cuda, oracle_lib):
    """eval_images under win = 9, block_size = 5, max_corners = 64: render (oracle) -> PredNet -> Lucas-Kanade -> score, the vectors bit for bit and
    the fitness within the scores' tolerance of the oracle pipeline run with the same LKParams -- and not what the defaults give."""
    import torch
    from oracle import grids, pipeline
    w, h, ch, structure = 64, 64, [1, 8, 16], 2
    kw = dict(win=9, block_size=5, max_corners=64)
    cfg = synth.make_config(2, 1)
    pop = synth.make_population(6, cfg, seed=4)
    wts = weights.synthetic_prednet_weights(ch, w, h, seed=2)
    grid = grids.create_grid(structure, w, h, 10)
    imgs = np.stack([pipeline.render_chw(g, cfg, grid, 1, w, h) for _, g in pop])
    e = Engine(w, h, ch, len(pop), **kw)
    e.set_weights(wts)
    got, vecs = e.eval_images(torch.from_numpy(imgs).to(cuda), len(pop), structure, pairing=PAIR_SINGLE)
    e.close()
    params = oracle_lib.LKParams(**kw)
    ref = np.array([pipeline.image_fitness(im, wts, ch, w, h, structure, pairing=PAIR_SINGLE, lk_params=params) for im in imgs])
    dflt = np.array([pipeline.image_fitness(im, wts, ch, w, h, structure, pairing=PAIR_SINGLE) for im in imgs])
    for i, im in enumerate(imgs):
        rv = pipeline.image_vectors(im, wts, ch, w, h, pairing=PAIR_SINGLE, lk_params=params)
        assert len(vecs[i]) == len(rv) and np.array_equal(vecs[i], rv), "genome %d: vectors differ" % i
    print("fitness", got, "oracle", ref, "oracle under the defaults", dflt)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.allclose(got, ref, rtol=1e-9, atol=1e-12, equal_nan=True), (got, ref)
    assert (np.isfinite(ref) & (ref != 0)).any(), "vacuous: the oracle scored nothing"
    assert (ref != dflt).any(), "vacuous: the defaults give the same fitness"
