"""The dense fitness's pyramidal, iterated solve on the GPU (eigen_dense_score_iter, eigen_eval_population_dense_iter,
eigen_eval_images_dense_iter, csrc/dense_pyr_kernels.h; DESIGN.md section 14, "The pyramidal, iterated solve").  The field is compared
with the numpy restatement `dense_pyr_support.dense_pyr_ref` bit for bit and the records by the bounds of
tests/test_gpu_dense_fitness.py (`check_records`, imported, not edited).  One level with one iteration is the single step, through the
iteration kernel and through the plain entries; the population path is the stage on the frames the roll-out emits; a genome's fitness
does not depend on its batch; refusals leave the handle as it was."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, fitness, genome
from evolutionary_illusion_generator_amd.engine import Engine, EngineError
from tests import dense_fitness_support as ds
from tests import dense_pyr_support as dp
from tests.flow_gpu_support import _p
from tests.test_gpu_dense_fitness import _e2e_engine, check_records

pytestmark = pytest.mark.gpu

SENT = -12345.5
STAGE = [(c[0], s) for c in dp.GPU_CASES for s in (0, 1, 2)]


def _median_norm(u):
    return float(np.median(np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])))


@pytest.mark.parametrize("name,structure", STAGE, ids=["%s-s%d" % c for c in STAGE])
def test_the_iterated_stage_is_the_numpy_restatement(cuda, name, structure):
    """`Engine.dense_score` with a solve on the four cases (8 x 8 gray 2 x 2: less than a tile, a coarsest level of 4 x 4; 20 x 15 colour
    3 x 2: odd sizes 10 x 8 and 5 x 4, samples clamped at the border; 48 x 32 colour 3 x 3: 3 x 2 tiles, taps beyond the staged patch;
    16 x 12 gray 1 x 5: iterations at one level; 40 x 24 gray 2 x 2 at radius 16: the launch with more than 64 KB of LDS) under every structure's score, max_norm the median norm of the restatement's field: u
    `np.array_equal` to `dense_pyr_ref`, the records within the bounds of the single step's stage test; a second call gives the same
    bytes."""
    img0, img1, levels, iters, r, want_u = dp.gpu_case(name)
    B, C, h, w = img0.shape
    dense = dp.dense_for(structure, r, _median_norm(want_u), levels, iters)
    sc = dp.restatement_score(dense, h)
    want = dp.Want(want_u, sc)
    eng = Engine(w, h, [C], B + 1)       # one layer: 20 x 15 halves to nothing a PredNet could pool
    try:
        assert eng.debug_dense_solve() == 0
        d0, d1 = torch.from_numpy(img0).to(cuda), torch.from_numpy(img1).to(cuda)
        fit, rec, u = eng.dense_score(d0, C * h * w, d1, C * h * w, B, dense, stats=True, flow=True)
        assert eng.debug_dense_solve() > 0
        fit2, rec2, u2 = eng.dense_score(d0, C * h * w, d1, C * h * w, B, dense, stats=True, flow=True)
    finally:
        eng.close()
    assert np.array_equal(u, want_u), np.abs(u - want_u).max()
    assert u2.tobytes() == u.tobytes() and rec2.tobytes() == rec.tobytes() and fit2.tobytes() == fit.tobytes()
    check_records(rec, fit, want, sc)
    assert (rec[:, 0] > 0).any()
    print("dense pyr stage %s s%d: N %s S %s" % (name, structure, rec[:, 0].astype(int).tolist(), rec[:, 8].tolist()))


def _raw_iter(eng, d0, d1, per, B, dense, solve, fit, rec, d_flow):
    """eigen_dense_score_iter called directly; solve: None (NULL) or (levels, iters)"""
    cfg, keep, d_mask = eng._dense_args(dense)
    s = None if solve is None else engine.DenseSolveC(*solve)
    rc = eng.lib.eigen_dense_score_iter(eng._h, _p(d0), ctypes.c_int64(per), _p(d1), ctypes.c_int64(per), ctypes.c_int32(B), ctypes.byref(cfg), d_mask,
                                        None if fit is None else ctypes.c_void_p(fit.ctypes.data), None if rec is None else ctypes.c_void_p(rec.ctypes.data),
                                        _p(d_flow), None, None if s is None else ctypes.byref(s))
    return rc, eng.lib.eigen_last_error().decode()


@pytest.mark.parametrize("name", ["16x12", "48x32"])
def test_one_level_one_iteration_is_the_single_step(cuda, name):
    """On a case's images under the single step's settings: `eigen_dense_score_iter` with {1, 1} forced through the iteration kernel
    (eigen_debug_dense_solve) gives `eigen_dense_score`'s field and records byte for byte, also on a pair of equal images, whose field is
    zero of either sign; the plain {1, 1} entry and NULL give the namesake's bytes and allocate no pyramid."""
    img0, img1, _, _, r, _ = dp.gpu_case(name)
    img0, img1 = np.concatenate([img0, img0[:1]]), np.concatenate([img1, img0[:1]])       # the last sample: equal images
    B, C, h, w = img0.shape
    per = C * h * w
    dense = dp.dense_for(1, r, 0.5, 1, 1)
    d0, d1 = torch.from_numpy(img0).to(cuda), torch.from_numpy(img1).to(cuda)
    eng = Engine(w, h, [C, 4], B)
    try:
        fit, rec, u = eng.dense_score(d0, per, d1, per, B, dense, stats=True, flow=True)
        assert u[:B - 1].any() and not u[B - 1].any()
        for solve in (None, (1, 1)):
            f2, r2 = np.full(B, SENT), np.full((B, 10), SENT)
            d_flow = torch.full((B, 2, h, w), SENT, dtype=torch.float64, device=cuda)
            rc, msg = _raw_iter(eng, d0, d1, per, B, dense, solve, f2, r2, d_flow)
            assert rc == 0, msg
            assert f2.tobytes() == fit.tobytes() and r2.tobytes() == rec.tobytes() and d_flow.cpu().numpy().tobytes() == u.tobytes()
        assert eng.debug_dense_solve() == 0
        assert eng.debug_dense_solve(force=True) == 0
        for solve in (None, (1, 1)):
            f3, r3 = np.full(B, SENT), np.full((B, 10), SENT)
            d_flow = torch.full((B, 2, h, w), SENT, dtype=torch.float64, device=cuda)
            rc, msg = _raw_iter(eng, d0, d1, per, B, dense, solve, f3, r3, d_flow)
            assert rc == 0, msg
            assert d_flow.cpu().numpy().tobytes() == u.tobytes()
            assert f3.tobytes() == fit.tobytes() and r3.tobytes() == rec.tobytes()
        assert eng.debug_dense_solve() > 0                   # the forced call went through the pyramid's planes
        # and the plain entry follows the hook too, then leaves it
        f4, _, u4 = eng.dense_score(d0, per, d1, per, B, dense, stats=True, flow=True)
        assert u4.tobytes() == u.tobytes() and f4.tobytes() == fit.tobytes()
        eng.debug_dense_solve(force=False)
        f5, _, u5 = eng.dense_score(d0, per, d1, per, B, dense, stats=True, flow=True)
        assert u5.tobytes() == u.tobytes() and f5.tobytes() == fit.tobytes()
    finally:
        eng.close()


E2E = [(s, p) for s in ds.E2E_STRUCTURES for p in (ds.PAIR_POPULATION, ds.PAIR_SINGLE)]


@pytest.mark.parametrize("structure,pairing", E2E, ids=["s%d-%s" % (s, "population" if p == ds.PAIR_POPULATION else "single") for s, p in E2E])
def test_the_population_path_is_the_iterated_stage_on_the_emitted_frames(cuda, structure, pairing):
    """48 x 32 colour, 7 genomes under "live" weights, 2 levels x 3 iterations (max_norm per pairing, `dense_pyr_support.E2E_MAX_NORM`; at
    least half of the samples are live): `eval_population(dense=...)` equals `dense_score` on the
    frames `render_cppn` + `prednet_rollout` return, bit for bit, and `dense_pyr_ref` on those frames (the field `np.array_equal`, the
    records by the stage test's bounds); `eval_images(dense=...)` gives the same bytes; the slices [0, 3), [3, 6), [6, 7) give the bytes of
    the batch of 7, and `fitness.evaluate_population(max_batch=3)` those of `max_batch=7`; the iterated fitness differs from the single
    step's."""
    w, h, ch = ds.E2E_SHAPES[1]
    n, C, nr = ds.E2E_GENOMES, ch[0], 20
    per = C * h * w
    dense = dp.e2e_dense(structure, pairing)
    sc = dp.restatement_score(dense, h)
    gb = genome.GenomeBatch(ds.e2e_genomes(), ds.e2e_config(), C, n_leaves=2)
    eng = _e2e_engine(w, h, ch, structure, n)
    try:
        fit = eng.eval_population(gb, structure, pairing=pairing, dense=dense)
        rec = eng.last_dense_stats
        single = eng.eval_population(gb, structure, pairing=pairing, dense=ds.e2e_dense(structure))
        d_img = torch.zeros((n, C, h, w), dtype=torch.uint8, device=cuda)
        eng.render_cppn(gb, d_img, bg=1, gradient=1)
        n_steps, first = (nr + 1, nr - 1) if pairing == ds.PAIR_POPULATION else (nr + 2, nr + 1)
        n_out = n_steps - first
        d_fr = torch.zeros((n, n_out, C, h, w), dtype=torch.uint8, device=cuda)
        eng.prednet_rollout(d_img, n, n_steps, first, d_fr)
        if pairing == ds.PAIR_POPULATION:
            d0, s0, d1, s1 = d_fr, n_out * per, d_fr.view(-1)[per:], n_out * per
            img0, img1 = d_fr[:, 0].cpu().numpy(), d_fr[:, 1].cpu().numpy()
        else:
            d0, s0, d1, s1 = d_img, per, d_fr, n_out * per
            img0, img1 = d_img.cpu().numpy(), d_fr[:, 0].cpu().numpy()
        fit2, rec2, u = eng.dense_score(d0, s0, d1, s1, n, dense, stats=True, flow=True)
        assert fit2.tobytes() == fit.tobytes() and rec2.tobytes() == rec.tobytes()
        fit3, vecs = eng.eval_images(d_img, n, structure, pairing=pairing, dense=dense)
        assert fit3.tobytes() == fit.tobytes() and eng.last_dense_stats.tobytes() == rec.tobytes() and len(vecs) == n
        parts = np.concatenate([eng.eval_population(gb.slice(lo, hi), structure, pairing=pairing, dense=dense) for lo, hi in ((0, 3), (3, 6), (6, 7))])
        assert parts.tobytes() == fit.tobytes()
        t = eng.timings()           # the stage is reported as the single step's: [2], and 0 as [3]
        stage_ms = t["flow_ms"]
        assert stage_ms > 0 and t["score_ms"] == 0
    finally:
        eng.close()
    want_u = dp.dense_pyr_ref(img0, img1, ds.E2E_RADIUS, ds.EPS, dp.E2E_LEVELS, dp.E2E_ITERS)
    assert np.array_equal(u, want_u), np.abs(u - want_u).max()
    check_records(rec, fit, dp.Want(want_u, sc), sc)
    assert fit.tobytes() != single.tobytes()
    live = (rec[:, 0] >= sc.min_count) & (fit != 0)
    assert 2 * int(live.sum()) >= n, (rec[:, 0], fit)
    wts = ds.e2e_weights(w, h, ch)
    kw = dict(c_dim=C, pairing=pairing, score=dense)
    try:
        whole = fitness.evaluate_population(structure, ds.e2e_genomes(), wts, ds.e2e_config(), w, h, list(ch), max_batch=7, **kw)
        split = fitness.evaluate_population(structure, ds.e2e_genomes(), wts, ds.e2e_config(), w, h, list(ch), max_batch=3, **kw)
    finally:
        fitness.clear_engines()
    assert whole.shape == (n,) and split.tobytes() == whole.tobytes()
    if ds.grid_structure(structure, w, h) == structure:
        assert whole.tobytes() == fit.tobytes()
    print("dense pyr end to end s%d pairing %d: N %s fitness %s (single step %s) stage %s" % (structure, pairing, rec[:, 0].astype(int).tolist(), fit.tolist(), single.tolist(), stage_ms))


def test_refusals_leave_the_handle_as_it_was(cuda):
    """EIGEN_ERR_INVALID with a message and nothing written: levels 0 and 7, iters 0 and 33, 16 x 12 with 3 levels (a coarsest level of
    4 x 3), through all three entries' shared check.  None of them allocates the pyramid, a handle that made only single-step calls has
    none, and after the refusals the handle scores on both paths as a fresh one does."""
    img0, img1, _, _, r, want_u = dp.gpu_case("16x12")
    B, C, h, w = img0.shape
    per = C * h * w
    dense = dp.dense_for(1, r, _median_norm(want_u), 1, 1)
    d0, d1 = torch.from_numpy(img0).to(cuda), torch.from_numpy(img1).to(cuda)
    eng = Engine(w, h, [C, 4], B)
    try:
        base = eng.dense_score(d0, per, d1, per, B, dense)
        for solve, words in (((0, 1), "dense solve levels 0 outside 1 .. 6"), ((7, 1), "dense solve levels 7 outside 1 .. 6"), ((1, 0), "dense solve iters 0 outside 1 .. 32"),
                             ((1, 33), "dense solve iters 33 outside 1 .. 32"), ((3, 2), "the coarsest level of a 16 x 12 image is 4 x 3, below 4 pixels"),
                             ((-1, -1), "dense solve levels -1")):
            fit = np.full(B, SENT)
            d_flow = torch.full((B, 2, h, w), SENT, dtype=torch.float64, device=cuda)
            rc, msg = _raw_iter(eng, d0, d1, per, B, dense, solve, fit, None, d_flow)
            assert rc == -1 and words in msg, (solve, rc, msg)
            assert (fit == SENT).all() and bool((d_flow == SENT).all())
        assert eng.debug_dense_solve() == 0
        with pytest.raises(EngineError, match="coarsest level"):
            eng.eval_images(d0, B, 1, dense=dp.dense_for(1, r, 0.5, 3, 2))
        bad = dp.dense_for(1, r, 0.5, 2, 2)
        bad.iters = 40                   # past the object's own rule: the C check is the one under test
        with pytest.raises(EngineError, match="dense solve iters 40"):
            eng.eval_images(d0, B, 1, dense=bad)
        with pytest.raises(EngineError, match="dense solve iters 40"):
            eng.dense_score(d0, per, d1, per, B, bad)
        assert eng.debug_dense_solve() == 0
        assert eng.dense_score(d0, per, d1, per, B, dense).tobytes() == base.tobytes()
        it = dp.dense_for(1, r, _median_norm(want_u), 1, 5)
        fit, rec, u = eng.dense_score(d0, per, d1, per, B, it, stats=True, flow=True)
        assert np.array_equal(u, want_u) and eng.debug_dense_solve() > 0
        assert eng.dense_score(d0, per, d1, per, B, dense).tobytes() == base.tobytes()
    finally:
        eng.close()
