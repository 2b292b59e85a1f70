"""The dense motion fitness's members on the GPU (eigen_dense_score_members, eigen_eval_population_dense_members,
eigen_eval_images_dense_members, fitness.DenseFitness(members=); DESIGN.md section 14, "Members").  Corner members are the CPU oracle's
corners of the first image of a pair; the records under them are the numpy restatement's by the bounds of tests/test_gpu_dense_fitness.py
and the trainer's stage with the same members bit for bit; the compacted pair pass of the Free structure leaves the record bytes of the
all-pixel kernel; the population path is the stage on the emitted frames, a genome's fitness does not depend on its batch, and the sparse
path of a handle is untouched by a members call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, fitness, genome, train
from evolutionary_illusion_generator_amd.engine import Engine, EngineError
from evolutionary_illusion_generator_amd.train import PredNetTrainer
from tests import dense_fitness_support as ds
from tests import dense_members_support as dm
from tests import flow_corner_support as fc
from tests.flow_gpu_support import _p
from tests.test_gpu_dense_fitness import check_records

pytestmark = pytest.mark.gpu

SENT = -12345.5


def _score(eng, cuda, img0, img1, dense, **kw):
    """`Engine.dense_score` on densely packed host images"""
    B, C, h, w = img0.shape
    return eng.dense_score(torch.from_numpy(np.ascontiguousarray(img0)).to(cuda), C * h * w, torch.from_numpy(np.ascontiguousarray(img1)).to(cuda), C * h * w, B, dense, **kw)


# ---- 1. the member planes
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.shape_id)
def test_the_member_planes_are_the_oracles_corners(cuda, shape):
    """On a smooth image, a random one and a constant one with no corner, the planes and the counts `dense_score(members_out=True)`
    returns are the CPU oracle's corners of img0 as planes: with max_corners 128, with a cap of 5 that decides, and under a shared mask
    that excludes the left half (the counts are before the mask)."""
    w, h, C, r = shape
    img0, img1 = dm.stage_pair(w, h, C)
    sc = fc.score_of("circles", h)
    eng = Engine(w, h, [C, 4], fc.B)
    try:
        for max_corners, mask in ((fc.MAX_CORNERS, None), (fc.CAPPED, None), (fc.MAX_CORNERS, fc.half_mask(w, h))):
            fit, (planes, counts) = _score(eng, cuda, img0, img1, dm.dense_of(sc, r, mask, fc.corner_members(max_corners)), members_out=True)
            want, n_want = fc.oracle_members(img0, max_corners, mask)
            assert planes.dtype == np.uint8 and planes.shape == (fc.B, h, w) and counts.dtype == np.int32
            assert np.array_equal(planes, want) and np.array_equal(counts, n_want), (max_corners, counts, n_want)
            assert n_want[2] == 0 and fit[2] == 0.0
        with pytest.raises(ValueError, match="members_out"):
            _score(eng, cuda, img0, img1, dm.dense_of(sc, r), members_out=True)
    finally:
        eng.close()


# ---- 2. the records
@functools.lru_cache(maxsize=None)
def _stage_reference(w, h, C, r, kind, solve):
    img0, img1 = dm.stage_pair(w, h, C)
    sc = fc.score_of(kind, h)
    planes, _ = fc.oracle_members(img0)
    return sc, dm.restate(sc, img0, img1, r, planes, solve)


@pytest.mark.parametrize("solve", dm.SOLVES, ids=dm.solve_id)
@pytest.mark.parametrize("kind", fc.SCORES)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.shape_id)
def test_the_records_under_corner_members(cuda, shape, kind, solve):
    """Under corner members and each of the three scores, with the single step and with 2 levels x 2 iterations: the field is the
    restatement's, `np.array_equal` (members do not touch the solve); against the restatement under the oracle's planes N is exact, the
    record sums lie within N 2^-53 sum |terms| and S_b within 1e-10; and the record is, bit for bit, that of the trainer's
    `flow_term_pair` with the same members on the float images of the bytes."""
    w, h, C, r = shape
    img0, img1 = dm.stage_pair(w, h, C)
    sc, want = _stage_reference(w, h, C, r, kind, solve)
    mem = fc.corner_members()
    eng = Engine(w, h, [C, 4], fc.B)
    try:
        fit, rec, u = _score(eng, cuda, img0, img1, dm.dense_of(sc, r, None, mem, solve), stats=True, flow=True)
    finally:
        eng.close()
    print("dense members %s %s %s: N %s S %s" % (fc.shape_id(shape), kind, dm.solve_id(solve), rec[:, 0].astype(int).tolist(), rec[:, 8].tolist()))
    assert np.array_equal(u, want.u), np.abs(u - want.u).max()
    check_records(rec, fit, want, sc)
    assert rec[0, 0] > 0 and rec[1, 0] > 0 and not rec[2].any()
    with PredNetTrainer("synthetic", [C, 4], w, h, fc.B, 2) as tr:
        flow = fc.flow_of(sc, r, None, pairing="prediction", members=mem).solved(*solve)
        _, tu, _ = tr.flow_term_pair(ds.as_float(img1)[0], ds.as_float(img0)[0], flow)
        trec = tr.last_flow_stats
    assert tu.tobytes() == u.tobytes() and trec.tobytes() == rec.tobytes()


# ---- 3. the compacted pair pass against the all-pixel kernel
@pytest.mark.parametrize("plane", dm.PAIR_PLANES)
@pytest.mark.parametrize("shape", dm.PAIR_SHAPES, ids=dm.pair_id)
def test_the_compacted_pair_pass_leaves_the_all_pixel_kernels_bytes(cuda, shape, plane):
    """At B = 1 under Free, a plane given as the shared `mask=` runs the all-pixel pair kernel and the same plane given as
    `members=plane[None]` runs the list and the compacted pass: the records are the same bytes.  192 pixels are less than one tile of the
    list, 594 three tiles with the last partial, 1536 six full ones; the planes are all ones (the list spans every tile), a random two
    thirds and exactly one member."""
    w, h = shape
    a, b = dm.pair_images(w, h)
    m = dm.pair_plane(plane, w, h)
    sc = dm.free_score()
    eng = Engine(w, h, [1], 3)       # one layer: 33 x 18 halves to nothing a PredNet could pool
    try:
        _, shared = _score(eng, cuda, a[:1], b[:1], dm.dense_of(sc, dm.PAIR_RADIUS, mask=m), stats=True)
        fit, listed = _score(eng, cuda, a[:1], b[:1], dm.dense_of(sc, dm.PAIR_RADIUS, members=m[None]), stats=True)
    finally:
        eng.close()
    print("pair pass %s %s: N %d swarm %r S %r" % (dm.pair_id(shape), plane, listed[0, 0], listed[0, 4], listed[0, 8]))
    assert listed.tobytes() == shared.tobytes() and fit[0] == listed[0, 8]
    assert 0 < listed[0, 0] <= m.sum() and (plane != "single" or listed[0, 0] == 1) and (plane != "ones" or listed[0, 0] > 0.9 * w * h)
    assert listed[0, 4] != 0 and listed[0, 8] != 0


@pytest.mark.parametrize("shape", dm.PAIR_SHAPES, ids=dm.pair_id)
def test_a_batch_of_planes_is_its_samples(cuda, shape):
    """Three different planes with an all-zero one in the middle, one call: every sample's record is the bytes of its own B = 1 call and,
    where it has members, of the all-pixel kernel under its plane as the shared mask; the middle sample scores exactly 0 (alone it is a plane
    set that counts no pixel, which is refused, as an all-zero set of three is); planes of another batch size are a ValueError."""
    w, h = shape
    a, b = dm.pair_images(w, h)
    planes = dm.batch_planes(w, h)
    sc = dm.free_score()
    eng = Engine(w, h, [1], 3)       # one layer: 33 x 18 halves to nothing a PredNet could pool
    try:
        fit, rec = _score(eng, cuda, a, b, dm.dense_of(sc, dm.PAIR_RADIUS, members=planes), stats=True)
        for i in (0, 2):
            _, one = _score(eng, cuda, a[i:i + 1], b[i:i + 1], dm.dense_of(sc, dm.PAIR_RADIUS, members=planes[i:i + 1]), stats=True)
            assert one.tobytes() == rec[i:i + 1].tobytes(), i
            _, shared = _score(eng, cuda, a[i:i + 1], b[i:i + 1], dm.dense_of(sc, dm.PAIR_RADIUS, mask=planes[i]), stats=True)
            assert shared.tobytes() == rec[i:i + 1].tobytes(), i
        # the middle sample alone is a plane set that counts no pixel, which is refused; in the batch it scores exactly 0
        with pytest.raises(EngineError, match="the flow mask counts no pixel"):
            _score(eng, cuda, a[1:2], b[1:2], dm.dense_of(sc, dm.PAIR_RADIUS, members=planes[1:2]))
        assert not rec[1].any() and fit[1] == 0.0 and rec[0, 8] != 0 and rec[2, 8] != 0
        # a batch of two whose second plane is empty: the empty sample still scores exactly 0 beside a live one
        f2, r2 = _score(eng, cuda, a[:2], b[:2], dm.dense_of(sc, dm.PAIR_RADIUS, members=planes[:2]), stats=True)
        assert r2.tobytes() == rec[:2].tobytes() and f2[1] == 0.0
        with pytest.raises(EngineError, match="the flow mask counts no pixel"):
            _score(eng, cuda, a, b, dm.dense_of(sc, dm.PAIR_RADIUS, members=np.zeros_like(planes)))
        with pytest.raises(ValueError, match="member planes are"):
            _score(eng, cuda, a[:2], b[:2], dm.dense_of(sc, dm.PAIR_RADIUS, members=planes))
        again = _score(eng, cuda, a, b, dm.dense_of(sc, dm.PAIR_RADIUS, members=planes))
        assert again.tobytes() == fit.tobytes()
    finally:
        eng.close()


# ---- 4. end to end
def _e2e_engine(w, h, ch, structure, max_batch):
    eng = Engine(w, h, list(ch), max_batch)
    eng.set_weights(ds.e2e_weights(w, h, ch))
    eng.set_grid(fitness.leaf_planes(ds.grid_structure(structure, w, h), w, h, 2))
    return eng


def _emitted(eng, cuda, gb, n, C, h, w, pairing, nr=20):
    """the pair of a pairing from `render_cppn` + `prednet_rollout`: (d0, s0, d1, s1 for dense_score, img0, img1 on the host, the images)"""
    per = C * h * w
    d_img = torch.zeros((n, C, h, w), dtype=torch.uint8, device=cuda)
    eng.render_cppn(gb, d_img, bg=1, gradient=1)
    n_steps, first = (nr + 1, nr - 1) if pairing == ds.PAIR_POPULATION else (nr + 2, nr + 1)
    n_out = n_steps - first
    d_fr = torch.zeros((n, n_out, C, h, w), dtype=torch.uint8, device=cuda)
    eng.prednet_rollout(d_img, n, n_steps, first, d_fr)
    if pairing == ds.PAIR_POPULATION:
        return d_fr, n_out * per, d_fr.view(-1)[per:], n_out * per, d_fr[:, 0].cpu().numpy(), d_fr[:, 1].cpu().numpy(), d_img
    return d_img, per, d_fr, n_out * per, d_img.cpu().numpy(), d_fr[:, 0].cpu().numpy(), d_img


@pytest.mark.parametrize("c", dm.E2E, ids=dm.e2e_id)
def test_the_population_path_under_corner_members(cuda, c):
    """7 genomes under "live" weights and `CornerMembers(**flow_corner_support.CORNER)`: `eval_population(dense=...)` equals `dense_score`
    on the frames `render_cppn` + `prednet_rollout` return, bit for bit, with the oracle's corners of the emitted img0 as the planes, and the
    numpy restatement under those planes by the bounds of the stage test; at least five of the seven samples are live, and the one sample
    of Free / single at 48 x 32 that keeps 2 members scores exactly 0; `eval_images(dense=...)` gives the same bytes; the slices [0, 3),
    [3, 6), [6, 7) give the bytes of the batch of 7, and `fitness.evaluate_population(max_batch=3)` those of `max_batch=7`, which are the
    engine's."""
    (w, h, ch), structure, pairing = c
    n, C = ds.E2E_GENOMES, ch[0]
    dense = dm.e2e_dense(structure)
    gb = genome.GenomeBatch(ds.e2e_genomes(), ds.e2e_config(), C, n_leaves=2)
    eng = _e2e_engine(w, h, ch, structure, n)
    try:
        fit = eng.eval_population(gb, structure, pairing=pairing, dense=dense)
        rec = eng.last_dense_stats
        d0, s0, d1, s1, img0, img1, d_img = _emitted(eng, cuda, gb, n, C, h, w, pairing)
        fit2, rec2, (planes, counts) = eng.dense_score(d0, s0, d1, s1, n, dense, stats=True, members_out=True)
        assert fit2.tobytes() == fit.tobytes() and rec2.tobytes() == rec.tobytes()
        fit3, vecs = eng.eval_images(d_img, n, structure, pairing=pairing, dense=dense)
        assert fit3.tobytes() == fit.tobytes() and eng.last_dense_stats.tobytes() == rec.tobytes() and len(vecs) == n
        parts = np.concatenate([eng.eval_population(gb.slice(lo, hi), structure, pairing=pairing, dense=dense) for lo, hi in ((0, 3), (3, 6), (6, 7))])
        assert parts.tobytes() == fit.tobytes()
    finally:
        eng.close()
    want_planes, want_counts = dm.e2e_planes(img0)
    assert np.array_equal(planes, want_planes) and np.array_equal(counts, want_counts)
    sc, want = dm.e2e_restate(structure, img0, img1, want_planes)
    print("dense members end to end %s: corners %s N %s fitness %s" % (dm.e2e_id(c), counts.tolist(), rec[:, 0].astype(int).tolist(), fit.tolist()))
    check_records(rec, fit, want, sc)
    live = (rec[:, 0] >= sc.min_count) & (fit != 0)
    assert int(live.sum()) >= 5, (rec[:, 0], fit)
    assert bool((fit == 0).any()) == (((w, h), structure, pairing) == dm.DEAD), (rec[:, 0], fit)
    wts = ds.e2e_weights(w, h, ch)
    kw = dict(c_dim=C, pairing=pairing, score=dense)
    try:
        whole = fitness.evaluate_population(structure, ds.e2e_genomes(), wts, ds.e2e_config(), w, h, list(ch), max_batch=7, **kw)
        split = fitness.evaluate_population(structure, ds.e2e_genomes(), wts, ds.e2e_config(), w, h, list(ch), max_batch=3, **kw)
    finally:
        fitness.clear_engines()
    assert whole.shape == (n,) and split.tobytes() == whole.tobytes() and whole.tobytes() == fit.tobytes()


def test_below_min_count_scores_zero(cuda):
    """16 x 12 yields a handful of corners a sample: under min_count 10 every sample is below it, N is the restatement's and every fitness
    is exactly 0"""
    w, h, ch = dm.SMALL
    n, C = ds.E2E_GENOMES, ch[0]
    dense = dm.e2e_dense(1, min_count=10)
    gb = genome.GenomeBatch(ds.e2e_genomes(), ds.e2e_config(), C, n_leaves=2)
    eng = _e2e_engine(w, h, ch, 1, n)
    try:
        fit = eng.eval_population(gb, 1, dense=dense)
        rec = eng.last_dense_stats
        _, _, _, _, img0, img1, _ = _emitted(eng, cuda, gb, n, C, h, w, ds.PAIR_POPULATION)
    finally:
        eng.close()
    planes, counts = dm.e2e_planes(img0)
    sc, want = dm.e2e_restate(1, img0, img1, planes, min_count=10)
    assert (counts >= 1).all() and np.array_equal(rec[:, 0], want.score.record[:, 0]) and (rec[:, 0] < 10).all()
    assert not fit.any() and not rec[:, 8].any()


def test_the_sparse_path_is_untouched_by_a_members_call(cuda):
    """A sparse `eval_population` on the same handle after dense calls with members returns the bytes it returned before them, and so
    does `eval_images` with its vectors; a dense call without members after them returns its earlier bytes too."""
    w, h, ch = ds.E2E_SHAPES[1]
    n, C = ds.E2E_GENOMES, ch[0]
    gb = genome.GenomeBatch(ds.e2e_genomes(), ds.e2e_config(), C, n_leaves=2)
    imgs = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (n, C, h, w), dtype=np.uint8)).to(cuda)
    planes = np.ascontiguousarray(np.broadcast_to(fc.random_masks(w, h)[:1], (n, h, w)))
    eng = _e2e_engine(w, h, ch, 1, n)
    try:
        want = eng.eval_population(gb, 1)
        want_i, want_v = eng.eval_images(imgs, n, 2)
        want_d = eng.eval_population(gb, 2, dense=ds.e2e_dense(2))
        for structure in (1, 2):
            eng.eval_population(gb, structure, dense=dm.e2e_dense(structure))
        by_planes = eng.eval_population(gb, 2, dense=ds.e2e_dense(2).with_members(planes))
        got = eng.eval_population(gb, 1)
        got_i, got_v = eng.eval_images(imgs, n, 2)
        got_d = eng.eval_population(gb, 2, dense=ds.e2e_dense(2))
    finally:
        eng.close()
    assert got.tobytes() == want.tobytes() and got_i.tobytes() == want_i.tobytes() and ((want != 0).any() or (want_i != 0).any())
    assert len(got_v) == len(want_v) and all(a.tobytes() == b.tobytes() for a, b in zip(got_v, want_v))
    assert got_d.tobytes() == want_d.tobytes() and by_planes.shape == (n,) and by_planes.tobytes() != want_d.tobytes()


# ---- 5. refusals
def test_refusals(cuda):
    """Every rule of the members, in the trainer's words: EIGEN_ERR_INVALID, every output untouched, and the handle still works."""
    w, h, C, B = 16, 12, 1, 2
    HW = per = h * w
    eng = Engine(w, h, [C, 4], B)
    rng = np.random.default_rng(3)
    d = torch.from_numpy(rng.integers(0, 256, (2, B, C, h, w), dtype=np.uint8)).to(cuda)
    ones = torch.ones((B, h, w), dtype=torch.uint8, device=cuda)
    zeros = torch.zeros((B, h, w), dtype=torch.uint8, device=cuda)
    score = train.FreeScore().settings(h)
    cfg = engine.DenseSettingsC(engine.FlowSettingsC(3, 0, 1e-2), None, ctypes.addressof(score))
    M = train.FlowMembersSettings
    corners = dict(kind=1, max_corners=20, block_size=3, reserved=0, quality_level=0.05, min_distance=3.0, mask_bstride=0)

    def members(**kw):
        f = dict(corners, **kw)
        return M(f["kind"], f["max_corners"], f["block_size"], f["reserved"], f["quality_level"], f["min_distance"], f["mask_bstride"])

    def call(mem, mask=None):
        fit, rec = np.full(B + 1, SENT), np.full((B + 1, 10), SENT)
        planes, counts = np.full((B, h, w), 9, np.uint8), np.full(B, -7, np.int32)
        u = torch.full((B * 2 * HW,), SENT, dtype=torch.float64, device=cuda)
        rc = eng.lib.eigen_dense_score_members(eng._h, _p(d[0]), ctypes.c_int64(per), _p(d[1]), ctypes.c_int64(per), ctypes.c_int32(B), ctypes.byref(cfg), _p(mask),
                                               ctypes.c_void_p(fit.ctypes.data), ctypes.c_void_p(rec.ctypes.data), _p(u), None, None, ctypes.byref(mem),
                                               ctypes.c_void_p(planes.ctypes.data), ctypes.c_void_p(counts.ctypes.data))
        untouched = (fit == SENT).all() and (rec == SENT).all() and (planes == 9).all() and (counts == -7).all() and bool((u == SENT).all())
        return rc, eng.lib.eigen_last_error().decode(), untouched

    def population_calls(mem, mask=None):
        """the two population entries on the same members: refused ahead of the render and the roll-out (the handle has no grid and no weights)"""
        fit = np.full(B, SENT)
        rc_i = eng.lib.eigen_eval_images_dense_members(eng._h, _p(d[0]), ctypes.c_int32(B), ctypes.c_int32(2), ctypes.c_int32(0), ctypes.byref(cfg), _p(mask),
                                                       ctypes.c_void_p(fit.ctypes.data), None, None, None, ctypes.byref(mem))
        msg_i = eng.lib.eigen_last_error().decode()
        from evolutionary_illusion_generator_amd import synth
        ncfg = synth.make_config(2, 1)
        gb = genome.GenomeBatch([g for _, g in synth.make_population(B, ncfg, seed=1)], ncfg, 1, n_leaves=2)
        s = eng._genome_struct(gb)
        rc_p = eng.lib.eigen_eval_population_dense_members(eng._h, ctypes.byref(s), ctypes.c_int32(2), ctypes.c_int32(1), ctypes.c_int32(1), ctypes.c_int32(0),
                                                           ctypes.byref(cfg), _p(mask), ctypes.c_void_p(fit.ctypes.data), None, None, None, ctypes.byref(mem))
        return rc_i, msg_i, rc_p, eng.lib.eigen_last_error().decode(), bool((fit == SENT).all())

    try:
        rc, msg, untouched = call(members())
        assert rc == 0 and not untouched, msg
        refused = ((members(kind=2), None, "flow members: unknown kind 2"), (members(reserved=1), None, "flow members: reserved must be 0, got 1"),
                   (members(max_corners=0), None, "flow members: max_corners 0 outside 1 .. 128"), (members(max_corners=129), None, "max_corners 129 outside 1 .. 128"),
                   (members(block_size=0), None, "flow members: block_size 0 outside 1 .. 9"), (members(block_size=10), None, "block_size 10 outside 1 .. 9"),
                   (members(quality_level=0.0), None, "quality_level 0: must be in (0, 1]"), (members(quality_level=1.5), None, "quality_level 1.5"),
                   (members(quality_level=float("nan")), None, "quality_level nan"), (members(min_distance=-1.0), None, "min_distance -1: must be finite and >= 0"),
                   (members(min_distance=float("inf")), None, "min_distance inf"), (members(mask_bstride=HW), None, "must be 0 with EIGEN_FLOW_MEMBERS_CORNERS"),
                   (members(kind=0, mask_bstride=HW), None, "EIGEN_FLOW_MEMBERS_MASK needs d_mask"),
                   (members(kind=0, mask_bstride=HW - 1), ones, "mask_bstride %d is smaller than one plane (%d bytes)" % (HW - 1, HW)),
                   (members(kind=0, mask_bstride=0), ones, "mask_bstride 0 is smaller than one plane"),
                   (members(kind=0, mask_bstride=HW), zeros, "the flow mask counts no pixel"),
                   (members(), zeros[0], "the flow mask counts no pixel"))
        for mem, mask, words in refused:
            rc, msg, untouched = call(mem, mask)
            assert rc == -1 and words in msg and untouched, (words, rc, msg, untouched)
            rc_i, msg_i, rc_p, msg_p, kept = population_calls(mem, mask)
            assert rc_i == -1 and rc_p == -1 and words in msg_i and words in msg_p and kept, (words, msg_i, msg_p)
        # the handle still works: corners, planes, and a call without members
        first = call(members())
        assert first[0] == 0 and call(members(kind=0, mask_bstride=HW), ones)[0] == 0
        plain = np.full(B, SENT)
        assert eng.lib.eigen_dense_score(eng._h, _p(d[0]), ctypes.c_int64(per), _p(d[1]), ctypes.c_int64(per), ctypes.c_int32(B), ctypes.byref(cfg), None,
                                         ctypes.c_void_p(plain.ctypes.data), None, None, None) == 0 and (plain != SENT).all()
        # a solve outside the accepted values is refused with members as without them
        solve = engine.DenseSolveC(7, 1)
        fit = np.full(B, SENT)
        mem = members()
        rc = eng.lib.eigen_dense_score_members(eng._h, _p(d[0]), ctypes.c_int64(per), _p(d[1]), ctypes.c_int64(per), ctypes.c_int32(B), ctypes.byref(cfg), None,
                                               ctypes.c_void_p(fit.ctypes.data), None, None, None, ctypes.byref(solve), ctypes.byref(mem), None, None)
        assert rc == -1 and "dense solve levels 7" in eng.lib.eigen_last_error().decode() and (fit == SENT).all()
    finally:
        eng.close()


def test_members_null_is_the_namesake(cuda):
    """`eigen_dense_score_members` with NULL members returns the bytes of `eigen_dense_score`, and all-ones planes those of no mask"""
    w, h = dm.PAIR_SHAPES[1]
    a, b = dm.pair_images(w, h)
    sc = dm.free_score()
    dense = dm.dense_of(sc, dm.PAIR_RADIUS)
    eng = Engine(w, h, [1], 3)       # one layer: 33 x 18 halves to nothing a PredNet could pool
    try:
        fit, rec = _score(eng, cuda, a, b, dense, stats=True)
        cfg, keep, _ = eng._dense_args(dense)
        d0, d1 = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
        f2, r2 = np.full(3, SENT), np.full((3, 10), SENT)
        assert eng.lib.eigen_dense_score_members(eng._h, _p(d0), ctypes.c_int64(h * w), _p(d1), ctypes.c_int64(h * w), ctypes.c_int32(3), ctypes.byref(cfg), None,
                                                 ctypes.c_void_p(f2.ctypes.data), ctypes.c_void_p(r2.ctypes.data), None, None, None, None, None, None) == 0
        assert f2.tobytes() == fit.tobytes() and r2.tobytes() == rec.tobytes()
        _, r3 = _score(eng, cuda, a, b, dm.dense_of(sc, dm.PAIR_RADIUS, members=np.ones((3, h, w), np.uint8)), stats=True)
        assert r3.tobytes() == rec.tobytes()
    finally:
        eng.close()
