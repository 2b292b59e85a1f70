"""The dense fitness on float frames on the GPU (eigen_dense_score_float, EIGEN_DENSE_FLOAT_FRAMES, eigen_debug_dense_gray,
fitness.DenseFitness(frames="float"); DESIGN.md section 14, "Float frames").  The bounds are `check_records` of
tests/test_gpu_dense_fitness.py: the field `np.array_equal`, N exact, every record sum within N 2^-53 sum |terms|, S_b within 1e-10 of the
restatement and exactly its formula on the device's record.  The float stage is the numpy restatement on unquantised images, the trainer's
stage bit for bit, the byte stage on float images that are bytes, alive where the byte stage is dead; the snapshots the roll-out takes are
the gray of the oracle's float P0, the emitted bytes do not move, the population path is the stage on the handle's own float pair, a
genome's fitness does not depend on its batch, and every refusal comes before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, fitness, genome, train
from evolutionary_illusion_generator_amd.engine import Engine, EngineError
from evolutionary_illusion_generator_amd.train import PredictionFlow, PredNetTrainer
from tests import dense_float_support as df
from tests import dense_fitness_support as ds
from tests import dense_members_support as dm
from tests import flow_corner_support as fc
from tests.flow_gpu_support import _padded
from tests.test_gpu_dense_fitness import check_records

pytestmark = pytest.mark.gpu

SENT = -12345.5


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _score(eng, cuda, img0, img1, dense, **kw):
    """`Engine.dense_score_float` on densely packed host images: img0 uint8 or float32, img1 float32"""
    B, C, h, w = img1.shape
    return eng.dense_score_float(_dev(img0, cuda), C * h * w, _dev(img1, cuda), C * h * w, B, dense, **kw)


# ---- 1. the stage against numpy
@pytest.mark.parametrize("c", df.FLOAT_CASES, ids=df.float_id)
def test_the_float_stage_is_the_numpy_restatement(cuda, c):
    """`Engine.dense_score_float` on unquantised images (a float prediction against a byte or a float reference) under the three scores,
    masked and not, radius 3 and 7: the field `np.array_equal`, the records by the bounds; the gray planes the stage started from are
    numpy's tflow_gray; a second call and padded strides give the same bytes and leave the padding alone."""
    pred, ref, ref64, mask, sc, r, want, _ = df.float_case(c)
    B, C, h, w = pred.shape
    per = C * h * w
    dense = df.dense_of(sc, r, mask, frames="float")
    eng = Engine(w, h, [C, 4], B + 1)
    try:
        fit, rec, u = _score(eng, cuda, ref, pred, dense, stats=True, flow=True)
        assert rec is eng.last_dense_stats
        I0, I1 = eng.last_dense_gray(B)
        assert np.array_equal(I0, df.gray64(ref)) and np.array_equal(I1, df.gray64(pred))
        again = _score(eng, cuda, ref, pred, df.dense_of(sc, r, mask))         # the entry is float by nature: either `frames` gives the same call
        assert again.tobytes() == fit.tobytes() and eng.last_dense_stats.tobytes() == rec.tobytes()
        assert np.array_equal(u, want.u), np.abs(u - want.u).max()
        check_records(rec, fit, want, sc)
        s0, s1 = per + 3, per + 5
        p0, p1 = _padded(ref, s0, ref.dtype.type(0.25 if ref.dtype == np.float32 else 7), cuda), _padded(pred, s1, np.float32(0.75), cuda)
        f2, r2, u2 = eng.dense_score_float(p0, s0, p1, s1, B, dense, stats=True, flow=True)
        assert f2.tobytes() == fit.tobytes() and r2.tobytes() == rec.tobytes() and u2.tobytes() == u.tobytes()
        assert (p0.cpu().numpy()[per:s0] == p0.cpu().numpy()[-1]).all() and (p1.cpu().numpy()[per:s1] == np.float32(0.75)).all()
    finally:
        eng.close()
    print("float stage %s: N %s S %s" % (df.float_id(c), rec[:, 0].astype(int).tolist(), rec[:, 8].tolist()))


# ---- 2. the stage is the trainer's, bit for bit
def _trainer_record(C, w, h, B, pred, ref, flow):
    with PredNetTrainer("synthetic", [C, 4], w, h, B, 2) as tr:
        out = tr.flow_term(pred, ref, flow) if ref.dtype == np.uint8 else tr.flow_term_pair(pred, ref, flow)
        return out[1], tr.last_flow_stats


TRAINER_CASES = [c for c in df.FLOAT_CASES if (c.kind, c.ref_kind) in (("circles", "floats"), ("circles", "bytes"), ("bands", "floats"), ("free", "floats"))
                 and (c.kind != "free" or c.w == 16) and (c.kind != "circles" or c.masked)]


@pytest.mark.parametrize("c", TRAINER_CASES, ids=df.float_id)
def test_the_float_stage_is_the_trainers_stage(cuda, c):
    """On the same arrays `PredNetTrainer.flow_term_pair(pred, prev, flow)` (a byte reference: `flow_term(pred, ref_bytes, flow)`) leaves the
    record bytes and the field bytes of `dense_score_float`: all three structures, a shared mask, and the byte-img0 form."""
    pred, ref, ref64, mask, sc, r, want, _ = df.float_case(c)
    B, C, h, w = pred.shape
    dense = df.dense_of(sc, r, mask, frames="float")
    eng = Engine(w, h, [C, 4], B)
    try:
        fit, rec, u = _score(eng, cuda, ref, pred, dense, stats=True, flow=True)
    finally:
        eng.close()
    tu, trec = _trainer_record(C, w, h, B, pred, ref, PredictionFlow(r, df.EPS, mask=mask).scored(dense.score))
    assert tu.tobytes() == u.tobytes() and trec.tobytes() == rec.tobytes() and rec[:, 8].any()


@pytest.mark.parametrize("kind", fc.SCORES)
def test_the_float_stage_under_members_is_the_trainers(cuda, kind):
    """Under `CornerMembers` (picked on the byte image of the float reference, as the trainer's membership stage does) and under per-sample
    planes, on a float pair that is no byte over 255: the record and field bytes of `flow_term_pair` with the same members."""
    w, h, C, r = fc.SHAPES[1]
    pred, prev, _, _ = fc.stage_inputs(w, h, C, "floats")
    B = pred.shape[0]
    sc = fc.score_of(kind, h)
    planes = fc.random_masks(w, h)[:B]
    eng = Engine(w, h, [C, 4], B)
    try:
        for members in (fc.corner_members(), planes):
            fit, rec, u = _score(eng, cuda, prev, pred, df.dense_of(sc, r, None, members, frames="float"), stats=True, flow=True)
            if isinstance(members, np.ndarray):
                flow = fc.flow_of(sc, r, planes, pairing="prediction")
            else:
                flow = fc.flow_of(sc, r, None, pairing="prediction", members=members)
            tu, trec = _trainer_record(C, w, h, B, pred, prev, flow)
            assert tu.tobytes() == u.tobytes() and trec.tobytes() == rec.tobytes() and rec[:, 0].any()
    finally:
        eng.close()


@pytest.mark.parametrize("solve", [(1, 1), (2, 2), (3, 3)], ids=dm.solve_id)
def test_the_float_stage_under_the_iterated_solve_is_the_trainers(cuda, solve):
    """48 x 32 (the coarsest of three levels is 12 x 8), a float pair, Circles: `levels, iters` = (1, 1) through the iteration kernel's
    namesake, (2, 2) and (3, 3) give the record and field bytes of the trainer's `.solved(levels, iters)`, and the numpy restatement's
    field."""
    w, h, C, r = fc.SHAPES[2]
    pred, prev, _, _ = fc.stage_inputs(w, h, C, "floats")
    B = pred.shape[0]
    sc = fc.score_of("circles", h)
    eng = Engine(w, h, [C, 4], B)
    try:
        fit, rec, u = _score(eng, cuda, prev, pred, df.dense_of(sc, r, solve=solve, frames="float"), stats=True, flow=True)
        I0, I1 = eng.last_dense_gray(B)
    finally:
        eng.close()
    assert np.array_equal(I0, df.gray64(prev)) and np.array_equal(I1, df.gray64(pred))
    tu, trec = _trainer_record(C, w, h, B, pred, prev, fc.flow_of(sc, r, None, pairing="prediction").solved(*solve))
    assert tu.tobytes() == u.tobytes() and trec.tobytes() == rec.tobytes() and rec[:, 8].any()
    want = df.restate_gray(sc, prev, pred, r, None, solve)
    assert np.array_equal(u, want.u)
    check_records(rec, fit, want, sc)


# ---- 3. float images that are bytes
BYTE_CASES = [("circles", ds.CIRCLES_CASES[5]), ("bands", next(c for c in ds.STRUCT_CASES if c.kind == "bands" and c.masked and c.min_count == 25)),
              ("free", next(c for c in ds.STRUCT_CASES if c.kind == "free" and c.masked))]


@pytest.mark.parametrize("kind,c", BYTE_CASES, ids=[k for k, _ in BYTE_CASES])
def test_float_images_that_are_bytes_give_the_byte_stage(cuda, kind, c):
    """On `as_float(img)` of byte stage cases `dense_score_float` returns `eigen_dense_score`'s fitness, records and field, byte for byte:
    with both images as floats and with img0 as the bytes themselves, under the single step and under 2 x 2."""
    case = ds.circles_case(*c) if kind == "circles" else ds.struct_case(c)
    img0, img1, pred, ref64, mask, sc, r, want = case
    B, C, h, w = img0.shape
    eng = Engine(w, h, [C, 4], B)
    try:
        for solve in ((1, 1), (2, 2)):
            dense = df.dense_of(sc, r, mask, solve=solve)
            fit, rec, u = eng.dense_score(_dev(img0, cuda), C * h * w, _dev(img1, cuda), C * h * w, B, dense, stats=True, flow=True)
            for first in (ds.as_float(img0)[0], img0):
                f2, r2, u2 = _score(eng, cuda, first, ds.as_float(img1)[0], dense, stats=True, flow=True)
                assert f2.tobytes() == fit.tobytes() and r2.tobytes() == rec.tobytes() and u2.tobytes() == u.tobytes()
            assert solve != (1, 1) or rec[:, 8].any()      # the cases' max_norm is the single step's: alive there
    finally:
        eng.close()


# ---- 4. the sub-byte case
@pytest.mark.parametrize("shape", df.SUB_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_sub_byte_case(cuda, shape):
    """Two float images that quantise to the same bytes: the byte stage on those bytes leaves an all-zero field and record, the float
    stage the restatement's field bit for bit and its records by the bounds, every sample alive."""
    w, h, C = shape
    case = df.sub_byte_case(w, h, C)
    dense = df.dense_of(case.score, df.SUB_RADIUS)
    eng = Engine(w, h, [C, 4], df.B)
    try:
        d_b = _dev(case.b, cuda)
        fit, rec, u = eng.dense_score(d_b, C * h * w, d_b, C * h * w, df.B, dense, stats=True, flow=True)
        assert not u.any() and not rec.any() and not fit.any()
        fit, rec, u = _score(eng, cuda, case.f0, case.f1, dense.on_frames("float"), stats=True, flow=True)
    finally:
        eng.close()
    assert np.array_equal(u, case.want_float.u)
    check_records(rec, fit, case.want_float, case.score)
    assert (rec[:, 0] >= case.score.min_count).all() and (fit != 0).all()
    print("sub-byte %dx%dx%d: N %s S %s" % (w, h, C, rec[:, 0].astype(int).tolist(), fit.tolist()))


# ---- 5. the snapshots
def _e2e_engine(w, h, ch, structure, max_batch, **kw):
    eng = Engine(w, h, list(ch), max_batch, **kw)
    eng.set_weights(ds.e2e_weights(w, h, ch))
    eng.set_grid(fitness.leaf_planes(ds.grid_structure(structure, w, h), w, h, 2))
    return eng


def _emitted(eng, cuda, d_img, n, C, h, w, pairing, nr=20):
    """the frames `prednet_rollout` emits for a pairing, uint8 [n, n_out, C, h, w]"""
    n_steps, first = (nr + 1, nr - 1) if pairing == ds.PAIR_POPULATION else (nr + 2, nr + 1)
    d_fr = torch.zeros((n, n_steps - first, C, h, w), dtype=torch.uint8, device=cuda)
    eng.prednet_rollout(d_img, n, n_steps, first, d_fr)
    return d_fr.cpu().numpy()


@pytest.mark.parametrize("shape", ds.E2E_SHAPES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("pairing", [ds.PAIR_POPULATION, ds.PAIR_SINGLE], ids=["population", "single"])
def test_the_snapshots_are_the_gray_of_the_oracles_float_predictions(cuda, shape, pairing):
    """After `eval_images(dense=float)` under live weights, `last_dense_gray()` is numpy's tflow_gray of the oracle's float P0 at the
    pair's steps (the input bytes for img0 under the single pairing), bit for bit, under the single step and under the iterated solve;
    the frames the roll-out emits are `(uint8)(int)(P0 255.0f)` of those floats, every byte, and the bytes a call without the flag emits."""
    w, h, ch = shape
    n, C, nr = ds.E2E_GENOMES, ch[0], 20
    images, frames, p0 = df.oracle_float_case(w, h, ch, 1)
    img0, img1 = df.float_pair(images, p0, pairing)
    eng = _e2e_engine(w, h, ch, 1, n)
    try:
        d_img = _dev(images, cuda)
        before = _emitted(eng, cuda, d_img, n, C, h, w, pairing)
        byte_fit, _ = eng.eval_images(d_img, n, 1, pairing=pairing, dense=df.e2e_dense(1, frames="byte"))
        for solve in ((1, 1), (2, 2)):
            fit, _ = eng.eval_images(d_img, n, 1, pairing=pairing, dense=df.e2e_dense(1, levels=solve[0], iters=solve[1]))
            I0, I1 = eng.last_dense_gray(n)
            assert np.array_equal(I0, df.gray64(img0)) and np.array_equal(I1, df.gray64(img1)), solve
        after = _emitted(eng, cuda, d_img, n, C, h, w, pairing)
        again, _ = eng.eval_images(d_img, n, 1, pairing=pairing, dense=df.e2e_dense(1, frames="byte"))
    finally:
        eng.close()
    first = nr - 1 if pairing == ds.PAIR_POPULATION else nr + 1
    assert np.array_equal(before, df.quantise(p0[:, first:first + before.shape[1]])) and np.array_equal(before, frames[:, first:first + before.shape[1]])
    assert after.tobytes() == before.tobytes() and again.tobytes() == byte_fit.tobytes()


# ---- 6. end to end
E2E = [(shape, s, p) for shape, s in ds.E2E_CASES for p in (ds.PAIR_POPULATION, ds.PAIR_SINGLE)]
e2e_id = lambda c: "%dx%d-s%d-%s" % (c[0][0], c[0][1], c[1], "population" if c[2] == ds.PAIR_POPULATION else "single")
VARIANTS = (("all", {}), ("corners", dict(members=True)), ("2x2", dict(levels=2, iters=2)))


@pytest.mark.parametrize("c", E2E, ids=e2e_id)
def test_the_population_path_on_float_frames(cuda, c):
    """7 genomes under live weights, `eval_population(dense=DenseFitness.for_structure(s, frames="float", ...))`, with every pixel, with
    `CornerMembers()` and with levels = iters = 2: the fitness and the records are `dense_score_float` on the handle's own float pair
    (the oracle's float P0, which the snapshot test holds the handle's gray planes to, and the emitted or input bytes for the corners),
    bit for bit, and the restatement on the oracle's floats by the bounds; `eval_images` gives the same bytes; the slices [0, 3), [3, 6),
    [6, 7) give the bytes of the batch of 7, and `fitness.evaluate_population(max_batch=3)` those of `max_batch=7`."""
    (w, h, ch), structure, pairing = c
    n, C, nr = ds.E2E_GENOMES, ch[0], 20
    per = C * h * w
    images, frames, p0 = df.oracle_float_case(w, h, ch, structure)
    img0, img1 = df.float_pair(images, p0, pairing)
    sc = ds.e2e_restatement_score(structure, h)
    gb = genome.GenomeBatch(ds.e2e_genomes(), ds.e2e_config(), C, n_leaves=2)
    eng = _e2e_engine(w, h, ch, structure, n)
    try:
        d_img = torch.zeros((n, C, h, w), dtype=torch.uint8, device=cuda)
        eng.render_cppn(gb, d_img, bg=1, gradient=1)
        assert np.array_equal(d_img.cpu().numpy(), images)
        for name, kw in VARIANTS:
            kw = dict(kw, members=train.CornerMembers()) if "members" in kw else kw
            dense = df.e2e_dense(structure, **kw)
            fit = eng.eval_population(gb, structure, pairing=pairing, dense=dense)
            rec = eng.last_dense_stats
            I0, I1 = eng.last_dense_gray(n)
            assert np.array_equal(I0, df.gray64(img0)) and np.array_equal(I1, df.gray64(img1))
            fit3, vecs = eng.eval_images(d_img, n, structure, pairing=pairing, dense=dense)
            assert fit3.tobytes() == fit.tobytes() and eng.last_dense_stats.tobytes() == rec.tobytes() and len(vecs) == n
            parts = np.concatenate([eng.eval_population(gb.slice(lo, hi), structure, pairing=pairing, dense=dense) for lo, hi in ((0, 3), (3, 6), (6, 7))])
            assert parts.tobytes() == fit.tobytes()
            # the stage alone on the float pair; under corner members a float img0 is quantised to the emitted frame, which is what the path reads
            fit2, rec2 = _score(eng, cuda, img0, img1, dense, stats=True)
            assert fit2.tobytes() == fit.tobytes() and rec2.tobytes() == rec.tobytes(), name
            planes = None
            if name == "corners":
                planes = df.oracle_planes(images if pairing == ds.PAIR_SINGLE else frames[:, nr - 1], dense.members)
            want = df.restate_gray(sc, img0, img1, ds.E2E_RADIUS, planes, (dense.levels, dense.iters))
            check_records(rec, fit, want, sc)
            print("float end to end %s %s: N %s fitness %s" % (e2e_id(c), name, rec[:, 0].astype(int).tolist(), fit.tolist()))
            if name == "all":
                assert (fit != 0).any(), fit
    finally:
        eng.close()
    kw = dict(c_dim=C, pairing=pairing, score=df.e2e_dense(structure))
    try:
        whole = fitness.evaluate_population(structure, ds.e2e_genomes(), ds.e2e_weights(w, h, ch), ds.e2e_config(), w, h, list(ch), max_batch=7, **kw)
        split = fitness.evaluate_population(structure, ds.e2e_genomes(), ds.e2e_weights(w, h, ch), ds.e2e_config(), w, h, list(ch), max_batch=3, **kw)
    finally:
        fitness.clear_engines()
    assert whole.shape == (n,) and split.tobytes() == whole.tobytes()


# ---- 7. nothing else moved
def test_the_byte_and_sparse_paths_are_untouched(cuda):
    """After float dense calls (single step and iterated, all pixels and corners) the handle's byte dense call and its sparse `eval_images`
    return the bytes they returned before them."""
    w, h, ch = ds.E2E_SHAPES[1]
    n, C = ds.E2E_GENOMES, ch[0]
    imgs = _dev(np.random.default_rng(5).integers(0, 256, (n, C, h, w), dtype=np.uint8), cuda)
    eng = _e2e_engine(w, h, ch, 1, n)
    try:
        byte = [df.e2e_dense(1, frames="byte"), df.e2e_dense(2, frames="byte", levels=2, iters=2, members=train.CornerMembers())]
        want = [(eng.eval_images(imgs, n, s, dense=d)[0], eng.last_dense_stats) for s, d in zip((1, 2), byte)]
        want_i, want_v = eng.eval_images(imgs, n, 2)
        for s, kw in ((1, {}), (2, dict(levels=2, iters=2)), (2, dict(members=train.CornerMembers())), (0, {})):
            for pairing in (ds.PAIR_POPULATION, ds.PAIR_SINGLE):
                eng.eval_images(imgs, n, s, pairing=pairing, dense=df.e2e_dense(s, **kw))
        got = [(eng.eval_images(imgs, n, s, dense=d)[0], eng.last_dense_stats) for s, d in zip((1, 2), byte)]
        got_i, got_v = eng.eval_images(imgs, n, 2)
    finally:
        eng.close()
    for (a, ra), (b, rb) in zip(want, got):
        assert a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes()
    assert got_i.tobytes() == want_i.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(got_v, want_v))
    assert any(a.any() for a, _ in want) or want_i.any()


# ---- 8. refusals
def test_refusals(cuda):
    """Each before any launch, the outputs untouched and the records of the earlier call intact: the flag on `eigen_dense_score` (the
    message names eigen_dense_score_float), flags 1, 3 and 4 on an eval entry, both or neither img0, a float img0 stride below C H W, a
    pairing n_ext cannot serve, and `eigen_debug_dense_gray` before any float call and with another batch."""
    w, h, C, B = 16, 12, 1, 2
    per = C * h * w
    eng = Engine(w, h, [C, 4], B)
    d8 = torch.zeros((B + 1, C, h, w), dtype=torch.uint8, device=cuda)
    rng = np.random.default_rng(3)
    f0, f1 = (_dev(rng.random((B, C, h, w)).astype(np.float32), cuda) for _ in range(2))
    sc = train.FlowScore().settings(h)

    def settings(flags):
        return engine.DenseSettingsC(engine.FlowSettingsC(3, flags, 1e-2), ctypes.addressof(sc), None)

    def refused(rc, fit, words):
        msg = eng.lib.eigen_last_error().decode()
        assert rc == -1 and words in msg and (fit == SENT).all(), (rc, msg)

    try:
        with pytest.raises(EngineError, match="no float dense call"):
            eng.last_dense_gray(B)
        dense = fitness.DenseFitness(train.FlowScore(min_count=2), radius=3, frames="float")
        ok = eng.dense_score_float(f0, per, f1, per, B, dense)
        kept = eng.last_dense_gray(B)
        with pytest.raises(EngineError, match="batch of 2, not 1"):
            eng.last_dense_gray(1)
        # the flag on the byte stage, through the binding and raw
        with pytest.raises(EngineError, match="eigen_dense_score_float"):
            eng.dense_score(d8, per, d8, per, B, dense)
        for entry, tail in ((eng.lib.eigen_dense_score, ()), (eng.lib.eigen_dense_score_iter, (None,)), (eng.lib.eigen_dense_score_members, (None, None, None, None))):
            fit, cfg = np.full(B, SENT), settings(df.DENSE_FLOAT_FRAMES)
            refused(entry(eng._h, engine._ptr(d8), ctypes.c_int64(per), engine._ptr(d8), ctypes.c_int64(per), ctypes.c_int32(B), ctypes.byref(cfg), None, engine._ptr(fit), None, None, None, *tail),
                    fit, "eigen_dense_score_float")
        for flags in (1, 3, 4):
            fit, cfg = np.full(B, SENT), settings(flags)
            refused(eng.lib.eigen_eval_images_dense(eng._h, engine._ptr(d8), ctypes.c_int32(B), ctypes.c_int32(1), ctypes.c_int32(ds.PAIR_POPULATION), ctypes.byref(cfg), None,
                                                    engine._ptr(fit), None, None), fit, "flow flags 0x%x" % flags)
            fit = np.full(B, SENT)
            refused(eng.lib.eigen_dense_score_float(eng._h, None, engine._ptr(f0), ctypes.c_int64(per), engine._ptr(f1), ctypes.c_int64(per), ctypes.c_int32(B), ctypes.byref(cfg), None, None,
                                                    None, engine._ptr(fit), None, None, None), fit, "flow flags 0x%x" % flags)
        cfg = settings(0)
        for a, b, s0, words in ((d8, f0, per, "exactly one of d_img0"), (None, None, per, "exactly one of d_img0"), (None, f0, per - 1, "smaller than one image")):
            fit = np.full(B, SENT)
            refused(eng.lib.eigen_dense_score_float(eng._h, engine._ptr(a), engine._ptr(b), ctypes.c_int64(s0), engine._ptr(f1), ctypes.c_int64(per), ctypes.c_int32(B), ctypes.byref(cfg), None, None,
                                                    None, engine._ptr(fit), None, None, None), fit, words)
        with pytest.raises(ValueError, match="float32"):
            eng.dense_score_float(f0, per, d8, per, B, dense)
        # nothing above launched anything: the planes and the fitness of the earlier call are what they were
        now = eng.last_dense_gray(B)
        assert now[0].tobytes() == kept[0].tobytes() and now[1].tobytes() == kept[1].tobytes()
        assert eng.dense_score_float(f0, per, f1, per, B, dense).tobytes() == ok.tobytes()
    finally:
        eng.close()
    short = Engine(w, h, [C, 4], B, n_ext=1)
    try:
        with pytest.raises(EngineError, match="pairing needs 2 extension steps"):
            short.eval_images(d8, B, 1, pairing=engine.PAIR_SINGLE, dense=fitness.DenseFitness.for_structure(1, frames="float"))
        with pytest.raises(EngineError, match="no float dense call"):
            short.last_dense_gray(B)
    finally:
        short.close()
