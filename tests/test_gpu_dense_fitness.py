"""The dense motion fitness on the GPU (eigen_dense_score, eigen_eval_population_dense, eigen_eval_images_dense, fitness.DenseFitness;
DESIGN.md section 14).  The stage alone is compared with the numpy restatements of tests/flow_score_support.py and
tests/flow_struct_support.py on the float images of its bytes, by the bounds of tests/test_gpu_flow_score.py and
tests/test_gpu_flow_struct.py: the field bit for bit, N exact, every record sum within N 2^-53 sum |terms|, S_b within 1e-10.  It is the
trainer's stage bit for bit, the population path is the stage on the frames the roll-out emits, a genome's fitness does not depend on its
batch, and the sparse path of a handle is untouched by a dense call."""
import ctypes
import math

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, fitness, genome
from evolutionary_illusion_generator_amd.engine import Engine, EngineError
from evolutionary_illusion_generator_amd.train import PredictionFlow, PredNetTrainer
from tests import dense_fitness_support as ds
from tests import flow_score_support as ss
from tests import flow_struct_support as st
from tests.flow_gpu_support import _p, _padded

pytestmark = pytest.mark.gpu

SENT = -12345.5


def _sum_bound(terms):
    """(the exact sum, N 2^-53 sum |terms|: the bound of a double-precision sum of the N terms in any order)"""
    t = np.asarray(terms, np.float64).ravel().tolist()
    return math.fsum(t), len(t) * 2.0 ** -53 * math.fsum(abs(v) for v in t)


def check_records(rec, fit, want, sc, L=None):
    """The bounds of the stage tests of the score mode and of the structure scores on the records [n, 10] of one dense call against the
    restatement `want` of the same images: N exact; every first-pass sum N m within N 2^-53 sum |terms| of the exactly summed one, every
    second-pass sum likewise against the exactly summed terms formed from the device's own means; S_b within 1e-10 of the restatement's
    and exactly what the restatement's formula gives on the device's record; the fitness is S_b; a sample below min_count scores exactly 0.
    L: the device's L planes [n, H, W] of a Free case where they were read back: the swarm sum is then checked against them."""
    pts, n = want.score.points, rec.shape[0]
    assert rec.shape == (n, 10) and np.isfinite(rec).all() and not rec[:, 9].any()
    assert np.array_equal(rec[:, 0], want.score.record[:, 0]), (rec[:, 0], want.score.record[:, 0])
    assert fit.tobytes() == np.ascontiguousarray(rec[:, 8]).tobytes()
    for b in range(n):
        N, m = rec[b, 0], pts.member[b]
        if N == 0:
            assert not rec[b].any()
            continue
        if isinstance(sc, ss.Score):
            cols = [pts.rho[b][m], pts.tau[b][m], np.abs(want.u[b, 0][m]), pts.nrm[b][m]]
            first, at1 = cols, 1
            second, at2 = [(t - mean) * (t - mean) for t, mean in ((cols[0], rec[b, 1]), (cols[1], rec[b, 2]), (cols[3], rec[b, 4]))], 5
            mine = ss.sample_value(rec[b], sc)
        else:
            first, second = st.sample_columns(want.u, pts, sc, b, None if st.is_bands(sc) else want.score.pairs[b], rec[b])
            at1, at2, second = 1, 3, second[:1]         # Free's swarm sum is made of the device's L
            r = rec[b].copy()
            st.fill_value(r, sc)
            mine = r[8]
            assert rec[b, 5] == r[5] and not rec[b, 6:8].any() and (not st.is_bands(sc) or not rec[b, 4:6].any())
            if L is not None:
                exact, bound = _sum_bound((st.PI - L[b][m] / N) / st.PI)
                assert abs(N * rec[b, 4] - exact) <= bound, (b, N * rec[b, 4], exact, bound)
        for k, t in enumerate(first):
            exact, bound = _sum_bound(t)
            assert abs(N * rec[b, at1 + k] - exact) <= bound, (b, k, N * rec[b, at1 + k], exact, bound)
        for k, t in enumerate(second):
            exact, bound = _sum_bound(t)
            assert abs(N * rec[b, at2 + k] - exact) <= bound, (b, k, N * rec[b, at2 + k], exact, bound)
        assert abs(rec[b, 8] - want.score.S[b]) <= 1e-10, (b, rec[b, 8], want.score.S[b])
        assert rec[b, 8] == mine, (b, rec[b, 8], mine)
        assert (rec[b, 8] == 0.0) == bool(N < sc.min_count)


def _raw_dense(eng, d0, s0, d1, s1, B, dense, d_mask, fit, rec, d_flow):
    """eigen_dense_score called directly on device buffers; fit, rec: numpy or None"""
    cfg, keep, _ = eng._dense_args(dense)
    return eng.lib.eigen_dense_score(eng._h, _p(d0), ctypes.c_int64(s0), _p(d1), ctypes.c_int64(s1), ctypes.c_int32(B), ctypes.byref(cfg), _p(d_mask),
                                     None if fit is None else ctypes.c_void_p(fit.ctypes.data), None if rec is None else ctypes.c_void_p(rec.ctypes.data),
                                     _p(d_flow), None)


def _stage(cuda, case, kind):
    """one stage case through Engine.dense_score, densely packed and on padded strides"""
    img0, img1, pred, ref64, mask, sc, r, want = case
    B, C, h, w = img0.shape
    per = C * h * w
    dense = ds.dense_of(sc, r, mask)
    with_L = None
    eng = Engine(w, h, [C, 4], B + 1)
    try:
        d0, d1 = torch.from_numpy(img0).to(cuda), torch.from_numpy(img1).to(cuda)
        fit, rec, u = eng.dense_score(d0, per, d1, per, B, dense, stats=True, flow=True)
        assert rec is eng.last_dense_stats
        again = eng.dense_score(d0, per, d1, per, B, dense)
        assert again.tobytes() == fit.tobytes() and eng.last_dense_stats.tobytes() == rec.tobytes()
        assert np.array_equal(u, want.u), np.abs(u - want.u).max()
        if kind == "free":
            # the pair pass cannot be read back from an inference handle: the trainer's stage on the same images leaves the same record,
            # bit for bit, and ITS planes are read back and held to the pair-pass rules of tests/test_gpu_flow_struct.py
            with PredNetTrainer("synthetic", [C, 4], w, h, B + 1, 2) as tr:
                flow = PredictionFlow(r, ds.EPS, mask=mask).scored(dense.score)
                tr.flow_term_pair(pred, ds.as_float(img0)[0], flow)
                assert tr.last_flow_stats.tobytes() == rec.tobytes()
                pl = tr.free_planes(B)
            pts = want.score.points
            assert np.array_equal(pl["member"], pts.member)
            for b in range(B):
                m = pts.member[b]
                assert not pl["theta"][b][~m].any() and not pl["L"][b][~m].any()
                if not m.any():
                    continue
                mine = want.score.pairs[b]
                assert np.abs(pl["theta"][b][m] - mine.theta).max() <= 2 * 2.0 ** -51
                fed = st.free_pairs(pts.nx[b], m, sc.max_distance * sc.max_distance, theta=pl["theta"][b])
                got = pl["L"][b][m]
                for i in range(int(m.sum())):
                    t = fed.terms[i][fed.terms[i] != 0]
                    exact = math.fsum(t.tolist())
                    assert abs(got[i] - exact) <= len(t) * 2.0 ** -53 * exact, (b, i, got[i], exact)
            with_L = pl["L"]
        check_records(rec, fit, want, sc, with_L)
        # padded strides: the same bits, and nothing is written outside the outputs
        s0, s1 = per + 3, per + 5
        p0, p1 = _padded(img0, s0, np.uint8(7), cuda), _padded(img1, s1, np.uint8(201), cuda)
        d_mask = None if mask is None else dense.mask_on(torch, 0, h, w)
        d_flow = torch.full((B * 2 * h * w + 4,), SENT, dtype=torch.float64, device=cuda)
        f2, r2 = np.full(B + 1, SENT), np.full((B + 1, 10), SENT)
        assert _raw_dense(eng, p0, s0, p1, s1, B, dense, d_mask, f2, r2, d_flow) == 0, eng.lib.eigen_last_error()
        uu = d_flow.cpu().numpy()
        assert (uu[B * 2 * h * w:] == SENT).all() and uu[:B * 2 * h * w].tobytes() == u.tobytes()
        assert f2[:B].tobytes() == fit.tobytes() and f2[B] == SENT and r2[:B].tobytes() == rec.tobytes() and (r2[B] == SENT).all()
        assert bytes(p0.cpu().numpy()[per:s0]) == bytes([7, 7, 7]) and bytes(p1.cpu().numpy()[per:s1]) == bytes([201] * 5)
        # every output is optional: the fitness alone comes back as one double per sample
        f3 = np.full(B + 1, SENT)
        assert _raw_dense(eng, p0, s0, p1, s1, B, dense, d_mask, f3, None, None) == 0
        assert f3.tobytes() == f2.tobytes()
        assert _raw_dense(eng, p0, s0, p1, s1, B, dense, d_mask, None, None, None) == 0
    finally:
        eng.close()
    return rec


@pytest.mark.parametrize("c", ds.CIRCLES_CASES, ids=ds.circles_id)
def test_the_circles_stage_is_the_numpy_restatement(cuda, c):
    """`Engine.dense_score` under a FlowScore on the byte pairs of the score mode's stage cases (12 x 8 to 40 x 24, C 1 and 3, r 2 / 3 / 7 /
    16, masked and not, min_count 4 and 25): u `np.array_equal`, N exact, the record sums within N 2^-53 sum |terms|, S_b within 1e-10;
    padded strides give the same bits and leave the padding alone."""
    rec = _stage(cuda, ds.circles_case(*c), "circles")
    print("dense stage %s: N %s S %s" % (ds.circles_id(c), rec[:, 0].astype(int).tolist(), rec[:, 8].tolist()))


@pytest.mark.parametrize("c", ds.STRUCT_CASES, ids=st.stage_id)
def test_the_structure_stage_is_the_numpy_restatement(cuda, c):
    """Likewise under a BandsScore and a FreeScore on the byte pairs of the structure scores' stage cases; for Free the pair pass is held
    to the rules of tests/test_gpu_flow_struct.py on the planes of the trainer's stage, whose record is the dense stage's bit for bit."""
    rec = _stage(cuda, ds.struct_case(c), c.kind)
    print("dense stage %s: N %s S %s" % (st.stage_id(c), rec[:, 0].astype(int).tolist(), rec[:, 8].tolist()))


TRAINER_CASES = [("circles", ds.CIRCLES_CASES[5]), ("bands", next(c for c in ds.STRUCT_CASES if c.kind == "bands" and c.masked and c.min_count == 25)),
                 ("free", next(c for c in ds.STRUCT_CASES if c.kind == "free" and c.masked))]


@pytest.mark.parametrize("kind,c", TRAINER_CASES, ids=[k for k, _ in TRAINER_CASES])
def test_the_stage_is_the_trainers_stage(cuda, kind, c):
    """On the same images `PredNetTrainer.flow_term_pair(img1 / 255, img0 / 255, flow)` gives the same u bytes and the same record bytes,
    and its value is the mean of the dense S_b as the trainer forms it: added in sample order, then divided by the batch."""
    case = ds.circles_case(*c) if kind == "circles" else ds.struct_case(c)
    img0, img1, pred, ref64, mask, sc, r, want = case
    B, C, h, w = img0.shape
    dense = ds.dense_of(sc, r, mask)
    eng = Engine(w, h, [C, 4], B)
    try:
        fit, rec, u = eng.dense_score(torch.from_numpy(img0).to(cuda), C * h * w, torch.from_numpy(img1).to(cuda), C * h * w, B, dense, stats=True, flow=True)
    finally:
        eng.close()
    with PredNetTrainer("synthetic", [C, 4], w, h, B, 2) as tr:
        value, tu, _ = tr.flow_term_pair(pred, ds.as_float(img0)[0], PredictionFlow(r, ds.EPS, mask=mask).scored(dense.score))
        trec = tr.last_flow_stats
    assert tu.tobytes() == u.tobytes() and trec.tobytes() == rec.tobytes()
    total = fit[0]
    for b in range(1, B):
        total = total + fit[b]
    assert value == total / float(B)


E2E = [(shape, s, p) for shape, s in ds.E2E_CASES for p in (ds.PAIR_POPULATION, ds.PAIR_SINGLE)]
e2e_id = lambda c: "%dx%d-s%d-%s" % (c[0][0], c[0][1], c[1], "population" if c[2] == ds.PAIR_POPULATION else "single")


def _e2e_engine(w, h, ch, structure, max_batch):
    eng = Engine(w, h, list(ch), max_batch)
    eng.set_weights(ds.e2e_weights(w, h, ch))
    eng.set_grid(fitness.leaf_planes(ds.grid_structure(structure, w, h), w, h, 2))
    return eng


@pytest.mark.parametrize("c", E2E, ids=e2e_id)
def test_the_population_path_is_the_stage_on_the_emitted_frames(cuda, c):
    """7 genomes under "live" weights: `eval_population(dense=...)` equals `dense_score` on the frames `render_cppn` + `prednet_rollout`
    return for the same genomes, bit for bit, and the numpy restatement on those frames by the bounds of the stage test; at least half of
    the samples are live; `eval_images(dense=...)` on the rendered images gives the same bytes; a genome's fitness does not depend on the
    batch it is in: the slices [0, 3), [3, 6), [6, 7) give the bytes of the batch of 7 through the engine, and
    `fitness.evaluate_population(..., score=..., max_batch=3)` gives the bytes of `max_batch=7` under every structure; those are the engine's
    bytes above wherever the renders above are on the structure's own grid (`dense_fitness_support.grid_structure`: all but Bands at
    16 x 12 and 48 x 32, whose own grid is constant and whose live check renders on the Circles grid)."""
    (w, h, ch), structure, pairing = c
    n, C, nr = ds.E2E_GENOMES, ch[0], 20
    per = C * h * w
    dense = ds.e2e_dense(structure)
    sc = ds.e2e_restatement_score(structure, h)
    gb = genome.GenomeBatch(ds.e2e_genomes(), ds.e2e_config(), C, n_leaves=2)
    eng = _e2e_engine(w, h, ch, structure, n)
    try:
        fit = eng.eval_population(gb, structure, pairing=pairing, dense=dense)
        rec = eng.last_dense_stats
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
        fit2, rec2 = eng.dense_score(d0, s0, d1, s1, n, dense, stats=True)
        assert fit2.tobytes() == fit.tobytes() and rec2.tobytes() == rec.tobytes()
        fit3, vecs = eng.eval_images(d_img, n, structure, pairing=pairing, dense=dense)
        assert fit3.tobytes() == fit.tobytes() and eng.last_dense_stats.tobytes() == rec.tobytes() and len(vecs) == n
        parts = np.concatenate([eng.eval_population(gb.slice(lo, hi), structure, pairing=pairing, dense=dense) for lo, hi in ((0, 3), (3, 6), (6, 7))])
        assert parts.tobytes() == fit.tobytes()
    finally:
        eng.close()
    want = ds.restate(sc, ds.as_float(img1)[0], ds.as_float(img0)[1], ds.E2E_RADIUS, None)
    check_records(rec, fit, want, sc)
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
    print("dense end to end %s: N %s fitness %s" % (e2e_id(c), rec[:, 0].astype(int).tolist(), fit.tolist()))


def test_the_default_path_is_untouched(cuda):
    """A sparse `eval_population` after a dense one on the same handle returns the bytes a fresh handle returns, and so does `eval_images`
    with its vectors."""
    w, h, ch = ds.E2E_SHAPES[1]
    n, C = ds.E2E_GENOMES, ch[0]
    gb = genome.GenomeBatch(ds.e2e_genomes(), ds.e2e_config(), C, n_leaves=2)
    imgs = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (n, C, h, w), dtype=np.uint8)).to(cuda)
    fresh = _e2e_engine(w, h, ch, 1, n)
    try:
        want = fresh.eval_population(gb, 1)
        want_i, want_v = fresh.eval_images(imgs, n, 2)
    finally:
        fresh.close()
    eng = _e2e_engine(w, h, ch, 1, n)
    try:
        for structure in (1, 2):
            eng.eval_population(gb, structure, dense=ds.e2e_dense(structure))
        got = eng.eval_population(gb, 1)
        got_i, got_v = eng.eval_images(imgs, n, 2)
    finally:
        eng.close()
    assert got.tobytes() == want.tobytes() and got_i.tobytes() == want_i.tobytes() and ((want != 0).any() or (want_i != 0).any())
    assert len(got_v) == len(want_v) and all(a.tobytes() == b.tobytes() for a, b in zip(got_v, want_v))


def test_refusals(cuda):
    """EIGEN_ERR_INVALID with a message, before anything is launched: both scores or neither, a radius, eps or score field the trainer
    refuses (in its words), a batch over max_batch, a stride below one image, a structure the score does not belong to"""
    from evolutionary_illusion_generator_amd import train
    w, h, C, B = 16, 12, 1, 2
    per = C * h * w
    eng = Engine(w, h, [C, 4], B)
    d = torch.zeros((B + 1, C, h, w), dtype=torch.uint8, device=cuda)
    fs_c = train.FlowScore().settings(h)
    st_c = train.FreeScore().settings(h)

    def call(radius=7, eps=1e-2, flags=0, score=fs_c, sscore=None, batch=B, stride=per, mask=None):
        cfg = engine.DenseSettingsC(engine.FlowSettingsC(radius, flags, eps), None if score is None else ctypes.addressof(score),
                                    None if sscore is None else ctypes.addressof(sscore))
        fit = np.full(B + 2, SENT)
        rc = eng.lib.eigen_dense_score(eng._h, _p(d), ctypes.c_int64(stride), _p(d), ctypes.c_int64(per), ctypes.c_int32(batch), ctypes.byref(cfg), _p(mask),
                                       ctypes.c_void_p(fit.ctypes.data), None, None, None)
        assert rc == 0 or (fit == SENT).all()
        return rc, eng.lib.eigen_last_error().decode()

    try:
        assert call()[0] == 0
        for kw, words in ((dict(sscore=st_c), "exactly one of the flow score and the flow structure score"), (dict(score=None), "exactly one of the flow score"),
                          (dict(radius=0), "flow radius 0 outside 1 .. 16"), (dict(radius=17), "flow radius 17"), (dict(eps=0.0), "flow eps 0"),
                          (dict(eps=float("inf")), "flow eps inf"), (dict(flags=1), "flow flags 0x1"), (dict(batch=B + 1), "max_batch"), (dict(batch=0), "batch 0"),
                          (dict(stride=per - 1), "smaller than one image"), (dict(mask=torch.zeros((h, w), dtype=torch.uint8, device=cuda)), "the flow mask counts no pixel")):
            rc, msg = call(**kw)
            assert rc == -1 and words in msg, (kw, rc, msg)
        bad = train.FlowScore().settings(h)
        bad.min_count = 1
        assert call(score=bad) == (-1, "flow score min_count 1: must be >= 2")
        bad = train.FreeScore().settings(h)
        bad.structure = 1
        rc, msg = call(score=None, sscore=bad)
        assert rc == -1 and "eigen_flow_score" in msg
        bad = train.FreeScore().settings(h)
        bad.max_distance = 0.0
        assert call(score=None, sscore=bad)[0] == -1
        with pytest.raises(EngineError, match="score of another structure"):
            eng.eval_images(d, B, 2, dense=fitness.DenseFitness.for_structure(1))
        with pytest.raises(EngineError, match="max_batch"):
            eng.eval_images(d, B + 1, 1, dense=fitness.DenseFitness.for_structure(1))
    finally:
        eng.close()
    # a pairing the handle's n_ext cannot serve is refused ahead of the render: no grid, no weights and still this message
    short = Engine(w, h, [C, 4], B, n_ext=1)
    try:
        from evolutionary_illusion_generator_amd import synth
        cfg = synth.make_config(2, 1)
        gb = genome.GenomeBatch([g for _, g in synth.make_population(B, cfg, seed=1)], cfg, 1, n_leaves=2)
        with pytest.raises(EngineError, match="pairing needs 2 extension steps"):
            short.eval_population(gb, 1, pairing=engine.PAIR_SINGLE, dense=fitness.DenseFitness.for_structure(1))
        with pytest.raises(EngineError, match="pairing needs 2 extension steps"):
            short.eval_images(d, B, 1, pairing=engine.PAIR_SINGLE, dense=fitness.DenseFitness.for_structure(1))
    finally:
        short.close()
