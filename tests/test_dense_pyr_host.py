"""The dense fitness's pyramidal, iterated solve without a GPU ("The pyramidal, iterated solve"): the numpy
restatement `dense_pyr_support.dense_pyr_ref` is the single step at one level and one iteration, and it is far more accurate than the
single step on moving textures whose flow is known exactly; the cases are live; the argument rules of `fitness.DenseFitness`, the ABI
surface, the forwarding through the sharded path and the resources of the new kernels in the built library."""
import os
import re
import socket
import sys

import numpy as np
import pytest

from tests import dense_pyr_support as dp
from tests import flow_obj_support as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [c[0] for c in dp.GPU_CASES] + ["acc"])
def test_one_level_one_iteration_is_the_single_step(name):
    """`dense_pyr_ref(levels=1, iters=1)` is `flow_obj_support.flow_stage_ref(...).u` on the byte forms, bit for bit: the sampler returns the
    pixel at integer coordinates, and the first step added to the -0.0 start is the step itself"""
    if name == "acc":
        img0, img1, _ = dp.shift_case(dp.ACC_W, dp.ACC_H, 1, dp.ACC_SEEDS[0], dp.ACC_SHIFTS[1])
        r = dp.ACC_R
    else:
        img0, img1, _, _, r, _ = dp.gpu_case(name)
    want = fs.flow_stage_ref(fs.byte_reference(img1).astype(np.float32), fs.byte_reference(img0), r, dp.EPS).u
    got = dp.dense_pyr_ref(img0, img1, r, dp.EPS, 1, 1)
    assert np.array_equal(got, want) and got.tobytes() == want.tobytes()
    same = dp.dense_pyr_ref(img0, img0, r, dp.EPS, 1, 1)      # a step of exactly -0.0 keeps its sign
    assert same.tobytes() == fs.flow_stage_ref(fs.byte_reference(img0).astype(np.float32), fs.byte_reference(img0), r, dp.EPS).u.tobytes()


def test_the_pyramid_keeps_a_constant_and_halves_a_ramp():
    """the reduction on its own: a constant plane stays that constant exactly, sizes are ((W + 1) / 2, (H + 1) / 2), and the interior of a
    ramp in x is the ramp at the even columns"""
    a = np.full((1, 9, 14), 0.375)
    assert np.array_equal(dp.pyr_down(a), np.full((1, 5, 7), 0.375))
    ramp = np.broadcast_to(np.arange(14.0) / 16.0, (1, 9, 14)).copy()
    down = dp.pyr_down(ramp)
    assert down.shape == (1, 5, 7) and np.array_equal(down[0, :, 1:6], np.broadcast_to(np.arange(2, 12, 2) / 16.0, (5, 5)))
    assert dp.level_sizes(20, 15, 3) == [(20, 15), (10, 8), (5, 4)]


def test_the_iterated_solve_halves_the_single_steps_error(capsys):
    """On the restatement alone, gray 48 x 32, radius 7, eps 1e-2, pixels at least 7 from the border, two genomes and three shifts: the
    mean endpoint error at 2 levels x 3 iterations is at most 0.5 times the single step's on the same pixels.  Measured ratios
    (iterated / single): genome 63: 0.332, 0.146, 0.120; genome 76: 0.372, 0.267, 0.145 for the shifts (0.5, -0.25), (1.25, -0.75),
    (2.5, 1.5); against the zero field the single step leaves 0.40 .. 0.49 of the error and the iterated solve 0.05 .. 0.17."""
    ratios = []
    for seed, shift in dp.ACC_CASES:
        img0, img1, truth = dp.shift_case(dp.ACC_W, dp.ACC_H, 1, seed, shift)
        single = dp.epe(dp.dense_pyr_ref(img0, img1, dp.ACC_R, dp.EPS), truth, dp.ACC_BORDER)
        iterated = dp.epe(dp.dense_pyr_ref(img0, img1, dp.ACC_R, dp.EPS, dp.ACC_LEVELS, dp.ACC_ITERS), truth, dp.ACC_BORDER)
        zero = dp.epe(np.zeros_like(truth), truth, dp.ACC_BORDER)
        ratios.append(iterated / single)
        with capsys.disabled():
            print("dense pyr accuracy: genome %d shift %s: single %.3f iterated %.3f of the zero field's error, ratio %.3f" % (seed, shift, single / zero, iterated / zero, ratios[-1]))
    for (seed, shift), ratio in zip(dp.ACC_CASES, ratios):
        assert ratio <= dp.ACC_BOUND, (seed, shift, ratio)


def test_the_cases_are_live():
    """No frame of an accuracy or GPU case is flat (at least 16 byte values per frame of every sample), the two frames of a sample
    differ, every level of every GPU case moves, and the 48 x 32 case samples taps beyond the staged patch at level 0"""
    pairs = [dp.shift_case(dp.ACC_W, dp.ACC_H, 1, seed, shift)[:2] for seed, shift in dp.ACC_CASES] + [dp.gpu_case(c[0])[:2] for c in dp.GPU_CASES]
    for img0, img1 in pairs:
        for b in range(len(img0)):
            assert len(np.unique(img0[b])) >= 16 and len(np.unique(img1[b])) >= 16
            assert not np.array_equal(img0[b], img1[b])
    for c in dp.GPU_CASES:
        img0, img1, levels, iters, r, want = dp.gpu_case(c[0])
        fields = dp.dense_pyr_ref(img0, img1, r, dp.EPS, levels, iters, all_levels=True)
        assert np.array_equal(fields[0], want) and np.isfinite(want).all()
        assert [(f.shape[3], f.shape[2]) for f in fields] == dp.level_sizes(c[1], c[2], levels)
        assert all(np.abs(f).max() > 1e-2 for f in fields)
        if c[0] == "48x32":
            assert dp.taps_beyond_patch(want, r) > 0
    # the coarsest level of the 8 x 8 case is 4 x 4: every window is the whole image
    assert dp.level_sizes(8, 8, 2)[-1] == (4, 4)


@pytest.mark.parametrize("structure", (0, 1, 2))
def test_the_end_to_end_cases_are_live_on_the_oracle(structure):
    """With the ORACLE's render and roll-out and the numpy restatement alone: under both pairings of the end-to-end GPU test at least half
    of the 7 samples have N >= min_count and a non-zero score, a sample scores exactly 0 where it is below min_count and nowhere else, and
    the iterated field differs from the single step's."""
    from tests import dense_fitness_support as ds
    w, h, ch = ds.E2E_SHAPES[1]
    images, frames = ds.oracle_case(w, h, ch, structure)
    for pairing in (ds.PAIR_POPULATION, ds.PAIR_SINGLE):
        img0, img1 = ds.frame_pair(images, frames, pairing, 20)
        u = dp.dense_pyr_ref(img0, img1, ds.E2E_RADIUS, dp.EPS, dp.E2E_LEVELS, dp.E2E_ITERS)
        assert not np.array_equal(u, dp.dense_pyr_ref(img0, img1, ds.E2E_RADIUS, dp.EPS))
        sc = dp.restatement_score(dp.e2e_dense(structure, pairing), h)
        score = dp.Want(u, sc).score
        N, S = score.record[:, 0], score.S
        live = (N >= sc.min_count) & (S != 0)
        assert 2 * int(live.sum()) >= len(S), (structure, pairing, N.tolist(), S.tolist())
        assert ((N < sc.min_count) == (S == 0)).all()


def test_dense_fitness_solve_rules():
    from evolutionary_illusion_generator_amd import fitness, train
    F = fitness.DenseFitness
    for bad in (dict(levels=0), dict(levels=7), dict(levels=2.0), dict(levels=True), dict(levels=None), dict(iters=0), dict(iters=33), dict(iters=1.5),
                dict(iters=False)):
        with pytest.raises(ValueError):
            F(**bad)
        with pytest.raises(ValueError):
            F.for_structure(1, **bad)
    d = F()
    assert (d.levels, d.iters) == (1, 1) and d.solve_on(16, 12) == (1, 1)
    d = F.for_structure(2, levels=3, iters=4, radius=5)
    assert (d.levels, d.iters, d.radius) == (3, 4, 5) and isinstance(d.score, train.FreeScore) and d.resolved(2) is d
    assert d.solve_on(20, 15) == (3, 4)         # 5 x 4
    with pytest.raises(ValueError, match="coarsest level"):
        d.solve_on(16, 12)                      # 4 x 3
    assert F(levels=6, iters=32).solve_on(128, 128) == (6, 32)
    with pytest.raises(ValueError, match="coarsest level"):
        F(levels=6).solve_on(128, 96)           # 96 -> 48, 24, 12, 6, 3
    # a fitness without a score of its own hands its solve to every structure's resolved copy
    r = F(levels=2, iters=3).resolved(0)
    assert (r.levels, r.iters) == (2, 3) and isinstance(r.score, train.BandsScore)
    # refinement climbs the single step: the objective carries no solve
    flow = F.for_structure(0, radius=4, levels=2, iters=3).flow_objective()
    assert isinstance(flow, train.PredictionFlow) and flow.radius == 4 and not hasattr(flow, "levels")
    assert "single" in F.flow_objective.__doc__


def test_the_engine_takes_the_plain_entry_for_the_single_step():
    """`Engine._dense_solve`: (1, 1), and an object without the two attributes, give no eigen_dense_solve at all, so the call is the plain
    entry's; anything else gives the struct"""
    from evolutionary_illusion_generator_amd import engine, fitness

    class Old:
        pass

    assert engine.Engine._dense_solve(Old()) is None and engine.Engine._dense_solve(fitness.DenseFitness()) is None
    s = engine.Engine._dense_solve(fitness.DenseFitness(levels=3, iters=2))
    assert isinstance(s, engine.DenseSolveC) and (s.levels, s.iters) == (3, 2)
    assert engine.Engine._dense_solve(fitness.DenseFitness(iters=2)).iters == 2


def test_evaluate_batch_refuses_a_pyramid_too_deep_before_any_engine(monkeypatch):
    from evolutionary_illusion_generator_amd import fitness, synth
    cfg = synth.make_config(2, 1)
    pop = synth.make_population(2, cfg, seed=0)
    monkeypatch.setattr(fitness, "_engine_for", lambda *a, **k: pytest.fail("an engine was asked for"))
    with pytest.raises(ValueError, match="coarsest level"):
        fitness.evaluate_population(1, [g for _, g in pop], "synthetic", cfg, 16, 12, [1, 4, 8], c_dim=1, score=fitness.DenseFitness(levels=3))


def test_abi_surface():
    import ctypes
    from evolutionary_illusion_generator_amd import engine
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    for n in ("eigen_dense_score_iter", "eigen_eval_population_dense_iter", "eigen_eval_images_dense_iter"):
        m = re.search(r"^int %s\(eigen_engine\* e,[^;]*;" % n, header, re.M)
        assert m and re.search(r"const eigen_dense_solve\* solve\);$", m.group(0)), n
        assert engine.EXPORTS.count(n) == 1
    assert engine.EXPORTS.count("eigen_debug_dense_solve") == 1
    assert re.search(r"typedef struct \{\s*int32_t levels;\s*int32_t iters;\s*\} eigen_dense_solve;", header)
    assert ctypes.sizeof(engine.DenseSolveC) == 8 and engine.DenseSolveC.iters.offset == 4
    assert re.search(r"#define EIGEN_ABI_VERSION 4\b", header) and engine.ABI_VERSION == 4
    # eigen_dense_settings keeps its layout
    assert ctypes.sizeof(engine.DenseSettingsC) == 32 and engine.DenseSettingsC.score.offset == 16 and engine.DenseSettingsC.sscore.offset == 24
    if os.path.exists(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "libeigen_hip.so")):
        lib = engine.load_library()
        assert lib.eigen_abi_version() == 4
        for n in ("eigen_dense_score_iter", "eigen_eval_population_dense_iter", "eigen_eval_images_dense_iter", "eigen_debug_dense_solve"):
            assert hasattr(lib, n)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _forward_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from evolutionary_illusion_generator_amd import fitness, genome, synth
    seen = []

    def fake_batch(structure, gb, n_in, *a, score=None, **k):
        seen.append((type(score).__name__, getattr(score, "levels", None), getattr(score, "iters", None)))
        return np.arange(gb.n_genomes) + 10.0 * getattr(score, "levels", 0) + getattr(score, "iters", 0) / 100.0 + 1000.0 * rank

    def fake_eval(structure, genomes, model, config, *a, **k):
        return fake_batch(structure, genome.GenomeBatch(genomes, config, 1, n_leaves=2, native=False), 2, **k)

    fitness.evaluate_batch, fitness.evaluate_population = fake_batch, fake_eval
    cfg = synth.make_config(2, 1)
    genomes = [g for _, g in synth.make_population(5, cfg, seed=3)]
    out, err = None, None
    try:
        out = fitness.population_fitness(1, genomes, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, score=fitness.DenseFitness.for_structure(1, levels=3, iters=2)).tolist()
    except Exception as e:  # noqa: BLE001
        err = "%s: %s" % (type(e).__name__, e)
    q.put((rank, out, seen, err))
    dist.destroy_process_group()


def test_population_fitness_forwards_the_solve_through_sharded_map():
    """gloo, world 2, a stubbed evaluator: a DenseFitness with levels 3 and iters 2 reaches every rank's evaluator as it was given, and the
    all-gather carries one float64 per genome as without it"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_forward_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out, seen, err in res:
        assert err is None, err
        assert out == [30.02, 31.02, 32.02, 1030.02, 1031.02], out
        assert seen == [("DenseFitness", 3, 2)], seen


@pytest.mark.parametrize("kernel", dp.PYR_KERNELS)
def test_new_kernels_have_no_scratch_and_no_spills(kernel):
    from tests.train_support import check_no_scratch_and_no_spills
    check_no_scratch_and_no_spills(kernel)
