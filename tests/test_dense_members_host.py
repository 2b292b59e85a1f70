"""The dense motion fitness's members without a GPU ("Members"): the argument rules of `fitness.DenseFitness(members=)`
and of the population functions, the byte round trip the trainer's membership stage relies on, the liveness of the end-to-end cases of
tests/test_gpu_dense_members.py on the oracle's frames, the ABI surface by the header's text, the resources of the two new kernels in
the built library, and the forwarding of a fitness with members through the sharded path."""
import os
import re
import socket
import sys

import numpy as np
import pytest

from tests import dense_fitness_support as ds
from tests import dense_members_support as dm
from tests import flow_corner_support as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_fitness_members_argument_rules():
    from evolutionary_illusion_generator_amd import fitness, train
    F = fitness.DenseFitness
    cm = train.CornerMembers(max_corners=40)
    d = F.for_structure(2, members=cm)
    assert d.members is cm and not d.member_planes and F(members=cm).resolved(1).members is cm
    assert F.for_structure(2).members is None and F().with_members(cm).members is cm
    planes = np.ones((3, 4, 5), bool)
    p = F.for_structure(1, members=planes)
    assert p.member_planes and p.members.dtype == np.uint8 and p.members.shape == (3, 4, 5) and p.members.all()
    assert np.array_equal(F(members=np.array([[[0, 2], [255, 0]]], np.uint8)).members, [[[0, 1], [1, 0]]])
    for bad in ("corners", 5, np.ones((4, 5), np.uint8), np.ones((1, 4, 5), np.float32), np.ones((1, 4, 5), np.int32), [cm]):
        with pytest.raises(ValueError, match="members must be"):
            F(members=bad)
    with pytest.raises(ValueError, match="do not go with a shared"):
        F(mask=np.ones((4, 5), np.uint8), members=planes)
    # the constructor's mask rule stays as it is, in its words
    with pytest.raises(ValueError, match=r"a per-sample \[n, H, W\] mask and members need a score"):
        F(mask=np.ones((2, 4, 4), np.uint8))
    # with_members replaces what resolved() made for the earlier members
    e = F()
    assert e.resolved(2).members is None
    assert e.with_members(cm) is e and e.resolved(2).members is cm and e.with_members(None).resolved(2).members is None
    # corner members go on to the objective, under the shared mask; planes do not
    mask = fc.half_mask(6, 4)
    flow = F.for_structure(2, radius=3, mask=mask, members=cm).flow_objective()
    assert isinstance(flow, train.PredictionFlow) and flow.members is cm and np.array_equal(flow.mask, mask) and isinstance(flow.score, train.FreeScore)
    assert F.for_structure(1, members=cm).flow_objective("frame").members is cm
    solved = F.for_structure(1, members=cm, levels=2, iters=3).solve_objective()
    assert solved.members is cm and solved.solve == (2, 3)
    assert F.for_structure(1).flow_objective().members is None
    for make in (p.flow_objective, p.solve_objective):
        with pytest.raises(ValueError, match="per-sample member planes"):
            make()
    assert "solve_objective" in F.flow_objective.__doc__ and "does not exist" not in " ".join(F.flow_objective.__doc__.split())


def test_members_on_gives_the_calls_settings():
    """what `Engine` asks of a fitness with members: the struct of the call, and the planes' shape checked against the call"""
    from evolutionary_illusion_generator_amd import fitness, train

    class FakeTensor:
        def __init__(self, a):
            self.a = a

        def cuda(self, device):
            return ("dev", device, self.a)

    class FakeTorch:
        from_numpy = staticmethod(FakeTensor)

    cm = train.CornerMembers(max_corners=40, quality_level=0.1, min_distance=2.0, block_size=5)
    mem, planes = fitness.DenseFitness.for_structure(1, members=cm).members_on(FakeTorch, 0, 3, 4, 5)
    assert planes is None and (mem.kind, mem.max_corners, mem.block_size, mem.reserved, mem.quality_level, mem.min_distance, mem.mask_bstride) == (1, 40, 5, 0, 0.1, 2.0, 0)
    d = fitness.DenseFitness.for_structure(1, members=np.ones((3, 4, 5), np.uint8))
    mem, planes = d.members_on(FakeTorch, 0, 3, 4, 5)
    assert (mem.kind, mem.mask_bstride) == (0, 20) and planes[:2] == ("dev", 0) and planes[2] is d.members
    assert d.members_on(FakeTorch, 0, 3, 4, 5)[1] is planes      # uploaded once
    for n, h, w in ((2, 4, 5), (3, 5, 4)):
        with pytest.raises(ValueError, match="member planes are"):
            d.members_on(FakeTorch, 0, n, h, w)


def test_population_functions_take_corner_members_and_refuse_planes(monkeypatch):
    from evolutionary_illusion_generator_amd import fitness, synth, train
    assert fitness.FITNESS_SCORES == ("corners", "dense") and fitness.DENSE_MEMBERS_CHOICES == ("all", "corners")
    cfg = synth.make_config(2, 1)
    genomes = [g for _, g in synth.make_population(2, cfg, seed=0)]
    planes = fitness.DenseFitness.for_structure(1, members=np.ones((2, 64, 64), np.uint8))
    args = (1, genomes, "synthetic", cfg, 64, 64, [1, 4, 8])
    for fn in (fitness.evaluate_population, fitness.population_fitness):
        with pytest.raises(ValueError, match="per-sample member planes"):      # before any engine exists
            fn(*args, c_dim=1, score=planes)
    seen = []

    class FakeEngine:
        max_batch, _grid_key = 4, None

        def set_grid(self, planes):
            pass

        def eval_population(self, gb, structure, **kw):
            seen.append(kw.get("dense"))
            return np.zeros(gb.n_genomes)

    monkeypatch.setattr(fitness, "_engine_for", lambda *a, **k: FakeEngine())
    corners = fitness.DenseFitness.for_structure(1, members=train.CornerMembers(max_corners=9))
    fitness.evaluate_population(*args, c_dim=1, score=corners)
    assert seen[-1] is corners
    # the module setting: "dense" follows it with CornerMembers()'s defaults; FITNESS_SCORES is what it was
    monkeypatch.setattr(fitness, "DENSE_MEMBERS", "all")
    fitness.evaluate_population(*args, c_dim=1, score="dense")
    assert seen[-1].members is None
    monkeypatch.setattr(fitness, "DENSE_MEMBERS", "corners")
    fitness.evaluate_population(*args, c_dim=1, score="dense")
    got, want = seen[-1].members, train.CornerMembers()
    assert isinstance(got, train.CornerMembers)
    assert (got.max_corners, got.quality_level, got.min_distance, got.block_size) == (want.max_corners, want.quality_level, want.min_distance, want.block_size)
    assert fitness.resolve_score("dense", 2) is fitness.resolve_score("dense", 2) and fitness.resolve_score("corners", 2) is None
    monkeypatch.setattr(fitness, "FITNESS_SCORE", "dense")
    fitness.get_fitnesses_neat(1, [(i, g) for i, g in enumerate(genomes)], "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, best_dir=None)
    assert isinstance(seen[-1].members, train.CornerMembers)
    monkeypatch.setattr(fitness, "DENSE_MEMBERS", "every")
    with pytest.raises(ValueError, match="DENSE_MEMBERS"):
        fitness.evaluate_population(*args, c_dim=1, score="dense")
    monkeypatch.setattr(fitness, "FITNESS_SCORE", "corners")
    fitness.evaluate_population(*args, c_dim=1)          # the sparse path does not read the setting
    assert seen[-1] is None


def test_the_float_to_byte_step_returns_every_byte():
    """A dense call's images are bytes and the trainer's stage sees (float)byte / 255.0f; its membership stage forms
    (uint8)(int)(v * 255.0f) of that float, in float32: every one of the 256 bytes comes back unchanged, so both pick their corners on the
    same image"""
    b = np.arange(256, dtype=np.uint8)
    f = b.astype(np.float32) / np.float32(255.0)
    assert f.dtype == np.float32
    assert np.array_equal(fc.quantise(f), b)
    assert np.array_equal((f * np.float32(255.0)).astype(np.int32).astype(np.uint8), b)


@pytest.mark.parametrize("shape,structure", dm.E2E_CASES, ids=lambda v: "%dx%d" % v[:2] if isinstance(v, tuple) else "s%d" % v)
def test_the_end_to_end_cases_are_live_on_the_oracle(shape, structure):
    """With the oracle's render, roll-out and corners and the numpy restatement alone: under both pairings of every case at least five of
    the seven samples have N >= min_count and a non-zero score; a sample scores exactly 0 where it is below min_count and nowhere else;
    the members of a sample are among its corners; the one sample below min_count is where tests/test_gpu_dense_members.py expects it."""
    w, h, ch = shape
    images, frames = ds.oracle_case(w, h, ch, structure)
    for pairing in (ds.PAIR_POPULATION, ds.PAIR_SINGLE):
        img0, img1 = ds.frame_pair(images, frames, pairing, 20)
        planes, counts = dm.e2e_planes(img0)
        sc, want = dm.e2e_restate(structure, img0, img1, planes)
        N, S = want.score.record[:, 0], want.score.S
        print("members end to end %dx%d s%d pairing %d: corners %s N %s" % (w, h, structure, pairing, counts.tolist(), N.astype(int).tolist()))
        live = (N >= sc.min_count) & (S != 0)
        assert int(live.sum()) >= 5, (structure, pairing, N.tolist(), S.tolist())
        assert ((N < sc.min_count) == (S == 0)).all()
        assert (N <= planes.reshape(len(N), -1).sum(1)).all() and (counts <= dm.e2e_members().max_corners).all()
        assert bool((N < sc.min_count).any()) == (((w, h), structure, pairing) == dm.DEAD), (structure, pairing, N.tolist())


def test_the_small_shape_falls_below_min_count():
    """16 x 12 yields a handful of corners a sample: under min_count 10 every sample of the Circles case is below it and scores exactly 0"""
    w, h, ch = dm.SMALL
    images, frames = ds.oracle_case(w, h, ch, 1)
    img0, img1 = ds.frame_pair(images, frames, ds.PAIR_POPULATION, 20)
    planes, counts = dm.e2e_planes(img0)
    assert (counts >= 1).all() and (counts < 10).all(), counts
    sc, want = dm.e2e_restate(1, img0, img1, planes, min_count=10)
    assert (want.score.record[:, 0] < 10).all() and not want.score.S.any()


def test_the_stage_inputs_have_corners_and_none():
    """the stage cases: the smooth and the random image have corners, the constant one has none, the cap of 5 decides, and the half mask
    removes some corners and keeps some"""
    for w, h, C, _ in fc.SHAPES:
        img0, _ = dm.stage_pair(w, h, C)
        planes, counts = fc.oracle_members(img0)
        capped, ccounts = fc.oracle_members(img0, fc.CAPPED)
        halved, _ = fc.oracle_members(img0, mask=fc.half_mask(w, h))
        assert counts[2] == 0 and (counts[:2] > fc.CAPPED).all() and ccounts.tolist() == [fc.CAPPED, fc.CAPPED, 0], (counts, ccounts)
        assert 0 < halved.sum() < planes.sum()


def test_the_pair_cases_span_the_tiles():
    """192 pixels are less than one tile of 256 slots, 594 three tiles with the last partial, 1536 six full ones; the planes are all
    ones, a random two thirds and exactly one pixel, and the batch's middle plane is empty beside two that are not"""
    assert [w * h for w, h in dm.PAIR_SHAPES] == [192, 594, 1536]
    for w, h in dm.PAIR_SHAPES:
        assert dm.pair_plane("ones", w, h).all() and dm.pair_plane("single", w, h).sum() == 1
        r = dm.pair_plane("random", w, h)
        assert 0.5 * w * h < r.sum() < 0.8 * w * h
        m = dm.batch_planes(w, h)
        assert not m[1].any() and m[0].any() and m[2].any() and not np.array_equal(m[0], m[2])
        a, b = dm.pair_images(w, h)
        assert len({x.tobytes() for x in a}) == 3 and not np.array_equal(a, b)


def test_abi_surface():
    from evolutionary_illusion_generator_amd import engine
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    flat = " ".join(header.split())
    tails = {"eigen_dense_score": "const eigen_dense_solve* solve, const eigen_flow_members* members, uint8_t* h_members, int32_t* h_counts);",
             "eigen_eval_population_dense": "const eigen_dense_solve* solve, const eigen_flow_members* members);",
             "eigen_eval_images_dense": "const eigen_dense_solve* solve, const eigen_flow_members* members);"}
    for base, tail in tails.items():
        n = base + "_members"
        assert re.search(r"^int %s\(eigen_engine\* e," % n, header, re.M), n
        assert engine.EXPORTS.count(n) == 1
        # the namesake's arguments, then the members
        mine = re.search(r"int %s\((.*?)\);" % n, flat).group(1)
        iters = re.search(r"int %s_iter\((.*?)\);" % base, flat).group(1)
        assert mine.startswith(iters + ", const eigen_flow_members* members") and (mine + ");").endswith(tail), (mine, iters)
    assert re.search(r"#define EIGEN_ABI_VERSION 4\b", header) and engine.ABI_VERSION == 4
    # no existing struct changes: the members' struct is the trainer's, the settings and the config keep their sizes
    import ctypes
    from evolutionary_illusion_generator_amd import train
    assert header.count("} eigen_flow_members;") == 1 and ctypes.sizeof(train.FlowMembersSettings) == 40
    assert ctypes.sizeof(engine.DenseSettingsC) == 32 and ctypes.sizeof(engine.DenseSolveC) == 8 and ctypes.sizeof(engine.EigenConfig) == 152


@pytest.mark.parametrize("kernel", dm.MEMBER_KERNELS)
def test_new_kernels_have_no_scratch_and_no_spills(kernel):
    from tests.train_support import check_no_scratch_and_no_spills
    check_no_scratch_and_no_spills(kernel)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _forward_worker(rank, world, port, q, source):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from evolutionary_illusion_generator_amd import fitness, genome, synth, train
    fitness.GENOME_SOURCE = source
    seen = []

    def fake_batch(structure, gb, n_in, *a, score=None, **k):   # the stubbed evaluator: the members it was given decide the value
        m = getattr(score, "members", None)
        seen.append(None if m is None else m.max_corners)
        return np.arange(gb.n_genomes) + (0.0 if m is None else float(m.max_corners)) + 1000.0 * rank

    def fake_eval(structure, genomes, model, config, *a, **k):
        return fake_batch(structure, genome.GenomeBatch(genomes, config, 1, n_leaves=2, native=False), 2, **k)

    fitness.evaluate_batch, fitness.evaluate_population = fake_batch, fake_eval
    cfg = synth.make_config(2, 1)
    genomes = [g for _, g in synth.make_population(5, cfg, seed=3)]
    out, err = {}, None
    try:
        for name, score in (("all", fitness.DenseFitness.for_structure(1)), ("corners", fitness.DenseFitness.for_structure(1, members=train.CornerMembers(max_corners=50)))):
            out[name] = fitness.population_fitness(1, genomes, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, score=score).tolist()
        try:
            fitness.population_fitness(1, genomes, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, score=fitness.DenseFitness.for_structure(1, members=np.ones((5, 64, 64), np.uint8)))
            out["planes"] = "no error"
        except ValueError:
            out["planes"] = "ValueError"
    except Exception as e:  # noqa: BLE001
        err = "%s: %s" % (type(e).__name__, e)
    q.put((rank, out, seen, err))
    dist.destroy_process_group()


@pytest.mark.parametrize("source", ["rank0", "replicated"])
def test_population_fitness_forwards_members_through_sharded_map(source):
    """gloo, world 2, a stubbed evaluator: a fitness with corner members reaches every rank's evaluator with them, the all-gather carries
    one float64 per genome as without them, and member planes raise on every rank before any collective"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_forward_worker, args=(r, 2, port, q, source)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out, seen, err in res:
        assert err is None, err
        plain = [0.0, 1.0, 2.0, 1000.0, 1001.0]
        assert out["all"] == plain and out["corners"] == [v + 50.0 for v in plain]
        assert out["planes"] == "ValueError"
        assert seen == [None, 50], seen
