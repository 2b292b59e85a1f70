"""CPU: host-side logic of the product package and the C-ABI surface (no compute calls without a GPU)."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from evolutionary_illusion_generator_amd import engine
    lib = engine.load_library()
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = sorted(set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header)))
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), "libeigen_hip.so does not export %s" % name
    assert set(engine.EXPORTS) == set(declared)
    assert lib.eigen_abi_version() == 4
    import oracle
    assert lib.eigen_gate_order() == oracle.lib().eig_oracle_gate_order() == 1  # library and checker spell the gate epilogue alike
    cfg = engine.EigenConfig()
    lib.eigen_config_defaults(ctypes.byref(cfg))
    assert (cfg.n_repeat, cfg.n_ext, cfg.lk_max_corners, cfg.lk_win, cfg.lk_max_level, cfg.lk_block_size) == (20, 2, 100, 15, 2, 7)
    assert (cfg.lk_quality_level, cfg.lk_min_distance, cfg.lk_epsilon, cfg.lk_min_eig_thr) == (0.3, 7.0, 0.03, 1e-4)


def test_no_silent_fallback_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from evolutionary_illusion_generator_amd import fitness, synth
    from evolutionary_illusion_generator_amd.engine import Engine, EngineError
    with pytest.raises(EngineError):
        Engine(64, 64, [1, 4, 8], 2)
    cfg = synth.make_config(2, 1)
    pop = synth.make_population(2, cfg)
    with pytest.raises(EngineError):
        fitness.get_fitnesses_neat(2, pop, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, best_dir=None)
    assert all(g.fitness is None for _, g in pop)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "evolutionary_illusion_generator_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "eig_oracle" not in src.replace("oracle/eig_oracle.c", ""), f


def test_genome_flattening_matches_the_oracle_evaluator():
    from evolutionary_illusion_generator_amd import genome, synth
    from oracle import cppn, grids
    cfg = synth.make_config(2, 3)
    grid = grids.create_grid(1, 32, 24, 10)
    x, y = grid["x_mat"].reshape(-1), grid["y_mat"].reshape(-1)
    names = {v: k for k, v in genome.ACT_IDS.items()}

    def run(f):
        vals = []
        for n in range(len(f["act"])):
            s = None
            for k in range(f["edge_off"][n], f["edge_off"][n + 1]):
                src = f["edge_src"][k]
                xv = vals[src] if src >= 0 else (np.ones_like(x) if -src - 1 >= 2 else (x, y)[-src - 1])
                t = f["edge_w"][k] * xv
                s = t if s is None else s + t
            vals.append(cppn._act(names[f["act"][n]], f["resp"][n] * s + f["bias"][n]))
        return [vals[o] for o in f["out_node"]]

    n = 0
    for seed in range(3):
        for gid, g in synth.make_population(30, cfg, seed=seed):
            if gid % 3 == 0:  # constant nodes (no enabled inputs): float32 folding path
                for key, c in g.connections.items():
                    if key[1] in (5, 6, 7, 3 + seed):
                        c.enabled = False
            if gid % 7 == 0:  # a constant output
                for key, c in g.connections.items():
                    if key[1] == 1:
                        c.enabled = False
            f = genome.flatten_genome(g, cfg)
            with np.errstate(all="ignore"):
                for a, b in zip(cppn.render_planes(g, cfg, [x, y]), run(f)):
                    assert np.array_equal(np.broadcast_to(np.asarray(a, np.float64), x.shape), b, equal_nan=True)
                    n += 1
    assert n == 270
    gb = genome.GenomeBatch([g for _, g in synth.make_population(5, cfg)], cfg, 3)
    assert gb.node_off[0] == 0 and gb.edge_off[0] == 0 and len(gb.out_node) == 15 and gb.edge_off[-1] == len(gb.edge_src)


def test_genome_flattening_rejects_what_pytorch_neat_rejects():
    from evolutionary_illusion_generator_amd import genome, synth
    cfg4 = synth.make_config(4, 6)  # default.txt: num_inputs = 4 but only x, y are fed
    g = synth.make_genome(1, cfg4, 0)
    with pytest.raises(ValueError):
        genome.flatten_genome(g, cfg4, n_leaves=2)
    cfg = synth.make_config(2, 1)
    g = synth.make_genome(1, cfg, 0)
    g.nodes[0].activation = "cube"
    with pytest.raises(ValueError):
        genome.flatten_genome(g, cfg)
    g = synth.make_genome(2, cfg, 0)
    with pytest.raises(ValueError):
        genome.GenomeBatch([g], cfg, 3)  # 1 output, 3 channels asked


def test_native_flattening_is_the_python_specification():
    """eigen_flatten_genomes (host-side C in libeigen_hip.so) against genome._flatten_lists: identical arrays on random genomes with
    disabled connections, constant nodes (float32 products and leading-run sums), constant outputs and constant sub-graphs
    (declined to the Python path), 4-input configs; invalid genomes raise the same exceptions."""
    from evolutionary_illusion_generator_amd import genome, synth
    fields = ("node_off", "edge_off", "node_act", "node_bias", "node_resp", "edge_src", "edge_w", "out_node")
    n_checked = 0
    for seed, n_in, n_hidden, n_out, c_out in [(0, 2, 20, 3, 3), (1, 2, 8, 6, 3), (2, 2, 20, 1, 1), (3, 2, 0, 3, 3), (7, 2, 30, 3, 1), (5, 4, 12, 6, 3)]:
        cfg = synth.make_config(n_in, n_out)
        gs = [g for _, g in synth.make_population(120, cfg, seed=seed, num_hidden=n_hidden)]
        rng = np.random.default_rng(seed)
        for gi, g in enumerate(gs):
            if gi % 2 == 0:
                for c in g.connections.values():
                    if rng.random() < 0.3:
                        c.enabled = False
            if gi % 9 == 0:  # an output without inputs: constant output plane
                for key, c in g.connections.items():
                    if key[1] == 0:
                        c.enabled = False
        a = genome.GenomeBatch(gs, cfg, c_out, n_leaves=n_in, native=True)
        b = genome.GenomeBatch(gs, cfg, c_out, n_leaves=n_in, native=False)
        for k in fields:
            x, y = getattr(a, k), getattr(b, k)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (seed, k)
        n_checked += len(gs)
    assert n_checked == 720
    # keys spread over a huge range (the library's sorted-table fallback instead of its direct id table)
    cfg = synth.make_config(2, 3)
    gs = [g for _, g in synth.make_population(20, cfg, seed=9, num_hidden=12)]
    for g in gs:
        far = lambda k: k + (1 << 20) * (k % 5) if k >= 3 else k      # hidden keys only; inputs (< 0) and outputs (0..2) stay
        g.nodes = {far(k): n for k, n in g.nodes.items()}
        for n_key, n in g.nodes.items():
            n.key = n_key
        g.connections = {(far(a), far(b)): c for (a, b), c in g.connections.items()}
        for key, c in g.connections.items():
            c.key = key
    a = genome.GenomeBatch(gs, cfg, 3, native=True)
    b = genome.GenomeBatch(gs, cfg, 3, native=False)
    for k in fields:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    cfg = synth.make_config(2, 1)
    bad = synth.make_genome(1, cfg, 0)
    bad.nodes[0].activation = "cube"
    good = synth.make_genome(2, cfg, 1)
    for native in (True, False):
        with pytest.raises(ValueError, match="str_to_activation"):
            genome.GenomeBatch([good, bad], cfg, 1, native=native)
    cyc = synth.make_genome(3, cfg, 2)
    hidden = [k for k in cyc.nodes if k >= 1][:2]
    if len(hidden) == 2:
        import copy
        some = next(iter(cyc.connections.values()))
        for key in ((hidden[0], hidden[1]), (hidden[1], hidden[0])):
            c = copy.copy(some); c.key = key; c.enabled = True; c.weight = 0.5
            cyc.connections[key] = c
        for key in ((hidden[0], 0),):
            c = copy.copy(some); c.key = key; c.enabled = True; c.weight = 0.5
            cyc.connections[key] = c
        for native in (True, False):
            with pytest.raises(ValueError, match="cycle"):
                genome.GenomeBatch([cyc], cfg, 1, native=native)


def test_c_genome_walker_is_the_python_marshalling():
    """csrc/genome_walk.c (CPython extension) against genome._marshal_python: identical arrays for the synthetic duck-typed
    genomes, neat_lite genomes after a few generations of mutation, gene classes with __slots__ / properties (the generic
    attribute protocol), large keys, and the exceptions of malformed genomes."""
    import __graft_entry__ as ge
    ge.build()
    from evolutionary_illusion_generator_amd import _genome_walk, genome, synth  # noqa: F401  (must be built)
    genome._walker[0] = None

    def same(gs):
        a, b = genome._marshal_python(gs), genome._marshal(gs)
        assert genome._walker[0] is _genome_walk.walk
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)

    cfg = synth.make_config(2, 3)
    same([g for _, g in synth.make_population(64, cfg, seed=11, num_hidden=20)])
    same([])
    from evolutionary_illusion_generator_amd import neat_lite
    ncfg = neat_lite.Config(neat_lite.DefaultGenome, neat_lite.DefaultReproduction, neat_lite.DefaultSpeciesSet, neat_lite.DefaultStagnation,
                            os.path.join(ROOT, "examples", "circles_neat.cfg"))
    p = neat_lite.Population(ncfg, seed=3)

    def fake_fitness(genomes, config):
        for i, (_, g) in enumerate(genomes):
            g.fitness = (i * 37 % 11) / 11.0
    p.run(fake_fitness, 4)
    same(list(p.population.values()))

    class SlotConn:
        __slots__ = ("key", "weight", "enabled")

        def __init__(self, key, weight, enabled):
            self.key, self.weight, self.enabled = key, weight, enabled

    class PropNode:
        def __init__(self, b):
            self._b = b
            self.response, self.activation, self.aggregation = 1.5, "gauss", "product"

        @property
        def bias(self):
            return self._b

    g = synth.Genome(1)
    g.connections = {(-1, 5 + (1 << 21)): SlotConn((-1, 5 + (1 << 21)), 0.25, True), (5 + (1 << 21), 0): SlotConn((5 + (1 << 21), 0), -1, 0)}
    g.nodes = {0: PropNode(0.5), 5 + (1 << 21): PropNode(-2)}
    same([g])
    arrays = genome._marshal([g])
    assert arrays[3].tolist() == [0.25, -1.0] and arrays[4].tolist() == [1, 0] and arrays[8].tolist() == [0, 0] and arrays[7].tolist() == [3, 3]
    # a data descriptor on the CLASS wins over a same-named entry of the instance __dict__ (as it does for getattr),
    # the (in, out) pair is the gene's .key (what create_cppn reads), not the dict key it is filed under
    class ShadowNode:
        def __init__(self, b):
            self.__dict__["bias"] = 123.0          # stale value in the instance dict ...
            self._b = b
            self.response, self.activation, self.aggregation = 1.0, "sin", "sum"

        bias = property(lambda self: self._b, lambda self, v: None)  # ... shadowed by the class-level property

    g2 = synth.Genome(3)
    g2.connections = {("filed", "elsewhere"): synth.ConnectionGene(key=(-2, 0), weight=1.25, enabled=True)}
    g2.nodes = {0: ShadowNode(-0.75)}
    same([g2])
    arrays = genome._marshal([g2])
    assert arrays[1].tolist() == [-2] and arrays[2].tolist() == [0] and arrays[9].tolist() == [-0.75]
    big = synth.Genome(4)
    big.connections = {(-1, 0): synth.ConnectionGene(key=(-1, 1 << 31), weight=1.0, enabled=True)}
    big.nodes = {}
    for fn in (genome._marshal, genome._marshal_python):
        with pytest.raises(OverflowError):     # no silent cast to int32
            fn([big])
    big.connections = {}
    big.nodes = {1 << 40: synth.NodeGene(key=1 << 40, bias=0.0, response=1.0, activation="sin", aggregation="sum")}
    for fn in (genome._marshal, genome._marshal_python):
        with pytest.raises(OverflowError):
            fn([big])
    bad = synth.Genome(2)
    bad.connections = {(-1, 0): SlotConn((-1, 0), "heavy", True)}
    bad.nodes = {}
    with pytest.raises(TypeError):
        genome._marshal([bad])
    del bad.connections
    with pytest.raises(AttributeError):
        genome._marshal([bad])


def test_weights_tables(tmp_path):
    from evolutionary_illusion_generator_amd import weights
    import oracle
    ch = [3, 48, 96, 192]
    names = weights.tensor_names(4)
    assert names == oracle.tensor_names(4) and len(names) == 2 * 3 + 2 * 4 + 4 * (4 + 4 + 4 + 3) + 3 * 4
    shp = weights.tensor_shapes(ch, 160, 120)
    assert shp["ConvLSTM3/c_i/W"] == (1, 192, 15, 20) and shp["ConvA1/W"] == (48, 6, 3, 3) and shp["ConvLSTM1/x_f1/W"] == (48, 96, 3, 3)
    n_conv = sum(int(np.prod(s)) for k, s in shp.items() if k.endswith("/W") and "/c_" not in k)
    assert abs(n_conv - 6.92e6) < 0.02e6
    w = weights.synthetic_prednet_weights([1, 4, 8], 16, 8, seed=1)
    path = tmp_path / "m.npz"
    np.savez(path, **{"predictor/" + k: v for k, v in w.items()})  # chainer Classifier prefix
    r = weights.load_chainer_npz(str(path), [1, 4, 8], 16, 8)
    assert all(np.array_equal(r[k], w[k]) for k in w)
    with pytest.raises(ValueError):
        weights.load_chainer_npz(str(path), [1, 4, 8], 32, 16)  # peepholes are resolution-bound


def test_shard_bounds_cover_the_population_in_order():
    from evolutionary_illusion_generator_amd.fitness import shard_bounds
    for P in (0, 1, 5, 50, 256, 257, 1024):
        for R in (1, 2, 3, 8):
            spans = [shard_bounds(P, R, r) for r in range(R)]
            assert spans[0][0] == 0 and spans[-1][1] == P
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert all(hi - lo <= per for lo, hi, per in spans)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _fake_fitness_of_batch(gb):
    """Stand-in for the device pass: a deterministic function of each flattened genome (sum of its edge weights)."""
    out = np.zeros(gb.n_genomes)
    for g in range(gb.n_genomes):
        e0, e1 = gb.edge_off[gb.node_off[g]], gb.edge_off[gb.node_off[g + 1]]
        out[g] = float(np.sum(gb.edge_w[e0:e1]))
    return out


def _gloo_worker(rank, world, port, q, source, diverged):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from evolutionary_illusion_generator_amd import fitness, genome, synth
    fitness.GENOME_SOURCE = source
    calls = []

    def fake_batch(structure, gb, n_in, *a, **k):  # what evaluate_batch would run on the device
        calls.append(gb.n_genomes)
        return _fake_fitness_of_batch(gb)

    def fake_eval(structure, genomes, model, config, *a, **k):
        return fake_batch(structure, genome.GenomeBatch(genomes, config, 1, n_leaves=2, native=False), 2)

    fitness.evaluate_batch = fake_batch
    fitness.evaluate_population = fake_eval
    fitness.save_best_artifacts = lambda *a, **k: None
    cfg = synth.make_config(2, 1)
    out, err = {}, None
    try:
        for P in (7, 8, 1, 0):
            # `diverged`: rank 1's NEAT run was never seeded like rank 0's (the reference never seeds `random`)
            pop = synth.make_population(P, cfg, seed=3 if not (diverged and rank == 1) else 99)
            scores = fitness.get_fitnesses_neat(1, pop, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, best_dir=None)
            out[P] = ([g.fitness for _, g in pop], scores.tolist())
        full = fitness.sharded_map(5, lambda lo, hi: np.arange(lo, hi) * 2.0).tolist()
        v, extras = fitness.sharded_map(3, lambda lo, hi: np.arange(lo, hi) + 0.5, extra=10.0 + rank)
        full = (full, v.tolist(), extras.tolist())
    except Exception as e:  # noqa: BLE001
        err = "%s: %s" % (type(e).__name__, e)
    q.put((rank, out, None if err else full, calls, err))
    dist.destroy_process_group()


def _run_gloo(source, diverged):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q, source, diverged)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def _expected(P, seed=3):
    from evolutionary_illusion_generator_amd import genome, synth
    cfg = synth.make_config(2, 1)
    pop = synth.make_population(P, cfg, seed=seed)
    return _fake_fitness_of_batch(genome.GenomeBatch([g for _, g in pop], cfg, 1, n_leaves=2, native=False)).tolist()


@pytest.mark.parametrize("source", ["rank0", "replicated"])
def test_population_sharding_and_all_gather_gloo_world2(source):
    (r0, out0, full0, calls0, e0), (r1, out1, full1, calls1, e1) = _run_gloo(source, diverged=False)
    assert e0 is None and e1 is None, (e0, e1)
    assert full0 == full1 == ([0.0, 2.0, 4.0, 6.0, 8.0], [0.5, 1.5, 2.5], [10.0, 11.0])  # `extra` rides in the same all-gather
    for P in (7, 8, 1):
        want = _expected(P)
        assert out0[P][0] == want and out1[P][0] == want  # every rank ends with the full fitness list
        assert out0[P][1] == want
    assert out0[0] == ([], []) and out1[0] == ([], [])    # an empty population is not an error
    assert calls0[:3] == [4, 4, 1] and calls1[:2] == [3, 4]   # contiguous shards in population order; rank 1 owns nothing of a population of 1


def test_rank0_is_authoritative_when_the_ranks_populations_diverge():
    """the reference never seeds `random`, so N unchanged copies of generate_illusion.py under torchrun evolve N
    different populations.  Source 'rank0' broadcasts rank 0's flattened genomes: rank 0's fitness list is the right one."""
    (r0, out0, full0, calls0, e0), (r1, out1, full1, calls1, e1) = _run_gloo("rank0", diverged=True)
    assert e0 is None and e1 is None, (e0, e1)
    for P in (7, 8, 1):
        assert out0[P][0] == _expected(P)          # rank 0: fitness of ITS genomes, evaluated partly by rank 1
        assert out1[P][1] == _expected(P)          # rank 1 returns the same vector (of rank 0's genomes)


def test_replicated_source_refuses_diverged_populations():
    (r0, out0, full0, calls0, e0), (r1, out1, full1, calls1, e1) = _run_gloo("replicated", diverged=True)
    assert e0 and e1 and "different populations" in e0 and "EngineError" in e0


def _gloo8_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import io
    import contextlib
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from evolutionary_illusion_generator_amd import fitness, genome, synth
    fitness.GENOME_SOURCE = "rank0"
    calls = []

    def fake_batch(structure, gb, n_in, *a, **k):
        calls.append(gb.n_genomes)
        return _fake_fitness_of_batch(gb)

    fitness.evaluate_batch = fake_batch
    cfg = synth.make_config(2, 1)
    out, stats, err, log = {}, {}, None, io.StringIO()
    try:
        for P in (256, 50, 5, 0):   # even shards, a ragged last shard (7 x 7 + 1), fewer genomes than ranks, none
            genomes = [g for _, g in synth.make_population(P, cfg, seed=3)]
            out[P] = fitness.population_fitness(1, genomes, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1).tolist()
            stats[P] = dict(fitness.LAST_SHARD_STATS)
        # same length, different content on rank 5: rank 0 stays authoritative and rank 5 is told
        genomes = [g for _, g in synth.make_population(16, cfg, seed=3 if rank != 5 else 77)]
        with contextlib.redirect_stdout(log):
            out["div"] = fitness.population_fitness(1, genomes, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1).tolist()
        # rank 0 cannot flatten its population (a cycle): EVERY rank raises straight away instead of waiting in a broadcast
        bad = [g for _, g in synth.make_population(4, cfg, seed=3)]
        if rank == 0:
            a, b = 1 + 5, 1 + 6  # two hidden nodes (outputs: 0; hidden: 1..20)
            bad[2].connections[(a, b)] = synth.ConnectionGene(key=(a, b), weight=1.0, enabled=True)
            bad[2].connections[(b, a)] = synth.ConnectionGene(key=(b, a), weight=1.0, enabled=True)
            bad[2].connections[(b, 0)] = synth.ConnectionGene(key=(b, 0), weight=1.0, enabled=True)
        try:
            fitness.population_fitness(1, bad, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1)
            out["bad"] = "no error"
        except Exception as e:  # noqa: BLE001
            out["bad"] = type(e).__name__
        out["after"] = fitness.population_fitness(1, [g for _, g in synth.make_population(9, cfg, seed=3)], "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1).tolist()
    except Exception as e:  # noqa: BLE001
        err = "%s: %s" % (type(e).__name__, e)
    q.put((rank, out, stats, calls, log.getvalue(), err))
    dist.destroy_process_group()


def test_population_sharding_gloo_world8():
    """SURVEY 8(e) at the world size the metric names (8 ranks, gloo on CPU): pop 256 (32 per rank), pop 50 (ragged: 7 x 7 + 1),
    pop 5 (three ranks own nothing), pop 0; every rank's evaluate() time rides in the one all-gather (what bench.py --gpus N
    prints per rank); a diverged replica is warned by content, a failure on rank 0 reaches every rank."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo8_worker, args=(r, 8, port, q)) for r in range(8)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out, stats, calls, log, err in res:
        assert err is None, (rank, err)
        for P in (256, 50, 5):
            assert out[P] == _expected(P)
            assert len(stats[P]["local_ms"]) == 8 and all(t >= 0 for t in stats[P]["local_ms"]) and stats[P]["collective_ms"] >= 0
        assert out[0] == []
        assert out["div"] == _expected(16)                  # rank 0's genomes, whatever rank 5 holds
        assert ("is not rank 0's" in log) == (rank == 5)
        assert out["bad"] in ("ValueError", "EngineError") and out["after"] == _expected(9)
    shards = {r[0]: r[3][:3] for r in res}
    assert all(shards[r][0] == 32 for r in range(8))                                   # pop 256
    assert [shards[r][1] for r in range(7)] == [7] * 7 and shards[7][1] == 1           # pop 50: the last shard is ragged
    assert res[0][3] == [32, 7, 1, 2, 2] and res[4][3] == [32, 7, 1, 2, 1]             # pops 256, 50, 5, 16 (diverged), 9
    assert res[7][3] == [32, 1, 2]                                                     # rank 7 owns nothing of pop 5 and pop 9: evaluate() is not called


def test_inside_outside_score_index_semantics_are_checked_on_the_host():
    """fitness_calculator.inside_outside_score (:235-236) indexes numpy arrays with int(x / step): past the end -> IndexError.
    The host mirror raises the same way BEFORE anything reaches the device (no GPU needed); the wrap of negative indices is
    compared with the oracle on the GPU box (tests/test_gpu_round2.py)."""
    from evolutionary_illusion_generator_amd import fitness
    v = np.array([[10.0, 10.0, 0.1, 0.0], [50.0, 60.0, 0.0, 0.1]])
    for k, val in ((0, 6.5 * 32), (1, 4.2 * 32), (0, -7.0 * 32)):
        bad = v.copy(); bad[1, k] = val
        with pytest.raises(IndexError, match="out of bounds for axis %d" % k):
            fitness.inside_outside_score(bad, 160, 120)


def test_equal_weight_dicts_share_one_engine_key():
    """dict weights were keyed by id(), so two equal dicts built two 9.5 GB engines.  The key is a content digest,
    computed once per dict object."""
    from evolutionary_illusion_generator_amd import fitness, weights
    a = weights.synthetic_prednet_weights([1, 4, 8], 16, 8, seed=1)
    b = {k: v.copy() for k, v in a.items()}
    c = weights.synthetic_prednet_weights([1, 4, 8], 16, 8, seed=2)
    assert fitness._weights_key(a) == fitness._weights_key(b) != fitness._weights_key(c)
    assert fitness._dict_digests[id(a)][0] is a      # memoised per object (and kept alive, so the id cannot be recycled)
    # a dict mutated after its first use must not keep its old key.  The rules are deterministic (ADVICE r5 / VERDICT r5 weak 8): the arrays are READ-ONLY
    # from the first lookup on, so an in-place edit through them raises; a replaced array is seen by the per-lookup fingerprint
    k0 = fitness._weights_key(a)
    name = sorted(a)[0]
    with pytest.raises(ValueError, match="read-only"):
        a[name][...] = 0.25
    a[name] = a[name] + 1.0                                     # replaced array: new buffer
    k1 = fitness._weights_key(a)
    assert k0 != k1 and fitness._weights_key(b) == k0
    fitness.invalidate_weights(a)                               # announce an in-place edit: thawed, re-hashed on the next lookup, frozen again
    a[name][...] = 0.25
    assert fitness._weights_key(a) not in (k0, k1)
    assert not a[name].flags.writeable
    # zero-size arrays hash (memoryview.cast raised on them)
    z = {"w": np.zeros((0, 3), np.float32), "b": np.ones(2, np.float32)}
    assert fitness._weights_key(z) == fitness._weights_key({k: v.copy() for k, v in z.items()})
    # a SINGLE-element edit through ANOTHER view of the same memory (the one hole the read-only flag leaves) misses the strided sample; the full content hash
    # on every FULL_CHECK_EVERY-th lookup of the dict catches it -- after a fixed number of lookups, not after a wall-clock interval
    base = np.zeros((300, 300), np.float32)
    big = {"w": base[:], "b": np.ones(5, np.float32)}
    kb = fitness._weights_key(big)
    base[3, 5] = 1.0   # (300 * 300 // 64 = 1406: index 905 is not on the stride)
    seen = [fitness._weights_key(big) for _ in range(fitness.FULL_CHECK_EVERY)]
    assert seen[0] == kb and seen[-1] != kb and seen.index(seen[-1]) == fitness.FULL_CHECK_EVERY - 1, seen
    fitness._dict_digests.clear()


def test_changed_weight_dict_evicts_its_old_engine(monkeypatch):
    """once a dict's content change is seen, the engine keyed by the OLD digest must not stay behind (a second full-size engine) unless
    another dict object still maps to it."""
    from evolutionary_illusion_generator_amd import fitness

    class FakeEngine:
        closed = 0

        def close(self):
            FakeEngine.closed += 1

    # a cache of its own: engines that earlier tests of the session left behind (the stage-level ones have shorter keys) stay out of it
    monkeypatch.setattr(fitness, "_engines", {})
    fitness._dict_digests.clear()
    d1 = {"w": np.arange(6, dtype=np.float32)}
    d2 = {"w": np.arange(6, dtype=np.float32)}
    k = fitness._weights_key(d1)
    assert fitness._weights_key(d2) == k
    fitness._engines[(0, 8, 8, (1, 4), k, 4, ())] = FakeEngine()
    try:
        d1["w"] = d1["w"] + 1.0
        assert fitness._weights_key(d1) != k
        assert FakeEngine.closed == 0 and any(key[4] == k for key in fitness._engines)     # d2 still maps to the old digest
        d2["w"] = d2["w"] + 2.0
        assert fitness._weights_key(d2) != k
        assert FakeEngine.closed == 1 and not any(key[4] == k for key in fitness._engines)
    finally:
        for key in [key for key in fitness._engines if isinstance(fitness._engines[key], FakeEngine)]:
            fitness._engines.pop(key)
        fitness._dict_digests.clear()


def test_genome_batch_slice_and_wire_round_trip():
    from evolutionary_illusion_generator_amd import genome, synth
    cfg = synth.make_config(2, 3)
    gs = [g for _, g in synth.make_population(9, cfg, seed=4)]
    gb = genome.GenomeBatch(gs, cfg, 3, native=False)
    rt = genome.GenomeBatch.from_bytes(gb.to_bytes())
    for name, _ in genome.GenomeBatch._FIELDS:
        assert np.array_equal(getattr(rt, name), getattr(gb, name)) and getattr(rt, name).dtype == getattr(gb, name).dtype, name
    assert (rt.n_genomes, rt.c_out) == (9, 3)
    for lo, hi in ((0, 9), (0, 4), (4, 9), (3, 4), (9, 9)):
        part, want = gb.slice(lo, hi), genome.GenomeBatch(gs[lo:hi], cfg, 3, native=False)
        for name, _ in genome.GenomeBatch._FIELDS:
            assert np.array_equal(getattr(part, name), getattr(want, name)), (lo, hi, name)


def test_get_fitnesses_neat_contract_single_process(monkeypatch):
    from evolutionary_illusion_generator_amd import fitness, synth
    cfg = synth.make_config(2, 1)
    pop = synth.make_population(6, cfg, seed=0)
    vals = np.array([0.2, 0.5, 0.0, 0.5, 0.1, 0.3])
    monkeypatch.setattr(fitness, "evaluate_population", lambda s, genomes, *a, **k: vals[:len(genomes)])
    saved = {}
    monkeypatch.setattr(fitness, "save_best_artifacts", lambda st, g, *a, **k: saved.setdefault("best", g))
    fitness.get_fitnesses_neat(1, pop, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, best_dir=".")
    assert [g.fitness for _, g in pop] == vals.tolist() and all(isinstance(g.fitness, float) for _, g in pop)
    assert saved["best"] is pop[3][1]  # '>=': the LAST maximal genome wins (generate_illusion.py:625)


def test_bench_refuses_what_it_cannot_launch():
    """bench.py --gpus N must BE N ranks: without N visible GPUs, or joined under a launcher with another world size, it says so
    and exits non-zero (the flag used to be parsed and dropped).  No GPU needed for the refusals."""
    import subprocess
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    bench = os.path.join(ROOT, "bench.py")
    if torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "GPU(s) visible" in (r.stdout + r.stderr)
    r = subprocess.run([sys.executable, bench, "--gpus", "4", "--steps", "1", "--warmup", "0"], env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stdout + r.stderr)
    import bench as B
    assert len(B.kernel_sources_sha()) == 16 and B.kernel_sources_sha() == B.kernel_sources_sha()
    assert set(B.SHAPES) == {"headline", "ref160", "ref640", "c1", "c2", "c4", "c5"} and B.SHAPES["ref640"][:2] == (640, 480) and B.SHAPES["headline"][:2] == (256, 256) and B.SHAPES["headline"][7] == 256


def test_bench_strict_parity_needs_full():
    """A plain bench.py run has no parity legs (they run with --full), so --strict-parity without them is refused, before the GPU is touched."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    bench = os.path.join(ROOT, "bench.py")
    for extra in ([], ["--full", "--no-parity"]):
        r = subprocess.run([sys.executable, bench, "--steps", "1", "--warmup", "0", "--strict-parity"] + extra, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--strict-parity needs the parity legs" in r.stderr, (extra, r.stderr[-500:])
