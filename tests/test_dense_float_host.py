"""The dense fitness on float frames without a GPU ("Float frames"): the float stage cases and the sub-byte case of
tests/test_gpu_dense_float.py are what they are meant to be on the numpy restatement alone, the argument rules of `frames=` and
`fitness.DENSE_FRAMES`, the forwarding of a float `DenseFitness` through the sharded path, the ABI surface and the resources of the two new
kernels in the built library."""
import os
import re
import socket
import sys

import numpy as np
import pytest

from tests import dense_float_support as df
from tests import dense_fitness_support as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", df.FLOAT_CASES, ids=df.float_id)
def test_the_float_stage_cases_are_live(c):
    """Every float stage case keeps at least min_count members in at least half of its samples, its max_norm sits in a gap between two
    norms, and no candidate's norm lies within 1e-6 relative of min_norm or max_norm: the device cannot put a pixel on the other side.
    The inputs are not bytes over 255: quantising them changes the images."""
    case = df.float_case(c)
    N, S = case.want.score.record[:, 0], case.want.score.S
    assert 2 * int((N >= case.score.min_count).sum()) >= len(N) and (S != 0).any(), (N, S)
    assert ((N < case.score.min_count) == (S == 0)).all()
    pts = case.want.score.points
    nrm = pts.nrm[pts.candidate]
    assert case.gap > 0
    for limit in (case.score.min_norm, case.score.max_norm):
        assert (np.abs(nrm - limit) > 1e-6 * limit).all(), (limit, np.abs(nrm - limit).min())
    assert case.pred.dtype == np.float32 and not np.array_equal(ds.as_float(df.quantise(case.pred))[0], case.pred)
    assert (case.ref.dtype == np.uint8) == (c.ref_kind == "bytes")


@pytest.mark.parametrize("shape", df.SUB_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_sub_byte_case_is_dead_on_bytes_and_live_on_floats(shape):
    """The reason for the feature: f0 and f1 differ by at most half a grey level and both quantise to b.  The byte restatement sees two
    equal images: the field is zero everywhere, N = 0 and S = 0 in every sample.  The float restatement has a field with a median norm of
    thousandths of a pixel, at least min_count members in every sample and a non-zero score; min_norm and max_norm each sit in a gap."""
    w, h, C = shape
    case = df.sub_byte_case(w, h, C)
    assert case.b.shape == (df.B, C, h, w) and case.b.max() <= 254
    assert np.array_equal(df.quantise(case.f0), case.b) and np.array_equal(df.quantise(case.f1), case.b)
    assert not np.array_equal(case.f0, case.f1) and np.abs(case.f1.astype(np.float64) - case.f0).max() <= 0.5001 / 255
    dead = case.want_byte
    assert not dead.u.any() and not dead.score.record.any() and not dead.score.S.any()
    live = case.want_float
    N, S = live.score.record[:, 0], live.score.S
    nrm = live.score.points.nrm
    print("sub-byte %dx%dx%d: N %s of %d, S %s, median norm %.3g, min norm %.3g, min_norm %.6g max_norm %.6g" %
          (w, h, C, N.astype(int).tolist(), h * w, S.tolist(), np.median(nrm), nrm.min(), case.score.min_norm, case.score.max_norm))
    assert (N >= case.score.min_count).all() and (S != 0).all()
    assert N.astype(int).tolist() == {(16, 12, 1): [45, 43], (24, 16, 3): [80, 76]}[shape]     # under the limits chosen here, by the gap rule
    assert 1e-4 < np.median(nrm) < 0.1
    assert case.gaps[0] > 0 and case.gaps[1] > 0 and 0 < case.score.min_norm < case.score.max_norm
    cand = nrm[live.score.points.candidate]
    for limit in (case.score.min_norm, case.score.max_norm):
        assert (np.abs(cand - limit) > 1e-6 * limit).all()


def test_frames_argument_rules(monkeypatch):
    from evolutionary_illusion_generator_amd import engine, fitness, train
    F = fitness.DenseFitness
    assert F().frames == "byte" and F(frames="float").frames == "float" and F.for_structure(1, frames="float").frames == "float"
    for bad in ("bytes", "Float", None, 1, True, b"float"):
        with pytest.raises(ValueError, match="frames"):
            F(frames=bad)
        with pytest.raises(ValueError, match="frames"):
            F().on_frames(bad)
    d = F(radius=5, members=train.CornerMembers(), levels=2, iters=3)
    assert d.on_frames("float") is d and d.frames == "float"
    for structure in (0, 1, 2, 3):
        r = d.resolved(structure)
        assert r.frames == "float" and (r.radius, r.levels, r.iters) == (5, 2, 3) and r.members is d.members
    assert d.on_frames("byte").resolved(1).frames == "byte"       # the objects resolved earlier carried the earlier frames
    # the flag in the settings the engine passes on; the objective does not depend on it
    pick = lambda dense: engine.Engine._dense_args(type("E", (), {"height": 12, "width": 16, "cfg": type("C", (), {"device": 0})()})(), dense)[0].flow.flags
    assert pick(F.for_structure(1)) == 0 and pick(F.for_structure(2, frames="float")) == engine.DENSE_FLOAT_FRAMES == 2
    a, b = F.for_structure(0, radius=4).flow_objective(), F.for_structure(0, radius=4, frames="float").flow_objective()
    assert type(a) is type(b) and (a.radius, a.eps) == (b.radius, b.eps) and a.score.settings(12).max_norm == b.score.settings(12).max_norm
    # the module setting, checked where DENSE_MEMBERS is
    assert fitness.DENSE_FRAMES_CHOICES == ("byte", "float")
    monkeypatch.setattr(fitness, "DENSE_FRAMES", "byte")
    assert fitness.resolve_score("dense", 1).frames == "byte"
    monkeypatch.setattr(fitness, "DENSE_FRAMES", "float")
    got = fitness.resolve_score("dense", 2)
    assert got.frames == "float" and got.members is None and type(got.score).__name__ == "FreeScore"
    monkeypatch.setattr(fitness, "DENSE_MEMBERS", "corners")
    got = fitness.resolve_score("dense", 1)
    assert got.frames == "float" and isinstance(got.members, train.CornerMembers)
    assert fitness.resolve_score(F.for_structure(1), 1).frames == "byte"      # an object carries its own
    monkeypatch.setattr(fitness, "FITNESS_SCORE", "dense")
    assert fitness.resolve_score(None, 0).frames == "float"
    monkeypatch.setattr(fitness, "DENSE_FRAMES", "floats")
    with pytest.raises(ValueError, match="DENSE_FRAMES"):
        fitness.resolve_score("dense", 1)
    from evolutionary_illusion_generator_amd import synth
    cfg = synth.make_config(2, 1)
    with pytest.raises(ValueError, match="DENSE_FRAMES"):        # before any engine exists
        fitness.get_fitnesses_neat(1, synth.make_population(2, cfg, seed=0), "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, best_dir=None)


def test_the_chunking_functions_pass_the_object_on(monkeypatch):
    """`evaluate_population` hands the engine the float DenseFitness it was given, resolved, chunk after chunk"""
    from evolutionary_illusion_generator_amd import fitness, synth
    seen = []

    class FakeEngine:
        max_batch, _grid_key = 2, None

        def set_grid(self, planes):
            pass

        def eval_population(self, gb, structure, dense=None, **kw):
            seen.append((gb.n_genomes, dense))
            return np.zeros(gb.n_genomes)

    monkeypatch.setattr(fitness, "_engine_for", lambda *a, **k: FakeEngine())
    cfg = synth.make_config(2, 1)
    pop = [g for _, g in synth.make_population(3, cfg, seed=0)]
    d = fitness.DenseFitness.for_structure(1, frames="float")
    fitness.evaluate_population(1, pop, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, score=d)
    assert [n for n, _ in seen] == [2, 1] and all(x is d and x.frames == "float" for _, x in seen)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _forward_worker(rank, world, port, q, source):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from evolutionary_illusion_generator_amd import fitness, genome, synth
    fitness.GENOME_SOURCE = source
    seen = []

    def fake_batch(structure, gb, n_in, *a, score=None, **k):   # the stubbed evaluator: the frames of the score it was given decide the value
        seen.append(getattr(score, "frames", score))
        return np.arange(gb.n_genomes) + (100.0 if getattr(score, "frames", None) == "float" else 0.0) + 1000.0 * rank

    def fake_eval(structure, genomes, model, config, *a, **k):
        return fake_batch(structure, genome.GenomeBatch(genomes, config, 1, n_leaves=2, native=False), 2, **k)

    fitness.evaluate_batch, fitness.evaluate_population = fake_batch, fake_eval
    cfg = synth.make_config(2, 1)
    genomes = [g for _, g in synth.make_population(5, cfg, seed=3)]
    out, err = {}, None
    try:
        for name, score in (("byte", fitness.DenseFitness.for_structure(1)), ("float", fitness.DenseFitness.for_structure(1, frames="float"))):
            out[name] = fitness.population_fitness(1, genomes, "synthetic", cfg, 64, 64, [1, 4, 8], c_dim=1, score=score).tolist()
    except Exception as e:  # noqa: BLE001
        err = "%s: %s" % (type(e).__name__, e)
    q.put((rank, out, seen, err))
    dist.destroy_process_group()


@pytest.mark.parametrize("source", ["rank0", "replicated"])
def test_population_fitness_forwards_float_frames_through_sharded_map(source):
    """gloo, world 2, a stubbed evaluator: a DenseFitness with frames="float" reaches every rank's evaluator as it was given, and the
    all-gather carries one float64 per genome as without it"""
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
        sparse = [0.0, 1.0, 2.0, 1000.0, 1001.0]       # 5 genomes over 2 ranks: rank 0 evaluates 3, rank 1 evaluates 2
        assert out["byte"] == sparse and out["float"] == [v + 100.0 for v in sparse]
        assert seen == ["byte", "float"], seen


def test_abi_surface():
    import ctypes
    from evolutionary_illusion_generator_amd import engine
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    for n in ("eigen_dense_score_float", "eigen_debug_dense_gray"):
        assert re.search(r"^int %s\(eigen_engine\* e," % n, header, re.M), n
        assert engine.EXPORTS.count(n) == 1
    assert re.search(r"^#define EIGEN_DENSE_FLOAT_FRAMES 2$", header, re.M) and engine.DENSE_FLOAT_FRAMES == df.DENSE_FLOAT_FRAMES == 2
    assert re.search(r"#define EIGEN_ABI_VERSION 4\b", header) and engine.ABI_VERSION == 4
    assert ctypes.sizeof(engine.DenseSettingsC) == 32 and ctypes.sizeof(engine.EigenConfig) == 152
    if os.path.exists(engine.LIB_PATH):
        lib = ctypes.CDLL(engine.LIB_PATH)
        for n in ("eigen_dense_score_float", "eigen_debug_dense_gray"):
            getattr(lib, n)


def test_the_new_header_is_the_flow_stages_alone():
    """csrc/dense_float_kernels.h is included by flow_stage.hip and by nothing else, and the kernels the byte stage is read by keep their text"""
    csrc = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if '#include "dense_float_kernels.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["flow_stage.hip"]
    text = open(os.path.join(csrc, "dense_float_kernels.h")).read()
    assert "namespace eigt" in text and all(k in text for k in df.FLOAT_KERNELS)


@pytest.mark.parametrize("kernel", df.FLOAT_KERNELS)
def test_new_kernels_have_no_scratch_and_no_spills(kernel):
    from tests.train_support import check_no_scratch_and_no_spills
    check_no_scratch_and_no_spills(kernel)
