"""The flow objective through the pyramidal, iterated solve, without a GPU ("The iterated solve's gradient"): the
rules and the routing of ``FlowObjective.solved`` / ``make_flow(levels=, iters=)`` / ``DenseFitness.solve_objective``, the ABI surface,
the resources of the new kernels in the built library, and the float64 autograd statement of tests/flow_iter_support.py against itself:
its forward is `dense_pyr_ref`, its gradient is alive (far from the single step's and from two cut variants), reordering its windows
moves it by less than 2^-30 of its maximum, and every training case passes the project's float32 yardstick."""
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, fitness, train
from tests import dense_pyr_support as dp
from tests import flow_iter_support as fi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {"reorder": 0.0, "yardstick": 0.0}


def test_solved_carries_the_rules_and_the_words_of_dense_fitness():
    for cls in (train.FlowObjective, train.PredictionFlow):
        flow = cls()
        assert flow.solve is None and not flow.real_solve and flow.solve_on(16, 12) is None
        assert flow.solved() is flow and flow.solve == (1, 1) and not flow.real_solve
        assert flow.solved(3, 2).solve == (3, 2) and flow.real_solve
        assert not hasattr(flow, "levels") and not hasattr(flow, "iters")
        for kw, words in ((dict(levels=0), "levels 0 outside 1 .. 6"), (dict(levels=7), "levels 7 outside 1 .. 6"), (dict(iters=0), "iters 0 outside 1 .. 32"),
                          (dict(iters=33), "iters 33 outside 1 .. 32"), (dict(levels=True), "levels True outside 1 .. 6"), (dict(iters=2.0), "iters 2.0 outside 1 .. 32")):
            with pytest.raises(ValueError, match=re.escape(words)):
                cls().solved(**kw)
            with pytest.raises(ValueError, match=re.escape(words)):       # the same words as the fitness's
                fitness.DenseFitness(**kw)
    s = train.FlowObjective().solved(2, 3).solve_on(16, 12)
    assert isinstance(s, engine.DenseSolveC) and (s.levels, s.iters) == (2, 3)
    with pytest.raises(ValueError, match=re.escape("levels 3: the coarsest level of a 16 x 12 image is 4 x 3, below 4 pixels")):
        train.FlowObjective().solved(3, 1).solve_on(16, 12)
    with pytest.raises(ValueError, match=re.escape("levels 3: the coarsest level of a 16 x 12 image is 4 x 3, below 4 pixels")):
        fitness.DenseFitness(levels=3).solve_on(16, 12)


def test_a_real_solve_routes_to_the_new_entries_and_one_by_one_to_todays():
    score, mem = train.FlowScore(), train.CornerMembers()
    plain = [train.FlowObjective(), train.PredictionFlow(), train.FlowObjective(score=score), train.FlowObjective(score=train.BandsScore()),
             train.FlowObjective(score=score, members=mem)]
    keys = ["frame", "prediction", "score", "structure", "members"]
    assert [train._entry_key(f) for f in plain] == keys
    assert [train._entry_key(f.solved(1, 1)) for f in plain] == keys
    assert [train._entry_key(f.solved(2, 1)) for f in plain] == ["iter"] * 5 == [train._entry_key(f.solved(1, 2)) for f in plain]
    assert train._ENTRIES[True, "iter"][0] == "eigen_trainer_loss_grad_flow_iter"
    assert train.make_flow("prediction").solve is None and train.make_flow("frame", levels=1, iters=1).solve is None
    f = train.make_flow("prediction", 5, score=score, levels=3, iters=2)
    assert isinstance(f, train.PredictionFlow) and f.solve == (3, 2) and f.radius == 5 and train._entry_key(f) == "iter"
    assert train.make_flow("frame", reference="moving", levels=2, iters=2).reference == "moving"
    with pytest.raises(ValueError, match="levels 9 outside 1 .. 6"):
        train.make_flow("frame", levels=9)


def test_solve_objective_carries_the_solve_and_flow_objective_still_does_not():
    F = fitness.DenseFitness
    d = F.for_structure(0, radius=4, levels=2, iters=3)
    flow = d.flow_objective()
    assert isinstance(flow, train.PredictionFlow) and flow.solve is None and train._entry_key(flow) == "structure"
    assert "single" in F.flow_objective.__doc__ and "A gradient through the iteration does" in F.flow_objective.__doc__
    climb = d.solve_objective()
    assert isinstance(climb, train.PredictionFlow) and climb.solve == (2, 3) and climb.radius == 4 and isinstance(climb.score, train.BandsScore)
    assert train._entry_key(climb) == "iter" and not hasattr(climb, "levels")
    assert isinstance(d.solve_objective("frame"), train.FlowObjective) and d.solve_objective("frame").pairing == "frame"
    assert train._entry_key(F.for_structure(1).solve_objective()) == "score"      # one level, one iteration: today's entry
    with pytest.raises(ValueError, match="no score yet"):
        F(levels=2).solve_objective()


def test_abi_surface():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    one_line = lambda n: re.sub(r"\s+", " ", re.search(r"^int %s\([^;]*;" % n, header, re.M).group(0))
    members, it = one_line("eigen_trainer_flow_term_members"), one_line("eigen_trainer_flow_term_iter")
    assert it == members.replace("_members(", "_iter(").replace("void* stream);", "void* stream, const float* d_dir, const eigen_dense_solve* solve);")
    members, it = one_line("eigen_trainer_loss_grad_flow_members"), one_line("eigen_trainer_loss_grad_flow_iter")
    assert it == members.replace("_members(", "_iter(").replace("void* stream);", "void* stream, const eigen_dense_solve* solve);")
    for n in ("eigen_trainer_flow_term_iter", "eigen_trainer_loss_grad_flow_iter", "eigen_trainer_debug_flow_iter"):
        assert engine.EXPORTS.count(n) == 1
    assert re.search(r"#define EIGEN_ABI_VERSION 4\b", header) and engine.ABI_VERSION == 4
    if os.path.exists(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "libeigen_hip.so")):
        lib = engine.load_library()
        assert lib.eigen_abi_version() == 4 and hasattr(lib, "eigen_trainer_flow_term_iter") and hasattr(lib, "eigen_trainer_loss_grad_flow_iter")


@pytest.mark.parametrize("kernel", fi.FLOW_ITER_KERNELS)
def test_new_kernels_have_no_scratch_and_no_spills(kernel):
    from tests.train_support import check_no_scratch_and_no_spills
    check_no_scratch_and_no_spills(kernel)


def test_the_new_kernel_file_names_every_kernel_and_adds_nothing_atomically():
    src = open(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc", "flow_iter_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert sorted(set(re.findall(r"\b(tfiter_\w+_kernel)\(", code))) == sorted(fi.FLOW_ITER_KERNELS)
    assert "atomic" not in code.lower()


@pytest.mark.parametrize("name", fi.STAGE_NAMES)
def test_the_statement_is_the_restatement_forward_and_alive_backward(name):
    """Per stage case: the forward of the autograd statement is `dense_pyr_ref` on the case's bytes to 1e-12; under the energy mode the
    full gradient differs from the single step's, from the coarse-path-cut one (cases of more than one level) and from the
    position-held-constant one by at least 0.05 of its maximum, for both images, and the reference gradient is not zero."""
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    pred, ref = fi.as_floats(img1), fi.as_floats(img0)
    full = fi.stage_reference(name)["energy"]
    want = dp.dense_pyr_ref(img0, img1, r, fi.EPS, levels, iters)
    assert np.abs(full.u - want).max() <= 1e-12
    assert np.abs(full.ref64).max() > 0 and np.abs(full.seed64).max() > 0
    others = {"single step": fi.single_step_grads(pred, ref, r, fi.EPS)}
    for key, kw in (("coarse path cut", dict(cut_coarse=True)), ("position held", dict(hold_position=True))):
        if key == "coarse path cut" and levels == 1:
            continue
        g = fi.stage_grads(pred, ref, r, fi.EPS, levels, iters, ("energy",), h, w, **kw)["energy"]
        assert np.array_equal(g.u, full.u)
        others[key] = (g.seed64, g.ref64)
    for key, (gP, gx) in others.items():
        for which, got, ref64 in (("I1", gP, full.seed64), ("I0", gx, full.ref64)):
            miss = np.abs(got - ref64).max() / np.abs(ref64).max()
            print("%s: %s gradient by %s differs by %.3f of the maximum" % (name, key, which, miss))
            assert miss >= 0.05, (name, key, which, miss)


def test_the_cases_reach_the_border_clamps_and_move_beyond_the_margin():
    """20 x 15 r 3 samples window positions at coordinates strictly outside the image, which the sampler's clamps replace (a coordinate
    on the border itself is not counted); 48 x 32 holds a displacement above PYR_MARGIN"""
    clamped = [0]
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case("20x15r3")
    img0, img1 = fi.stage_images("20x15r3")
    with torch.no_grad():
        fi.torch_iter_field(torch.tensor(fi.as_floats(img1), dtype=torch.float64), torch.tensor(fi.as_floats(img0), dtype=torch.float64), r, fi.EPS, levels, iters,
                            clamped=clamped)
    assert clamped[0] > 0
    assert np.abs(fi.stage_reference("48x32")["energy"].u).max() > dp.PYR_MARGIN


@pytest.mark.parametrize("name", fi.STAGE_NAMES)
def test_reordering_the_windows_stays_nine_orders_below_the_float32_store(name):
    """Per stage case and mode: summing every window of the statement in the opposite order moves the seed and the reference gradient by
    less than 2^-30 of their maximum (the GPU's bound is 2^-23).  Measured: at worst 8.0e-6 of that bound, 7e-15 of the maximum."""
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    fwd = fi.stage_reference(name)
    rev = fi.stage_grads(fi.as_floats(img1), fi.as_floats(img0), r, fi.EPS, levels, iters, fi.MODES, h, w, reverse=True)
    for mode in fi.MODES:
        for which in ("seed64", "ref64"):
            err, bound = fi.within(getattr(rev[mode], which), getattr(fwd[mode], which), fi.REORDER)
            WORST["reorder"] = max(WORST["reorder"], err / bound)
            print("%s %s %s: reversed windows move it by %.3e, bound %.3e (ratio %.2e, worst so far %.2e)" % (name, mode, which, err, bound, err / bound, WORST["reorder"]))
            assert err < bound, (name, mode, which, err, bound)


@pytest.mark.parametrize("c", fi.TRAIN_CASES, ids=fi.train_case_id)
def test_training_cases_pass_the_float32_yardstick_on_the_reference_alone(c):
    """network in float32 against float64 (the flow term float64 on the widened images either way): the worst element of every weight
    gradient within 8.07e-5 of its tensor's maximum, and every gradient is alive"""
    r64 = fi.train_case_reference(c, leaf=None)
    fed = None
    if "requant" in c.form:
        from tests.train_support import _fed_from
        fed = _fed_from(r64.pred.astype(np.float32))
    r32 = fi.train_case_reference(c, fed=fed, leaf=None, dtype=torch.float32)
    worst = max(np.abs(r32.grads[k] - r64.grads[k]).max() / np.abs(r64.grads[k]).max() for k in r64.grads)
    WORST["yardstick"] = max(WORST["yardstick"], worst)
    print("%s: float32 network against float64, worst element %.3e of its tensor's maximum (worst so far %.3e)" % (fi.train_case_id(c), worst, WORST["yardstick"]))
    assert worst <= fi.YARDSTICK, (fi.train_case_id(c), worst)
    assert r64.scale > 0 and all(np.abs(g).max() > 0 for g in r64.grads.values())


def test_refinement_on_the_reference_alone_is_recorded():
    """`refine_stills` with `DenseFitness.solve_objective()` on float64 autograd alone (tests/flow_iter_support.py `refine_reference`): the
    history is finite, its first term is a live score, and the stills move.  What the term does over the eight steps is printed and is
    what tests/test_gpu_flow_iter.py asserts of the GPU; no direction is demanded here."""
    stills, hist = fi.refine_reference()
    print("refinement through the solve on the reference alone: %s" % " ".join("%.5e" % v for v in hist))
    assert hist.shape == (9,) and np.isfinite(hist).all() and hist[0] > 0 and stills.dtype == np.uint8


def test_the_command_lines_state_the_solve():
    """--flow-levels / --flow-iters reach the objective through `examples/flow_args.py` (default: no solve, today's objective); the
    benchmark script names both flags and the evolution example offers --refine-solve"""
    import argparse
    from examples import flow_args
    assert "levels" in flow_args.FLOW_ARGUMENTS and "iters" in flow_args.FLOW_ARGUMENTS
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="flow")
    flow_args.add_flow_arguments(ap)
    of = lambda *argv: flow_args.flow_of(ap.parse_args(list(argv)), 16, 12)
    assert of().solve is None and train._entry_key(of()) == "frame"
    f = of("--flow-levels", "2", "--flow-iters", "3", "--flow-pairing", "prediction", "--flow-score")
    assert isinstance(f, train.PredictionFlow) and f.solve == (2, 3) and train._entry_key(f) == "iter" and isinstance(f.score, train.FlowScore)
    assert of("--flow-iters", "4").solve == (1, 4)
    with pytest.raises(ValueError, match="levels 7 outside 1 .. 6"):
        of("--flow-levels", "7")
    bench = open(os.path.join(ROOT, "scripts", "train_bench.py")).read()
    assert '"levels", "iters")' in bench and "levels=a.flow_levels, iters=a.flow_iters" in bench
    for script in ("refine_illusion.py", "refine_genomes.py", "evolve_illusion.py"):
        src = open(os.path.join(ROOT, "examples", script)).read()
        assert "add_flow_arguments(ap" in src and "flow_of(a, w, h" in src, script
    assert '"--refine-solve", default="single", choices=["single", "fitness"]' in open(os.path.join(ROOT, "examples", "evolve_illusion.py")).read()
