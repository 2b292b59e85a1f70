"""CPU: the flow objective's structure scores, Bands and Free ("The structure scores").
tests/flow_struct_support.py's numpy restatement is pinned to oracle/scores.py on the member vectors and to torch autograd, the cases are
shown to satisfy the conditions the GPU test relies on, and the host side (the Python classes' argument rules, the command line, the
header and the exports, the kernels' register metadata) is checked."""
import argparse
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, train
from tests import flow_score_support as ss
from tests import flow_struct_support as st
from tests.train_support import check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _stage(c):
    pred, ref, ref64, mask, sc = st.stage_case(c)
    return pred, ref64, mask, sc, st.struct_stage_ref(pred, ref64, c.r, 1e-2, mask, sc, scale=0.75)


@pytest.mark.parametrize("c", st.STAGE_CASES, ids=st.stage_id)
def test_the_cases_satisfy_their_conditions(c):
    """From the restatement alone.  Every sample meant to be live has members, and at least a tenth of its candidates are excluded by
    max_norm; no candidate's norm is within 1e-9 relative of either limit.  Bands: members on both sides of middle, and members with
    y == lim_hi and with y == middle; with min_count = 25 the 12 x 8 shape has one sample below the count beside a live one, and every
    case keeps a live sample.  Free: the smallest |theta_j - opt_ij| over the close pairs and the smallest distance of theta_i + f pi from a
    multiple of 2 are at least 1e-9, seven orders over an ulp of pi, and no member has |ny| < 1e-9: an arccos that differs in the last
    place between numpy and the device cannot then change a sign or a wrap.  The `empty` case's second sample has a zero field."""
    pred, ref64, mask, sc, s = _stage(c)
    pts, rec = s.score.points, s.score.record
    for b in range(st.B_STAGE):
        cand = pts.candidate[b]
        if c.empty and b == 1:
            assert not s.u[b].any() and rec[b, 0] == 0 and s.score.S[b] == 0.0
            continue
        assert rec[b, 0] == pts.member[b].sum() >= 1
        assert (cand & (pts.nrm[b] > sc.max_norm)).sum() >= 0.1 * cand.sum()
        for limit in (sc.max_norm, sc.min_norm):
            assert np.abs(pts.nrm[b][cand] - limit).min() > 1e-9 * limit
        if c.kind == "bands":
            ys = np.nonzero(pts.member[b])[0]
            middle = int(sc.lim_hi / 2.0)
            assert (ys < middle).any() and (ys >= middle).any() and (ys == middle).any() and (ys == int(sc.lim_hi)).any() and ys.max() == int(sc.lim_hi), (b, sorted(set(ys)))
        else:
            p = s.score.pairs[b]
            assert p.min_gap >= 1e-9 and p.min_wrap >= 1e-9, (p.min_gap, p.min_wrap)
            assert np.abs(pts.ny[b][pts.member[b]]).min() >= 1e-9
    if c.kind == "bands":
        assert (sc.lim_lo, sc.lim_hi) == (0.0, (c.h / 4.0) * 2.0)
        below = [bool(rec[b, 0] < c.min_count) for b in range(st.B_STAGE)]
        assert below.count(True) <= 1 and (c.min_count == 25 or not any(below)), rec[:, 0]
        if (c.w, c.h) == (12, 8):
            assert below.count(True) == (1 if c.min_count == 25 else 0), rec[:, 0]
        assert [bool(v == 0.0) for v in s.score.S] == below
    elif c.max_distance < 100.0:
        # both sides of the comparison occur, and at 16 x 12 a pair sits on it: d2 == D D exactly
        ys, xs = np.nonzero(pts.member[0])
        d2 = (xs[None] - xs[:, None]) ** 2 + (ys[None] - ys[:, None]) ** 2
        DD = c.max_distance ** 2
        assert (d2 < DD).any() and (d2 > DD).any() and ((d2 == DD).any() or c.max_distance != 5.0)


@pytest.mark.parametrize("c", st.STAGE_CASES, ids=st.stage_id)
def test_the_restatement_is_the_oracles_score_on_the_member_vectors(c):
    """S_b against oracle.scores.horizontal_symmetry_score, respectively 0.5 swarm_score + 0.1 strength_number + 0.4 min(n, 15) / 15, on
    the members as [x, y, dx, dy] rows in pixel order: within 1e-10 absolute.  The oracle's swarm_score has the distance 100 built in, so
    the Free cases are compared with max_distance 100 on their own members, whatever distance the case itself uses."""
    pred, ref64, mask, sc, s = _stage(c)
    if c.kind == "free" and sc.max_distance != 100.0:
        sc = sc._replace(max_distance=100.0)
        s = st.struct_stage_ref(pred, ref64, c.r, 1e-2, mask, sc, scale=0.75)
    for b in range(st.B_STAGE):
        m = s.score.points.member[b]
        if not m.any():
            assert s.score.S[b] == 0.0
            continue
        want = st.oracle_value(s.u[b], m, sc, c.w, c.h)
        live = s.score.record[b].copy()
        live[0] = max(live[0], c.min_count) if c.kind == "bands" else live[0]      # the value of the members, whatever the count rule makes of the sample
        assert abs(st.sample_value(live, sc) - want) <= 1e-10, (b, st.sample_value(live, sc), want)
        assert s.score.S[b] == (0.0 if m.sum() < c.min_count else st.sample_value(live, sc))
    assert s.value == (s.score.S[0] + s.score.S[1]) / 2.0 and s.value != 0


@pytest.mark.parametrize("c", st.STAGE_CASES, ids=st.stage_id)
def test_the_analytic_gradient_is_autograds(c):
    """g = d S_b / d u against torch float64 autograd of `torch_struct_of_field` with membership detached: within 1e-12 of the largest
    element; and the seed and the reference gradient through the whole stage, scale 0.75, against autograd of `torch_struct_term`, by
    the same rule.  A sample below min_count, or with no member, has an exactly zero g, seed and reference gradient."""
    pred, ref64, mask, sc, s = _stage(c)
    ut = torch.from_numpy(s.u.copy()).requires_grad_(True)
    (gu,) = torch.autograd.grad(st.torch_struct_of_field(ut, mask, sc)[0].sum(), ut)
    gu = gu.numpy()
    assert np.abs(gu).max() > 0 and np.abs(s.score.g - gu).max() <= 1e-12 * np.abs(gu).max(), np.abs(s.score.g - gu).max() / np.abs(gu).max()
    assert not s.score.g[:, :, ~s.score.points.member.any(0)].any()
    P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    x = torch.from_numpy(ref64.copy()).requires_grad_(True)
    f, scale, u = st.torch_struct_term(P, x, c.r, 1e-2, mask, sc)
    gp, gx = (g.numpy() for g in torch.autograd.grad(0.75 * f, [P, x]))
    assert abs(float(f.detach()) - s.value) <= 1e-12 and scale >= abs(float(f.detach()))
    assert np.abs(s.seed64 - gp).max() <= 1e-12 * np.abs(gp).max(), np.abs(s.seed64 - gp).max() / np.abs(gp).max()
    assert np.abs(s.grad64 - gx).max() <= 1e-12 * np.abs(gx).max(), np.abs(s.grad64 - gx).max() / np.abs(gx).max()
    for b in range(st.B_STAGE):
        if s.score.record[b, 0] < c.min_count or s.score.record[b, 0] == 0:
            assert not s.seed64[b].any() and not s.grad64[b].any() and not gp[b].any() and not gx[b].any()
        else:
            assert s.seed64[b].any() and s.grad64[b].any()


def test_a_given_record_is_taken_as_it_is():
    for c in (st.STAGE_CASES[0], st.STAGE_CASES[-2]):
        pred, ref64, mask, sc, s = _stage(c)
        again = st.struct_ref(s.u, mask, sc, record=s.score.record)
        assert again.value == s.value and np.array_equal(again.g, s.score.g)
        rec = s.score.record.copy()
        rec[0, 1] += 0.25
        assert not np.array_equal(st.struct_ref(s.u, mask, sc, record=rec).g[0], s.score.g[0])


def test_structure_score_argument_rules():
    b, f = train.BandsScore(), train.FreeScore()
    assert (b.max_norm, b.min_norm, b.limits, b.min_count, b.structure) == (0.15, 1e-3, None, 1, 0)
    assert (f.max_norm, f.min_norm, f.max_distance, f.min_count, f.weights, f.structure) == (0.4, 1e-3, 100.0, 1, (0.5, 0.1, 0.4), 2)
    c = b.settings(10)
    assert (c.structure, c.min_count, c.max_norm, c.min_norm, c.lim_lo, c.lim_hi) == (0, 1, 0.15, 1e-3, 0.0, 5.0)
    assert train.BandsScore(limits=(2, 9.5)).settings(120).lim_hi == 9.5 and train.BandsScore(limits=(-3, -3)).settings(8).lim_lo == -3.0
    c = f.settings(10)
    assert (c.structure, c.min_count, c.max_norm, c.min_norm, c.max_distance, list(c.w)) == (2, 1, 0.4, 1e-3, 100.0, [0.5, 0.1, 0.4])
    nan, inf = float("nan"), float("inf")
    common = [dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=nan), dict(max_norm=inf), dict(min_norm=-1e-3), dict(min_norm=0.5), dict(min_norm=nan),
              dict(min_count=0), dict(min_count=-1), dict(min_count=2.5), dict(min_count=True)]
    for kw in common + [dict(limits=(5, 4)), dict(limits=(0, inf)), dict(limits=(nan, 3)), dict(limits=(1,)), dict(limits=(0, 2.1e9)), dict(limits=(-3e9, -2.1e9))]:
        with pytest.raises(ValueError):
            train.BandsScore(**kw)
    for kw in common + [dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=nan), dict(max_distance=inf), dict(weights=(-0.1, 1, 1)),
                        dict(weights=(0, 0, 0)), dict(weights=(inf, 1, 1)), dict(weights=(1, nan, 0)), dict(weights=(1, 1))]:
        with pytest.raises(ValueError):
            train.FreeScore(**kw)
    assert train.FreeScore(min_norm=0.0, weights=(0, 0, 1)).weights == (0.0, 0.0, 1.0)
    # accepted wherever a FlowScore is; anything else is still refused
    d = train.flow_direction("tangent", 6, 4)
    with_score = lambda cls: lambda score=None, **kw: cls(**kw).scored(score)
    for s in (b, f):
        for make in (train.FlowObjective, with_score(train.FlowObjective), with_score(train.PredictionFlow), lambda **kw: train.make_flow("frame", **kw),
                     lambda **kw: train.make_flow("prediction", **kw)):
            assert make(score=s).score is s
            with pytest.raises(ValueError):
                make(direction=d, score=s)
            with pytest.raises(ValueError):
                make(score={"max_norm": 0.3})
        assert train._entry_key(train.FlowObjective(score=s)) == "structure"
    assert train._entry_key(train.FlowObjective(score=train.FlowScore())) == "score" and train._entry_key(train.PredictionFlow()) == "prediction"
    assert train._ENTRIES[True, "structure"][0] == "eigen_trainer_loss_grad_flow_structure"
    assert len(train.BANDS_STATS) == len(train.FREE_STATS) == st.REC and train.BANDS_STATS[8] == train.FREE_STATS[8] == "score"
    assert b.stats is train.BANDS_STATS and f.stats is train.FREE_STATS
    for name in ("BandsScore", "FreeScore", "structure_score"):
        assert name in train.__all__
    # structure_score: the fitness's numbering
    from evolutionary_illusion_generator_amd.fitness import StructureType
    kinds = {StructureType.Bands: train.BandsScore, StructureType.Circles: train.FlowScore, StructureType.Free: train.FreeScore, StructureType.CirclesFree: train.FlowScore}
    for k, cls in kinds.items():
        assert type(train.structure_score(k)) is cls and type(train.structure_score(int(k))) is cls
    assert train.structure_score(0, max_norm=0.2).max_norm == 0.2 and train.structure_score(2, max_distance=7).max_distance == 7.0
    for bad in (4, -1, 1.5, True, "bands"):
        with pytest.raises((ValueError, TypeError)):
            train.structure_score(bad)
    with pytest.raises(TypeError):
        train.structure_score(0, max_distance=5)


def test_the_command_line():
    """--flow-score-structure: circles by default, so every existing command line states what it did; auto follows --structure; and
    --flow-max-norm, left unset, is the chosen structure's own limit"""
    from examples import flow_args
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="flow")
    ap.add_argument("--structure", type=int, default=1)
    flow_args.add_flow_arguments(ap)
    of = lambda *argv: flow_args.flow_of(ap.parse_args(list(argv)), 16, 12)
    assert of().score is None and of("--flow-score-structure", "bands").score is None
    for argv, cls, limit in (((), train.FlowScore, 0.3), (("--flow-score-structure", "circles"), train.FlowScore, 0.3),
                             (("--flow-score-structure", "bands"), train.BandsScore, 0.15), (("--flow-score-structure", "free"), train.FreeScore, 0.4),
                             (("--flow-score-structure", "auto"), train.FlowScore, 0.3), (("--flow-score-structure", "auto", "--structure", "0"), train.BandsScore, 0.15),
                             (("--flow-score-structure", "auto", "--structure", "2"), train.FreeScore, 0.4),
                             (("--flow-score-structure", "auto", "--structure", "3"), train.FlowScore, 0.3)):
        s = of("--flow-score", *argv).score
        assert type(s) is cls and s.max_norm == limit, argv
        assert of("--flow-score", "--flow-max-norm", "0.25", *argv).score.max_norm == 0.25
    assert of("--flow-score", "--flow-pairing", "prediction", "--flow-score-structure", "free").pairing == "prediction"
    with pytest.raises(SystemExit):
        of("--flow-score-structure", "rings")
    assert flow_args.flow_of(ap.parse_args(["--objective", "mse", "--flow-score"]), 16, 12) is None


def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    for name in ("eigen_trainer_flow_term_structure", "eigen_trainer_loss_grad_flow_structure", "eigen_trainer_debug_free_planes"):
        assert name in declared and name in engine.EXPORTS, name
    assert engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header
    body = re.search(r"typedef struct \{([^}]*)\} eigen_flow_structure_score;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(double|int32_t)\s+([^;]+);", body)
    names = [n.strip().split("[")[0] for _, group in fields for n in group.split(",")]
    assert names == [n for n, _ in train.FlowStructureSettings._fields_]
    assert ctypes.sizeof(train.FlowStructureSettings) == 2 * 4 + 8 * 8 and train.FlowStructureSettings.max_norm.offset == 8 and train.FlowStructureSettings.w.offset == 48
    args = lambda name: [a.strip() for a in re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).replace("\n", " ").split(",")]
    pair, struct = args("eigen_trainer_loss_grad_flow_pair"), args("eigen_trainer_loss_grad_flow_structure")
    assert struct == pair[:-1] + ["const eigen_flow_structure_score* score", "void* stream"]
    swap = lambda a: [v.replace("eigen_flow_score", "eigen_flow_structure_score") for v in a]
    assert args("eigen_trainer_flow_term_structure") == swap(args("eigen_trainer_flow_term_score"))


def test_the_kernels_live_in_their_own_header():
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    text = open(os.path.join(CSRC, "flow_struct_kernels.h")).read()
    assert set(re.findall(pat, text)) == set(st.FLOW_STRUCT_KERNELS)
    assert set(re.findall(pat, open(os.path.join(CSRC, "flow_score_kernels.h")).read())) == set(ss.FLOW_SCORE_KERNELS)
    for name in os.listdir(CSRC):
        if name != "flow_struct_kernels.h" and name.endswith((".h", ".hip")):
            assert not set(re.findall(pat, open(os.path.join(CSRC, name)).read())) & set(st.FLOW_STRUCT_KERNELS), name
    assert '#include "flow_struct_kernels.h"' in open(os.path.join(CSRC, "flow_stage.hip")).read()
    assert re.search(r"STRUCT_REC\s*=\s*%d\b" % st.REC, text) and re.search(r"STRUCT_SLICES\s*=\s*%d\b" % st.SLICES, text)
    assert "atomic" not in text.replace("no float atomics", "")
    assert ("STRUCT_PI = %r" % st.PI) in text


@pytest.mark.parametrize("kernel", st.FLOW_STRUCT_KERNELS)
def test_no_scratch_and_no_spills(kernel):
    """every instantiation (both structures and both passes of the moment and the final kernel, both structures of the gradient kernel) has
    no scratch and no spills, and its LDS stays under 64 KB"""
    check_no_scratch_and_no_spills(kernel)
    from tests.train_support import _kernel_stats
    stats = _kernel_stats()
    names = [n for n in stats if re.match(r"_ZN4eigt\d+%s" % kernel, n)]
    want = {"tflow_struct_moment_kernel": 4, "tflow_struct_final_kernel": 4, "tflow_struct_grad_kernel": 2}.get(kernel, 1)
    assert len(names) == want, names
    for n in names:
        for s in stats[n]:
            assert s["group_segment_fixed_size"] < 64 * 1024, (n, s)


TRAIN_HOST = st.TRAIN_CASES


@functools.lru_cache(maxsize=None)
def _train_case(c):
    _, fields = st.train_case_reference(c, st.train_case_score(c, 1.0), leaf=None)
    max_norm, half = st.case_max_norm(fields, st.train_case_score(c, 1.0))
    sc = st.train_case_score(c, max_norm)
    return (sc, half) + st.train_case_reference(c, sc, leaf=None) + st.train_case_reference(c, sc, dtype=torch.float32, leaf=None)


@pytest.mark.parametrize("c", TRAIN_HOST, ids=st.train_case_id)
def test_the_training_cases_keep_their_members_under_float32(c):
    """For every training case of tests/test_gpu_flow_struct.py, on the CPU: with max_norm chosen by
    `case_max_norm` every sample of every weighted term has members; the norms of the float32 network's fields stay within a hundredth
    of half the gap max_norm sits in, and of the nearest norm's distance to min_norm, so membership is the same on both sides; for Free, whose
    gradient is piecewise constant in the angles, no close pair is nearer to a change of sign or to a wrap than the float32 network moves
    its two angles (`free_pairs_at_risk(safety=1)`); with the network in float32 the loss stays within the GPU test's bound, 1e-5 of its
    scale.  Printed, not asserted, because both depend on the CPU's float32 rounding: the pairs at risk under FOUR times that movement
    and every weight gradient's distance from the float64 one.  The weight seeds of `STRUCT_SEEDS` were chosen where these were measured,
    so that the first is 0 and the second at most 6.3e-5 of the largest element and of the norm (the float32 yardstick of
    tests/test_flow_obj_host.py is 8.07e-5)."""
    sc, half, r64, f64, r32, f32 = _train_case(c)
    assert len(f64) >= 1
    n64, n32 = np.concatenate(st.candidate_norms(f64, sc)), np.concatenate(st.candidate_norms(f32, sc))
    dev = np.abs(n32 - n64).max()
    assert dev <= 0.01 * half and dev <= 0.01 * np.abs(n64 - sc.min_norm).min(), (dev, half)
    for u64, u32 in zip(f64, f32):
        a, b = st.struct_ref(u64, None, sc), st.struct_ref(u32, None, sc)
        assert (a.record[:, 0] >= 1).all() and np.array_equal(a.points.member, b.points.member), a.record[:, 0]
    if c.kind == "free":
        print("%s: close pairs at risk under four times the float32 movement: %d" % (st.train_case_id(c), sum(st.free_pairs_at_risk(u64, u32, None, sc) for u64, u32 in zip(f64, f32))))
        assert sum(st.free_pairs_at_risk(u64, u32, None, sc, safety=1.0) for u64, u32 in zip(f64, f32)) == 0
    assert r64.scale > 0 and abs(r32.loss - r64.loss) <= 1e-5 * r64.scale, (r32.loss, r64.loss)
    for k, r in r64.grads.items():
        a = r32.grads[k]
        assert r.any(), "%s: the reference gradient is zero" % k
        print("%s %s: float32 network against float64, max %.3e norm %.3e of the reference's" % (
            st.train_case_id(c), k, np.abs(a - r).max() / max(np.abs(r).max(), 1e-300), np.linalg.norm((a - r).ravel()) / max(np.linalg.norm(r.ravel()), 1e-300)))


@pytest.mark.parametrize("kind,w,h,ch", st.REFINE_ROWS)
def test_refinement_on_the_reference_alone(kind, w, h, ch):
    """refine_stills' loop under PredictionFlow(score=...) on the float64 reference alone, 8 steps of 2 bytes: the term rises at exactly
    the shapes of RISING_SHAPES.  Measured, first -> last.  Bands: 12x8 0.279 -> 0.349, 16x12 0.486 -> 0.509, 24x16 0.357 -> 0.509,
    40x24 0.575 -> 0.640.  Free (max_distance 10): 12x8 0.593 -> 0.690, 16x12 0.746 -> 0.774, 40x24 0.8836 -> 0.8900; at 24x16 it moves
    within 0.7476 .. 0.7524 and ends below its start, 0.7510 -> 0.7476."""
    stills, hist = st.refine_reference(kind, w, h, ch)
    assert hist.shape == (9,) and np.isfinite(hist).all()
    assert (hist[-1] > hist[0]) == ((w, h, ch) in st.RISING_SHAPES[kind]), hist
