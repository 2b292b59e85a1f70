"""CPU: the flow objective's score mode ("The score mode").  tests/flow_score_support.py's numpy restatement is
pinned to oracle/scores.py on the member vectors and to torch autograd, the cases are shown to satisfy the conditions the GPU test
relies on, and the host side (the Python classes' argument rules, the header and the exports, the kernels' register metadata) is
checked."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd import engine, train
from oracle import scores
from tests import flow_score_support as ss
from tests.train_support import check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
CASES = [(w, h, C, r, masked, ref_kind, mc) for w, h, C, r, masked in ss.STAGE_CASES for ref_kind, _ in ss.REFS for mc in ss.MIN_COUNTS]
case_id = lambda c: "%dx%dx%d-r%d-%s-min%d" % (c[0], c[1], c[2], c[3], c[5], c[6])


@functools.lru_cache(maxsize=None)
def _stage(case):
    w, h, C, r, masked, ref_kind, mc = case
    pred, ref, ref64, mask, sc = ss.stage_case(w, h, C, r, masked, ref_kind, mc)
    return pred, ref64, mask, sc, ss.score_stage_ref(pred, ref64, r, 1e-2, mask, sc, scale=0.75)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_cases_satisfy_their_conditions(case):
    """From the restatement alone: max_norm is the median |u| of the case; every sample has at least 4 members; at least a tenth of its
    geometric candidates are excluded by max_norm; no candidate's norm is within 1e-9 relative of either limit.  With min_count = 25 both
    12 x 8 shapes have one sample below the count beside a live one, and every larger shape has none below it."""
    w, h, C, r, masked, ref_kind, mc = case
    pred, ref64, mask, sc, st = _stage(case)
    pts, rec = st.score.points, st.score.record
    assert sc.max_norm == float(np.median(pts.nrm)) and sc.min_norm == 1e-3 and (sc.r_min, sc.r_max) == (0.0, h / 2.0)
    for b in range(ss.B_STAGE):
        cand = pts.candidate[b]
        assert rec[b, 0] == pts.member[b].sum() >= 4, rec[b, 0]
        assert (cand & (pts.nrm[b] > sc.max_norm)).sum() >= 0.1 * cand.sum()
        for limit in (sc.max_norm, sc.min_norm):
            assert np.abs(pts.nrm[b][cand] - limit).min() > 1e-9 * limit
    below = [bool(rec[b, 0] < mc) for b in range(ss.B_STAGE)]
    assert below.count(True) == (1 if mc == 25 and (w, h) == (12, 8) else 0), rec[:, 0]
    assert [bool(v == 0.0) for v in st.score.S] == below


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_restatement_is_the_oracles_circles_score_on_the_member_vectors(case):
    """S_b against 0.7 oracle.scores.rotation_symmetry_score + 0.3 oracle.scores.strength_number on the members as [x, y, dx, dy] rows,
    with the oracle's own limits test: within 1e-10 absolute.  Values are O(1); the error of the exactly summed moments against numpy's
    sums is about N dist 2^-53, 1e-12 here, while a wrong membership, ddof or weight moves the value by 1e-5 or more."""
    w, h, C, r, masked, ref_kind, mc = case
    pred, ref64, mask, sc, st = _stage(case)
    for b in range(ss.B_STAGE):
        m = st.score.points.member[b]
        yy, xx = np.nonzero(m)
        vec = np.stack([xx.astype(np.float64), yy.astype(np.float64), st.u[b, 0][m], st.u[b, 1][m]], 1)
        want = sc.w_direction * scores.rotation_symmetry_score(vec, w, h, (sc.r_min, sc.r_max)) + sc.w_strength * scores.strength_number(vec, sc.max_norm)
        live = st.score.record[b].copy()
        live[0] = max(live[0], mc)     # the value of the members, whatever the count rule makes of the sample
        assert abs(ss.sample_value(live, sc) - want) <= 1e-10, (b, ss.sample_value(live, sc), want)
        assert st.score.S[b] == (0.0 if len(vec) < mc else ss.sample_value(live, sc))
    assert st.value == (st.score.S[0] + st.score.S[1]) / 2.0 and st.value > 0


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_analytic_gradient_is_autograds(case):
    """g = d S_b / d u against torch float64 autograd of `torch_score_of_field` with membership detached: within 1e-12 of the largest
    element (measured 8e-14 at worst); and the seed through the whole stage, scale 0.75, against autograd of `torch_score_term` by the
    prediction, by the same rule.  A sample below min_count has an exactly zero g, seed and reference gradient."""
    w, h, C, r, masked, ref_kind, mc = case
    pred, ref64, mask, sc, st = _stage(case)
    ut = torch.from_numpy(st.u.copy()).requires_grad_(True)
    (gu,) = torch.autograd.grad(ss.torch_score_of_field(ut, mask, sc).sum(), ut)
    gu = gu.numpy()
    assert np.abs(gu).max() > 0 and np.abs(st.score.g - gu).max() <= 1e-12 * np.abs(gu).max(), np.abs(st.score.g - gu).max() / np.abs(gu).max()
    assert not st.score.g[:, :, ~st.score.points.member.any(0)].any()
    P = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    x = torch.from_numpy(ref64.copy()).requires_grad_(True)
    f, scale, u = ss.torch_score_term(P, x, r, 1e-2, mask, sc)
    gp, gx = (g.numpy() for g in torch.autograd.grad(0.75 * f, [P, x]))
    assert abs(float(f.detach()) - st.value) <= 1e-12 and scale == abs(float(f.detach()))
    assert np.abs(st.seed64 - gp).max() <= 1e-12 * np.abs(gp).max(), np.abs(st.seed64 - gp).max() / np.abs(gp).max()
    assert np.abs(st.grad64 - gx).max() <= 1e-12 * np.abs(gx).max(), np.abs(st.grad64 - gx).max() / np.abs(gx).max()
    for b in range(ss.B_STAGE):
        if st.score.record[b, 0] < mc:
            assert not st.seed64[b].any() and not st.grad64[b].any() and not gp[b].any() and not gx[b].any()
        else:
            assert st.seed64[b].any() and st.grad64[b].any()


def test_a_given_record_is_taken_as_it_is():
    """`score_ref(record=...)` forms S_b, f and g from the moments it is given: with its own record it repeats itself to the bit, with a
    moved mean the gradient moves"""
    case = CASES[0]
    pred, ref64, mask, sc, st = _stage(case)
    again = ss.score_ref(st.u, mask, sc, record=st.score.record)
    assert again.value == st.value and np.array_equal(again.g, st.score.g) and np.array_equal(again.record[:, :9], st.score.record[:, :9])
    rec = st.score.record.copy()
    rec[0, 1] += 0.25
    assert not np.array_equal(ss.score_ref(st.u, mask, sc, record=rec).g[0], st.score.g[0])


def test_flow_score_argument_rules():
    s = train.FlowScore()
    assert (s.max_norm, s.min_norm, s.limits, s.min_count, s.weights) == (0.3, 1e-3, None, 25, (0.7, 0.3))
    c = s.settings(120)
    assert (c.max_norm, c.min_norm, c.r_min, c.r_max, c.w_direction, c.w_strength, c.min_count, c.reserved) == (0.3, 1e-3, 0.0, 60.0, 0.7, 0.3, 25, 0)
    assert train.FlowScore(limits=(2, 9.5)).settings(120).r_max == 9.5
    bad = [dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(max_norm=float("inf")), dict(min_norm=-1e-3), dict(min_norm=0.3),
           dict(min_norm=float("nan")), dict(limits=(-1, 5)), dict(limits=(5, 4)), dict(limits=(0, float("inf"))), dict(limits=(float("nan"), 3)), dict(limits=(1,)),
           dict(min_count=1), dict(min_count=0), dict(min_count=2.5), dict(min_count=True), dict(weights=(-0.1, 1)), dict(weights=(0, 0)),
           dict(weights=(float("inf"), 1)), dict(weights=(1, float("nan"))), dict(weights=(1,))]
    for kw in bad:
        with pytest.raises(ValueError):
            train.FlowScore(**kw)
    assert train.FlowScore(min_norm=0.0, min_count=2, weights=(0, 1), limits=(3, 3)).min_count == 2
    # score= on FlowObjective and make_flow, scored() on any objective (a PredictionFlow's constructor is pinned by
    # tests/test_flow_pair_host.py); the default changes nothing; a direction does not go with a score
    d = train.flow_direction("tangent", 6, 4)
    with_score = lambda cls: lambda score=None, **kw: cls(**kw).scored(score)
    for make in (train.FlowObjective, with_score(train.FlowObjective), with_score(train.PredictionFlow), lambda **kw: train.make_flow("frame", **kw),
                 lambda **kw: train.make_flow("prediction", **kw)):
        assert make().score is None and make(score=s).score is s
        with pytest.raises(ValueError):
            make(direction=d, score=s)
        with pytest.raises(ValueError):
            make(score={"max_norm": 0.3})
    assert type(train.make_flow("prediction", score=s)) is train.PredictionFlow and train.PredictionFlow().scored(s).scored(None).score is None
    assert train.FlowObjective(reference="moving", score=s).settings().flags == train.FLOW_MOVING_REFERENCE
    for fn in (train.FlowObjective.__init__, train.make_flow):
        assert inspect.signature(fn).parameters["score"].default is None
    assert inspect.signature(train.PredNetTrainer.flow_term).parameters["stats"].default is False
    assert len(train.SCORE_STATS) == ss.REC and "FlowScore" in train.__all__
    assert train._ENTRIES[True, "score"][0] == "eigen_trainer_loss_grad_flow_score"


def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    for name in ("eigen_trainer_flow_term_score", "eigen_trainer_loss_grad_flow_score"):
        assert name in declared and name in engine.EXPORTS, name
    assert engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header
    body = re.search(r"typedef struct \{([^}]*)\} eigen_flow_score;", header).group(1)
    fields = re.findall(r"\b(double|int32_t)\s+([^;]+);", body)
    names = [n.strip() for _, group in fields for n in group.split(",")]
    assert names == [n for n, _ in train.FlowScoreSettings._fields_]
    assert ctypes.sizeof(train.FlowScoreSettings) == 6 * 8 + 2 * 4
    # the training entry is eigen_trainer_loss_grad_flow_pair's arguments plus the score, the stream last
    args = lambda name: [a.strip() for a in re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).replace("\n", " ").split(",")]
    pair, score = args("eigen_trainer_loss_grad_flow_pair"), args("eigen_trainer_loss_grad_flow_score")
    assert score == pair[:-1] + ["const eigen_flow_score* score", "void* stream"]
    stage = args("eigen_trainer_flow_term_score")
    assert "const float* d_dir" not in stage and "const eigen_flow_score* score" in stage and "double* h_stats" in stage
    assert "const uint8_t* d_ref" in stage and "const float* d_fref" in stage


def test_the_kernels_live_in_their_own_header():
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    text = open(os.path.join(CSRC, "flow_score_kernels.h")).read()
    assert set(re.findall(pat, text)) == set(ss.FLOW_SCORE_KERNELS)
    assert '#include "flow_score_kernels.h"' in open(os.path.join(CSRC, "flow_stage.hip")).read()
    assert re.search(r"SCORE_REC\s*=\s*%d\b" % ss.REC, text) and re.search(r"SCORE_SLICES\s*=\s*%d\b" % ss.SLICES, text)
    assert "atomic" not in text.replace("no float atomics", "")
    # the q kernel's static LDS: three fields of 48 x 16 doubles, 18 KB, far under 64 KB at r = 16
    assert "rs[3][FLOW_ROWS][FLOW_TILE]" in text and 3 * 48 * 16 * 8 == 18432


@pytest.mark.parametrize("kernel", ss.FLOW_SCORE_KERNELS)
def test_no_scratch_and_no_spills(kernel):
    """every instantiation (both passes of the moment and the final kernel) has no scratch and no spills, and its LDS stays under 64 KB"""
    check_no_scratch_and_no_spills(kernel)
    from tests.train_support import _kernel_stats
    stats = _kernel_stats()
    names = [n for n in stats if re.match(r"_ZN4eigt\d+%s" % kernel, n)]
    if kernel != "tflow_score_q_kernel":
        assert {1, 2} == {int(re.search(r"ILi(\d)EE", n).group(1)) for n in names}, names
    for n in names:
        for s in stats[n]:
            assert s["group_segment_fixed_size"] < 64 * 1024, (n, s)


@functools.lru_cache(maxsize=None)
def _train_case(c):
    """(the case's Score, half the gap max_norm sits in, the float64 reference, its fields, the float32 one, its fields)"""
    _, fields = ss.train_case_reference(c, ss.train_case_score(c, 1.0), leaf=None)
    max_norm, half = ss.case_max_norm(fields, c.h)
    sc = ss.train_case_score(c, max_norm)
    return (sc, half) + ss.train_case_reference(c, sc, leaf=None) + ss.train_case_reference(c, sc, dtype=torch.float32, leaf=None)


@pytest.mark.parametrize("c", ss.TRAIN_CASES, ids=ss.train_case_id)
def test_the_training_cases_keep_their_members_under_float32(c):
    """For every training case of tests/test_gpu_flow_score.py, on the CPU: with max_norm chosen by `case_max_norm` every sample of every
    weighted term has at least min_count members; the norms of the float32 network's fields stay within a hundredth of half the gap
    max_norm sits in, and of the distance of the nearest norm to min_norm, of the float64 ones (measured: at most 4.2e-7 against gaps of
    4.7e-4 and more), so membership is the same on both sides; and with the network in float32 the loss and the terms stay within a tenth
    of the bound the GPU test takes, 1e-5 of their un-cancelled scale, and every weight gradient at or under the float32 yardstick of
    tests/test_flow_obj_host.py, 8.07e-5 of its largest element and of its norm."""
    sc, half, r64, f64, r32, f32 = _train_case(c)
    assert len(f64) == sum(1 for v in (ss.train_case_call(c)["step_weights"] or [1.0] * 4) if v != 0) >= 1
    n64, n32 = np.concatenate(ss.candidate_norms(f64, c.h)), np.concatenate(ss.candidate_norms(f32, c.h))
    dev = np.abs(n32 - n64).max()
    assert dev <= 0.01 * half and dev <= 0.01 * np.abs(n64 - sc.min_norm).min(), (dev, half)
    for u64, u32 in zip(f64, f32):
        a, b = ss.score_ref(u64, None, sc), ss.score_ref(u32, None, sc)
        assert (a.record[:, 0] >= sc.min_count).all() and np.array_equal(a.points.member, b.points.member), a.record[:, 0]
    assert r64.scale > 0 and abs(r32.loss - r64.loss) <= 0.1 * 1e-5 * r64.scale, (r32.loss, r64.loss)
    live = r64.term_scales > 0
    assert (np.abs(r32.terms - r64.terms)[live] <= 0.1 * 1e-5 * r64.term_scales[live]).all()
    for k, r in r64.grads.items():
        a = r32.grads[k]
        assert r.any(), "%s: the reference gradient is zero" % k
        assert np.abs(a - r).max() <= 8.07e-5 * np.abs(r).max(), (k, np.abs(a - r).max() / np.abs(r).max())
        assert np.linalg.norm((a - r).ravel()) <= 8.07e-5 * np.linalg.norm(r.ravel()), k


def test_the_training_case_list():
    ids = [ss.train_case_id(c) for c in ss.TRAIN_CASES]
    assert len(ids) == len(set(ids)) == 48 and {(c.w, c.h) for c in ss.TRAIN_CASES} == {(12, 8), (16, 12), (24, 16), (40, 24)}
    assert {c.r for c in ss.TRAIN_CASES} == {2, 7} and {c.form for c in ss.TRAIN_CASES} == {"still", "still_requant", "drifting"}
    assert {c.pairing for c in ss.TRAIN_CASES} == {"moving", "prediction"}


@pytest.mark.parametrize("w,h,ch", ss.REFINE_SHAPES)
def test_refinement_on_the_reference_alone(w, h, ch):
    """refine_stills' loop under PredictionFlow(score=...) on the float64 reference alone, 8 steps of 2 bytes: the score term rises at
    exactly the shapes of RISING_SHAPES.  Measured: 16x12 0.429 -> 0.570, 24x16 0.381 -> 0.597, 40x24 0.383 -> 0.432; at 12x8 it goes
    0.392 -> 0.632 over six steps and then drops to 0.229, where a sample's members fall below min_count: membership is a constant of
    the gradient, not of the loop."""
    stills, hist = ss.refine_reference(w, h, tuple(ch))
    assert hist.shape == (9,) and np.isfinite(hist).all()
    assert (hist[-1] > hist[0]) == ((w, h, tuple(ch)) in ss.RISING_SHAPES), hist
