"""CPU: per-sample membership of the flow objective's scores ("The corner members").  The Python classes'
argument rules, the struct layout, the header and the exports, the new kernels' register metadata, the command line, the conditions the
GPU cases rely on (from the CPU oracle) and the statement that a per-sample mask needs no new mathematics: the float64 reference under
an [n, H, W] mask is the mean of single-sample references."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import engine, train
from tests import flow_corner_support as cs
from tests.train_support import check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
ENTRIES = ("eigen_trainer_flow_members", "eigen_trainer_flow_term_members", "eigen_trainer_loss_grad_flow_members")


def test_corner_members_argument_rules():
    m = train.CornerMembers()
    assert (m.max_corners, m.quality_level, m.min_distance, m.block_size) == (100, 0.3, 7.0, 7)     # eigen_config's lk_* defaults
    for kw in (dict(max_corners=0), dict(max_corners=129), dict(max_corners=2.5), dict(max_corners=True), dict(block_size=0), dict(block_size=10),
               dict(quality_level=0.0), dict(quality_level=1.01), dict(quality_level=float("nan")), dict(min_distance=-0.5), dict(min_distance=float("inf")),
               dict(min_distance=float("nan"))):
        with pytest.raises(ValueError):
            train.CornerMembers(**kw)
    assert train.CornerMembers(max_corners=128, block_size=9, quality_level=1.0, min_distance=0.0).settings().max_corners == 128


def test_settings_and_struct_layout_round_trip():
    s = train.CornerMembers(max_corners=17, quality_level=0.05, min_distance=3.0, block_size=3).settings()
    assert (s.kind, s.max_corners, s.block_size, s.reserved, s.quality_level, s.min_distance, s.mask_bstride) == (train.FLOW_MEMBERS_CORNERS, 17, 3, 0, 0.05, 3.0, 0)
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} eigen_flow_members;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(double|int32_t|int64_t)\s+([^;]+);", body)
    ctype = {"double": ctypes.c_double, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    assert [(n.strip(), ctype[t]) for t, group in fields for n in group.split(",")] == list(train.FlowMembersSettings._fields_)
    assert ctypes.sizeof(train.FlowMembersSettings) == 4 * 4 + 3 * 8 and train.FlowMembersSettings.quality_level.offset == 16
    assert "enum { EIGEN_FLOW_MEMBERS_MASK = 0, EIGEN_FLOW_MEMBERS_CORNERS = 1 };" in header
    assert (train.FLOW_MEMBERS_MASK, train.FLOW_MEMBERS_CORNERS) == (0, 1)
    # a per-sample mask states kind MASK with one plane per sample
    f = train.FlowObjective(mask=np.ones((3, 4, 6)), score=train.FlowScore())
    m = f.members_settings(3, 4, 6)
    assert (m.kind, m.mask_bstride, m.reserved) == (train.FLOW_MEMBERS_MASK, 24, 0)
    assert train.FlowObjective(mask=np.ones((4, 6)), score=train.FlowScore()).members_settings(3, 4, 6) is None


def test_objective_argument_rules():
    score, mem = train.FlowScore(), train.CornerMembers()
    m2, m3 = np.ones((4, 6)), np.ones((3, 4, 6))
    assert train.FlowObjective(mask=m2, score=score, members=mem).members is mem
    # `reference` was the sixth positional argument before `members` existed: such a call keeps its meaning
    old = train.FlowObjective(7, 1e-2, None, None, score, "moving")
    assert old.reference == "moving" and old.members is None and train.FlowObjective(7, 1e-2, None, None, score, mem, "moving").members is mem
    for kw in (dict(mask=m3), dict(members=mem), dict(mask=m3, score=score, members=mem), dict(score=score, members="corners")):
        with pytest.raises(ValueError):
            train.FlowObjective(**kw)
    # a PredictionFlow takes its score behind the constructor: a per-sample mask without one is refused where the objective is used
    with pytest.raises(ValueError):
        train.PredictionFlow(mask=m3).on_device(None, 0, 4, 6)
    with pytest.raises(ValueError):
        train.make_flow("prediction", mask=m3)
    for cls in (train.FlowObjective, train.PredictionFlow):
        make = lambda mask=None, cls=cls: cls(mask=mask, score=score) if cls is train.FlowObjective else cls(mask=mask).scored(score)
        assert make(m3).per_sample and not make(m2).per_sample and make(m2).with_members(mem).members is mem and make().with_members(None).members is None
        for mask in (np.ones((2, 3, 4, 6)), np.zeros((3, 4, 6))):
            with pytest.raises(ValueError):
                cls(mask=mask)
        with pytest.raises(ValueError):
            cls().with_members(mem)
        with pytest.raises(ValueError):
            make(m3).with_members(mem)
        with pytest.raises(ValueError):
            make().with_members(mem).scored(None)
        with pytest.raises(ValueError):
            make(m3).scored(None)
        # n and H, W are checked against the call
        f = make(m3)
        for shape in ((2, 4, 6), (3, 5, 6), (3, 4, 7)):
            with pytest.raises(ValueError):
                f.members_settings(*shape)
    assert train.make_flow("prediction", score=score, members=mem).members is mem and train.make_flow("frame", score=score, members=mem).members is mem
    with pytest.raises(ValueError):
        train.make_flow("frame", members=mem)
    assert train._entry_key(train.FlowObjective(score=score, members=mem)) == "members" == train._entry_key(train.PredictionFlow(mask=m3).scored(train.FreeScore()))
    assert train._entry_key(train.FlowObjective(mask=m2, score=score)) == "score" and train._ENTRIES[True, "members"][0] == "eigen_trainer_loss_grad_flow_members"


def test_header_declares_the_entries_and_the_library_has_them():
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    for name in ENTRIES:
        assert name in declared and name in engine.EXPORTS, name
    assert engine.ABI_VERSION == 4 and "#define EIGEN_ABI_VERSION 4" in header
    args = lambda name: [a.strip() for a in re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1).replace("\n", " ").split(",")]
    widest = args("eigen_trainer_loss_grad_flow_score")
    assert args("eigen_trainer_loss_grad_flow_members") == widest[:-1] + ["const eigen_flow_structure_score* sscore", "const eigen_flow_members* members", "double* h_stats",
                                                                         "void* stream"]
    term = args("eigen_trainer_flow_term_score")
    i = term.index("const eigen_flow_score* score")
    assert args("eigen_trainer_flow_term_members") == term[:i + 1] + ["const eigen_flow_structure_score* sscore", "const eigen_flow_members* members"] + term[i + 1:]
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libeigen_hip.so not built")
    lib = engine.load_library()
    train._bind(lib)
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.eigen_trainer_flow_term_members.argtypes) == len(args("eigen_trainer_flow_term_members"))
    assert len(lib.eigen_trainer_loss_grad_flow_members.argtypes) == len(args("eigen_trainer_loss_grad_flow_members"))
    assert len(lib.eigen_trainer_flow_members.argtypes) == len(args("eigen_trainer_flow_members"))


def test_the_kernels_live_in_their_own_header():
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    text = open(os.path.join(CSRC, "flow_corner_kernels.h")).read()
    assert set(re.findall(pat, text)) == set(cs.FLOW_CORNER_KERNELS)
    assert '#include "flow_kernels.h"' in text and '#include "flow_corner_kernels.h"' in open(os.path.join(CSRC, "flow_stage.hip")).read()
    # the corner kernels themselves are included, not copied: they are defined in flow_kernels.h alone
    for kernel in ("gray_kernel", "mineig_kernel", "corner_select_kernel"):
        homes = [n for n in os.listdir(CSRC) if n.endswith((".h", ".hip")) and kernel in re.findall(pat, open(os.path.join(CSRC, n)).read())]
        assert homes == ["flow_kernels.h"], (kernel, homes)
    assert "atomic" not in text.replace("no atomics", "")


@pytest.mark.parametrize("kernel", cs.FLOW_CORNER_KERNELS)
def test_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)


def test_the_command_line():
    from examples import flow_args
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="flow")
    ap.add_argument("--structure", type=int, default=1)
    flow_args.add_flow_arguments(ap)
    of = lambda *argv: flow_args.flow_of(ap.parse_args(list(argv)), 16, 12)
    assert of("--flow-score").members is None and of("--flow-score", "--flow-members", "all").members is None
    m = of("--flow-score", "--flow-members", "corners").members
    assert (m.max_corners, m.quality_level, m.min_distance, m.block_size) == (100, 0.3, 7.0, 7)
    m = of("--flow-score", "--flow-members", "corners", "--flow-corner-quality", "0.1", "--flow-corner-distance", "4", "--flow-pairing", "prediction").members
    assert (m.quality_level, m.min_distance) == (0.1, 4.0)
    with pytest.raises(ValueError):
        of("--flow-members", "corners")
    with pytest.raises(SystemExit):
        of("--flow-members", "edges")


@pytest.mark.parametrize("shape", cs.SHAPES, ids=cs.shape_id)
@pytest.mark.parametrize("ref_kind", cs.REF_KINDS)
def test_the_corner_cases_satisfy_their_conditions(shape, ref_kind):
    """From the CPU oracle: samples 0 and 1 have at least 4 corners and fewer than max_corners, the constant sample none; with
    max_corners 5 the cap decides; the half mask removes corners of both samples and leaves some; and under every score's settings both
    samples keep at least min_count members among their corners, alone and under the half mask."""
    w, h, C, r = shape
    pred, _, ref64, as_bytes = cs.stage_inputs(w, h, C, ref_kind)
    planes, counts = cs.oracle_members(as_bytes)
    assert (counts[:2] >= 4).all() and (counts[:2] < cs.MAX_CORNERS).all() and counts[2] == 0 and not planes[2].any()
    assert cs.oracle_members(as_bytes, cs.CAPPED)[1].tolist() == [cs.CAPPED, cs.CAPPED, 0]
    halved, _ = cs.oracle_members(as_bytes, mask=cs.half_mask(w, h))
    assert (halved.sum((1, 2)) < planes.sum((1, 2)))[:2].all() and halved[:2].any((1, 2)).all()
    for kind in cs.SCORES:
        sc = cs.score_of(kind, h)
        for p in (planes, halved):
            N = cs.stage_ref(pred, ref64, r, p, sc).record[:, 0]
            assert (N[:2] >= sc.min_count).all() and N[2] == 0 and (N <= p.sum((1, 2))).all(), (kind, N)


def test_quantise_is_the_fed_back_byte():
    v = np.array([-0.5, 0.0, 0.0039, 1.0 / 255.0, 0.5, 254.999 / 255.0, 1.0, 1.5, np.nextafter(np.float32(1.0), np.float32(0.0))], np.float32)
    assert cs.quantise(v).tolist() == [0, 0, 0, 1, 127, 254, 255, 255, 254]


@pytest.mark.parametrize("kind", cs.SCORES)
def test_a_per_sample_mask_is_the_mean_of_single_sample_references(kind):
    """the float64 reference under an [n, H, W] mask: value, records, seed and reference gradient of sample b are those of the
    single-sample reference under mask b, and the value is the mean of the three in sample order"""
    w, h, C, r = cs.SHAPES[0]
    pred, _, ref64, _ = cs.stage_inputs(w, h, C, "bytes")
    masks, sc = cs.random_masks(w, h), cs.score_of(kind, h)
    whole = cs.stage_ref(pred, ref64, r, masks, sc, scale=3.0)
    singles = [cs.stage_ref(pred[b:b + 1], ref64[b:b + 1], r, masks[b], sc, scale=1.0) for b in range(cs.B)]
    for b, s in enumerate(singles):
        assert np.array_equal(s.record[0], whole.record[b]) and np.array_equal(s.u[0], whole.u[b])
        assert np.array_equal(s.seed[0], whole.seed[b]) and np.array_equal(s.grad[0], whole.grad[b])
    assert whole.value == ((singles[0].value + singles[1].value) + singles[2].value) / 3.0
    assert whole.record[0, 0] > 0 and whole.record[0, 0] != whole.record[1, 0]


@pytest.mark.parametrize("cid", sorted(cs.FRAME_SEEDS))
def test_the_listed_frame_seeds_meet_the_member_count(cid):
    """the training cases whose frames take a seed of their own: on the float64 reference, with the CPU oracle's corners, every sample of
    every weighted term has at least min_count members (tests/test_gpu_flow_corner.py asserts it for every case, from the device too)"""
    c = next(c for c in cs.TRAIN_CASES if cs.train_case_id(c) == cid)
    pred = cs.train_reference(c, cs.all_pixels(c), leaf=None).pred.astype(np.float32)
    N = cs.member_counts(c, cs.oracle_planes(c, pred), pred)
    assert sorted(N) == cs.weighted_terms(c) and all((n >= cs.score_of(c.kind, c.h).min_count).all() for n in N.values()), N
