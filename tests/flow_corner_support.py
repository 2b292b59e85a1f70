"""Shared by tests/test_flow_corner_host.py and tests/test_gpu_flow_corner.py ("The corner members"):
(a) the membership reference: the quantisation of a float reference in numpy and the corners of the CPU oracle as member planes;
(b) the float64 references of tests/flow_score_support.py and tests/flow_struct_support.py under a per-sample mask.  They need no new
    mathematics: their `mask` is broadcast against [B, H, W], and a score term is the mean over the samples of per-sample values;
(c) the cases: shapes, settings and inputs, with the conditions tests/test_flow_corner_host.py asserts on the CPU;
(d) the names of the kernels of the new header.
It imports the other support modules and changes none."""
import functools
from collections import namedtuple

import numpy as np

from tests import flow_obj_support as fs
from tests import flow_pair_support as ps
from tests import flow_score_support as ss
from tests import flow_struct_support as st

FLOW_CORNER_KERNELS = ["tcorner_quant_kernel", "tcorner_member_kernel"]
# (w, h, C, radius): 40 x 24 is ragged against both the solve's tile and mineig_kernel's 16 x 16 tile, two tiles each way at least;
# 48 x 32 = 1536 pixels is more than corner_select_kernel's 1024 threads, so its strided loops run more than once
SHAPES = [(24, 16, 1, 2), (40, 24, 3, 3), (48, 32, 3, 2)]
B = 3
CORNER = dict(quality_level=0.05, min_distance=3.0, block_size=3)
MAX_CORNERS = 128
CAPPED = 5          # the max_corners of the case in which the cap decides
SCORES = ("circles", "bands", "free")
REF_KINDS = ("bytes", "floats")
shape_id = lambda s: "%dx%dx%d-r%d" % s


# ---- (a) membership
def quantise(ref):
    """float32 -> the bytes the membership stage forms: clamped to [0, 1], then (uint8_t)(int)(v * 255.0f), each a float operation"""
    v = np.clip(np.asarray(ref, np.float32), np.float32(0), np.float32(1))
    return (v * np.float32(255.0)).astype(np.int32).astype(np.uint8)


def corner_members(max_corners=MAX_CORNERS):
    from evolutionary_illusion_generator_amd import train
    return train.CornerMembers(max_corners=max_corners, **CORNER)


def oracle_members(images, max_corners=MAX_CORNERS, mask=None):
    """images uint8 [n, C, H, W] -> (member planes uint8 [n, H, W], corner counts int32 [n]) by the CPU oracle: the corners
    ``good_features(gray(img))`` picks, as a plane, less those a shared mask [H, W] does not count; the counts are before the mask"""
    import oracle
    images = np.asarray(images, np.uint8)
    n, _, H, W = images.shape
    planes, counts = np.zeros((n, H, W), np.uint8), np.zeros(n, np.int32)
    for b in range(n):
        pts = oracle.good_features(oracle.gray(images[b]), oracle.LKParams(max_corners=max_corners, **CORNER))
        counts[b] = len(pts)
        for x, y in pts:
            assert x == int(x) and y == int(y)
            planes[b, int(y), int(x)] = 1
        assert planes[b].sum() == len(pts), "the corners of one sample are distinct pixels"
    if mask is not None:
        planes &= (np.asarray(mask) != 0).astype(np.uint8)[None]
    return planes, counts


def half_mask(w, h):
    """a shared mask that excludes the left half of the image"""
    m = np.ones((h, w), np.uint8)
    m[:, :w // 2] = 0
    return m


# ---- (c) the cases
@functools.lru_cache(maxsize=None)
def stage_inputs(w, h, C, ref_kind):
    """-> (pred float32 [3, C, h, w], the reference as given to the trainer, the reference widened to float64, the reference as the
    bytes the membership stage sees).  Sample 0 is the "smooth" and sample 1 the "random" image of tests/flow_score_support.py's
    generators (their seeds are functions of the shape), sample 2 a constant image: no corner."""
    pred = fs.field_inputs(w, h, C, "random", B)[0]
    if ref_kind == "bytes":
        ref = np.stack([fs.field_inputs(w, h, C, "smooth")[1][0], fs.field_inputs(w, h, C, "random")[1][0], np.full((C, h, w), 77, np.uint8)])
        return pred, ref, fs.byte_reference(ref), ref
    ref = np.stack([ps.pair_field_inputs(w, h, C, "smooth")[1][0], ps.pair_field_inputs(w, h, C, "random")[1][0], np.full((C, h, w), 0.3, np.float32)])
    return pred, ref, ref.astype(np.float64), quantise(ref)


def random_masks(w, h, seed=5):
    """three different random [h, w] masks as one [3, h, w] mask, about two thirds of the pixels counted"""
    rng = np.random.default_rng(seed + 100 * w + h)
    return (rng.random((B, h, w)) < 0.66).astype(np.uint8)


BIG_NORM = 1e6     # a max_norm that excludes nothing


def score_of(kind, h):
    """the test settings of a score: min_count 2 (FlowScore) or 1, min_norm 0, max_norm BIG_NORM -> membership is mask and geometry"""
    if kind == "circles":
        return ss.Score(BIG_NORM, 0.0, 0.0, h / 2.0, ss.WEIGHTS[0], ss.WEIGHTS[1], 2)
    if kind == "bands":
        return st.Bands(BIG_NORM, 0.0, 0.0, (h / 4.0) * 2.0, 1)
    return st.Free(BIG_NORM, 0.0, 10.0, 1, st.FREE_W)


def train_score(sc):
    """the train.FlowScore / BandsScore / FreeScore of a score tuple"""
    return ss.as_flow_score(sc) if isinstance(sc, ss.Score) else st.as_score(sc)


def flow_of(sc, radius, mask=None, pairing="frame", reference="constant", members=None):
    from evolutionary_illusion_generator_amd import train
    return train.make_flow(pairing, radius, 1e-2, None, mask, reference=reference, score=train_score(sc), members=members)


StageRef = namedtuple("StageRef", "value u seed grad record")


def stage_ref(pred, ref64, r, mask, sc, scale=1.0, record=None):
    """the float64 reference of the stage under a score tuple; mask None, [H, W] or [B, H, W]"""
    if isinstance(sc, ss.Score):
        s = ss.score_stage_ref(pred, ref64, r, 1e-2, mask, sc, scale=scale, record=record)
        return StageRef(s.value, s.u, s.seed, s.grad, s.score.record)
    s = st.struct_stage_ref(pred, ref64, r, 1e-2, mask, sc, scale=scale, record=record)
    return StageRef(s.value, s.u, s.seed, s.grad, s.score.record)


# ---- training calls against float64 autograd.  The member planes are constants of the reference: those `flow_members` gives on the
# frames (frame pairing) or on the float32 predictions the call itself returned (prediction pairing: the image the device quantised).
# pairing: "constant" and "moving" are the frame pairing with the frame a constant or in the graph, "prediction" the prediction
# pairing.  form: "still_requant" (a still repeated 6 times, 2 self-fed steps through the byte) and "drifting" (T = 5, teacher-forced).
# Under the prediction pairing term 0 of a reset call has the zero image as its reference and no corner, so "drifting" weighs
# [0, 1, 1, 1] there.  Dense live weights (tests/state_support.py), B = 3.
TrainCase = namedtuple("TrainCase", "w h ch r kind pairing form")
TRAIN_CHANNELS = {(24, 16): (1, 4, 8), (40, 24): (3, 4), (48, 32): (3, 4)}
TRAIN_PAIRINGS = ("constant", "moving", "prediction")
TRAIN_FORMS = ("still_requant", "drifting")
TRAIN_CASES = ([TrainCase(w, h, TRAIN_CHANNELS[w, h], r, "circles", p, f) for w, h, _, r in SHAPES for p in TRAIN_PAIRINGS for f in TRAIN_FORMS]
               + [TrainCase(24, 16, TRAIN_CHANNELS[24, 16], 2, kind, p, f) for kind in ("bands", "free") for p in TRAIN_PAIRINGS for f in TRAIN_FORMS])
# the seed of a case's frames (tests/train_support.py `_drifting`): FRAME_SEED unless the case is listed, with the condition it missed;
# the conditions are tests/test_flow_corner_host.py `test_the_training_cases_satisfy_their_conditions`
FRAME_SEED = 1
# at 24 x 16 the ring of FlowScore holds few corners of a drifting sequence: with seed 1 (and 2) a sample of a weighted term keeps one member
# under the frame pairing, and with seeds 1 .. 9 under the prediction pairing (min_count is 2)
FRAME_SEEDS = {"24x16-1_4_8-r2-circles-constant-drifting": 3, "24x16-1_4_8-r2-circles-moving-drifting": 3, "24x16-1_4_8-r2-circles-prediction-drifting": 10}


def train_case_id(c):
    return "%dx%d-%s-r%d-%s-%s-%s" % (c.w, c.h, "_".join(map(str, c.ch)), c.r, c.kind, c.pairing, c.form)


@functools.lru_cache(maxsize=None)
def train_case_frames(c):
    from tests.train_support import _drifting
    T = 5 if c.form == "drifting" else 6
    frames = _drifting(FRAME_SEEDS.get(train_case_id(c), FRAME_SEED), B, T, c.ch[0], c.h, c.w)
    if c.form != "drifting":
        frames = np.ascontiguousarray(np.broadcast_to(frames[:, :1], frames.shape))
    return frames


def train_case_weights(c):
    from tests.state_support import dense_weights
    return dense_weights(list(c.ch), c.w, c.h)


def train_case_call(c):
    """the keywords the trainer and run_flow share"""
    if c.form == "drifting":
        return dict(n_fed=None, requant=False, step_weights=[0.0, 1.0, 1.0, 1.0] if c.pairing == "prediction" else None)
    return dict(n_fed=4, requant=True, step_weights=list(ps.POPULATION_WEIGHTS) if c.pairing == "prediction" else list(fs.STILL_WEIGHTS))


def train_case_flow(c, members=True):
    """the objective of a case; members False: the same objective on every pixel"""
    sc = score_of(c.kind, c.h)
    pairing, reference = ("prediction", "constant") if c.pairing == "prediction" else ("frame", c.pairing)
    return flow_of(sc, c.r, pairing=pairing, reference=reference, members=corner_members() if members else None)


def weighted_terms(c):
    T = train_case_frames(c).shape[1]
    w = train_case_call(c)["step_weights"]
    return [s for s in range(T - 1) if w is None or w[s] != 0]


def member_sources(c, pred):
    """{s: the image the members of weighted term s come from}: frame s + 1 (uint8), or P0_{s-1} of pred (float32) under the prediction pairing"""
    frames = train_case_frames(c)
    if c.pairing == "prediction":
        return {s: np.ascontiguousarray(pred[:, s - 1], dtype=np.float32) for s in weighted_terms(c)}
    return {s: np.ascontiguousarray(frames[:, s + 1]) for s in weighted_terms(c)}


class MemberTerm:
    """`run_flow`'s term with the member planes of every term given: planes {s: [B, H, W] or None (every pixel)}; a term that is not
    listed has weight zero and is not formed"""

    def __init__(self, c, planes, start):
        import torch
        self.c, self.planes, self.s, self.prev, self.torch = c, planes, 0, start.detach(), torch
        self.sc = score_of(c.kind, c.h)

    def __call__(self, P, xn):
        torch = self.torch
        s, prev = self.s, self.prev
        self.s, self.prev = s + 1, P
        if s not in self.planes:
            return P.sum() * 0.0, 0.0
        ref = prev if self.c.pairing == "prediction" else xn if self.c.pairing == "moving" else xn.detach()
        term = ss.torch_score_term if self.c.kind == "circles" else st.torch_struct_term
        f, scale, _ = term(P.to(torch.float64), ref.to(torch.float64), self.c.r, 1e-2, self.planes[s], self.sc)
        return f, scale


def train_reference(c, planes, pred=None, dtype=None, leaf="frames"):
    """`run_flow` of a case under `MemberTerm`.  pred: the float32 predictions whose bytes a requantised case is fed (the GPU's own);
    None: the run is repeated on its own requantised predictions."""
    import torch
    from tests.train_support import _fed_from
    dtype = dtype or torch.float64
    wts, frames, call = train_case_weights(c), train_case_frames(c), train_case_call(c)
    n, T, C, H, W = frames.shape

    def run(fed):
        return fs.run_flow(wts, list(c.ch), frames, term=MemberTerm(c, planes, torch.zeros(n, C, H, W, dtype=dtype)), leaf=leaf, dtype=dtype, fed=fed, **call)

    if not call["requant"]:
        return run(None)
    if pred is not None:
        return run(_fed_from(pred))
    fed = np.zeros(frames.shape, np.float32)
    for _ in range(T - call["n_fed"] + 1):
        out = run(fed)
        fed = _fed_from(out.pred.astype(np.float32))
    return out


def all_pixels(c):
    """the planes under which the reference counts every pixel"""
    return {s: None for s in weighted_terms(c)}


def oracle_planes(c, pred):
    """the member planes of a case from the CPU oracle, on the images `member_sources` names"""
    return {s: oracle_members(img if img.dtype == np.uint8 else quantise(img))[0] for s, img in member_sources(c, pred).items()}


def member_counts(c, planes, pred):
    """N of every (weighted term, sample) on the float64 reference: the score's own members among the planes, {s: [B]}"""
    from tests.train_support import _fed_from  # noqa: F401
    frames = train_case_frames(c)
    sc = score_of(c.kind, c.h)
    out = {}
    for s in weighted_terms(c):
        ref64 = pred[:, s - 1].astype(np.float64) if c.pairing == "prediction" else fs.byte_reference(frames[:, s + 1])
        out[s] = stage_ref(pred[:, s].astype(np.float32), ref64, c.r, planes[s], sc).record[:, 0]
    return out
