"""Shared by tests/test_dense_fitness_host.py and tests/test_gpu_dense_fitness.py (the dense motion fitness):
(a) the stage cases of tests/flow_score_support.py and tests/flow_struct_support.py as pairs of BYTE images, with the numpy restatements of
    those two files as the reference (`score_stage_ref`, `struct_stage_ref`; neither file is edited);
(b) the end-to-end cases: shapes, genomes, weights, the DenseFitness of every structure, and the oracle's frames of a case;
(c) the names of the new kernels.
The stage has no reference of its own: eigen_dense_score on bytes b0, b1 is eigen_trainer_flow_term_pair's stage on the float images
(float)byte / 255.0f, so the restatement is given pred = b1.astype(float32) / float32(255) and ref64 = the same of b0, widened."""
import functools
from collections import namedtuple

import numpy as np

from tests import flow_obj_support as fs
from tests import flow_score_support as ss
from tests import flow_struct_support as st

DENSE_KERNELS = ["tdense_prep_kernel", "tdense_solve_kernel", "tdense_free_pair_kernel"]
EPS = 1e-2


# ---- (a) the stage cases as bytes
def floor_bytes(v):
    """floor(v 255) of a float field in [0, 1], as uint8"""
    return np.clip(np.floor(np.asarray(v, np.float64) * 255.0), 0, 255).astype(np.uint8)


def as_float(b):
    """(the float32 image (float)byte / 255.0f, that widened to float64): what the device forms of a byte"""
    f = np.asarray(b, np.uint8).astype(np.float32) / np.float32(255.0)
    return f, f.astype(np.float64)


def byte_pair(w, h, C, ref_kind):
    """(img0, img1) uint8 [B, C, h, w] of a stage case: img1 is floor(pred 255) of the support's float prediction, img0 its byte reference
    as it is or floor(prev 255) of its float reference"""
    pred, ref, _ = ss.stage_inputs(w, h, C, dict(ss.REFS)[ref_kind], ref_kind)
    return (np.ascontiguousarray(ref) if ref_kind == "bytes" else floor_bytes(ref)), floor_bytes(pred)


CIRCLES_CASES = [(w, h, C, r, masked, ref_kind, mc) for w, h, C, r, masked in ss.STAGE_CASES for ref_kind, _ in ss.REFS for mc in ss.MIN_COUNTS]
circles_id = lambda c: "circles-%dx%dx%d-r%d-%s-min%d" % (c[0], c[1], c[2], c[3], c[5], c[6])
# every Bands and Free stage case; "empty" (Free, 16 x 12): sample 1's two images are the same bytes, so its field is exactly zero and it has
# no member at all
STRUCT_CASES = list(st.STAGE_CASES)
StageCase = namedtuple("StageCase", "img0 img1 pred ref64 mask score r want")


@functools.lru_cache(maxsize=None)
def circles_case(w, h, C, r, masked, ref_kind, min_count):
    """a Circles stage case on bytes: max_norm the median norm of the restatement's own field on these bytes, as `flow_score_support.stage_case`"""
    img0, img1 = byte_pair(w, h, C, ref_kind)
    (pred, _), (_, ref64) = as_float(img1), as_float(img0)
    mask = fs.field_mask(w, h) if masked else None
    probe = ss.Score(1.0, ss.MIN_NORM, 0.0, h / 2.0, ss.WEIGHTS[0], ss.WEIGHTS[1], min_count)
    field = ss.score_stage_ref(pred, ref64, r, EPS, mask, probe)
    sc = probe._replace(max_norm=float(np.median(field.score.points.nrm)))
    return StageCase(img0, img1, pred, ref64, mask, sc, r, ss.score_stage_ref(pred, ref64, r, EPS, mask, sc))


@functools.lru_cache(maxsize=None)
def struct_case(c):
    """a Bands or Free stage case on bytes: max_norm between two distinct norms of the candidates, as `flow_struct_support.stage_case`"""
    img0, img1 = byte_pair(c.w, c.h, c.C, c.ref_kind)
    if c.empty:
        img0 = img0.copy()
        img0[1] = img1[1]
    (pred, _), (_, ref64) = as_float(img1), as_float(img0)
    mask = (st.bands_mask if c.kind == "bands" else fs.field_mask)(c.w, c.h) if c.masked else None
    probe = st.bands_for(c.h, 1.0, c.min_count) if c.kind == "bands" else st.Free(1.0, 1e-3, c.max_distance, c.min_count, st.FREE_W)
    pts = st.struct_stage_ref(pred, ref64, c.r, EPS, mask, probe).score.points
    live = pts.candidate & (pts.nrm > 0)
    v = np.unique(pts.nrm[live])
    k = min(int(np.searchsorted(v, np.quantile(pts.nrm[live], 0.4 if c.kind == "bands" else 0.5), side="right")) - 1, len(v) - 2)
    sc = probe._replace(max_norm=float(0.5 * (v[k] + v[k + 1])))
    return StageCase(img0, img1, pred, ref64, mask, sc, c.r, st.struct_stage_ref(pred, ref64, c.r, EPS, mask, sc))


def dense_of(sc, r, mask=None):
    """the fitness.DenseFitness of a Score, a Bands or a Free"""
    from evolutionary_illusion_generator_amd import fitness
    return fitness.DenseFitness(ss.as_flow_score(sc) if isinstance(sc, ss.Score) else st.as_score(sc), radius=r, eps=EPS, mask=mask)


def restate(sc, pred, ref64, r, mask, record=None):
    return (ss.score_stage_ref if isinstance(sc, ss.Score) else st.struct_stage_ref)(pred, ref64, r, EPS, mask, sc, record=record)


# ---- (b) end to end
# 16 x 12 with radius 7: the window is wider than the image is high, every window is truncated; 48 x 32, four layers: interior windows
E2E_SHAPES = [(16, 12, (3, 4, 6)), (48, 32, (3, 4, 6, 8))]
E2E_GENOMES, E2E_RADIUS = 7, 7
E2E_STRUCTURES = (0, 1, 2)
# Bands on its OWN grid: at the two shapes above the Bands grid is constant (see `grid_structure`); at 60 x 48 a band is 12 rows high, two
# more than the gap, and a tile 6 columns wide, so the planes vary and the renders differ from genome to genome
BANDS_SHAPE = (60, 48, (3, 4, 6))
E2E_CASES = [(shape, s) for shape in E2E_SHAPES for s in E2E_STRUCTURES] + [(BANDS_SHAPE, 0)]
PAIR_POPULATION, PAIR_SINGLE = 0, 1
# The settings of the end-to-end scores, one set for the three structures: max_norm 0.3 pixels (the fitness's own Circles limit) lies near
# the median norm of the fields these weights give under either pairing (0.15 .. 0.4 on the oracle's frames), so the norm limit decides
# membership for about half of the pixels; min_norm is the classes' floor; min_count 8 is far below the 192 pixels of the small shape.
# tests/test_dense_fitness_host.py asserts on the oracle's frames that at least half of the samples of every case are live and that no norm
# sits on a limit.
E2E_LIMITS = dict(max_norm=0.3, min_norm=1e-3, min_count=8)


def e2e_config():
    from evolutionary_illusion_generator_amd import synth
    return synth.make_config(2, 3)


@functools.lru_cache(maxsize=None)
def e2e_genomes():
    from evolutionary_illusion_generator_amd import synth
    return [g for _, g in synth.make_population(E2E_GENOMES, e2e_config(), seed=41)]


@functools.lru_cache(maxsize=None)
def e2e_weights(w, h, ch):
    """the "live" set of tests/train_support.py: random convolutions, the prediction starts inside [0, 1]"""
    from tests.train_support import _live_weights
    return _live_weights(list(ch), w, h)


def e2e_dense(structure):
    from evolutionary_illusion_generator_amd import fitness
    return fitness.DenseFitness.for_structure(structure, radius=E2E_RADIUS, eps=EPS, **E2E_LIMITS)


def e2e_restatement_score(structure, h):
    """the Score / Bands / Free of `e2e_dense` for the numpy restatement"""
    d = e2e_dense(structure).score
    if structure in (1, 3):
        return ss.Score(d.max_norm, d.min_norm, 0.0, h / 2.0, d.weights[0], d.weights[1], d.min_count)
    if structure == 0:
        return st.Bands(d.max_norm, d.min_norm, 0.0, (h / 4.0) * 2.0, d.min_count)
    return st.Free(d.max_norm, d.min_norm, d.max_distance, d.min_count, d.weights)


def frame_pair(images, frames, pairing, n_repeat):
    """(img0, img1) of a pairing from the input images [n, C, H, W] and all the frames of a roll-out [n, T, C, H, W]"""
    if pairing == PAIR_POPULATION:
        return frames[:, n_repeat - 1], frames[:, n_repeat]
    return images, frames[:, n_repeat + 1]


def grid_structure(structure, w, h):
    """The structure whose grid the LIVE check of a case renders on: its own, except for Bands at a shape where its grid is constant.  The
    Bands grid is four bands of ramps with a gap of 10 rows: where a band is no higher than the gap (H / 4 <= 10: 16 x 12, 48 x 32) `x_mat`
    and `y_mat` hold one value each, every genome renders one flat image and the pair is dead.  There the live check scores Bands on renders
    of the Circles grid (the grid and the score are separate arguments of the engine); `fitness.evaluate_population`, which derives the
    grid from the structure, still runs under Bands at those shapes for the comparison that needs no liveness, max_batch 3 against 7."""
    return 1 if structure == 0 and h // 4 <= 10 else structure


@functools.lru_cache(maxsize=None)
def oracle_case(w, h, ch, structure, n_repeat=20):
    """(images, frames) of the case's genomes on the ORACLE: its render on its own grid and its roll-out"""
    import oracle
    from oracle import grids as ogrids, pipeline
    grid = ogrids.create_grid(grid_structure(structure, w, h), w, h, 10)
    images = np.stack([pipeline.render_chw(g, e2e_config(), grid, ch[0], w, h) for g in e2e_genomes()])
    frames = np.stack([oracle.prednet_rollout(e2e_weights(w, h, ch), list(ch), w, h, im, n_repeat=n_repeat, n_ext=2) for im in images])
    return images, frames
