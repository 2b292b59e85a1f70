"""Shared by tests/test_dense_float_host.py and tests/test_gpu_dense_float.py ("Float frames": the dense fitness on
PredNet's float predictions, eigen_dense_score_float, EIGEN_DENSE_FLOAT_FRAMES):
(a) the float stage cases: the UNQUANTISED inputs of tests/flow_score_support.py `stage_inputs` (a float prediction against a byte or a
    float reference) on their small shapes, with the numpy restatements of tests/flow_score_support.py and tests/flow_struct_support.py
    as the reference and max_norm in a gap between two norms;
(b) the sub-byte case: two float images that differ by less than one grey level and quantise to the same bytes, the reason for the feature;
(c) the oracle's float predictions of the end-to-end cases of tests/dense_fitness_support.py, and numpy's statement of tflow_gray;
(d) the names of the new kernels."""
import functools
from collections import namedtuple
from unittest import mock

import numpy as np

from tests import dense_fitness_support as ds
from tests import dense_pyr_support as dp
from tests import flow_obj_support as fs
from tests import flow_score_support as ss
from tests import flow_struct_support as st

FLOAT_KERNELS = ["tdense_gray_of_kernel", "tdense_prep_gray_kernel"]
EPS = ds.EPS
DENSE_FLOAT_FRAMES = 2      # EIGEN_DENSE_FLOAT_FRAMES
B = ss.B_STAGE


def quantise(f):
    """(uint8)(int)(v * 255.0f) of float32 values in [0, 1]: the byte the roll-out emits for a prediction"""
    return (np.asarray(f, np.float32) * np.float32(255.0)).astype(np.int32).astype(np.uint8)


def gray64(img):
    """tflow_gray of a float32 or uint8 image batch [n, C, H, W] -> float64 [n, H, W]"""
    img = np.asarray(img)
    return fs._gray(fs.byte_reference(img) if img.dtype == np.uint8 else img.astype(np.float32).astype(np.float64))


def ref64_of(ref):
    """the reference as the device widens it: (float)byte / 255.0f of bytes, floats as they are"""
    return fs.byte_reference(ref) if ref.dtype == np.uint8 else ref.astype(np.float64)


def gap_norm(pts, q):
    """(the midpoint of the two distinct norms of the live candidates around their q quantile, half the gap between the two): a limit
    no norm sits on, the rule of `dense_fitness_support.struct_case`"""
    live = pts.candidate & (pts.nrm > 0)
    v = np.unique(pts.nrm[live])
    k = max(0, min(int(np.searchsorted(v, np.quantile(pts.nrm[live], q), side="right")) - 1, len(v) - 2))
    return float(0.5 * (v[k] + v[k + 1])), float(0.5 * (v[k + 1] - v[k]))


# ---- (a) the float stage cases: (kind, w, h, C, r, masked, ref_kind, min_count, max_distance).  Radius 3 and 7 of every score, masked and
# not, a byte and a float reference; r = 7 at 24 x 16 has windows wider than a tile, 40 x 24 spans several tiles, rows and blocks.
FloatCase = namedtuple("FloatCase", "kind w h C r masked ref_kind min_count max_distance")
FLOAT_CASES = ([FloatCase("circles", 16, 12, 3, 3, True, rk, 4, 0.0) for rk in ("bytes", "floats")] + [FloatCase("circles", 24, 16, 1, 7, False, "floats", 25, 0.0)]
               + [FloatCase("bands", 16, 10, 3, 3, True, "floats", 1, 0.0), FloatCase("bands", 24, 16, 1, 7, False, "bytes", 1, 0.0)]
               + [FloatCase("free", 16, 12, 1, 3, False, "floats", 1, 5.0), FloatCase("free", 24, 16, 1, 7, False, "bytes", 1, 100.0),
                  FloatCase("free", 40, 24, 3, 7, True, "floats", 1, 10.0)])
float_id = lambda c: "%s-%dx%dx%d-r%d-%s%s" % (c.kind, c.w, c.h, c.C, c.r, c.ref_kind, "-masked" if c.masked else "")
StageCase = namedtuple("StageCase", "pred ref ref64 mask score r want gap")


def probe_of(c):
    if c.kind == "circles":
        return ss.Score(1.0, ss.MIN_NORM, 0.0, c.h / 2.0, ss.WEIGHTS[0], ss.WEIGHTS[1], c.min_count)
    return st.bands_for(c.h, 1.0, c.min_count) if c.kind == "bands" else st.Free(1.0, 1e-3, c.max_distance, c.min_count, st.FREE_W)


@functools.lru_cache(maxsize=None)
def float_case(c):
    """a float stage case: the prediction and the reference as `flow_score_support.stage_inputs` gives them, unquantised"""
    pred, ref, ref64 = ss.stage_inputs(c.w, c.h, c.C, dict(ss.REFS)[c.ref_kind], c.ref_kind)
    mask = (st.bands_mask if c.kind == "bands" else fs.field_mask)(c.w, c.h) if c.masked else None
    probe = probe_of(c)
    max_norm, gap = gap_norm(ds.restate(probe, pred, ref64, c.r, mask).score.points, 0.4 if c.kind == "bands" else 0.5)
    sc = probe._replace(max_norm=max_norm)
    return StageCase(pred, np.ascontiguousarray(ref), ref64, mask, sc, c.r, ds.restate(sc, pred, ref64, c.r, mask), gap)


def dense_of(sc, r, mask=None, members=None, solve=(1, 1), frames="byte"):
    from evolutionary_illusion_generator_amd import fitness
    score = ss.as_flow_score(sc) if isinstance(sc, ss.Score) else st.as_score(sc)
    return fitness.DenseFitness(score, radius=r, eps=EPS, mask=mask, levels=solve[0], iters=solve[1], members=members, frames=frames)


def restate_gray(sc, img0, img1, r, mask, solve=(1, 1)):
    """the restatement of the float stage on img0 (uint8 or float32) and img1 (float32) under a shared mask or member planes"""
    if solve == (1, 1):
        return ds.restate(sc, np.asarray(img1, np.float32), ref64_of(np.asarray(img0)), r, mask)
    with mock.patch.object(dp, "gray_planes", lambda g: g):       # dense_pyr_ref from the gray planes themselves
        return dp.Want(dp.dense_pyr_ref(gray64(img0), gray64(img1), r, EPS, solve[0], solve[1]), sc, mask)


# ---- (b) the sub-byte case
SUB_SHAPES = [(16, 12, 1), (24, 16, 3)]
SUB_RADIUS, SUB_MIN_COUNT = 3, 4
SubCase = namedtuple("SubCase", "b f0 f1 score want_byte want_float gaps")


@functools.lru_cache(maxsize=None)
def sub_byte_case(w, h, C):
    """Bytes b and two float images f0 = (b + 0.25) / 255, f1 = (b + 0.25 + 0.5 g) / 255 with g in [0, 1]: both quantise to b, so the byte
    stage sees two equal images, and the float stage a motion of thousandths of a pixel.  Circles score, radius 3; min_norm and
    max_norm each in a gap between two norms of the float restatement (at its 0.1 quantile and at its median)."""
    s, c, y, x = np.meshgrid(np.arange(B), np.arange(C), np.arange(h), np.arange(w), indexing="ij")
    b = np.clip(np.round(127 + 90 * np.sin(0.9 * x + 0.5 * c + s) * np.cos(0.7 * y - 0.3 * c)), 0, 254)
    g = 0.5 + 0.5 * np.sin(0.4 * x + 0.6 * y)
    f0, f1 = ((b + 0.25) / 255).astype(np.float32), ((b + 0.25 + 0.5 * g) / 255).astype(np.float32)
    b = b.astype(np.uint8)
    probe = ss.Score(1.0, 0.0, 0.0, h / 2.0, ss.WEIGHTS[0], ss.WEIGHTS[1], SUB_MIN_COUNT)
    pts = ds.restate(probe, f1, f0.astype(np.float64), SUB_RADIUS, None).score.points
    (lo, gap_lo), (hi, gap_hi) = gap_norm(pts, 0.1), gap_norm(pts, 0.5)
    sc = probe._replace(min_norm=lo, max_norm=hi)
    fb, fb64 = ds.as_float(b)
    return SubCase(b, f0, f1, sc, ds.restate(sc, fb, fb64, SUB_RADIUS, None), ds.restate(sc, f1, f0.astype(np.float64), SUB_RADIUS, None), (gap_lo, gap_hi))


# ---- (c) the oracle's float predictions of the end-to-end cases
@functools.lru_cache(maxsize=None)
def oracle_float_case(w, h, ch, structure, n_repeat=20):
    """(images uint8 [n, C, H, W], frames uint8 [n, T, C, H, W], P0 float32 [n, T, C, H, W]) of the case's genomes on the ORACLE"""
    import oracle
    from oracle import grids as ogrids, pipeline
    grid = ogrids.create_grid(ds.grid_structure(structure, w, h), w, h, 10)
    images = np.stack([pipeline.render_chw(g, ds.e2e_config(), grid, ch[0], w, h) for g in ds.e2e_genomes()])
    out = [oracle.prednet_rollout(ds.e2e_weights(w, h, ch), list(ch), w, h, im, n_repeat=n_repeat, n_ext=2, return_float=True) for im in images]
    return images, np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def float_pair(images, p0, pairing, n_repeat=20):
    """(img0, img1) of a pairing under float frames: consecutive float predictions, or the input bytes against the second extension's"""
    if pairing == ds.PAIR_POPULATION:
        return p0[:, n_repeat - 1], p0[:, n_repeat]
    return images, p0[:, n_repeat + 1]


def e2e_dense(structure, frames="float", **kw):
    from evolutionary_illusion_generator_amd import fitness
    return fitness.DenseFitness.for_structure(structure, radius=ds.E2E_RADIUS, eps=EPS, frames=frames, **dict(ds.E2E_LIMITS, **kw))


def oracle_planes(images, members):
    """the member planes uint8 [n, H, W] of the CPU oracle's corners of byte images under a ``train.CornerMembers``' own settings"""
    import oracle
    images = np.asarray(images, np.uint8)
    planes = np.zeros((images.shape[0],) + images.shape[2:], np.uint8)
    par = oracle.LKParams(max_corners=members.max_corners, quality_level=members.quality_level, min_distance=members.min_distance, block_size=members.block_size)
    for b, img in enumerate(images):
        for x, y in oracle.good_features(oracle.gray(img), par):
            planes[b, int(y), int(x)] = 1
    return planes
