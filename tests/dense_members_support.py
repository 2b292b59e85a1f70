"""Shared by tests/test_dense_members_host.py and tests/test_gpu_dense_members.py ("Members"): the dense motion
fitness with corner members and per-sample member planes.
(a) the stage cases: the inputs of tests/flow_corner_support.py as pairs of byte images, the settings of its scores;
(b) the cases of the compacted pair pass: shapes against the tile of 256 slots, the planes;
(c) the end-to-end cases: the genomes and weights of tests/dense_fitness_support.py under `CornerMembers(**flow_corner_support.CORNER)`;
(d) the names of the kernels of the new header.
It imports the other support modules and changes none."""
import functools

import numpy as np

from tests import dense_fitness_support as ds
from tests import dense_pyr_support as dp
from tests import flow_corner_support as fc
from tests import flow_struct_support as st

MEMBER_KERNELS = ["tdense_member_list_kernel", "tdense_free_pair_list_kernel"]
EPS = ds.EPS
SOLVES = ((1, 1), (2, 2))
solve_id = lambda s: "%dx%d" % s


# ---- (a) the stage cases
@functools.lru_cache(maxsize=None)
def stage_pair(w, h, C):
    """(img0, img1) uint8 [3, C, h, w]: img0 the byte reference of `flow_corner_support.stage_inputs` (a smooth image, a random one and
    a constant one with no corner), img1 floor(pred 255) of its float prediction"""
    pred, ref, _, _ = fc.stage_inputs(w, h, C, "bytes")
    return np.ascontiguousarray(ref), ds.floor_bytes(pred)


def dense_of(sc, r, mask=None, members=None, solve=(1, 1)):
    from evolutionary_illusion_generator_amd import fitness
    return fitness.DenseFitness(fc.train_score(sc), radius=r, eps=EPS, mask=mask, levels=solve[0], iters=solve[1], members=members)


def restate(sc, img0, img1, r, planes, solve=(1, 1)):
    """the numpy restatement of a dense call on the bytes under member planes [B, H, W]: the single step through
    `dense_fitness_support.restate`, a real solve through `dense_pyr_support.dense_pyr_ref` and the same score"""
    if solve == (1, 1):
        return ds.restate(sc, ds.as_float(img1)[0], ds.as_float(img0)[1], r, planes)
    return dp.Want(dp.dense_pyr_ref(img0, img1, r, EPS, solve[0], solve[1]), sc, planes)


# ---- (b) the compacted pair pass against the all-pixel kernel.  The list is walked in tiles of 256 slots: 192 pixels are less than one
# tile, 594 three tiles with the last partial, 1536 six full ones
PAIR_SHAPES = [(16, 12), (33, 18), (48, 32)]
PAIR_RADIUS = 2
PAIR_PLANES = ("ones", "random", "single")
pair_id = lambda s: "%dx%d" % s


def free_score():
    """Free with a max_norm that excludes nothing: the members are the plane's pixels whose field is not zero"""
    return st.Free(fc.BIG_NORM, 0.0, 10.0, 1, st.FREE_W)


@functools.lru_cache(maxsize=None)
def pair_images(w, h):
    """(img0, img1) uint8 [3, 1, h, w], three different random pairs"""
    rng = np.random.default_rng(7 + 100 * w + h)
    return rng.integers(0, 256, (3, 1, h, w), dtype=np.uint8), rng.integers(0, 256, (3, 1, h, w), dtype=np.uint8)


def pair_plane(kind, w, h):
    """one [h, w] plane: all ones, about two thirds of the pixels, or exactly one pixel"""
    if kind == "ones":
        return np.ones((h, w), np.uint8)
    if kind == "random":
        return np.ascontiguousarray(fc.random_masks(w, h)[0])
    m = np.zeros((h, w), np.uint8)
    m[h // 2, w // 3] = 1
    return m


def batch_planes(w, h):
    """three different planes with an all-zero one in the middle"""
    m = fc.random_masks(w, h).copy()
    m[1] = 0
    return m


# ---- (c) end to end
E2E_LIMITS = dict(max_norm=0.3, min_norm=1e-3, min_count=4)
E2E_CASES = [(ds.E2E_SHAPES[1], 1), (ds.E2E_SHAPES[1], 2), (ds.BANDS_SHAPE, 0)]
E2E = [(shape, s, p) for shape, s in E2E_CASES for p in (ds.PAIR_POPULATION, ds.PAIR_SINGLE)]
e2e_id = lambda c: "%dx%d-s%d-%s" % (c[0][0], c[0][1], c[1], "population" if c[2] == ds.PAIR_POPULATION else "single")
DEAD = ((48, 32), 2, ds.PAIR_SINGLE)     # the one case with a sample below min_count (tests/test_dense_members_host.py)
SMALL = ds.E2E_SHAPES[0]                 # 16 x 12: 1 .. 9 corners a sample, used for "below min_count scores 0" alone


def e2e_members():
    from evolutionary_illusion_generator_amd import train
    return train.CornerMembers(**fc.CORNER)


def e2e_dense(structure, **limits):
    from evolutionary_illusion_generator_amd import fitness
    return fitness.DenseFitness.for_structure(structure, radius=ds.E2E_RADIUS, eps=EPS, members=e2e_members(), **dict(E2E_LIMITS, **limits))


def e2e_planes(img0):
    """the member planes and corner counts of the CPU oracle on the first images of the pairs, under `e2e_members`' max_corners"""
    return fc.oracle_members(img0, max_corners=e2e_members().max_corners)


def e2e_restate(structure, img0, img1, planes, **limits):
    sc = dp.restatement_score(e2e_dense(structure, **limits), img0.shape[2])
    return sc, ds.restate(sc, ds.as_float(img1)[0], ds.as_float(img0)[1], ds.E2E_RADIUS, planes)
