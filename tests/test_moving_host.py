"""Moving CPPN textures without a GPU ("Moving textures"): the ABI surface, the argument rules, ``describe`` and
its closed-form affines, the new kernel's register metadata, the liveness of the shared cases on the numpy restatement alone, and how
far the reference dense solve is from the true flow of the exact quarter-pixel shift."""
import os
import re

import numpy as np
import pytest

from tests import moving_support as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface():
    from evolutionary_illusion_generator_amd import engine
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    assert re.search(r"^int eigen_render_moving_cppn\(eigen_engine\* e, const eigen_genome_batch\* h_genomes, int32_t n, int32_t n_frames, int32_t n_layers,",
                     header, re.M)
    assert engine.EXPORTS.count("eigen_render_moving_cppn") == 1
    assert re.search(r"#define EIGEN_ABI_VERSION 4\b", header) and engine.ABI_VERSION == 4
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libeigen_hip.so not built")
    lib = engine.load_library()
    assert lib.eigen_render_moving_cppn is not None and lib.eigen_abi_version() == 4


def test_moving_textures_argument_rules():
    from evolutionary_illusion_generator_amd.train import MovingTextures, check_moving_textures
    ok = dict(w=16, h=12, c_dim=1, seq=3)
    got = check_moving_textures(**ok)
    assert got[:6] == (16, 12, 1, 3, 0, 1) and got[9] == 3.0 / 16 and got[10] == 20
    bad = [dict(w=0), dict(h=-1), dict(w=16.0), dict(w=True), dict(c_dim=2), dict(c_dim=True), dict(seq=0), dict(seed=-1), dict(seed=0.5), dict(layers=0),
           dict(layers=3), dict(layers=True), dict(max_shift=-0.1), dict(max_shift=np.inf), dict(max_shift="1"), dict(max_turn=-1e-3), dict(max_turn=np.nan),
           dict(max_zoom=1.0), dict(max_zoom=-0.1), dict(texture_scale=0.0), dict(texture_scale=np.inf), dict(texture_scale=False), dict(num_hidden=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            check_moving_textures(**dict(ok, **kw))
        with pytest.raises(ValueError):
            MovingTextures(**dict(ok, **kw))       # the object says it in the same words, before anything touches a device
    src = MovingTextures(**ok)
    for k, n in ((-1, 2), (0, 0), (0.0, 2), (0, True)):
        with pytest.raises(ValueError):
            src.describe(k, n)

    class Other:
        width, height, c_dim = 16, 12, 3
    with pytest.raises(ValueError, match="engine renders"):
        MovingTextures(engine=Other(), **ok)


def test_engine_affine_rules():
    from evolutionary_illusion_generator_amd.engine import check_moving_affines
    a = np.zeros((2, 3, 2, 6))
    assert check_moving_affines(a, None, 4, False)[1] is None
    assert check_moving_affines(a, a + 1, 4, True)[1].shape == a.shape
    for args in ((a[0], None, 4, False), (np.zeros((2, 3, 3, 6)), None, 6, False), (np.zeros((2, 3, 2, 5)), None, 4, False), (np.zeros((0, 3, 1, 6)), None, 0, False),
                 (a, None, 3, False), (a, None, 4, True), (a[:, :1], a[:, :1], 4, True), (a, a[:, :2], 4, True)):
        with pytest.raises(ValueError):
            check_moving_affines(*args)


def _apply(a, z):
    return np.stack([(a[0] * z[:, 0] + a[1] * z[:, 1]) + a[2], (a[3] * z[:, 0] + a[4] * z[:, 1]) + a[5]], 1)


def _corners(w, h):
    x, y = (w - 1) / 2.0, (h - 1) / 2.0
    return np.array([[-x, -y], [x, -y], [-x, y], [x, y]])


def test_describe_is_deterministic_and_differs_between_batches_and_seeds():
    from evolutionary_illusion_generator_amd.train import MovingTextures
    mk = lambda seed: MovingTextures(32, 24, 3, 5, seed=seed, layers=2)
    a, b, other_k, other_seed = mk(7).describe(3, 4), mk(7).describe(3, 4), mk(7).describe(4, 4), mk(8).describe(3, 4)
    assert a["gb"].to_bytes() == b["gb"].to_bytes() and np.array_equal(a["affine"], b["affine"]) and np.array_equal(a["affine_inv"], b["affine_inv"])
    for other in (other_k, other_seed):
        assert a["gb"].to_bytes() != other["gb"].to_bytes() and not np.array_equal(a["affine"], other["affine"])
    assert a["affine"].shape == a["affine_inv"].shape == (4, 5, 2, 6) and a["affine"].dtype == np.float64
    assert a["gb"].n_genomes == 8 and a["gb"].c_out == 3 and len(a["genomes"]) == 8
    # a batch is a prefix of a larger one of the same index: sample b does not depend on n
    small = mk(7).describe(3, 2)
    assert np.array_equal(small["affine"], a["affine"][:2]) and small["gb"].to_bytes() == a["gb"].slice(0, 4).to_bytes()


@pytest.mark.parametrize("layers", [1, 2])
def test_closed_form_affines_invert_and_move_by_the_drawn_similarity(layers):
    from evolutionary_illusion_generator_amd.train import MovingTextures
    w, h, T = 32, 24, 6
    src = MovingTextures(w, h, 1, T, seed=5, layers=layers)
    d = src.describe(11, 5)
    z = _corners(w, h)
    for b in range(5):
        for l in range(layers):
            dx, dy, turn, zoom = d["motion"][b, l]
            assert np.hypot(dx, dy) <= src.max_shift and abs(turn) <= src.max_turn and abs(zoom - 1) <= src.max_zoom
            zc = z[:, 0] + 1j * z[:, 1]
            moved = zoom * np.exp(1j * turn) * zc + complex(dx, dy)
            for t in range(T):
                assert np.abs(_apply(d["affine_inv"][b, t, l], _apply(d["affine"][b, t, l], z)) - z).max() < 1e-12
                if t + 1 < T:
                    q = _apply(d["affine_inv"][b, t + 1, l], _apply(d["affine"][b, t, l], z))
                    assert np.abs(q[:, 0] + 1j * q[:, 1] - moved).max() < 1e-12
    if layers == 2:   # the disc of frame 0 covers part of the image: its centre is inside, its radius below the shorter side's half
        for b in range(5):
            centre = _apply(d["affine_inv"][b, 0, 1], np.zeros((1, 2)))[0]
            radius = 1.0 / np.hypot(d["affine"][b, 0, 1, 0], d["affine"][b, 0, 1, 1])
            assert abs(centre[0]) <= 0.25 * w and abs(centre[1]) <= 0.25 * h and 0.2 * h <= radius <= 0.35 * h


def test_the_exact_shift_case_is_exact():
    """every coordinate of the binary shift sample is a multiple of 2^-7: no rounding anywhere, the true flow is the shift itself"""
    name, b = ms.SHIFT_SAMPLE
    c, r = ms.case(name), ms.reference(name)
    assert np.array_equal(r["u"][b] * 128, np.round(r["u"][b] * 128)) and np.array_equal(r["v"][b] * 128, np.round(r["v"][b] * 128))
    assert (r["flow"][b, :, 0] == ms.SHIFT[0]).all() and (r["flow"][b, :, 1] == ms.SHIFT[1]).all()
    assert np.array_equal(c["motion"][b, 0], [ms.SHIFT[0], ms.SHIFT[1], 0.0, 1.0])


def test_new_kernel_has_no_scratch_and_no_spills():
    from tests import test_isa_stats as isa
    from tests.train_support import _kernel_stats
    if not os.path.exists(isa.LIB):
        pytest.skip("libeigen_hip.so not built")
    if not os.path.exists(isa.READELF):
        pytest.skip("llvm-readelf not found")
    stats = _kernel_stats()
    names = [n for n in stats if re.match(r"_ZN3eig\d+cppn_motion_kernel", n)]
    assert names, "cppn_motion_kernel not in the library"
    for n in names:
        for s in stats[n]:
            assert s["private_segment_fixed_size"] == 0, (n, s)
            assert s["vgpr_spill_count"] == 0, (n, s)
            assert s["sgpr_spill_count"] == 0, (n, s)


@pytest.mark.parametrize("name", ms.CASES)
def test_cases_are_live_on_the_restatement(name):
    c, r = ms.case(name), ms.reference(name)
    f, lay = r["frames"], r["layer"]
    assert f.shape == (c["n"], c["T"], c["c_dim"], c["h"], c["w"]) and r["flow"].shape == (c["n"], c["T"] - 1, 2, c["h"], c["w"])
    for b in range(c["n"]):
        for t in range(c["T"]):
            assert len(np.unique(f[b, t])) >= 16, (name, b, t)
            if t + 1 < c["T"]:
                differ = (f[b, t] != f[b, t + 1]).mean()
                if (name, b) == ms.IDENTITY_SAMPLE:
                    assert differ == 0.0 and np.abs(r["flow"][b, t]).max() < 1e-12     # (the inverse is rounded: not exactly zero)
                else:
                    assert differ >= 0.25, (name, b, t, differ)
            if c["L"] == 2:
                cover = lay[b, t].mean()
                if (name, b) == ms.EXIT_SAMPLE and t == c["T"] - 1:
                    assert cover == 0.0
                else:
                    assert 0.05 <= cover <= 0.60, (name, b, t, cover)
            else:
                assert not lay[b, t].any()
    if c["L"] == 2:
        assert np.abs(r["r2"] - 1.0).min() > 1e-9           # the disc's edge cannot hinge on a rounding
    if name == ms.EXIT_SAMPLE[0]:
        b = ms.EXIT_SAMPLE[1]
        for t in range(c["T"] - 1):                         # cut by the right border before it leaves
            assert lay[b, t, :, -1].any() and not lay[b, t, :, 0].any()


def test_case_shapes_reach_what_they_are_for():
    assert ms.case("8x8")["w"] * ms.case("8x8")["h"] < ms.RENDER_THREADS
    c = ms.case("16x12")
    assert ms.RENDER_THREADS < c["w"] * c["h"] < 2 * ms.RENDER_THREADS and len(set(np.diff(c["gb"].node_off))) == 3
    assert ms.motion_lds(ms.case("44x36")) > 64 * 1024 > ms.motion_lds(ms.case("20x15"))
    assert ms.motion_lds(ms.case("44x36")) <= 160 * 1024


# mean endpoint error of the reference dense solve over that of the zero field, on the two frame pairs of the exact (0.25, -0.125) shift
# at 16 x 12 (radius 3, eps 1e-4, pixels at least 3 from the border), as this test prints it: the shape of the case was enough
MEASURED_FLOW_RATIO = 0.202


def test_reference_dense_solve_recovers_the_quarter_pixel_shift():
    from tests import flow_obj_support as fo
    name, b = ms.SHIFT_SAMPLE
    c, r = ms.case(name), ms.reference(name)
    radius, eps, w, h = 3, 1e-4, c["w"], c["h"]
    inner = (slice(None), slice(radius, h - radius), slice(radius, w - radius))
    err, zero = [], []
    for t in range(c["T"] - 1):
        f0, f1 = r["frames"][b:b + 1, t], r["frames"][b:b + 1, t + 1]
        s = fo.flow_stage_ref(f1.astype(np.float32) / np.float32(255.0), fo.byte_reference(f0), radius, eps)
        truth = r["flow"][b, t]
        err.append(np.hypot(*(s.u[0] - truth)[inner]).mean())
        zero.append(np.hypot(*truth[inner]).mean())
    ratio = float(np.mean(err) / np.mean(zero))
    print("endpoint error %.4f px against %.4f px of the zero field: ratio %.3f" % (np.mean(err), np.mean(zero), ratio))
    assert MEASURED_FLOW_RATIO < 0.25
    assert ratio <= 2 * MEASURED_FLOW_RATIO, ratio
