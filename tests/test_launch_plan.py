"""What runs, in which shape, on which grid: the planner of csrc/conv_plan.h, read through the host-only ABI entry eigen_plan_text (no GPU needed).

No result bit depends on the launch shape (block shape, half blocks, packed tiles, the walk), so no parity test can see a heuristic that an edit broke; this test
pins the choices that DESIGN.md and the planner's comments state, with the numbers of the kernel traces in profiles/plan_*_launches.txt (n_cu = 256, the MI355X),
and checks the planner's operator forms against the ones the CPU oracle takes.  Skipped when the library is not built."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "libeigen_hip.so")
N_CU = 256
COLOUR, GRAY = [3, 48, 96, 192], [1, 16, 32, 64]
WINO_DEFAULT = 0x0FFFFFFE
# (W, H, channels, batch) of bench.SHAPES' headline, ref160, c1, c2, ref640
HEADLINE, REF160, C1, C2, REF640 = (256, 256, COLOUR, 256), (160, 120, COLOUR, 50), (64, 64, GRAY, 10), (160, 120, GRAY, 50), (640, 480, COLOUR, 16)


@pytest.fixture(scope="module")
def plan():
    if not os.path.exists(LIB):
        pytest.skip("libeigen_hip.so not built")
    from evolutionary_illusion_generator_amd import engine

    def run(shape, batch=None, **kw):
        w, h, ch, b = shape
        return engine.plan_text(ch, w, h, b if batch is None else batch, n_cu=N_CU, **kw)
    return run


def one(rows, op, layer):
    hit = [r for r in rows if r["op"] == op and r["layer"] == layer]
    assert len(hit) == 1, (op, layer, rows)
    return hit[0]


def ceil8(n):
    return (n + 7) // 8 * 8


def test_headline_step(plan):
    rows = plan(HEADLINE)
    assert [(r["op"], r["layer"]) for r in rows] == [("convA", 1), ("convA", 2), ("convA", 3), ("lstm", 3), ("convP", 3), ("lstm", 2), ("convP", 2),
                                                     ("lstm", 1), ("convP", 1), ("up4", 0), ("lstm", 0), ("convP", 0)]   # the only 2x2-form pass is layer 0's
    a1 = one(rows, "convA", 1)   # its source has 6 channels: direct
    assert (a1["wino"], a1["NI"], a1["n_nblk"]) == (0, 3, 1) and a1["kernel"].startswith("mfma")
    for op, layers in (("convA", (2, 3)), ("convP", (1, 2, 3)), ("lstm", (1, 2, 3))):
        for l in layers:
            r = one(rows, op, l)
            assert (r["kernel"], r["shape"], r["wino"]) == ("wino", "wide", 1), r
    # n_nblk, nparts, nwalk, grid.  profiles/plan_headline_launches.txt: the three wino4_kernel<4, 1, false, false, false, false> lines (768 threads per block),
    # grid = 6291456 / 768 = 8192 (layer 1), 3145728 / 768 = 4096 (layer 2), 1572864 / 768 = 2048 (layer 3)
    want = {1: (3, 1, 3, 8192), 2: (6, 2, 3, 4096), 3: (12, 4, 3, 2048)}
    for l, w in want.items():
        r = one(rows, "lstm", l)
        assert (r["n_nblk"], r["nparts"], r["nwalk"], r["grid"]) == w, r
        assert r["fused"] == (1 if l < 3 else 0)   # the unpooled source inside the chains: no 2x2-form pass for layers 1 and 2
    assert one(rows, "lstm", 0)["kernel"] == "lstm0" and one(rows, "convP", 0)["kernel"] == "convp0"   # the per-pixel image-layer kernels
    assert not any(r["shape"] in ("half", "tall", "pack") for r in rows)


def test_step0_runs_the_same_shapes_over_fewer_sources(plan):
    for shape in (HEADLINE, REF160, C1):
        assert plan(shape, step0=True) == plan(shape)   # the geometry of every launch is the same; only the K range differs


def test_tall_blocks_where_they_cover_the_map_with_fewer_blocks(plan):
    # profiles/plan_ref640_launches.txt: wino4_kernel<4, 1, true, ...> grid = 1474560 / 768 = 1920 = 12 N-blocks x 16 images x 10 blocks;
    # plan_ref160_launches.txt: wino4_kernel<4, 1, true, ...> grid = 700416 / 768 = 912 = 6 x ceil8(50 images x 3 blocks)
    r = one(plan(REF640), "lstm", 3)   # 80 x 60
    assert r["shape"] == "tall" and r["tilesX"] * r["tilesY"] == 10
    r = one(plan(REF160), "lstm", 2)   # 40 x 30
    assert r["shape"] == "tall" and r["tilesX"] * r["tilesY"] == 3
    r = one(plan(HEADLINE), "lstm", 1)   # 128 x 128
    assert r["shape"] == "wide" and r["tilesX"] * r["tilesY"] == 32


def test_packed_tiles(plan):
    # the 20 x 15 top layer: five half blocks per four images; ref160: 12 x (50 + 13) = 756 blocks, c2: 4 x 63 = 252 (the grid pads the 63 to a multiple of 8)
    # profiles/plan_ref160_launches.txt: wino4_kernel<4, 1, false, true, true, true> grid = 589824 / 768 = 768; plan_c2_launches.txt: 196608 / 768 = 256
    for shape, n_nblk in ((REF160, 12), (C2, 4)):
        rows = plan(shape)
        r = one(rows, "lstm", 3)
        assert (r["shape"], r["n_nblk"], r["nparts"], r["nwalk"]) == ("pack", n_nblk, n_nblk, 1), r
        assert r["grid"] == n_nblk * ceil8(50 + 13)
        assert one(rows, "convP", 3)["shape"] == "pack"
    for shape in (HEADLINE, REF160, C1, C2, REF640):
        for batch in (1, 10, 50, 256):
            assert not any(r["op"] == "convA" and r["shape"] == "pack" for r in plan(shape, batch))


def test_half_blocks_only_while_at_most_one_per_cu(plan):
    rows = plan(C1)
    wino = [r for r in rows if r["kernel"] == "wino"]
    assert wino and all(r["shape"] == "half" for r in wino), rows   # c1's small launches take them
    assert not any(r["shape"] == "half" for r in plan(HEADLINE))
    for shape in (HEADLINE, REF160, C1, C2, REF640):
        for batch in (1, 4, 10, 50, 256):
            for r in plan(shape, batch):
                if r["shape"] == "half":
                    assert r["n_nblk"] * batch * r["tilesX"] * r["tilesY"] <= N_CU, r


def test_walk_rule(plan):
    for shape in (HEADLINE, REF160, C1, C2, REF640):
        for batch in (1, 10, 50, 256):
            for step0 in (False, True):
                for r in plan(shape, batch, step0=step0):
                    if r["kernel"] != "wino":
                        assert (r["nparts"], r["nwalk"]) == (0, 0)
                        continue
                    assert r["nparts"] * r["nwalk"] == r["n_nblk"], r
                    if r["shape"] != "wide":   # tall, half and packed blocks do not walk
                        assert r["nwalk"] == 1, r
                        continue
                    tiles = batch * r["tilesX"] * r["tilesY"]
                    nwalk = 3 if r["n_nblk"] % 3 == 0 else 2 if r["n_nblk"] % 2 == 0 else 1
                    if (r["n_nblk"] // nwalk) * tiles < 4 * N_CU:   # the launch would not give every CU four blocks
                        nwalk = 1
                    assert r["nwalk"] == nwalk, r
                    assert r["grid"] == r["nparts"] * ceil8(tiles), r


def test_operator_form_does_not_depend_on_the_batch(plan):
    for shape in (HEADLINE, REF160, C1, C2, REF640):
        forms = [[(r["op"], r["layer"], r["epi"], r["wino"], r["fused"], r["NI"], r["n_nblk"]) for r in plan(shape, batch)] for batch in (1, 50, 256)]
        assert forms[0] == forms[1] == forms[2]


def test_planner_and_oracle_agree_on_the_operator_forms(plan):
    import bench
    import oracle
    shapes = [(s[0], s[1], s[2]) for s in bench.SHAPES.values()]
    shapes.append((160, 120, COLOUR))   # odd top-layer height: 20 x 15
    shapes.append((80, 64, COLOUR))     # layer 2 is 20 wide, a multiple of 4 but not of 8: the rows of its unpooled source are no 16-byte chunks
    kinds = {"lstm": 0, "convA": 1, "convP": 2}
    for w, h, ch in shapes:
        L = len(ch)
        for mask in (0, WINO_DEFAULT, WINO_DEFAULT & ~(1 << 24)):
            rows = plan((w, h, ch, 4), wino_mask=mask)
            for op, kind in kinds.items():
                for l in range(1 if op == "convA" else 0, L):
                    r = one(rows, op, l)
                    assert (bool(r["wino"]), bool(r["fused"])) == oracle.wino_form(mask, kind, l, ch, w, h), (w, h, ch, hex(mask), r)
            for l in range(L - 1):   # a 2x2-form pass exactly where the unpooled source is not inside the chains
                assert len([r for r in rows if r["op"] == "up4" and r["layer"] == l]) == (0 if one(rows, "lstm", l)["fused"] else 1)
