"""CPU side of the wide-block parity test (tests/test_gpu_wino_wide.py): which launch forms of the F(4x4) kernel its nets and settings reach, asked of the planner
(eigen_plan_text_sw through engine.plan_text(switches=...)); what the older switch runs do NOT reach, pinned; and the liveness of the dense weights on every net.
Cases and cells are tests/wino_wide_support.py.  No GPU; the plan tests are skipped when the library is not built."""
import functools
import os

import pytest

from tests import state_support as ss
from tests import wino_wide_support as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "libeigen_hip.so")
GEOMETRY = ("op", "layer", "kernel", "shape", "epi", "wino", "fused", "vec", "NI", "n_nblk", "tilesX", "tilesY", "nparts", "nwalk", "threads")   # a plan row without its grid


@pytest.fixture(scope="module")
def plan():
    if not os.path.exists(LIB):
        pytest.skip("libeigen_hip.so not built")
    from evolutionary_illusion_generator_amd import engine
    return engine.plan_text


def census(plan, cases):
    have = {}
    for name, i in cases:
        for c in ws.case_cells(plan, name, i):
            have.setdefault(c, []).append((name, ws.NETS[i]))
    return have


def test_census_the_cases_hold_every_wide_cell_of_the_bench_plans(plan):
    """The union of the cells of every (setting, net) at n_cu = 256 contains the required set: every wide cell of the default plans of bench.SHAPES at their
    bench batches and the ragged variants (wino_wide_support.missing_cells names a missing one).  No case plans a launch that is not wide or a walk longer than the
    planner's own rule gives (case_cells).  Under the forced settings neither the batch nor the number of compute units changes a launch's geometry, so the cells
    planned here are the cells that run on whatever device runs them.  Taking a setting away leaves a required cell out, and so does taking a net away, but for the two nets kept for what the cell does not say."""
    import bench
    have = census(plan, ws.CASES)
    for c, where in sorted(have.items()):
        print("CELL %-78s %s" % (ws.cell_name(c), "; ".join("%s %dx%d %s" % (n, w, h, ch) for n, (w, h, ch) in where)))
    need = ws.bench_wide_cells(plan)
    assert {"headline", "ref640"} <= {s for shapes in need.values() for s in shapes} and len(need) >= 8, need   # (the required set is not empty by accident)
    assert any(c.split and c.walk == 3 for c in need) and any(c.op == "lstm" and not c.fused and c.walk == 3 for c in need)
    assert ws.missing_cells(plan, have) == []
    # the two entries agree on the default plan (eigen_plan_text, eigen_plan_text_sw under the default switches), so `need` is the plan a benchmark process runs
    for s in bench.SHAPES.values():
        for step0 in (False, True):
            assert plan(s[2], s[0], s[1], s[7], ws.N_CU, step0=step0) == plan(s[2], s[0], s[1], s[7], ws.N_CU, step0=step0, switches={})
    # batch and compute units do not matter under the forced settings
    for name, i in ws.CASES:
        w, h, ch = ws.NETS[i]
        kw = dict(wino_mask=ws.SETTINGS[name].mask, switches=ws.setting_switches(name))
        base = [{k: r[k] for k in GEOMETRY} for r in plan(ch, w, h, ws.BATCH, ws.N_CU, **kw) if r["kernel"] == "wino"]
        for batch, n_cu in ((1, 1), (ws.BATCH, 304), (ws.BATCH, 8), (2048, ws.N_CU), (2048, 1)):
            assert [{k: r[k] for k in GEOMETRY} for r in plan(ch, w, h, batch, n_cu, **kw) if r["kernel"] == "wino"] == base, (name, ws.NETS[i], batch, n_cu)
            assert ws.case_cells(plan, name, i, batch, n_cu).keys() == ws.case_cells(plan, name, i).keys()
    # every setting is needed, and every net but the ones wino_wide_support.BEYOND_CENSUS gives a reason for
    for name in ws.SETTINGS:
        assert ws.missing_cells(plan, census(plan, [c for c in ws.CASES if c[0] != name])), "the census passes without setting %s" % name
    spare = [i for i in range(len(ws.NETS)) if not ws.missing_cells(plan, census(plan, [c for c in ws.CASES if c[1] != i]))]
    assert spare == sorted(ws.BEYOND_CENSUS), [ws.NETS[i] for i in spare]


def _switches_of(switch):
    """a setting of state_support.SWITCHES as plan_text takes it: (mask, switches)"""
    env = ss.switch_env(switch, {})
    sw = {"w4_" + k[len("EIGEN_W4_"):].lower(): int(v) for k, v in env.items() if k.startswith("EIGEN_W4_")}
    return ss.switch_mask(switch), sw


def test_the_shared_rollouts_reach_no_wide_launch_and_parts_1_changes_none(plan):
    """Pinned, so that whoever changes state_support.ROLLOUTS sees it: under the default switches every F(4x4) launch of the six roll-outs shared by
    test_winograd_operators_frames_bit_exact and test_state_of_every_layer_bit_exact is half, tall or packed, and such blocks do not walk -- EIGEN_W4_PARTS=1 changes
    no row of any of their plans.  The wide walking forms are tests/test_gpu_wino_wide.py's."""
    assert "parts=1" in ss.SWITCHES
    mask1, parts1 = _switches_of("parts=1")
    assert (mask1, parts1) == (ss.MASK_DEFAULT, {"w4_parts": 1})
    n = 0
    for w, h, ch, B in ss.ROLLOUTS:
        for step0 in (False, True):
            rows = plan(ch, w, h, B, ws.N_CU, step0=step0, switches={})
            wino = [r for r in rows if r["kernel"] == "wino"]
            n += len(wino)
            assert wino and all(r["shape"] in ("half", "tall", "pack") and r["nwalk"] == 1 for r in wino), (w, h, ch, B, wino)
            assert plan(ch, w, h, B, ws.N_CU, step0=step0, switches=parts1) == rows, (w, h, ch, B)
    assert n >= 6 * 2 * 3


@functools.lru_cache(maxsize=None)
def _final_state(i, mask):
    import oracle
    oracle.build()
    return ws.oracle_states(oracle, i, mask)[1][ws.STATE_STEPS[-1]]


@pytest.mark.parametrize("i", range(len(ws.NETS)), ids=["%dx%d-%s" % (w, h, "_".join(map(str, ch))) for w, h, ch in ws.NETS])
def test_dense_weights_keep_every_net_alive(oracle_lib, i):
    """state_support.is_live on the ORACLE's state after the three steps, for every operator-form mask the net runs under: the condition the dense weights must meet
    for a wrong N-block or edge tile to show in the state (tests/test_state_parity_host.py)."""
    masks = sorted({ws.SETTINGS[name].mask for name, j in ws.CASES if j == i})
    assert masks, "net %s runs under no setting" % (ws.NETS[i],)
    for mask in masks:
        rows, clamp = ss.liveness(_final_state(i, mask))
        print("LIVENESS %s mask %08x: P0 at clamp %.3f | " % (ws.NETS[i], mask, clamp) + " | ".join("l%d: E>0 %.2f, |R| in (1e-3, 0.9) %.3f, std(R) %.3f" % ((l + 1,) + r) for l, r in enumerate(rows)))
        assert ss.is_live(rows, clamp), (ws.NETS[i], hex(mask), rows, clamp)
