"""Shared by the wide-block parity tests (tests/test_wino_wide_host.py, tests/test_gpu_wino_wide.py): the WIDE block shape of the F(4x4) Winograd kernel
(csrc/conv_wino4.h) walking N-blocks, split over several blocks per tile and ragged at its edges, under weights that keep every layer alive.

The headline plan is wide full blocks on every operator, walking two or three N-blocks, some of them from a later part of the tile's N-blocks
(csrc/conv_plan.h: plan_launch); at test sizes the default plan takes half, tall or packed blocks instead.  EIGEN_W4_TALL=0 with EIGEN_W4_HALF=0 forces
the wide shape (and rules the packed one out), EIGEN_W4_PARTS the split, so small nets at batch 3 reach the headline's launch forms.  Which forms a
(net, setting) reaches is asked of the planner itself (engine.plan_text), never typed in.  Numpy only: the GPU children import this module too."""
import collections

from tests import state_support as ss

BATCH = 3      # the tile count is no multiple of 8
N_CU = 256     # the MI355X; under the forced settings the plan does not depend on it (test_wino_wide_host.py)
MAX_WALK = 3   # the longest walk the planner's own rule produces (csrc/conv_plan.h): no setting here may plan a longer one
N_FED, N_SELF = 2, 1
# (reset, n_in, n_ext): reset and one step -- the step-0 twins alone --, one fed step, one self-fed step
PIECES = [(1, 1, 0), (0, 1, 0), (0, 0, 1)]
STATE_STEPS = [1, 2, 3]

# (w, h, channels) and what each is there for
NETS = [
    (128, 64, [3, 96, 192]),   # maps 64 x 32 and 32 x 16, exact blocks: n_nblk 6 fused, 12 unfused; ConvA_2 / ConvP_2 with NI 4 and n_nblk 3; ConvP_1 NI 3, n_nblk 2
    (96, 48, [3, 48, 96]),     # maps 48 x 24 and 24 x 12: ragged both ways
    (96, 48, [3, 96, 16]),     # a fused n_nblk 6 ConvLSTM with no 12-block operator in the net
    (96, 48, [1, 32, 64]),     # n_nblk 2 fused, 4 at the top; NI 4 single-block ConvA and ConvP
    (80, 48, [3, 48, 96]),     # maps 40 x 24 and 20 x 12: ragged by an odd number of 4-column tiles
    (64, 64, [3, 48, 96]),     # maps 32 x 32: one block wide exactly -- the headline's ConvLSTM_1 (3 -> 1 x 3), ConvA_2 (NI 3, 1 x 2), ConvP_1 (one N-block)
    (128, 48, [3, 96, 16]),    # maps 64 x 24: ragged at the bottom only (640 x 480's 160 x 120 maps): fused 6 -> 2 x 3, ConvP NI 3 split in two
    (128, 48, [3, 96, 192]),   # the same maps: ConvA NI 4 split in three; with the ConvLSTMs direct, the NI 4 walks of three on a ragged map
    (128, 64, [3, 96, 16]),    # exact blocks: the headline's ConvLSTM_2, fused 6 -> 2 x 3, again with no 12-block operator in the net
]
# every setting forces the wide shape; each runs in a fresh process (the switches are read once per process)
FORCE_WIDE = {"EIGEN_W4_TALL": "0", "EIGEN_W4_HALF": "0"}
MASK_LSTM_DIRECT = 0x0C0E0E00   # ConvA and ConvP in F(4x4), every ConvLSTM direct
Setting = collections.namedtuple("Setting", "env mask nets")
SETTINGS = {
    "parts=4": Setting({"EIGEN_W4_PARTS": "4"}, ss.MASK_DEFAULT, (0, 7)),                 # 12 -> 4 x 3, 6 -> 3 x 2, 3 -> 3 x 1
    "parts=2": Setting({"EIGEN_W4_PARTS": "2"}, ss.MASK_DEFAULT, (1, 2, 3, 4, 5, 6, 8)),   # 6 -> 2 x 3, 3 -> 1 x 3, 4 -> 2 x 2
    "parts=1,lstm-direct": Setting({"EIGEN_W4_PARTS": "1", "EIGEN_WINOGRAD": "0x0C0E0E00"}, MASK_LSTM_DIRECT, (0, 1, 5, 7)),   # ConvA / ConvP NI 4 as 1 x 3, NI 3 as 1 x 2
}
CASES = [(name, i) for name, s in SETTINGS.items() for i in s.nets]   # every (setting, net) that runs

# One launch form of the F(4x4) kernel.  walk: nwalk (1, 2 or 3); split: nparts > 1 (a block starts at N-block part * nwalk); ragged_right / ragged_bottom: the
# operator's map is no multiple of the wide block's 32 columns / 16 rows; step0: the step-0 twin (the first step after a reset reads fewer sources).
Cell = collections.namedtuple("Cell", "op NI fused shape walk split ragged_right ragged_bottom step0")


def cell_name(c):
    return ("%s NI=%d %s %s nwalk=%d %s%s%s%s" % (c.op, c.NI, "fused" if c.fused else "unfused", c.shape, c.walk, "split" if c.split else "whole",
                                                 " ragged-right" if c.ragged_right else "", " ragged-bottom" if c.ragged_bottom else "", " step-0 twin" if c.step0 else ""))


def setting_env(name, env):
    """`env` with the EIGEN_* variables of one setting and no other"""
    env = dict(env)
    for k in ("EIGEN_WINOGRAD", "EIGEN_WINO_FUSEUP", "EIGEN_W4_PARTS", "EIGEN_W4_TALL", "EIGEN_W4_HALF", "EIGEN_W4_PACK"):
        env.pop(k, None)
    env.update(FORCE_WIDE)
    env.update(SETTINGS[name].env)
    return env


def setting_switches(name):
    """the setting as engine.plan_text(switches=...) takes it"""
    env = setting_env(name, {})
    return {"w4_tall": int(env["EIGEN_W4_TALL"]), "w4_half": int(env["EIGEN_W4_HALF"]), "w4_parts": int(env["EIGEN_W4_PARTS"])}


def map_size(op, layer, w, h):
    """the map an operator runs at: ConvA_l reads E_{l-1} at the finer resolution"""
    l = layer - 1 if op == "convA" else layer
    return w >> l, h >> l


def cells_of(plan, w, h, ch, batch, n_cu, wino_mask, switches):
    """{Cell: [(op, layer), ...]} of the F(4x4) launches of a net's steady-state step and of its first step (`plan`: engine.plan_text).  ConvP has no step-0 twin."""
    out = {}
    for step0 in (False, True):
        for r in plan(ch, w, h, batch, n_cu, wino_mask=wino_mask, step0=step0, switches=switches):
            if r["kernel"] != "wino" or (step0 and r["op"] == "convP"):
                continue
            assert r["nparts"] * r["nwalk"] == r["n_nblk"], r
            mw, mh = map_size(r["op"], r["layer"], w, h)
            c = Cell(r["op"], r["NI"], bool(r["fused"]), r["shape"], r["nwalk"], r["nparts"] > 1, mw % 32 != 0, mh % 16 != 0, step0)
            out.setdefault(c, []).append((r["op"], r["layer"]))
    return out


def case_cells(plan, name, i, batch=BATCH, n_cu=N_CU, switches="setting"):
    """The cells of one (setting, net), with the two conditions every case must meet BEFORE anything launches: every F(4x4) launch is wide, none walks more
    than MAX_WALK N-blocks.  switches: "setting" plans under the setting's switches, None under the calling process's own."""
    w, h, ch = NETS[i]
    mask = -1 if switches is None else SETTINGS[name].mask   # (None: the process's own mask too)
    cells = cells_of(plan, w, h, ch, batch, n_cu, mask, setting_switches(name) if switches == "setting" else switches)
    assert cells, (name, NETS[i], "no F(4x4) launch")
    for c in cells:
        assert c.shape == "wide", (name, NETS[i], cell_name(c))
        assert 1 <= c.walk <= MAX_WALK, (name, NETS[i], cell_name(c))
    return cells


def bench_wide_cells(plan):
    """every wide cell of the default plans of bench.SHAPES at their bench batches"""
    import bench
    out = {}
    for shape, s in bench.SHAPES.items():
        w, h, ch, batch = s[0], s[1], s[2], s[7]
        for c, ops in cells_of(plan, w, h, ch, batch, N_CU, -1, {}).items():
            if c.shape == "wide":
                out.setdefault(c, []).append(shape)
    return out


# Nets the required set does not need, and what each is there for all the same (a property the cell does not carry)
BEYOND_CENSUS = {3: "a ConvLSTM walk of two (4 -> 2 x 2) and the NI = 4 ConvA / ConvP of ONE N-block, which neither walk nor split",
                 4: "edge blocks with an odd number of 4-column tiles (40 and 20 columns), where 96 x 48 has an even one"}


def ragged_variants(need):
    """The ragged variants of the walking wide cells in `need`: the same cell -- operator, NI, fused or not, walk, split or whole, step-0 twin or not -- on a map ragged at
    BOTH edges (an edge tile must stay an edge tile in every N-block of the walk).  Not for the NI = 4 ConvA / ConvP: those walks take 192 channels, which run
    here on exact maps and on maps ragged at the bottom only."""
    return {c._replace(ragged_right=True, ragged_bottom=True) for c in need if c.walk > 1 and not (c.NI == 4 and c.op in ("convA", "convP"))}


def missing_cells(plan, have):
    """names of the required cells that `have` (a collection of Cell) lacks: the bench shapes' wide cells and the ragged variants"""
    need = bench_wide_cells(plan)
    miss = [cell_name(c) + " (bench: %s)" % ", ".join(shapes) for c, shapes in sorted(need.items()) if c not in have]
    return miss + [cell_name(c) + " (ragged variant)" for c in sorted(ragged_variants(need)) if c not in have]


def weights(i):
    return ss.dense_weights(NETS[i][2], NETS[i][0], NETS[i][1])


def images(i):
    w, h, ch = NETS[i]
    return ss.images(w, h, ch, BATCH)


def oracle_states(oracle, i, mask):
    """(frames, {step: state}) of the oracle's 2 fed + 1 self-fed steps of net i under `mask`"""
    w, h, ch = NETS[i]
    return ss.oracle_states(oracle, weights(i), ch, w, h, images(i), mask, False, steps=STATE_STEPS, n_fed=N_FED, n_self=N_SELF)
