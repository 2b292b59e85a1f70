"""CPU: the host side of the CPPN parameter gradients ("CPPN parameter gradients") -- the two float64 statements
of tests/cppn_grad_support.py against each other and against central differences, the teeth of the bound, the conditions the cases
must meet, ``genome.flatten_genome_map``, ``train.refine_genomes`` simulated with the references alone, its argument checks, and
the new entry point in header, binding and library with the register metadata of its two kernels."""
import copy
import os
import re
import types

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import fitness, genome, synth, train
from tests import cppn_grad_support as S
from tests.train_support import _kernel_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPPN_GRAD_KERNELS = ["cppn_grad_kernel", "cppn_grad_sum_kernel"]
MUTANTS = [dict(quant=False), dict(background=False), dict(resp_from_z=True), dict(assign_fanout=True)]
case_id = lambda c: "seed%d-h%d-%dx%d" % c


def test_the_bound_is_a_thousand_times_the_measured_deviation():
    assert S.E == 1000 * S.MEASURED_DEVIATION and len(S.CASES) == 24


@pytest.mark.parametrize("c", S.CASES, ids=case_id)
def test_the_two_statements_agree_within_a_hundredth_of_the_bound(c):
    flat, leaves, gimg = S.case(*c)
    ref, _ = S.case_reference(*c)
    n, e = S.deviation(S.grads_reverse(flat, leaves, gimg, 3), ref)
    print("%s: (b) from (a): %.3g in norm, %.3g element-wise" % (case_id(c), n, e))
    assert n <= S.E / 100 and e <= S.E / 100, (n, e)


# Central differences with step 1e-6 on parameters of order 1.  Truncation: h^2 f''' / 6 with third derivatives of a few 1e3 (slopes 5 and
# 2.5 per activation, weights up to ~3, three layers deep) is of order 1e-9 of the gradient; rounding: 2^-53 |terms| / h = 1e-10 times the
# cancellation of a signed sum over the pixels.  1e-7 leaves two orders of magnitude above both and is five below a wrong term.
FD_STEP, FD_BOUND = 1e-6, 1e-7


@pytest.mark.parametrize("c", S.CASES, ids=case_id)
def test_the_reference_is_the_slope_of_the_masked_objective(c):
    flat, leaves, gimg = S.case(*c)
    ref, outs = S.case_reference(*c)
    masks = [S.seed_mask(outs[k], leaves[0]) for k in range(3)]
    got = []
    for name in ("edge_w", "bias", "resp"):
        g = np.zeros(len(flat[name]))
        for i in range(len(g)):
            f, v = dict(flat), flat[name].copy()
            f[name] = v
            v[i] = flat[name][i] + FD_STEP
            up = S.masked_objective(f, leaves, gimg, 3, masks)
            v[i] = flat[name][i] - FD_STEP
            g[i] = (up - S.masked_objective(f, leaves, gimg, 3, masks)) / (2 * FD_STEP)
        got.append(g)
    n, e = S.deviation(got, ref)
    print("%s: differences from (a): %.3g in norm, %.3g element-wise" % (case_id(c), n, e))
    assert n <= FD_BOUND and e <= FD_BOUND, (n, e)


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: next(iter(m)))
def test_the_bound_has_teeth(mutant):
    """Every wrong reverse pass misses the bound on the case list: on every case with 20 hidden nodes (which has background, wrapped
    pixels, responses that matter and nodes with more than one consumer), and so on the list."""
    missed = [c for c in S.CASES if not S.within(S.grads_reverse(*S.case(*c), 3, **mutant), S.case_reference(*c)[0])]
    print("%s: misses %d of %d cases" % (mutant, len(missed), len(S.CASES)))
    assert missed
    assert all(c in missed for c in S.CASES if c[1] == 20), [c for c in S.CASES if c[1] == 20 and c not in missed]


def test_no_case_has_a_pixel_at_the_edge_of_the_mask():
    """The mask of statement (a) comes from torch's values, that of (b) and of the device from the render's: a pixel whose 255 v lies
    within 1e-6 of -1 or of 256 could flip between them.  None does (the nearest is 0.07 away), and every case has seeded pixels,
    background, and parameters whose reference is exactly zero beside a gradient that is not."""
    nearest = np.inf
    for c in S.CASES:
        flat, leaves, gimg = S.case(*c)
        ref, outs = S.case_reference(*c)
        live = leaves[0] != -1.0
        assert live.any() and not live.all()
        nearest = min(nearest, np.abs(outs[:, live] * 255.0 + 1.0).min(), np.abs(outs[:, live] * 255.0 - 256.0).min())
        assert any(S.seed_mask(outs[k], leaves[0]).any() for k in range(3)), c
        assert np.linalg.norm(np.concatenate(ref)) > 0, c
    print("nearest pixel to the edge of the mask: %.3g" % nearest)
    assert nearest > 1e-6


# ---- flatten_genome_map
def _check_map(g, cfg, n_leaves=2):
    m, flat = genome.flatten_genome_map(g, cfg, n_leaves), genome.flatten_genome(g, cfg, n_leaves)
    assert set(m) == set(flat) | {"node_key", "edge_key"}
    for k, v in flat.items():
        assert m[k].dtype == v.dtype and np.array_equal(m[k], v), k
    assert len(m["node_key"]) == len(flat["act"]) and len(m["edge_key"]) == len(flat["edge_w"])
    for n, key in enumerate(m["node_key"]):
        if key is not None:
            assert m["bias"][n] == g.nodes[key].bias and m["resp"][n] == g.nodes[key].response
    for k, key in enumerate(m["edge_key"]):
        if key is not None:
            assert m["edge_w"][k] == g.connections[key].weight and g.connections[key].enabled
    mapped = [k for k in m["node_key"] if k is not None], [k for k in m["edge_key"] if k is not None]
    assert len(set(mapped[0])) == len(mapped[0]) and len(set(mapped[1])) == len(mapped[1])
    return m


@pytest.mark.parametrize("seed", range(12))
def test_flatten_genome_map_names_the_gene_of_every_flat_parameter(seed):
    cfg = synth.make_config(2, 3)
    _check_map(synth.make_genome(seed + 1, cfg, seed, num_hidden=S.HIDDEN[seed % 3]), cfg)   # (seed 5 has a constant output: a None node)
    cfg4 = synth.make_config(4, 3)
    _check_map(synth.make_genome(seed + 1, cfg4, seed, num_hidden=6), cfg4, 4)


def test_flatten_genome_map_marks_exactly_the_folded_constants():
    cfg = synth.make_config(2, 3)
    m = _check_map(S.folding_genome(), cfg)
    assert m["node_key"] == S.EXPECTED_FOLDING_MAP["node_key"]
    assert m["edge_key"] == S.EXPECTED_FOLDING_MAP["edge_key"]
    assert (-1, 2) not in m["edge_key"]                       # the disabled connection has no flat edge
    m = _check_map(S.all_activations_genome(), cfg)
    assert None not in m["node_key"] and None not in m["edge_key"] and sorted(set(m["act"])) == list(range(7))


def test_flatten_lists_returns_what_it_returned():
    cfg = synth.make_config(2, 3)
    for g in (S.folding_genome(), synth.make_genome(1, cfg, 0)):
        assert len(genome._flatten_lists(g, cfg)) == 7
        assert genome._flatten_lists(g, cfg) == genome._flatten_lists_keys(g, cfg)[:7]


# ---- refine_genomes, simulated with the references alone
SIM, sim_genomes = S.SIM, S.sim_genomes


def simulate_refine(weights, genomes, cfg, w, h, ch, structure, n_repeat, n_ext, iters, lr):
    """train.refine_genomes with tests/frame_grad_support.run_frames(tied=True) for the trainer call (float feedback), statement (b)
    for the kernel, the render's quantisation in numpy, and train.genome_update itself for the update."""
    from tests.frame_grad_support import run_frames
    leaves = [np.asarray(p, np.float64).reshape(-1) for p in fitness.leaf_planes(structure, w, h, 2)]
    out = [copy.deepcopy(g) for g in genomes]
    maps = [genome.flatten_genome_map(g, cfg) for g in out]
    T, sw = n_repeat + n_ext, [0.0] * (n_repeat - 1) + [1.0] * n_ext
    history = np.zeros(iters + 1)

    def loss_of():
        flats = [genome.flatten_genome(g, cfg) for g in out]
        img = np.stack([S.quantise(S.forward_np(f, leaves)[0], f, leaves, ch[0]) for f in flats]).reshape(len(out), ch[0], h, w)
        frames = np.ascontiguousarray(np.repeat(img[:, None], T, 1))
        r = run_frames(weights, list(ch), frames, n_fed=n_repeat, requant=False, step_weights=sw, tied=True)
        return r.loss, r.frame_grad.astype(np.float32), flats

    for i in range(iters):
        history[i], grad, flats = loss_of()
        for g, m, f, gi in zip(out, maps, flats, grad):
            g_w, g_bias, g_resp = S.grads_reverse(f, leaves, gi.reshape(ch[0], -1), ch[0])
            train.genome_update(g, m, g_bias, g_resp, g_w, lr)
    history[iters] = loss_of()[0]
    return out, history


@pytest.mark.parametrize("wset", ["synthetic", "live"])
def test_simulated_refinement_raises_the_loss(wset):
    from tests.train_support import _weight_sets
    w, h, ch = SIM["w"], SIM["h"], SIM["ch"]
    leaves = fitness.leaf_planes(SIM["structure"], w, h, 2)
    assert int((np.asarray(leaves[0]) == -1.0).sum()) == 104 and np.asarray(leaves[0]).size == 192
    cfg, genomes = sim_genomes()
    before = copy.deepcopy(genomes)
    out, history = simulate_refine(dict(_weight_sets(list(ch), w, h))[wset], genomes, cfg, **SIM)
    print("%s: history %s (%+.2f %%)" % (wset, history, 100 * (history[-1] / history[0] - 1)))
    assert history[-1] > history[0]
    for a, b, o in zip(before, genomes, out):   # the inputs are untouched, the copies moved by at most iters * lr
        for k in a.nodes:
            assert a.nodes[k] == b.nodes[k]
            assert abs(o.nodes[k].bias - a.nodes[k].bias) <= SIM["iters"] * SIM["lr"] * (1 + 1e-12)
        for k in a.connections:
            assert a.connections[k] == b.connections[k]
            assert abs(o.connections[k].weight - a.connections[k].weight) <= SIM["iters"] * SIM["lr"] * (1 + 1e-12)


def test_genome_update_moves_only_what_is_selected_and_trainable():
    cfg = synth.make_config(2, 3)
    g = S.folding_genome()
    m = genome.flatten_genome_map(g, cfg)
    rng = np.random.default_rng(0)
    gb, gr, gw = rng.normal(size=len(m["node_key"])), rng.normal(size=len(m["node_key"])), rng.normal(size=len(m["edge_key"]))
    gw[0] = 100.0                                      # a frozen edge: neither moved nor counted in the normalisation
    h = copy.deepcopy(g)
    assert train.genome_update(h, m, gb, gr, gw, 0.5, ("bias",))
    top = max(abs(gb[n]) for n, k in enumerate(m["node_key"]) if k is not None)
    for n, k in enumerate(m["node_key"]):
        if k is not None:
            assert h.nodes[k].bias == g.nodes[k].bias + 0.5 * (gb[n] / top) and h.nodes[k].response == g.nodes[k].response
    assert all(h.connections[k] == g.connections[k] for k in g.connections)
    assert all(h.nodes[k] == g.nodes[k] for k in (1, 10, 11))           # the constant output and the folded sub-graph
    h = copy.deepcopy(g)
    assert train.genome_update(h, m, gb, gr, gw, 0.5, bounds={"weight": (-0.1, 0.1)})
    assert all(-0.1 <= h.connections[k].weight <= 0.1 for k in m["edge_key"] if k is not None)
    assert h.connections[(-1, 2)] == g.connections[(-1, 2)] and h.connections[(10, 3)] == g.connections[(10, 3)]
    for bad in (np.zeros_like(gb), np.full_like(gb, np.nan)):
        h = copy.deepcopy(g)
        assert not train.genome_update(h, m, bad, gr * 0, gw * 0, 0.5)
        assert all(h.nodes[k] == g.nodes[k] for k in g.nodes)


def test_python_argument_errors_need_no_device():
    cfg, genomes = sim_genomes()
    fake = types.SimpleNamespace(max_steps=5, batch=2, channels=[3, 4], w=16, h=12)
    with pytest.raises(ValueError, match="max_steps"):
        train.refine_genomes(fake, genomes[:2], cfg, 1, n_repeat=4, n_ext=2)
    with pytest.raises(ValueError, match="max_steps"):
        train.refine_genomes(fake, genomes[:2], cfg, 1)                       # the defaults: 22 frames
    with pytest.raises(ValueError, match="batch"):
        train.refine_genomes(fake, genomes[:3], cfg, 1, n_repeat=3, n_ext=2)
    with pytest.raises(ValueError, match="batch"):
        train.refine_genomes(fake, [], cfg, 1, n_repeat=3, n_ext=2)
    for lr in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lr"):
            train.refine_genomes(fake, genomes[:2], cfg, 1, n_repeat=3, n_ext=2, lr=lr)
    with pytest.raises(ValueError, match="params"):
        train.refine_genomes(fake, genomes[:2], cfg, 1, n_repeat=3, n_ext=2, params=("weights",))
    with pytest.raises(ValueError, match="bounds"):
        train.refine_genomes(fake, genomes[:2], cfg, 1, n_repeat=3, n_ext=2, bounds={"weight": (1.0, -1.0)})
    assert "refine_genomes" in train.__all__


# ---- the entry point and its kernels
def test_header_binding_and_library_hold_the_entry_point():
    from evolutionary_illusion_generator_amd import engine
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    assert "eigen_cppn_param_grads" in declared and "eigen_cppn_param_grads" in engine.EXPORTS
    assert re.search(r"#define\s+EIGEN_ABI_VERSION\s+4\b", header) and engine.ABI_VERSION == 4
    assert os.path.exists(engine.LIB_PATH), "libeigen_hip.so is not built"
    lib = engine.load_library()
    assert lib.eigen_abi_version() == 4 and hasattr(lib, "eigen_cppn_param_grads")


def test_the_kernels_live_in_their_own_header():
    csrc = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
    pat = r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\("
    assert set(re.findall(pat, open(os.path.join(csrc, "cppn_grad_kernel.h")).read())) == set(CPPN_GRAD_KERNELS)
    assert set(re.findall(pat, open(os.path.join(csrc, "cppn_kernel.h")).read())) == {"cppn_render_kernel"}
    assert '#include "cppn_grad_kernel.h"' in open(os.path.join(csrc, "eigen_engine.hip")).read()


@pytest.mark.parametrize("kernel", CPPN_GRAD_KERNELS)
def test_the_kernels_have_no_scratch_and_no_spills(kernel):
    from tests import test_isa_stats as isa
    assert os.path.exists(isa.LIB), "libeigen_hip.so is not built"
    assert os.path.exists(isa.READELF), "llvm-readelf not found"
    stats = _kernel_stats()
    names = [n for n in stats if re.match(r"_ZN3eig\d+%sE" % kernel, n)]
    assert len(names) == 1, (kernel, names)
    for s in stats[names[0]]:
        print(kernel, {k: s.get(k) for k in ("vgpr_count", "sgpr_count", "agpr_count")})
        assert s["private_segment_fixed_size"] == 0 and s["vgpr_spill_count"] == 0 and s["sgpr_spill_count"] == 0, (names[0], s)
