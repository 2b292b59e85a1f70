"""Shared by tests/test_cppn_grad_host.py and tests/test_gpu_cppn_grad.py: two float64 statements of the gradient of a loss by the
parameters of a flattened CPPN ("CPPN parameter gradients"), the case list, the bound, and hand-built genomes.

Both statements take ``genome.flatten_genome``'s arrays, the leaf planes [n_leaves][N] and the image gradient [c_dim][N], and return
(g_w, g_bias, g_resp) of  L = sum over c < c_dim, p of  gimg[c, p] * v[out_node[c], p] * mask[c, p],  where v is the node value and
mask the straight-through rule of the render's uint8 quantisation: the pixel is not background (plane 0 != -1) and
t = trunc(255 v) lies in [0, 255] (-0.0 passes, NaN fails).
  (a) ``grads_autograd``: torch autograd, torch's own transcendentals;
  (b) ``grads_reverse``: a numpy reverse pass written out node by node and edge by edge as csrc/cppn_grad_kernel.h is, over a forward
      that uses oracle.detmath64 (the device's transcendentals, so its node values are the render's)."""
import functools

import numpy as np
import torch

from evolutionary_illusion_generator_amd import synth
from evolutionary_illusion_generator_amd.genome import flatten_genome
from oracle import detmath64 as dm

# ---- the bound.  Per genome, over the concatenated (g_w, g_bias, g_resp): |got - ref|_2 <= E |ref|_2 and max |got - ref| <= E max |ref|.
# MEASURED_DEVIATION is the worst deviation of statement (b) from statement (a) over CASES, as tests/test_cppn_grad_host.py prints it:
# 1.08e-15 in norm and 1.40e-15 element-wise were measured on the 24 cases; the constant is the larger.  The host test asserts that every case stays within E / 100, ten times this figure.
# E is 1000 x that: the device adds a third summation order (per thread, a butterfly over the wave, the slabs in block order) and its
# own cos, and the summation error grows with the pixel count (the largest GPU shape, 64 x 48, has ten times the pixels of the
# largest case).
MEASURED_DEVIATION = 1.4e-15
E = 1000 * MEASURED_DEVIATION


def deviation(got, ref):
    """(norm ratio, element ratio) of one genome: |got - ref|_2 / |ref|_2 and max |got - ref| / max |ref| over the concatenated
    (g_w, g_bias, g_resp).  A reference that is zero altogether compares nothing and fails."""
    a, r = np.concatenate([np.ravel(x) for x in got]).astype(np.float64), np.concatenate([np.ravel(x) for x in ref]).astype(np.float64)
    nr = float(np.linalg.norm(r))
    assert nr > 0, "the reference gradient is zero: nothing is compared"
    return float(np.linalg.norm(a - r)) / nr, float(np.abs(a - r).max()) / float(np.abs(r).max())


def within(got, ref, bound=E):
    n, e = deviation(got, ref)
    return n <= bound and e <= bound


# ---- forward
def _leaf(src, leaves, n_leaves):
    li = -src - 1
    return None if li >= n_leaves else leaves[li]     # None: the constant-1 leaf


def forward_np(flat, leaves, math="det"):
    """Node values, sums and pre-activations, [n_nodes][N] each, in the render's operation order.  math: "det" (oracle.detmath64) or
    "np" (numpy's libm)."""
    exp, tanh, sin = (dm.det_exp, dm.det_tanh, dm.det_sin) if math == "det" else (np.exp, np.tanh, np.sin)
    sig = dm.det_sigmoid if math == "det" else (lambda z: 1.0 / (1.0 + np.exp(-z)))
    N, nn = leaves[0].shape[0], len(flat["act"])
    vals, sums, zs = np.zeros((nn, N)), np.zeros((nn, N)), np.zeros((nn, N))
    with np.errstate(all="ignore"):
        for n in range(nn):
            s = None
            for k in range(flat["edge_off"][n], flat["edge_off"][n + 1]):
                src = int(flat["edge_src"][k])
                x = vals[src] if src >= 0 else _leaf(src, leaves, len(leaves))
                t = flat["edge_w"][k] * (np.ones(N) if x is None else x)
                s = t if s is None else s + t
            s = np.zeros(N) if s is None else s
            z = flat["resp"][n] * s + flat["bias"][n]
            a = int(flat["act"][n])
            y = (sig(5.0 * z) if a == 0 else tanh(2.5 * z) if a == 1 else np.abs(z) if a == 2 else exp(-5.0 * (z * z)) if a == 3 else z if a == 4
                 else sin(z) if a == 5 else np.where((z > 0) | np.isnan(z), z, 0.0))
            vals[n], sums[n], zs[n] = y, s, z
    return vals, sums, zs


def seed_mask(v, leaf0, quant=True, background=True):
    """the straight-through rule for one output plane v [N]; the two switches drop a part (the mutants of the host test)"""
    with np.errstate(invalid="ignore"):
        t = np.trunc(v * 255.0)
        m = np.ones(v.shape, bool)
        if quant:
            m &= (t >= 0.0) & (t <= 255.0)
        if background:
            m &= leaf0 != -1.0
    return m


def quantise(vals, flat, leaves, c_dim, bg=1):
    """the uint8 [c_dim][N] image of the gradient = 1 render from node values"""
    out = np.zeros((c_dim, leaves[0].shape[0]), np.uint8)
    for c in range(c_dim):
        v = np.where(leaves[0] == -1.0, float(bg), vals[int(flat["out_node"][c])])
        with np.errstate(invalid="ignore"):
            t = np.trunc(v * 255.0)
            out[c] = (np.where(np.abs(t) < 2147483648.0, t, 0.0).astype(np.int64) & 0xFF).astype(np.uint8)
    return out


# ---- statement (a)
def grads_autograd(flat, leaves, gimg, c_dim):
    """-> (g_w, g_bias, g_resp), values of the output nodes [c_dim][N] (float64 numpy)"""
    dt = torch.float64
    w = torch.tensor(np.asarray(flat["edge_w"], np.float64), dtype=dt, requires_grad=True)
    bias = torch.tensor(np.asarray(flat["bias"], np.float64), dtype=dt, requires_grad=True)
    resp = torch.tensor(np.asarray(flat["resp"], np.float64), dtype=dt, requires_grad=True)
    lv = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)) for p in leaves]
    N = lv[0].shape[0]
    vals = []
    for n in range(len(flat["act"])):
        s = None
        for k in range(int(flat["edge_off"][n]), int(flat["edge_off"][n + 1])):
            src = int(flat["edge_src"][k])
            x = vals[src] if src >= 0 else (lv[-src - 1] if -src - 1 < len(lv) else torch.ones(N, dtype=dt))
            t = w[k] * x
            s = t if s is None else s + t
        s = torch.zeros(N, dtype=dt) if s is None else s
        z = resp[n] * s + bias[n]
        a = int(flat["act"][n])
        vals.append(torch.sigmoid(5.0 * z) if a == 0 else torch.tanh(2.5 * z) if a == 1 else torch.abs(z) if a == 2 else torch.exp(-5.0 * (z * z)) if a == 3
                    else z if a == 4 else torch.sin(z) if a == 5 else torch.relu(z))
    loss = torch.zeros((), dtype=dt)
    outs = []
    for c in range(c_dim):
        v = vals[int(flat["out_node"][c])]
        outs.append(v.detach().numpy())
        m = torch.from_numpy(seed_mask(outs[-1], leaves[0]))
        loss = loss + (torch.from_numpy(np.asarray(gimg[c], np.float64)) * v * m).sum()
    g = torch.autograd.grad(loss, [w, bias, resp], allow_unused=True)
    z = lambda t, ref: np.zeros(ref.shape) if t is None else t.numpy()
    return (z(g[0], w), z(g[1], bias), z(g[2], resp)), np.stack(outs)


# ---- statement (b)
def grads_reverse(flat, leaves, gimg, c_dim, quant=True, background=True, resp_from_z=False, assign_fanout=False):
    """The kernel's reverse pass in numpy.  The four switches are the MUTANTS the host test needs to miss the bound: the
    quantisation mask dropped, the background mask dropped, g_resp formed from z instead of sum, and the fan-out accumulation
    (adj[src] += ...) replaced by assignment."""
    vals, sums, zs = forward_np(flat, leaves, "det")
    nn, N = vals.shape
    adj = np.zeros((nn, N))
    for c in range(c_dim):
        o = int(flat["out_node"][c])
        adj[o] += np.where(seed_mask(vals[o], leaves[0], quant, background), np.asarray(gimg[c], np.float64), 0.0)
    g_w, g_bias, g_resp = np.zeros(len(flat["edge_w"])), np.zeros(nn), np.zeros(nn)
    with np.errstate(all="ignore"):
        for n in reversed(range(nn)):
            y, z, s, a = vals[n], zs[n], sums[n], int(flat["act"][n])
            dact = ((5.0 * y) * (1.0 - y) if a == 0 else 2.5 * (1.0 - y * y) if a == 1 else np.sign(z) if a == 2 else (-10.0 * z) * y if a == 3
                    else np.ones(N) if a == 4 else np.cos(z) if a == 5 else (z > 0).astype(np.float64))
            d = adj[n] * dact
            g_bias[n] = d.sum()
            g_resp[n] = (d * (z if resp_from_z else s)).sum()
            ds = d * flat["resp"][n]
            for k in range(int(flat["edge_off"][n]), int(flat["edge_off"][n + 1])):
                src = int(flat["edge_src"][k])
                x = vals[src] if src >= 0 else _leaf(src, leaves, len(leaves))
                g_w[k] = ds.sum() if x is None else (ds * x).sum()
                if src >= 0:
                    adj[src] = ds * flat["edge_w"][k] if assign_fanout else adj[src] + ds * flat["edge_w"][k]
    return g_w, g_bias, g_resp


def masked_objective(flat, leaves, gimg, c_dim, masks):
    """sum gimg * v * mask in float64 with numpy's transcendentals, the masks held fixed: what the central differences perturb"""
    vals, _, _ = forward_np(flat, leaves, "np")
    return float(sum((np.asarray(gimg[c], np.float64) * vals[int(flat["out_node"][c])] * masks[c]).sum() for c in range(c_dim)))


# ---- grids, image gradients, genomes
def plain_grid(w, h, n_leaves=2):
    """x, y on [-1, 1] scaled by 2.9 (no live x is exactly -1 at any width used), the four corners (x^2 + y^2 > 1.45 before scaling) background: plane 0 AND plane 1 are -1 there,
    as grids.create_grid leaves them.  n_leaves = 4 appends r and a constant 1 (fitness.leaf_planes)."""
    yy, xx = np.meshgrid(np.linspace(-1.0, 1.0, h), np.linspace(-1.0, 1.0, w), indexing="ij")
    bgm = (xx * xx + yy * yy) > 1.45
    x, y = np.where(bgm, -1.0, 2.9 * xx).reshape(-1), np.where(bgm, -1.0, 2.9 * yy).reshape(-1)
    assert bgm.any() and not bgm.all() and not (x[~bgm.reshape(-1)] == -1.0).any()
    if n_leaves == 2:
        return [x, y]
    return [x, y, np.sqrt(x * x + y * y), np.ones_like(x)]


def image_grad(seed, n, c_dim, N):
    """float32 [n, c_dim, N] from a seeded normal, of the size a mean over an image has"""
    return (np.random.default_rng(seed).normal(0.0, 1.0, (n, c_dim, N)) / N).astype(np.float32)


HIDDEN = (20, 6, 0)
CASE_SHAPES = ((12, 8), (20, 15))
CASES = [(seed, HIDDEN[seed % 3], w, h) for (w, h) in CASE_SHAPES for seed in range(12)]   # 24


@functools.lru_cache(maxsize=None)
def case(seed, hidden, w, h, c_dim=3):
    """(flat, leaves, gimg [c_dim][N]) of one case, made once (read-only by convention)"""
    cfg = synth.make_config(2, 3)
    flat = flatten_genome(synth.make_genome(seed + 1, cfg, seed, num_hidden=hidden), cfg)
    leaves = plain_grid(w, h)
    return flat, leaves, image_grad(1000 + seed, 1, c_dim, w * h)[0]


@functools.lru_cache(maxsize=None)
def case_reference(seed, hidden, w, h, c_dim=3):
    flat, leaves, gimg = case(seed, hidden, w, h, c_dim)
    return grads_autograd(flat, leaves, gimg, c_dim)


def build_genome(key, nodes, conns):
    """nodes: {key: (activation, bias, response)}; conns: [(i, o, weight, enabled)] in genome.connections order"""
    g = synth.Genome(key)
    for k, (act, bias, resp) in nodes.items():
        g.nodes[k] = synth.NodeGene(key=k, bias=float(bias), response=float(resp), activation=act, aggregation="sum")
    for i, o, w, en in conns:
        g.connections[(i, o)] = synth.ConnectionGene(key=(i, o), weight=float(w), enabled=bool(en))
    return g


def all_activations_genome(key=100, inputs=(-1, -2)):
    """All seven activations; node 3 feeds three consumers, 3 -> 4 -> 5 -> 7 is a hidden chain; responses other than 1; output 1 (tanh)
    goes negative and output 2 (identity) leaves [0, 1] on both sides, so the wrap of the quantisation is exercised."""
    x, y = inputs[0], inputs[1]
    nodes = {0: ("sigmoid", 0.1, 1.0), 1: ("tanh", -0.2, 0.7), 2: ("identity", 0.45, 1.3),
             3: ("sin", 0.3, 1.1), 4: ("gauss", 0.05, 0.6), 5: ("abs", -0.4, 1.0), 6: ("relu", 0.2, 0.9), 7: ("identity", 0.0, 0.5)}
    conns = [(x, 3, 0.9, True), (y, 3, -0.7, True), (x, 4, 0.35, True), (3, 4, 0.5, True), (y, 5, 0.6, True), (4, 5, -1.2, True),
             (3, 6, 0.8, True), (x, 6, -0.5, True), (5, 7, 1.1, True), (6, 7, -0.9, True), (7, 0, 0.6, True), (3, 0, 0.4, True),
             (7, 1, 0.5, True), (4, 1, -0.8, True), (6, 2, 0.45, True), (y, 2, 0.12, True)]
    return build_genome(key, nodes, conns)


def folding_genome(key=101, inputs=(-1, -2)):
    """Everything the flattener folds: node 10 has no inputs (a float32 constant), node 11 reads 10 alone (a folded sub-graph), node 3
    starts with a leading constant run (10, 11), then x, then the constant 10 again behind a live term; output 1 reads constants only
    (a constant output: an identity node is synthesised); (x, 2) is disabled.  The expected map is EXPECTED_FOLDING_MAP."""
    x, y = inputs[0], inputs[1]
    nodes = {0: ("sigmoid", 0.0, 1.0), 1: ("tanh", 0.1, 1.0), 2: ("tanh", -0.1, 0.8), 3: ("sin", 0.2, 1.2),
             10: ("identity", 0.7, 1.0), 11: ("tanh", 0.05, 1.0), 12: ("sigmoid", 0.3, 1.0)}
    conns = [(10, 11, 0.6, True), (10, 3, 0.5, True), (11, 3, -0.4, True), (x, 3, 0.8, True), (12, 3, 0.3, True), (10, 12, 0.25, True), (y, 12, -0.6, True),
             (3, 0, 0.9, True), (y, 0, 0.3, True), (11, 1, 0.55, True), (x, 2, 0.5, False), (3, 2, 0.4, True), (10, 2, 0.3, True)]
    return build_genome(key, nodes, conns)


# flat order: depth-first post-order from output 0: 12 (reads 10: folded edge, then y), 3, 0; output 1 is constant (synthesised last); 2
EXPECTED_FOLDING_MAP = dict(
    node_key=[12, 3, 0, 2, None],
    edge_key=[None, (-2, 12),                       # node 12: the leading run (10), y
              None, (-1, 3), (12, 3),               # node 3: the leading run (10, 11) as one edge, x, node 12
              (3, 0), (-2, 0),                      # output 0
              (3, 2), None,                         # output 2: node 3, then the constant 10 behind a live term; (x, 2) is disabled
              None])                                # the identity node of the constant output 1


# ---- the setting of the refinement tests, host (simulated) and GPU: 16 x 12 colour, structure 1 (104 of 192 pixels are background)
SIM = dict(w=16, h=12, ch=(3, 4, 6), structure=1, n_repeat=4, n_ext=2, iters=8, lr=0.02)


def sim_genomes():
    cfg = synth.make_config(2, 3)
    return cfg, [synth.make_genome(s + 1, cfg, s, num_hidden=(20, 6)[s % 2]) for s in range(4)]
