"""Shared by tests/test_moving_host.py and tests/test_gpu_moving.py: the cases of the moving-texture render (csrc/cppn_motion_kernel.h,
eigen_render_moving_cppn; DESIGN.md section 13, "Moving textures") and ``moving_ref``, its numpy restatement, operation for operation,
over oracle.cppn.render_planes and oracle.cppn.to_u8 (not postprocess: its x == -1 mask does not apply here).  numpy only, no GPU.

A case is a dict as ``train.MovingTextures.describe`` returns one: w, h, c_dim, n, T, L, genomes (n * L, sample-major), config, gb,
affine / affine_inv [n, T, L, 6], motion [n, L, 4] = (shift x, shift y, turn, zoom) per layer.

  "8x8"    8 x 8 gray, T 2, one sample, one layer: N = 64, less than one block of 128
  "16x12"  16 x 12 gray, T 3, three samples of different node counts (the LDS carve depends on them), one layer: N = 192, the second
           block half empty.  Motions: identity; the exact binary shift (0.25, -0.125) on a power-of-two texture scale, so that every
           coordinate is exact; a turn with a zoom
  "20x15"  20 x 15 colour (half-integer pixel centres), T 4, two samples of two layers moving against each other; in sample 1 the disc
           is cut by the right border in frames 0 .. 2 and has left the image in frame 3, which is all layer 0
  "44x36"  44 x 36 colour, T 2, one sample of two layers; layer 1 is the 68-node genome "n68a" of tests/cppn_edge_support.py, whose
           columns need more than 64 KB of LDS: the dynamic-LDS attribute of the launch"""
import functools

import numpy as np

from evolutionary_illusion_generator_amd import synth
from evolutionary_illusion_generator_amd.genome import flatten_genome
from evolutionary_illusion_generator_amd.train import flat_genome_batch, similarity_affines

CASES = ("8x8", "16x12", "20x15", "44x36")
IDENTITY_SAMPLE = ("16x12", 0)       # (case, sample) whose motion is the identity: its frames are equal, every other pair differs
SHIFT_SAMPLE = ("16x12", 1)          # the exact binary shift
SHIFT = (0.25, -0.125)
EXIT_SAMPLE = ("20x15", 1)           # the disc has left the image in the last frame
RENDER_THREADS = 128                 # csrc/cppn_kernel.h: CPPN_THREADS


def _unit(angle):
    return complex(np.cos(angle), np.sin(angle))


def _layer0(scale, angle, offset, shift, turn=0.0, zoom=1.0):
    """(c, o, m, d) of ``similarity_affines`` for a texture under the whole image: `scale` texture units per pixel"""
    return scale * _unit(angle), complex(*offset), zoom * _unit(turn), complex(*shift)


def _disc(radius, centre, angle, shift, turn=0.0, zoom=1.0):
    """... for a disc of `radius` pixels about the pixel-centre coordinate `centre` in frame 0"""
    c = _unit(angle) / radius
    return c, -c * complex(*centre), zoom * _unit(turn), complex(*shift)


def _program_bytes(nn, ne):
    """csrc/cppn_motion_kernel.h: cppn_program_bytes"""
    b = 32 + nn * 16 + ne * 8 + (nn + 1) * 4 + ne * 4 + nn
    return (b + 7) & ~7


def motion_lds(case):
    """csrc/eigen_engine.hip, eigen_render_moving_cppn: the LDS of the launch, the largest over the samples of the columns of the larger
    program beside both programs"""
    gb, L, need = case["gb"], case["L"], 0
    for b in range(case["n"]):
        nn = [int(gb.node_off[g + 1] - gb.node_off[g]) for g in range(b * L, (b + 1) * L)]
        ne = [int(gb.edge_off[gb.node_off[g + 1]] - gb.edge_off[gb.node_off[g]]) for g in range(b * L, (b + 1) * L)]
        need = max(need, max(nn) * RENDER_THREADS * 8 + sum(_program_bytes(a, e) for a, e in zip(nn, ne)))
    return need


def build_case(w, h, c_dim, T, genomes, layers, L):
    """genomes: n * L synth genomes; layers: their (c, o, m, d)"""
    cfg = synth.make_config(2, c_dim)
    n = len(genomes) // L
    affine, affine_inv, motion = np.zeros((n, T, L, 6)), np.zeros((n, T, L, 6)), np.zeros((n, L, 4))
    for i, (c, o, m, d) in enumerate(layers):
        affine[i // L, :, i % L], affine_inv[i // L, :, i % L] = similarity_affines(c, o, m, d, T)
        motion[i // L, i % L] = (d.real, d.imag, np.arctan2(m.imag, m.real), abs(m))
    gb = flat_genome_batch([flatten_genome(g, cfg) for g in genomes], c_dim)
    for a in (affine, affine_inv, motion):
        a.setflags(write=False)
    return dict(w=w, h=h, c_dim=c_dim, n=n, T=T, L=L, genomes=list(genomes), config=cfg, gb=gb, affine=affine, affine_inv=affine_inv, motion=motion)


def _genome(c_dim, seed, num_hidden=20):
    return synth.make_genome(seed + 1, synth.make_config(2, c_dim), seed, num_hidden=num_hidden)


# the genome seeds were picked so that the liveness rules of tests/test_moving_host.py hold for moving_ref (it asserts them)
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "8x8":
        return build_case(8, 8, 1, 2, [_genome(1, 2)], [_layer0(0.3, 0.4, (0.1, -0.2), (0.7, -0.4), turn=0.01)], 1)
    if name == "16x12":
        genomes = [_genome(1, 11, 5), _genome(1, 76, 20), _genome(1, 13, 40)]
        layers = [_layer0(0.2, 0.3, (0.2, 0.1), (0.0, 0.0)),
                  (complex(0.125, 0.0), complex(0.5, -0.25), complex(1.0, 0.0), complex(*SHIFT)),
                  _layer0(0.2, 1.1, (-0.3, 0.2), (0.0, 0.0), turn=0.05, zoom=1.03)]
        return build_case(16, 12, 1, 3, genomes, layers, 1)
    if name == "20x15":
        genomes = [_genome(3, 21), _genome(3, 22), _genome(3, 23), _genome(3, 24)]
        layers = [_layer0(0.15, 0.2, (0.3, 0.1), (0.8, 0.3), turn=0.02), _disc(5.05, (-2.03, 1.02), 0.7, (-0.9, -0.4), zoom=1.02),
                  _layer0(0.15, 2.0, (-0.2, 0.4), (-0.6, 0.5)), _disc(6.1, (4.03, 0.02), 1.3, (4.0, 0.0))]
        return build_case(20, 15, 3, 4, genomes, layers, 2)
    if name == "44x36":
        from tests import cppn_edge_support as ce
        genomes = [_genome(3, 31), ce.big_genome("n68a")]
        layers = [_layer0(0.07, 0.5, (0.1, 0.2), (1.1, -0.6), turn=0.01), _disc(11.03, (3.02, -2.01), 0.9, (-1.2, 0.7), turn=-0.03)]
        c = build_case(44, 36, 3, 2, genomes, layers, 2)
        assert motion_lds(c) > 64 * 1024, motion_lds(c)
        return c
    raise KeyError(name)


def pixel_centres(w, h):
    """(px, py), float64 [h * w] in row-major pixel order: col - (w - 1) / 2 and row - (h - 1) / 2, exact"""
    rows, cols = np.divmod(np.arange(h * w), w)
    return cols.astype(np.float64) - (w - 1) / 2.0, rows.astype(np.float64) - (h - 1) / 2.0


def texture_coords(a, px, py):
    """u = (a0 px + a1 py) + a2, v = (a3 px + a4 py) + a5: every product and sum one float64 rounding, in this order"""
    return (a[0] * px + a[1] * py) + a[2], (a[3] * px + a[4] * py) + a[5]


def moving_ref(desc, flow=True):
    """dict(frames uint8 [n, T, C, h, w], flow float64 [n, T - 1, 2, h, w] (None without flow or with T = 1), layer uint8 [n, T, h, w],
    r2 float64 [n, T, h, w]: u1^2 + v1^2 of layer 1, inf with one layer, u / v float64 [n, T, h, w]: the visible layer's coordinates)"""
    from oracle import cppn
    w, h, C, n, T, L = (desc[k] for k in ("w", "h", "c_dim", "n", "T", "L"))
    px, py = pixel_centres(w, h)
    frames, layer = np.zeros((n, T, C, h * w), np.uint8), np.zeros((n, T, h * w), np.uint8)
    r2, us, vs = np.full((n, T, h * w), np.inf), np.zeros((n, T, h * w)), np.zeros((n, T, h * w))
    fl = np.zeros((n, T - 1, 2, h * w)) if flow and T > 1 else None
    for b in range(n):
        for t in range(T):
            u, v = texture_coords(desc["affine"][b, t, 0], px, py)
            vis = np.zeros(h * w, bool)
            coords = [(u, v)]
            if L == 2:
                u1, v1 = texture_coords(desc["affine"][b, t, 1], px, py)
                r2[b, t] = u1 * u1 + v1 * v1
                vis = r2[b, t] < 1.0
                coords.append((u1, v1))
                u, v = np.where(vis, u1, u), np.where(vis, v1, v)
            for l in range(L):
                planes = cppn.render_planes(desc["genomes"][b * L + l], desc["config"], [coords[l][0], coords[l][1]])
                for c in range(C):
                    byte = cppn.to_u8(np.asarray(planes[c], np.float64) * 255.0)
                    frames[b, t, c] = np.where(vis == bool(l), byte, frames[b, t, c])
            layer[b, t], us[b, t], vs[b, t] = vis, u, v
            if fl is not None and t < T - 1:
                inv = desc["affine_inv"][b, t + 1]
                i = [np.where(vis, inv[L - 1][k], inv[0][k]) for k in range(6)]
                fl[b, t, 0] = ((i[0] * u + i[1] * v) + i[2]) - px
                fl[b, t, 1] = ((i[3] * u + i[4] * v) + i[5]) - py
    out = dict(frames=frames.reshape(n, T, C, h, w), layer=layer.reshape(n, T, h, w), r2=r2.reshape(n, T, h, w), u=us.reshape(n, T, h, w),
               v=vs.reshape(n, T, h, w), flow=None if fl is None else fl.reshape(n, T - 1, 2, h, w))
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """moving_ref of case(name), made once and read-only"""
    return moving_ref(case(name))


def sub_case(desc, samples=None, frames=None):
    """samples [lo, hi) and / or frames [lo, hi) of a case as a case of their own"""
    L = desc["L"]
    s0, s1 = samples or (0, desc["n"])
    t0, t1 = frames or (0, desc["T"])
    out = dict(desc, n=s1 - s0, T=t1 - t0, genomes=desc["genomes"][s0 * L:s1 * L], gb=desc["gb"].slice(s0 * L, s1 * L),
               affine=np.ascontiguousarray(desc["affine"][s0:s1, t0:t1]), affine_inv=np.ascontiguousarray(desc["affine_inv"][s0:s1, t0:t1]),
               motion=desc["motion"][s0:s1])
    return out
