"""Moving CPPN textures on the GPU (eigen_render_moving_cppn, Engine.render_moving_cppn, train.MovingTextures; DESIGN.md section 13,
"Moving textures") against ``tests.moving_support.moving_ref``, the numpy restatement: frames, flow and layer map bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionary_illusion_generator_amd.engine import Engine
from evolutionary_illusion_generator_amd.train import MovingTextures, PredNetTrainer
from tests import moving_support as ms

pytestmark = pytest.mark.gpu


def _engine(c, max_batch=1):
    return Engine(c["w"], c["h"], [c["c_dim"]], max_batch)


def _render(e, c, flow=True, layer=True, out=None):
    frames, fl, lay = e.render_moving_cppn(c["gb"], c["affine"], c["affine_inv"] if flow else None, flow=flow, layer=layer, out=out)
    torch.cuda.synchronize()
    return frames.cpu().numpy(), None if fl is None else fl.cpu().numpy(), None if lay is None else lay.cpu().numpy()


@pytest.mark.parametrize("name", ms.CASES)
def test_frames_flow_and_layer_map_are_the_restatement_bit_for_bit(cuda, name):
    c, r = ms.case(name), ms.reference(name)
    e = _engine(c)
    try:
        frames, fl, lay = _render(e, c)
        assert np.array_equal(frames, r["frames"]), (name, int((frames != r["frames"]).sum()))
        assert np.array_equal(lay, r["layer"]), name
        assert np.array_equal(fl, r["flow"]), (name, float(np.abs(fl - r["flow"]).max()))
        # outputs that are not asked for are not written, and the frames do not depend on them
        alone, no_flow, no_layer = _render(e, c, flow=False, layer=False)
        assert no_flow is None and no_layer is None and np.array_equal(alone, r["frames"])
        only_layer = _render(e, c, flow=False, layer=True)
        assert np.array_equal(only_layer[0], r["frames"]) and only_layer[1] is None and np.array_equal(only_layer[2], r["layer"])
        only_flow = _render(e, c, flow=True, layer=False)
        assert np.array_equal(only_flow[0], r["frames"]) and np.array_equal(only_flow[1], r["flow"]) and only_flow[2] is None
    finally:
        e.close()


def test_identity_motion_is_the_still_render_on_the_same_coordinates(cuda):
    name, b = ms.IDENTITY_SAMPLE
    c = ms.sub_case(ms.case(name), samples=(b, b + 1), frames=(0, 2))
    r = ms.moving_ref(c)
    u, v = r["u"][0, 0].ravel(), r["v"][0, 0].ravel()
    assert not (u == -1.0).any()                       # the still render would fill such a pixel with the background
    assert np.array_equal(r["u"][0, 0], r["u"][0, 1]) and np.array_equal(r["v"][0, 0], r["v"][0, 1])
    e = _engine(c)
    try:
        frames = _render(e, c, flow=False, layer=False)[0]
        e.set_grid([u, v])
        still = torch.zeros((1, c["c_dim"], c["h"], c["w"]), dtype=torch.uint8, device="cuda")
        e.render_cppn(c["gb"], still)
        torch.cuda.synchronize()
        still = still.cpu().numpy()[0]
        assert np.array_equal(frames[0, 0], still) and np.array_equal(frames[0, 1], still)
        # with a grid on the handle the moving render still reads its own coordinates
        assert np.array_equal(_render(e, c, flow=False, layer=False)[0], frames)
    finally:
        e.close()


def test_samples_and_frames_do_not_depend_on_the_call_they_are_in(cuda):
    c, r = ms.case("16x12"), ms.reference("16x12")
    e = _engine(c)
    try:
        for lo, hi in ((0, 2), (2, 3)):
            frames, fl, lay = _render(e, ms.sub_case(c, samples=(lo, hi)))
            assert np.array_equal(frames, r["frames"][lo:hi]) and np.array_equal(fl, r["flow"][lo:hi]) and np.array_equal(lay, r["layer"][lo:hi])
    finally:
        e.close()
    c, r = ms.case("20x15"), ms.reference("20x15")
    e = _engine(c)
    try:
        frames, fl, lay = _render(e, ms.sub_case(c, frames=(1, 3)))
        assert np.array_equal(frames, r["frames"][:, 1:3]) and np.array_equal(lay, r["layer"][:, 1:3])
        assert fl.shape[1] == 1 and np.array_equal(fl[:, 0], r["flow"][:, 1])
    finally:
        e.close()


def test_a_stride_between_samples_keeps_the_gap(cuda):
    c, r = ms.case("16x12"), ms.reference("16x12")
    seq = c["T"] * c["c_dim"] * c["h"] * c["w"]
    buf = torch.full((c["n"], seq + 37), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:, :seq].view(c["n"], c["T"], c["c_dim"], c["h"], c["w"])
    assert out.stride(0) == seq + 37
    e = _engine(c)
    try:
        frames = _render(e, c, flow=False, layer=False, out=out)[0]
    finally:
        e.close()
    assert np.array_equal(frames, r["frames"])
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :seq].reshape(r["frames"].shape), r["frames"]) and (host[:, seq:] == 0xA5).all()


def _raw(e, gb, n, T, L, affine, inv, frames, bstride, flow=None, layer=None, handle=True, batch=True):
    """eigen_render_moving_cppn itself: -> its return code"""
    s = Engine._genome_struct(gb)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
    return e.lib.eigen_render_moving_cppn(e._h if handle else None, ctypes.byref(s) if batch else None, ctypes.c_int32(n), ctypes.c_int32(T), ctypes.c_int32(L), p(affine),
                                          p(inv), p(frames), ctypes.c_int64(bstride), p(flow), p(layer), None)


def _with(gb, **arrays):
    out = gb._from_arrays(gb.n_genomes, gb.c_out, [getattr(gb, n) for n, _ in gb._FIELDS])
    for k, v in arrays.items():
        setattr(out, k, np.ascontiguousarray(v, dtype=getattr(gb, k).dtype))
    return out


def test_every_refusal_and_the_handle_renders_afterwards(cuda):
    from tests import cppn_edge_support as ce
    c, r = ms.case("20x15"), ms.reference("20x15")
    n, T, L, C, h, w = c["n"], c["T"], c["L"], c["c_dim"], c["h"], c["w"]
    seq = T * C * h * w
    A, I, gb = np.ascontiguousarray(c["affine"]), np.ascontiguousarray(c["affine_inv"]), c["gb"]
    frames = torch.full((n, seq), 0x5A, dtype=torch.uint8, device="cuda")
    flow = torch.full((n, T - 1, 2, h, w), -7.0, dtype=torch.float64, device="cuda")
    layer = torch.full((n, T, h, w), 9, dtype=torch.uint8, device="cuda")
    INVALID, CAPACITY = -1, -4
    later = gb.edge_src.copy()
    k0 = int(gb.edge_off[gb.node_off[1]])                     # the first edge of genome 1's first node
    later[k0] = 1000                                          # ... reads a node that is not topologically earlier
    leaf = gb.edge_src.copy()
    leaf[k0] = -4                                             # beyond x, y and the constant
    outs = gb.out_node.copy()
    outs[C] = int(gb.node_off[2] - gb.node_off[1])            # one past genome 1's last node
    empty = gb.node_off.copy()
    empty[1] = empty[0]                                       # genome 0 has no nodes
    one = ms.case("16x12")                                    # gray genomes: c_out 1 < c_dim 3
    big = ce.big_flat(ce.REFUSED)
    from evolutionary_illusion_generator_amd.train import flat_genome_batch
    big_gb = flat_genome_batch([big], 3)
    e = _engine(c)
    try:
        ok = dict(e=e, gb=gb, n=n, T=T, L=L, affine=A, inv=I, frames=frames, bstride=seq, flow=flow, layer=layer)
        refused = [("handle", dict(handle=False), INVALID), ("batch", dict(batch=False), INVALID), ("affine", dict(affine=None), INVALID),
                   ("frames", dict(frames=None), INVALID), ("layers 0", dict(L=0), INVALID), ("layers 3", dict(L=3), INVALID),
                   ("no frame", dict(T=0), INVALID), ("no sample", dict(n=0), INVALID), ("flow of one frame", dict(T=1), INVALID),
                   ("flow without inverse", dict(inv=None), INVALID), ("inverse without flow", dict(flow=None), INVALID),
                   ("genome count", dict(n=n + 1), INVALID), ("genome count by layers", dict(L=1), INVALID),
                   ("outputs", dict(gb=one["gb"], n=one["n"], L=1), INVALID), ("stride", dict(bstride=seq - 1), INVALID),
                   ("later node", dict(gb=_with(gb, edge_src=later)), INVALID), ("leaf", dict(gb=_with(gb, edge_src=leaf)), INVALID),
                   ("output node", dict(gb=_with(gb, out_node=outs)), INVALID), ("empty genome", dict(gb=_with(gb, node_off=empty)), INVALID),
                   ("samples of one launch", dict(n=65536), CAPACITY), ("LDS", dict(gb=big_gb, n=1, L=1, flow=None, inv=None, layer=None), CAPACITY)]
        for what, change, code in refused:
            assert _raw(**dict(ok, **change)) == code, what
            assert e.lib.eigen_last_error(), what
        torch.cuda.synchronize()
        assert (frames.cpu().numpy() == 0x5A).all() and (flow.cpu().numpy() == -7.0).all() and (layer.cpu().numpy() == 9).all()   # nothing was launched
        assert _raw(**ok) == 0
        torch.cuda.synchronize()
        assert np.array_equal(frames.cpu().numpy().reshape(r["frames"].shape), r["frames"])
        assert np.array_equal(flow.cpu().numpy(), r["flow"]) and np.array_equal(layer.cpu().numpy(), r["layer"])
    finally:
        e.close()


def test_python_refuses_what_the_pointers_cannot_show(cuda):
    c = ms.case("16x12")
    e = _engine(c)
    try:
        with pytest.raises(ValueError):
            e.render_moving_cppn(c["gb"], c["affine"], None, flow=True)
        with pytest.raises(ValueError):
            e.render_moving_cppn(c["gb"], c["affine"][:2])
        with pytest.raises(ValueError):
            e.render_moving_cppn(c["gb"], c["affine"], out=torch.zeros((c["n"], c["T"], 1, c["h"], c["w"] + 1), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            e.render_moving_cppn(c["gb"], c["affine"], out=torch.zeros((c["n"], c["T"], 1, c["h"], c["w"]), dtype=torch.uint8))
    finally:
        e.close()


def test_batches_repeat_and_feed_the_trainer_from_the_device(cuda):
    w, h, T, B = 32, 24, 6, 4
    with MovingTextures(w, h, 1, T, seed=3, layers=2) as a, MovingTextures(w, h, 1, T, seed=3, layers=2) as b, MovingTextures(w, h, 1, T, seed=4, layers=2) as other:
        first, again, twin = a.batch(5, B), a.batch(5, B), b.batch(5, B)
        assert first.is_cuda and first.dtype == torch.uint8 and tuple(first.shape) == (B, T, 1, h, w)
        assert torch.equal(first, again) and torch.equal(first, twin)
        assert not torch.equal(first, a.batch(6, B)) and not torch.equal(first, other.batch(5, B))
        frames, fl, lay = a.batch(5, B, flow=True)
        assert torch.equal(frames, first) and tuple(fl.shape) == (B, T - 1, 2, h, w) and tuple(lay.shape) == (B, T, h, w)
        d = a.describe(5, B)
        ref = ms.moving_ref(d)
        assert np.array_equal(first.cpu().numpy(), ref["frames"]) and np.array_equal(fl.cpu().numpy(), ref["flow"]) and np.array_equal(lay.cpu().numpy(), ref["layer"])
        with PredNetTrainer("synthetic:0", [1, 8, 16], w, h, B, T) as tr:
            on_device = tr.step(first)
        with PredNetTrainer("synthetic:0", [1, 8, 16], w, h, B, T) as tr:
            from_host = tr.step(first.cpu().numpy())
        assert np.isfinite(on_device) and abs(on_device - from_host) <= 1e-6 * abs(from_host)     # the same frames, whichever side they come from
    # an engine of the caller's is used and left open
    e = Engine(w, h, [1], 1)
    try:
        with MovingTextures(w, h, 1, T, seed=3, layers=2, engine=e) as shared:
            assert torch.equal(shared.batch(5, B), first)
        assert e._h.value
    finally:
        e.close()


# held-out loss before -> after 200 Adam steps, as the first run of this test on an MI355X printed them; the assertion asks for half
# of the measured reduction, the margin of tests/test_gpu_train.py::test_adam_steps_on_drifting_patterns_cut_the_held_out_loss
MEASURED_TRAINING = {1: (0.044239, 0.028870), 2: (0.061125, 0.043402)}     # 34.7 % and 29.0 % lower: 17.4 % and 14.5 % are asked for


@pytest.mark.parametrize("layers", [1, 2])
def test_adam_steps_on_moving_textures_cut_the_held_out_loss(cuda, layers):
    """The setup of the drifting-pattern test: 32x24 gray, [1, 8, 16], B = 4, T = 6, 200 Adam steps at alpha 3e-3, held-out batch 10**6."""
    w, h, ch = 32, 24, [1, 8, 16]
    B, T = 4, 6
    with MovingTextures(w, h, 1, T, seed=0, layers=layers) as src, PredNetTrainer("synthetic:0", ch, w, h, B, T, alpha=3e-3) as tr:
        held = src.batch(10 ** 6, B)
        before = tr.forward_backward(held)
        for i in range(200):
            tr.step(src.batch(i, B))
        after = tr.forward_backward(held)
    print("layers %d: held-out loss %.6f -> %.6f (%.1f %% lower)" % (layers, before, after, 100 * (1 - after / before)))
    m_before, m_after = MEASURED_TRAINING[layers]
    assert after < before, (before, after)
    assert after <= (1 - 0.5 * (1 - m_after / m_before)) * before, (before, after)
