"""PredNet over sequences of different frames (eigen_prednet_sequence, fitness.prednet_sequence_predictions / PredNetStream /
sequence_flow).

The bit-exact bar comes from the CPU oracle's constant-image roll-out: with requant=True every extension step of it is fed the
previous uint8 prediction with the arithmetic of an input image (oracle/eig_oracle.c), so the sequence
[img] * R + [F[R-1], ..., F[R+E-2]] -- different frames at every extension step -- must reproduce the oracle's frames F byte for byte.
"""
import ctypes

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import fitness, weights
from evolutionary_illusion_generator_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

EIGEN_ERR_INVALID, EIGEN_ERR_STATE, EIGEN_ERR_CAPACITY = -1, -3, -4


def _textures(seed, n, c, h, w):
    """n smooth uint8 [c, h, w] textures."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, c, h, w), np.uint8)
    for i in range(n):
        for ch in range(c):
            v = np.zeros((h, w))
            for _ in range(4):
                fy, fx, ph = rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4), rng.uniform(0, 2 * np.pi)
                v += np.sin(fy * yy + fx * xx + ph)
            out[i, ch] = np.clip(128 + 30 * v, 0, 255).astype(np.uint8)
    return out


def _drifting(seed, n, T, c, h, w):
    """n sequences of T frames: a texture shifted by one pixel per frame (each sequence its own direction)."""
    base = _textures(seed, n, c, h + 2 * T, w + 2 * T)
    out = np.zeros((n, T, c, h, w), np.uint8)
    for i in range(n):
        dy, dx = [(1, 0), (0, 1), (1, 1), (-1, 1)][i % 4]
        for t in range(T):
            y0, x0 = T + dy * t, T + dx * t
            out[i, t] = base[i, :, y0:y0 + h, x0:x0 + w]
    return out


def _engine(w, h, ch, B, seed=4, **kw):
    e = Engine(w, h, ch, B, **kw)
    wts = weights.synthetic_prednet_weights(ch, w, h, seed=seed)
    e.set_weights(wts)
    return e, wts


def _sequence(e, cuda, frames, n_ext=0, reset=True, first_out_step=0, pad=0):
    """frames uint8 [B, T, C, H, W] (numpy) -> predictions [B, T + n_ext - first_out_step, C, H, W]; pad > 0 places the
    sequences pad frames apart (a batch stride that is not T frames)."""
    import torch
    B, T = frames.shape[:2]
    buf = np.zeros((B, T + pad) + frames.shape[2:], np.uint8)
    buf[:, :T] = frames
    d = torch.from_numpy(buf).to(cuda)
    out = torch.zeros((B, T + n_ext - first_out_step) + frames.shape[2:], dtype=torch.uint8, device=cuda)
    e.prednet_sequence(d, buf[0].size, B, T, n_ext, reset, first_out_step, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("w,h,ch", [(64, 64, [1, 16, 32, 64]), (48, 32, [3, 8, 16, 32]), (20, 12, [1, 4, 8]),
                                    (160, 120, [1, 8, 12, 8]), (160, 128, [1, 4, 8, 8, 8])])
def test_changing_frames_bit_exact_against_oracle(cuda, oracle_lib, w, h, ch):
    R, E, B = 4, 3, 3
    imgs = _textures(w * h + len(ch), B, ch[0], h, w)
    e, wts = _engine(w, h, ch, B)
    F = np.stack([oracle_lib.prednet_rollout(wts, ch, w, h, imgs[i], n_repeat=R, n_ext=E, requant=True) for i in range(B)])
    seq = np.concatenate([np.repeat(imgs[:, None], R, axis=1), F[:, R - 1:R + E - 1]], axis=1)   # a different frame at every extension step
    assert not np.array_equal(seq[:, R], seq[:, R + 1])
    got = _sequence(e, cuda, seq, pad=2)
    for i in range(B):
        for t in range(R + E):
            assert np.array_equal(got[i, t], F[i, t]), "sequence %d step %d: %d bytes differ" % (i, t, (got[i, t] != F[i, t]).sum())
    assert np.array_equal(_sequence(e, cuda, seq, first_out_step=R + 1), F[:, R + 1:])


def test_constant_image_sequence_is_the_rollout(cuda, oracle_lib):
    import torch
    w, h, ch, B = 48, 32, [3, 8, 16, 32], 2
    imgs = _textures(5, B, 3, h, w)
    e, wts = _engine(w, h, ch, B)
    seq = _sequence(e, cuda, np.repeat(imgs[:, None], 20, axis=1), n_ext=2)
    fr = torch.zeros((B, 22, 3, h, w), dtype=torch.uint8, device=cuda)
    e.prednet_rollout(torch.from_numpy(imgs).to(cuda), B, 22, 0, fr)
    torch.cuda.synchronize()
    assert np.array_equal(seq, fr.cpu().numpy())
    for i in range(B):
        assert np.array_equal(seq[i], oracle_lib.prednet_rollout(wts, ch, w, h, imgs[i], n_repeat=20, n_ext=2))


# 64 x 64, batch 2: layer 1 is 2 x 32 x 32 pixels, the ConvP_l run on the side stream; 256 x 256 colour, batch 8: 8 x 128 x 128 >= 512 x CUs pixels, one stream
@pytest.mark.parametrize("w,h,ch,B,requant", [(64, 64, [1, 16, 32, 64], 2, False), (64, 64, [1, 16, 32, 64], 2, True),
                                              (256, 256, [3, 16, 32, 64], 8, False)])
def test_split_sequence_is_one_call(cuda, w, h, ch, B, requant):
    T, n_ext = 12, 2
    frames = _drifting(w + B, B, T, ch[0], h, w)
    e, _ = _engine(w, h, ch, B, requant_feedback=requant)
    whole = _sequence(e, cuda, frames, n_ext=n_ext)
    parts = [_sequence(e, cuda, frames[:, :1]), _sequence(e, cuda, frames[:, 1:8], reset=False),
             _sequence(e, cuda, frames[:, 8:], reset=False)]
    import torch
    ext = torch.zeros((B, n_ext, ch[0], h, w), dtype=torch.uint8, device=cuda)
    e.prednet_sequence(None, 0, B, 0, n_ext, False, 0, ext)
    torch.cuda.synchronize()
    parts.append(ext.cpu().numpy())
    pieces = np.concatenate(parts, axis=1)
    assert pieces.shape == whole.shape
    for t in range(T + n_ext):
        assert np.array_equal(pieces[:, t], whole[:, t]), "step %d: %d bytes differ" % (t, (pieces[:, t] != whole[:, t]).sum())
    assert not np.array_equal(whole[:, T - 1], whole[:, T - 2])


def test_sequences_in_a_batch_are_independent(cuda):
    w, h, ch, B, T = 48, 32, [3, 8, 16, 32], 3, 6
    frames = _drifting(9, B, T, 3, h, w)
    e, _ = _engine(w, h, ch, B)
    together = _sequence(e, cuda, frames, n_ext=2)
    for i in range(B):
        assert np.array_equal(_sequence(e, cuda, frames[i:i + 1], n_ext=2)[0], together[i])
    assert not np.array_equal(together[0], together[1])


def _raw_sequence(e, d_in, batch, n_in, n_ext, reset, first, d_out):
    lib = e.lib
    return lib.eigen_prednet_sequence(e._h, None if d_in is None else ctypes.c_void_p(d_in.data_ptr()), ctypes.c_int64(n_in * e.c_dim * e.height * e.width),
                                      ctypes.c_int32(batch), ctypes.c_int32(n_in), ctypes.c_int32(n_ext), ctypes.c_int32(reset),
                                      ctypes.c_int32(first), None if d_out is None else ctypes.c_void_p(d_out.data_ptr()), None)


def test_state_rules_and_errors(cuda):
    import torch
    w, h, ch, B = 32, 32, [1, 4, 8], 3
    e, _ = _engine(w, h, ch, B)
    err = lambda: e.lib.eigen_last_error().decode()
    d_in = torch.from_numpy(_drifting(2, B, 4, 1, h, w)).to(cuda)
    d_out = torch.zeros((B, 6, 1, h, w), dtype=torch.uint8, device=cuda)
    # nothing kept yet
    assert _raw_sequence(e, d_in, B, 2, 0, 0, 0, d_out) == EIGEN_ERR_STATE and "reset = 0" in err()
    assert _raw_sequence(e, d_in, B, 2, 0, 1, 0, d_out) == 0
    assert _raw_sequence(e, d_in, B, 2, 1, 0, 0, d_out) == 0                  # continues
    assert _raw_sequence(e, d_in, 2, 2, 0, 0, 0, d_out) == EIGEN_ERR_STATE and "batch of 3" in err()
    # a roll-out / evaluation overwrites the layer state
    e.prednet_rollout(d_in, B, 3, 0, d_out)
    assert _raw_sequence(e, d_in, B, 2, 0, 0, 0, d_out) == EIGEN_ERR_STATE
    assert _raw_sequence(e, d_in, B, 2, 0, 1, 0, d_out) == 0
    e.eval_images(d_in, B, 2)
    assert _raw_sequence(e, d_in, B, 2, 0, 0, 0, d_out) == EIGEN_ERR_STATE
    # invalid arguments
    assert _raw_sequence(e, d_in, B, 0, 2, 1, 0, d_out) == EIGEN_ERR_INVALID and "at least one input frame" in err()
    assert _raw_sequence(e, None, B, 2, 0, 1, 0, d_out) == EIGEN_ERR_INVALID and "null" in err()
    assert _raw_sequence(e, d_in, B, 2, 0, 1, 0, None) == EIGEN_ERR_INVALID and "null" in err()
    assert _raw_sequence(e, d_in, B + 1, 2, 0, 1, 0, d_out) == EIGEN_ERR_CAPACITY and "max_batch" in err()
    assert _raw_sequence(e, d_in, B, 2, 1, 1, 3, d_out) == EIGEN_ERR_INVALID and "first_out_step" in err()
    assert _raw_sequence(e, d_in, B, 2, 1, 1, -1, d_out) == EIGEN_ERR_INVALID and "first_out_step" in err()
    # the Python wrapper refuses buffers the C side would overrun
    with pytest.raises(ValueError):
        e.prednet_sequence(d_in, 4 * h * w, B, 5, 0, True, 0, d_out)
    with pytest.raises(EngineError):
        e.prednet_sequence(d_in, 4 * h * w, B, 0, 1, True, 0, d_out)


def test_python_layer(cuda, monkeypatch):
    import torch
    w, h, ch, T = 64, 64, [1, 8, 16], 6
    model = "synthetic:3"
    frames = _drifting(21, 5, T, 1, h, w)
    monkeypatch.setenv("EIGEN_MAX_BATCH", "2")
    batched = fitness.prednet_sequence_predictions(frames, model, ch, w, h, n_ext=2)
    assert batched.shape == (5, T + 2, 1, h, w) and batched.dtype == np.uint8
    for i in range(5):
        assert np.array_equal(fitness.prednet_sequence_predictions(frames[i:i + 1], model, ch, w, h, n_ext=2)[0], batched[i])
    # a stream fed in pieces: the bytes of one call
    s = fitness.PredNetStream(model, ch, w, h, 2)
    try:
        got = np.concatenate([s.feed(frames[:2, :1]), s.feed(frames[:2, 1:4]), s.feed(frames[:2, 4:]), s.extend(2)], axis=1)
        assert np.array_equal(got, batched[:2])
        s.reset()
        one = s.feed(torch.from_numpy(frames[2:4]).to(cuda))              # CUDA tensors in, CUDA tensors out
        ext = s.extend(2)
        torch.cuda.synchronize()
        assert isinstance(one, torch.Tensor) and np.array_equal(torch.cat([one, ext], 1).cpu().numpy(), batched[2:4])
        s.reset()
        with pytest.raises(ValueError):
            s.extend(1)
        with pytest.raises(ValueError):
            s.feed(frames[:3])
    finally:
        s.close()
    # flow between consecutive frames of every sequence
    flows = fitness.sequence_flow(frames[:3])
    assert len(flows) == 3 and all(len(f) == T - 1 for f in flows)
    assert sum(len(v) for f in flows for v in f) > 0
    for i in range(3):
        for t in range(T - 1):
            assert np.array_equal(flows[i][t], fitness.flow_vectors(frames[i, t], frames[i, t + 1]))
