"""PredNet training on frame sequences (include/eigen_engine.h eigen_trainer_*).

Next-frame MSE of the float prediction, full backprop through time within a call, Adam as chainer defines it; every kernel is
HIP for gfx950 (csrc/prednet_train.hip), there is no CPU or PyTorch fallback.  The trained weights are a plain
``{name: float32 array}`` table, usable as ``model_name`` anywhere the fitness path takes one, and
``weights.save_chainer_npz`` writes them as a chainer npz file.
"""
import ctypes

import numpy as np

from . import engine
from .engine import EngineError, _check, _ptr, _stream_arg
from .weights import tensor_names, tensor_shapes


class TrainerConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("n_layers", ctypes.c_int32),
                ("channels", ctypes.c_int32 * engine.MAX_LAYERS), ("max_batch", ctypes.c_int32), ("max_steps", ctypes.c_int32)]


def _bind(lib):
    if getattr(lib, "_trainer_bound", False):
        return
    lib.eigen_trainer_loss_grad.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_void_p]
    lib.eigen_trainer_adam.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    lib.eigen_trainer_tape_bytes.restype = ctypes.c_int64
    lib.eigen_trainer_tape_bytes.argtypes = [ctypes.c_void_p]
    lib._trainer_bound = True


class PredNetTrainer:
    """One trainer handle on the current HIP device.  batch and max_steps size the tape (``tape_bytes``).

    model_name: anything ``fitness._resolve_weights`` takes (a weight dict, ``"synthetic[:seed]"`` or a chainer npz path): the
    starting weights.  alpha, beta1, beta2, eps: Adam (chainer's defaults)."""

    def __init__(self, model_name, channels, w, h, batch, max_steps, alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, device=None):
        import torch
        from .fitness import _local_device, _resolve_weights
        self.lib = engine.load_library()
        _bind(self.lib)
        self.channels, self.w, self.h = [int(c) for c in channels], int(w), int(h)
        self.batch, self.max_steps = int(batch), int(max_steps)
        self.alpha, self.beta1, self.beta2, self.eps = alpha, beta1, beta2, eps
        self.device = _local_device() if device is None else int(device)
        if len(self.channels) > engine.MAX_LAYERS:
            raise ValueError("at most %d layers" % engine.MAX_LAYERS)
        cfg = TrainerConfig()
        cfg.device, cfg.width, cfg.height, cfg.n_layers = self.device, self.w, self.h, len(self.channels)
        for i, c in enumerate(self.channels):
            cfg.channels[i] = c
        cfg.max_batch, cfg.max_steps = self.batch, self.max_steps
        self._h = ctypes.c_void_p()
        _check(self.lib.eigen_trainer_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        self._names = tensor_names(len(self.channels))
        self._shapes = tensor_shapes(self.channels, self.w, self.h)
        self._torch = torch
        self.set_weights(_resolve_weights(model_name, self.channels, self.w, self.h))

    # -- weights -------------------------------------------------------------------------------------
    def set_weights(self, weights):
        """Load a weight table; clears the Adam moments and step count and any kept sequence state."""
        arrs = []
        for n in self._names:
            a = np.ascontiguousarray(weights[n], dtype=np.float32)
            if a.shape != self._shapes[n]:
                raise ValueError("tensor %r has shape %s, expected %s" % (n, a.shape, self._shapes[n]))
            arrs.append(a)
        tab = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        _check(self.lib.eigen_trainer_set_weights(self._h, tab, ctypes.c_int32(len(arrs))))

    def _read(self, fn):
        out = {n: np.empty(self._shapes[n], np.float32) for n in self._names}
        tab = (ctypes.c_void_p * len(self._names))(*[out[n].ctypes.data for n in self._names])
        _check(fn(self._h, tab, ctypes.c_int32(len(self._names))))
        return out

    def weights(self):
        """A fresh {name: float32 array} table of the current weights."""
        return self._read(self.lib.eigen_trainer_get_weights)

    def grads(self):
        """The gradients of the last loss_and_grad call, {name: float32 array}."""
        return self._read(self.lib.eigen_trainer_get_grads)

    @property
    def tape_bytes(self):
        return int(self.lib.eigen_trainer_tape_bytes(self._h))

    # -- training ------------------------------------------------------------------------------------
    def _frames(self, frames):
        from .fitness import _check_sequence_frames
        torch = self._torch
        if isinstance(frames, torch.Tensor):
            if frames.dtype != torch.uint8:
                raise ValueError("frames must be uint8")
            _check_sequence_frames(frames, self.channels, self.w, self.h)
            return frames.contiguous() if frames.is_cuda else frames.contiguous().cuda(self.device)
        frames = np.asarray(frames)
        if frames.dtype != np.uint8:
            raise ValueError("frames must be uint8")
        _check_sequence_frames(frames, self.channels, self.w, self.h)
        return torch.from_numpy(np.ascontiguousarray(frames)).cuda(self.device)

    def forward_backward(self, frames, reset=True, pred=False, stream=None):
        """Loss of frames uint8 [n, T, C, H, W] (numpy or a device tensor, n <= batch) and the gradients, kept on the device
        (``grads()``).  reset=False continues from the state the previous call left (the same n), as a constant.
        pred=True also returns the float predictions P0 [n, T, C, H, W] (numpy)."""
        d = self._frames(frames)
        n, T = int(d.shape[0]), int(d.shape[1])
        loss = ctypes.c_double(0.0)
        d_pred = self._torch.empty(tuple(d.shape), dtype=self._torch.float32, device=d.device) if pred else None
        _check(self.lib.eigen_trainer_loss_grad(self._h, _ptr(d), ctypes.c_int64(T * int(np.prod(d.shape[2:]))), ctypes.c_int32(n),
                                                ctypes.c_int32(T), ctypes.c_int32(int(bool(reset))), ctypes.byref(loss), _ptr(d_pred),
                                                _stream_arg(stream)))
        if pred:
            return loss.value, d_pred.cpu().numpy()
        return loss.value

    def loss_and_grad(self, frames, reset=True):
        """(loss, {name: gradient}) of frames uint8 [n, T, C, H, W]; overwrites the gradients."""
        loss = self.forward_backward(frames, reset)
        return loss, self.grads()

    def adam(self, stream=None):
        """One Adam step on the current gradients."""
        _check(self.lib.eigen_trainer_adam(self._h, self.alpha, self.beta1, self.beta2, self.eps, _stream_arg(stream)))

    def step(self, frames, reset=True):
        """Gradient and one Adam step; returns the loss before the step."""
        loss = self.forward_backward(frames, reset)
        self.adam()
        return loss

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.eigen_trainer_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


__all__ = ["PredNetTrainer", "EngineError"]
