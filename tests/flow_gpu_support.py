"""Shared by tests/test_gpu_flow_obj.py, test_gpu_flow_ref.py, test_gpu_flow_pair.py and test_gpu_trainer_entries.py: padded device buffers
and the flow entries of include/eigen_engine.h called directly through ctypes, on a `PredNetTrainer`'s handle.  A plain module: no fixtures."""
import ctypes

import numpy as np
import torch

from evolutionary_illusion_generator_amd.train import FlowSettings

SENT = np.float32(-12345.5)


def _p(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def _padded(a, stride, fill, cuda):
    """[B, ...] as a flat device buffer with `stride` elements between samples, `fill` in between and behind"""
    B, per = a.shape[0], int(np.prod(a.shape[1:]))
    buf = np.full(B * stride + 3, fill, a.dtype)
    for b in range(B):
        buf[b * stride:b * stride + per] = a[b].ravel()
    return torch.from_numpy(buf).to(cuda)


def _unpad(t, stride, B, shp):
    """the samples of a padded buffer, and whether everything between and behind them is still SENT"""
    buf, per = t.cpu().numpy(), int(np.prod(shp))
    written = np.zeros(buf.shape, bool)
    for b in range(B):
        written[b * stride:b * stride + per] = True
    return np.stack([buf[b * stride:b * stride + per].reshape(shp) for b in range(B)]), bool((buf[~written] == SENT).all())


def _stage_args(tr, d_pred, p_b, d_ref, r_b, B, cfg, d_dir, d_mask, scale, value, d_flow, d_seed, s_b):
    """the arguments the three stage-alone entries share; cfg: FlowSettings or None"""
    return [tr._h, _p(d_pred), p_b, _p(d_ref), r_b, B, None if cfg is None else ctypes.byref(cfg), _p(d_dir), _p(d_mask), ctypes.c_double(scale),
            None if value is None else ctypes.byref(value), _p(d_flow), _p(d_seed), s_b]


def _raw_term(tr, d_pred, p_b, d_ref, r_b, B, radius, eps, d_dir, d_mask, scale, value, d_flow, d_seed, s_b, settings=True):
    """eigen_trainer_flow_term called directly on device buffers"""
    cfg = FlowSettings(radius, 0, eps) if settings else None
    return tr.lib.eigen_trainer_flow_term(*_stage_args(tr, d_pred, p_b, d_ref, r_b, B, cfg, d_dir, d_mask, scale, value, d_flow, d_seed, s_b), None)


def _raw_ref(tr, d_pred, p_b, d_ref, r_b, B, radius, eps, d_dir, d_mask, scale, value, d_flow, d_seed, s_b, d_rg, rg_b, flags=0, entry="eigen_trainer_flow_term_ref"):
    """eigen_trainer_flow_term_ref likewise"""
    args = _stage_args(tr, d_pred, p_b, d_ref, r_b, B, FlowSettings(radius, flags, eps), d_dir, d_mask, scale, value, d_flow, d_seed, s_b)
    return getattr(tr.lib, entry)(*args, _p(d_rg), rg_b, None)


def _raw_pair(tr, d_pred, p_b, d_prev, r_b, B, radius, eps, d_dir, d_mask, scale, value, d_flow, d_seed, s_b, d_pg, pg_b, flags=0):
    """eigen_trainer_flow_term_pair likewise: a float reference, the same arguments"""
    return _raw_ref(tr, d_pred, p_b, d_prev, r_b, B, radius, eps, d_dir, d_mask, scale, value, d_flow, d_seed, s_b, d_pg, pg_b, flags, "eigen_trainer_flow_term_pair")


def _raw_loss_grad(tr, entry, d, B, T, n, flags, pairing, loss, terms, buf=None, objective=2, settings=True):
    """eigen_trainer_loss_grad_flow (entry "flow") or eigen_trainer_loss_grad_flow_pair ("pair"): one reset call on frames d [B, T, n bytes],
    radius 7, eps 1e-2, no direction and no mask, per-frame frame gradients into buf where given"""
    cfg = FlowSettings(7, flags, 1e-2)
    args = [tr._h, _p(d), T * n, B, T, T, 0, 1, None, objective, None, ctypes.byref(loss), None, None, _p(buf), T * n if buf is not None else 0,
            n if buf is not None else 0, ctypes.byref(cfg) if settings else None, None, None, terms]
    if entry == "pair":
        return tr.lib.eigen_trainer_loss_grad_flow_pair(*args, pairing, None)
    return tr.lib.eigen_trainer_loss_grad_flow(*args, None)
