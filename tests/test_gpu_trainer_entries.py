"""The six exported training entries on the GPU (include/eigen_engine.h eigen_trainer_loss_grad*): each is the
widest one, eigen_trainer_loss_grad_flow_pair, called with the defaults the narrower entry implies, bit for bit; and a call that breaks
two rules at once is refused with the code and the text of the rule that comes first, before anything is launched."""
import ctypes

import pytest
import torch

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.train import FlowSettings, PredNetTrainer, TrainerConfig
from tests.flow_gpu_support import SENT, _p
from tests.frame_grad_support import case_inputs

pytestmark = pytest.mark.gpu

W, H, CH, B, T = 16, 12, (3, 4, 6), 2, 4
N = CH[0] * H * W   # bytes of a frame, floats of its gradient


def _call(tr, entry, d, loss=None, d_pred=None, batch=B, n_steps=T, objective=0, layer_w=None, grad=None, g_b=0, g_t=0, cfg=None, terms=None, pairing=0, handle=True):
    """one reset call, all frames fed, through `entry` with the arguments that entry has: the others are dropped, not defaulted"""
    h = tr._h if handle else None
    lam = None if layer_w is None else (ctypes.c_double * len(layer_w))(*layer_w)
    loss = None if loss is None else ctypes.byref(loss)
    head = [h, _p(d), T * N, batch, n_steps]
    obj = head + [n_steps, 0, 1, None, objective, lam, loss, None, _p(d_pred)]
    fg = [_p(grad), g_b, g_t]
    flow = [None if cfg is None else ctypes.byref(cfg), None, None, terms]
    tail = {"eigen_trainer_loss_grad": head + [1, loss, _p(d_pred)], "eigen_trainer_loss_grad_ext": head + [n_steps, 0, 1, None, loss, _p(d_pred)],
            "eigen_trainer_loss_grad_obj": obj, "eigen_trainer_loss_grad_frames": obj + fg, "eigen_trainer_loss_grad_flow": obj + fg + flow,
            "eigen_trainer_loss_grad_flow_pair": obj + fg + flow + [pairing]}[entry]
    return getattr(tr.lib, entry)(*tail, None)


ENTRIES = ["eigen_trainer_loss_grad", "eigen_trainer_loss_grad_ext", "eigen_trainer_loss_grad_obj", "eigen_trainer_loss_grad_frames",
           "eigen_trainer_loss_grad_flow", "eigen_trainer_loss_grad_flow_pair"]


def test_every_entry_is_the_widest_entry_with_its_defaults(cuda):
    """16x12 [3, 4, 6], B = 2, T = 4, "live" weights.  Under the squared error, one reset call through each of the six entries: the 8
    bytes of the loss, d_pred and every weight gradient are those of eigen_trainer_loss_grad_flow_pair(pairing 0).  Under the flow
    objective with tied frame gradients, constant and moving reference: eigen_trainer_loss_grad_flow against the same, the terms and the
    frame gradient included."""
    frames, sets = case_inputs(W, H, CH, B, T)
    d = torch.from_numpy(frames).to(cuda)
    with PredNetTrainer(sets["live"], list(CH), W, H, B, T) as tr:
        got = {}
        for entry in ENTRIES:
            loss = ctypes.c_double(float(SENT))
            pred = torch.full((B, T, N), float(SENT), dtype=torch.float32, device=cuda)
            assert _call(tr, entry, d, loss, pred) == 0, (entry, tr.lib.eigen_last_error())
            got[entry] = (bytes(loss), pred.cpu().numpy(), tr.grads())
        l0, p0, g0 = got["eigen_trainer_loss_grad_flow_pair"]
        assert l0 != bytes(ctypes.c_double(float(SENT))) and not (p0 == SENT).any() and any(g.any() for g in g0.values())
        for entry in ENTRIES[:-1]:
            l1, p1, g1 = got[entry]
            assert l1 == l0 and p1.tobytes() == p0.tobytes(), entry
            assert sorted(g1) == sorted(g0) and all(g1[k].tobytes() == g0[k].tobytes() for k in g0), entry
        for flags in (0, train.FLOW_MOVING_REFERENCE):
            out = []
            for entry in ENTRIES[-2:]:
                loss, terms = ctypes.c_double(float(SENT)), (ctypes.c_double * (T - 1))(*([float(SENT)] * (T - 1)))
                pred = torch.full((B, T, N), float(SENT), dtype=torch.float32, device=cuda)
                tied = torch.full((B, N), float(SENT), dtype=torch.float32, device=cuda)
                assert _call(tr, entry, d, loss, pred, objective=2, grad=tied, g_b=N, g_t=0, cfg=FlowSettings(7, flags, 1e-2), terms=terms) == 0, entry
                out.append((bytes(loss), bytes(terms), pred.cpu().numpy().tobytes(), tied.cpu().numpy(), tr.grads()))
            (la, ta, pa, fa, ga), (lb, tb, pb, fb, gb) = out
            assert la == lb and ta == tb and pa == pb and fa.tobytes() == fb.tobytes() and not (fa == SENT).any() and fa.any()
            assert all(ga[k].tobytes() == gb[k].tobytes() for k in ga) and any(g.any() for g in ga.values()) and la != l0


# what the parent of the commit that un-telescoped the entries returned for each of these calls: (code, eigen_last_error)
NEEDS_SETTINGS = (-1, "EIGEN_OBJ_FLOW needs the settings eigen_trainer_loss_grad_flow takes")
CAPACITY = (-4, "batch 2 / 5 steps exceed the trainer's 2 / 4")
PRECEDENCE = {
    "obj: objective 2, no weights set": NEEDS_SETTINGS,                  # not -3, eigen_trainer_set_weights has not been called
    "frames: objective 2, batch = max_batch + 1": NEEDS_SETTINGS,        # not -4
    "frames: objective 2, NULL handle": NEEDS_SETTINGS,                  # not the null argument
    "ext: n_steps > max_steps": CAPACITY,
    "loss_grad: n_steps > max_steps": CAPACITY,
    "flow_pair: pairing 7, g_tstride 1": (-1, "pairing 7 is neither EIGEN_FLOW_PAIR_FRAME nor EIGEN_FLOW_PAIR_PREDICTION"),
    "flow_pair: pairing 7, NULL frames": (-1, "null argument"),
    "flow: mse with settings, g_tstride 1": (-1, "g_tstride 1 is neither 0 (tied) nor at least a frame (576 floats)"),
    "flow: objective 2, layer weight < 0, radius 0": (-1, "layer weight 1 is -0.5: weights must be finite and >= 0"),
    "flow_pair: pairing 1, moving flag, unknown flag": (-1, "flow flags 0x3: this entry takes 0x1 at most"),
}


def test_refusal_precedence_is_unchanged(cuda):
    """calls that break two rules at once: the code and the eigen_last_error text are those of PRECEDENCE, and nothing was launched or
    written: the loss, the predictions and the frame gradient keep their sentinel, the weight gradients stay zero"""
    frames, sets = case_inputs(W, H, CH, B, T)
    d = torch.from_numpy(frames).to(cuda)
    big = torch.zeros(((B + 1) * (T + 1) * N,), dtype=torch.uint8, device=cuda)   # enough frames for the calls refused for their size
    loss = ctypes.c_double(float(SENT))
    pred = torch.full(((B + 1) * (T + 1) * N,), float(SENT), dtype=torch.float32, device=cuda)
    grad = torch.full((B * T * N,), float(SENT), dtype=torch.float32, device=cuda)
    terms = (ctypes.c_double * (T - 1))(*([float(SENT)] * (T - 1)))
    got = {}
    with PredNetTrainer(sets["live"], list(CH), W, H, B, T) as tr:
        # a second handle of the same shape on which eigen_trainer_set_weights is never called
        cfg = TrainerConfig()
        cfg.device, cfg.width, cfg.height, cfg.n_layers, cfg.max_batch, cfg.max_steps = tr.device, W, H, len(CH), B, T
        for i, c in enumerate(CH):
            cfg.channels[i] = c
        bare = ctypes.c_void_p()
        assert tr.lib.eigen_trainer_create(ctypes.byref(cfg), ctypes.byref(bare)) == 0

        class Bare:
            lib, _h = tr.lib, bare

        def record(what, rc):
            got[what] = (rc, tr.lib.eigen_last_error().decode())

        try:
            record("obj: objective 2, no weights set", _call(Bare, "eigen_trainer_loss_grad_obj", d, loss, pred, objective=2))
        finally:
            tr.lib.eigen_trainer_destroy(bare)
        kw = dict(loss=loss, d_pred=pred)
        record("frames: objective 2, batch = max_batch + 1", _call(tr, "eigen_trainer_loss_grad_frames", big, objective=2, batch=B + 1, grad=grad, g_b=T * N, g_t=N, **kw))
        record("frames: objective 2, NULL handle", _call(tr, "eigen_trainer_loss_grad_frames", d, objective=2, handle=False, **kw))
        record("ext: n_steps > max_steps", _call(tr, "eigen_trainer_loss_grad_ext", big, n_steps=T + 1, **kw))
        record("loss_grad: n_steps > max_steps", _call(tr, "eigen_trainer_loss_grad", big, n_steps=T + 1, **kw))
        flow = dict(kw, grad=grad, g_b=T * N, terms=terms)
        record("flow_pair: pairing 7, g_tstride 1", _call(tr, "eigen_trainer_loss_grad_flow_pair", d, objective=2, g_t=1, cfg=FlowSettings(7, 0, 1e-2), pairing=7, **flow))
        record("flow_pair: pairing 7, NULL frames", _call(tr, "eigen_trainer_loss_grad_flow_pair", None, objective=2, g_t=N, cfg=FlowSettings(7, 0, 1e-2), pairing=7, **flow))
        record("flow: mse with settings, g_tstride 1", _call(tr, "eigen_trainer_loss_grad_flow", d, objective=0, g_t=1, cfg=FlowSettings(7, 0, 1e-2), **flow))
        record("flow: objective 2, layer weight < 0, radius 0",
               _call(tr, "eigen_trainer_loss_grad_flow", d, objective=2, layer_w=[1.0, -0.5, 0.0], g_t=N, cfg=FlowSettings(0, 0, 1e-2), **flow))
        record("flow_pair: pairing 1, moving flag, unknown flag",
               _call(tr, "eigen_trainer_loss_grad_flow_pair", d, objective=2, g_t=N, cfg=FlowSettings(7, 1 | 2, 1e-2), pairing=1, **flow))
        torch.cuda.synchronize()
        grads = tr.grads()
    for what, (rc, msg) in got.items():
        print("%s -> %d %r" % (what, rc, msg))
    assert got == PRECEDENCE
    assert loss.value == float(SENT) and list(terms) == [float(SENT)] * (T - 1)
    assert (pred == float(SENT)).all() and (grad == float(SENT)).all() and all(not g.any() for g in grads.values())
