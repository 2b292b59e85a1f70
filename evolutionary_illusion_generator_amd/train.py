"""PredNet training on frame sequences (include/eigen_engine.h eigen_trainer_*).

Next-frame MSE of the float prediction or, per call, PredNet's own objective on the error units (``objective="error"``: L_0 by
default, L_all with ``layer_weights=[1, 0.1, ...]``) or the displacement a dense Lucas-Kanade solve finds between the next frame and
the prediction (``objective="flow"`` with a ``FlowObjective``), full backprop through time within a call, Adam as chainer defines it; every kernel is
HIP for gfx950 (csrc/prednet_train.hip), there is no CPU or PyTorch fallback.  The trained weights are a plain
``{name: float32 array}`` table, usable as ``model_name`` anywhere the fitness path takes one, and
``weights.save_chainer_npz`` writes them as a chainer npz file.
"""
import ctypes

import numpy as np

from . import engine
from .engine import EngineError, _check, _ptr, _stream_arg
from .weights import tensor_names, tensor_shapes


class FlowSettings(ctypes.Structure):
    """eigen_flow_settings"""
    _fields_ = [("radius", ctypes.c_int32), ("flags", ctypes.c_int32), ("eps", ctypes.c_double)]


class FlowScoreSettings(ctypes.Structure):
    """eigen_flow_score"""
    _fields_ = [("max_norm", ctypes.c_double), ("min_norm", ctypes.c_double), ("r_min", ctypes.c_double), ("r_max", ctypes.c_double),
                ("w_direction", ctypes.c_double), ("w_strength", ctypes.c_double), ("min_count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class FlowStructureSettings(ctypes.Structure):
    """eigen_flow_structure_score"""
    _fields_ = [("structure", ctypes.c_int32), ("min_count", ctypes.c_int32), ("max_norm", ctypes.c_double), ("min_norm", ctypes.c_double),
                ("lim_lo", ctypes.c_double), ("lim_hi", ctypes.c_double), ("max_distance", ctypes.c_double), ("w", ctypes.c_double * 3)]


class FlowMembersSettings(ctypes.Structure):
    """eigen_flow_members"""
    _fields_ = [("kind", ctypes.c_int32), ("max_corners", ctypes.c_int32), ("block_size", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("quality_level", ctypes.c_double), ("min_distance", ctypes.c_double), ("mask_bstride", ctypes.c_int64)]


class FlowJointSettings(ctypes.Structure):
    """eigen_flow_joint: the frame weight (0: no frame term), the validity planes with their strides in bytes (NULL: none) and the two
    doubles (L_flow, L_mse) the call writes (NULL: not wanted)"""
    _fields_ = [("frame_weight", ctypes.c_double), ("d_valid", ctypes.c_void_p), ("v_bstride", ctypes.c_int64), ("v_tstride", ctypes.c_int64),
                ("h_parts", ctypes.c_void_p)]


class AdamSettings(ctypes.Structure):
    """eigen_adam_settings"""
    _fields_ = [("alpha", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("clip_norm", ctypes.c_double), ("skip_nonfinite", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AdamReport(ctypes.Structure):
    """eigen_adam_report"""
    _fields_ = [("norm", ctypes.c_double), ("rate", ctypes.c_double), ("applied", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class TrainerConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("n_layers", ctypes.c_int32),
                ("channels", ctypes.c_int32 * engine.MAX_LAYERS), ("max_batch", ctypes.c_int32), ("max_steps", ctypes.c_int32)]


# the argument groups of include/eigen_engine.h's trainer entries; every entry ends with its stream
_I32, _I64, _P, _PD = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
_CALL = [_P, _P, _I64, _I32, _I32, _I32, _I32, _I32]   # t, d_frames, bstride, batch, n_steps, n_fed, requant, reset
_OBJ = [_P, _I32, _P, _PD, _P, _P]                     # h_step_w, objective, h_layer_w, h_loss, h_layer_err, d_pred
_FRAMEGRAD = [_P, _I64, _I64]                          # d_frame_grad, g_bstride, g_tstride
_FLOW = [_P, _P, _P, _P]                               # flow, d_dir, d_mask, h_terms
# t, d_pred, p_bstride, d_ref, r_bstride, batch, flow, d_dir, d_mask, scale, h_value, d_flow, d_seed, s_bstride
_TERM = [_P, _P, _I64, _P, _I64, _I32, _P, _P, _P, ctypes.c_double, _P, _P, _P, _I64]
# The narrowest entry that takes a training request: the entry and the argument groups that follow _CALL and _OBJ.  Keys: (False, frame
# gradient wanted) for the mse and error objectives, (True, pairing) for the flow objective, whose entries take the frame gradient anyway.
_ENTRIES = {(False, False): ("eigen_trainer_loss_grad_obj", ()), (False, True): ("eigen_trainer_loss_grad_frames", ("frame_grad",)),
            (True, "frame"): ("eigen_trainer_loss_grad_flow", ("frame_grad", "flow")),
            (True, "prediction"): ("eigen_trainer_loss_grad_flow_pair", ("frame_grad", "flow", "pairing")),
            (True, "score"): ("eigen_trainer_loss_grad_flow_score", ("frame_grad", "flow", "pairing", "score")),
            (True, "structure"): ("eigen_trainer_loss_grad_flow_structure", ("frame_grad", "flow", "pairing", "score")),
            (True, "members"): ("eigen_trainer_loss_grad_flow_members", ("frame_grad", "flow", "pairing", "members")),
            # a real solve (``FlowObjective.solved``): the members entry's arguments, then, behind the stream, the solve
            (True, "iter"): ("eigen_trainer_loss_grad_flow_iter", ("frame_grad", "flow", "pairing", "members")),
            # a target field (``flow_target=``): the iter entry's arguments, then, behind the solve, the target and its two strides
            (True, "target"): ("eigen_trainer_loss_grad_flow_target", ("frame_grad", "flow", "pairing", "members")),
            # a frame weight or validity planes (``frame_weight=``, ``flow_valid=``): the target entry's arguments (the target may be NULL), then
            # the eigen_flow_joint record
            (True, "joint"): ("eigen_trainer_loss_grad_flow_joint", ("frame_grad", "flow", "pairing", "members"))}
SOLVE_MAX_LEVELS, SOLVE_MAX_ITERS, SOLVE_MIN_COARSE = 6, 32, 4   # eigen_dense_solve's accepted values (fitness.DenseFitness states the same)


def _bind(lib):
    if getattr(lib, "_trainer_bound", False):
        return
    lib.eigen_trainer_loss_grad.argtypes = [_P, _P, _I64, _I32, _I32, _I32, _PD, _P, _P]
    lib.eigen_trainer_loss_grad_ext.argtypes = _CALL + [_P, _PD, _P, _P]
    lib.eigen_trainer_evaluate.argtypes = _CALL + [_P, _P, _P]
    lib.eigen_trainer_evaluate_err.argtypes = _CALL + [_P, _P, _P, _P]
    lib.eigen_trainer_loss_grad_obj.argtypes = _CALL + _OBJ + [_P]
    lib.eigen_trainer_loss_grad_frames.argtypes = _CALL + _OBJ + _FRAMEGRAD + [_P]
    lib.eigen_trainer_loss_grad_flow.argtypes = _CALL + _OBJ + _FRAMEGRAD + _FLOW + [_P]
    lib.eigen_trainer_loss_grad_flow_pair.argtypes = _CALL + _OBJ + _FRAMEGRAD + _FLOW + [_I32, _P]
    lib.eigen_trainer_flow_term.argtypes = _TERM + [_P]
    lib.eigen_trainer_flow_term_ref.argtypes = _TERM + [_P, _I64, _P]
    lib.eigen_trainer_flow_term_pair.argtypes = _TERM + [_P, _I64, _P]
    lib.eigen_trainer_loss_grad_flow_score.argtypes = _CALL + _OBJ + _FRAMEGRAD + _FLOW + [_I32, _P, _P]
    # t, d_pred, p_bstride, d_ref, d_fref, r_bstride, batch, flow, d_mask, score, scale, h_value, h_stats, d_flow, d_seed, s_bstride, d_ref_grad, rg_bstride, stream
    lib.eigen_trainer_flow_term_score.argtypes = [_P, _P, _I64, _P, _P, _I64, _I32, _P, _P, _P, ctypes.c_double, _P, _P, _P, _P, _I64, _P, _I64, _P]
    lib.eigen_trainer_loss_grad_flow_structure.argtypes = lib.eigen_trainer_loss_grad_flow_score.argtypes
    lib.eigen_trainer_flow_term_structure.argtypes = lib.eigen_trainer_flow_term_score.argtypes
    lib.eigen_trainer_debug_free_planes.argtypes = [_P, _I32, _P, _P, _P, _P, _P, _P]
    # ... pairing, score, sscore, members, h_stats, stream
    lib.eigen_trainer_loss_grad_flow_members.argtypes = _CALL + _OBJ + _FRAMEGRAD + _FLOW + [_I32, _P, _P, _P, _P, _P]
    # eigen_trainer_flow_term_score's with (score, sscore, members) in place of score
    lib.eigen_trainer_flow_term_members.argtypes = [_P, _P, _I64, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, ctypes.c_double, _P, _P, _P, _P, _I64, _P, _I64, _P]
    # t, d_ref, d_fref, r_bstride, batch, members, d_mask, h_members, h_counts, stream
    lib.eigen_trainer_flow_members.argtypes = [_P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P]
    # the members entries' arguments, then (stage alone) d_dir and the solve, (training call) the solve
    lib.eigen_trainer_flow_term_iter.argtypes = lib.eigen_trainer_flow_term_members.argtypes + [_P, _P]
    lib.eigen_trainer_loss_grad_flow_iter.argtypes = lib.eigen_trainer_loss_grad_flow_members.argtypes + [_P]
    lib.eigen_trainer_debug_flow_iter.argtypes = [_P, _I32, ctypes.POINTER(ctypes.c_int64)]
    # the iter entries' arguments, then d_target and t_bstride, (training call) t_tstride
    lib.eigen_trainer_flow_term_target.argtypes = lib.eigen_trainer_flow_term_iter.argtypes + [_P, _I64]
    lib.eigen_trainer_loss_grad_flow_target.argtypes = lib.eigen_trainer_loss_grad_flow_iter.argtypes + [_P, _I64, _I64]
    # the target entries' arguments, then (stage alone) d_valid and v_bstride, (training call) the eigen_flow_joint record
    lib.eigen_trainer_flow_term_valid.argtypes = lib.eigen_trainer_flow_term_target.argtypes + [_P, _I64]
    lib.eigen_trainer_loss_grad_flow_joint.argtypes = lib.eigen_trainer_loss_grad_flow_target.argtypes + [_P]
    lib.eigen_trainer_still_step.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_int32,
                                             ctypes.c_void_p]
    lib.eigen_trainer_get_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_int32]
    lib.eigen_trainer_set_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_int32]
    lib.eigen_trainer_adam.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    lib.eigen_trainer_tape_bytes.restype = ctypes.c_int64
    lib.eigen_trainer_tape_bytes.argtypes = [ctypes.c_void_p]
    lib.eigen_trainer_grad_norms.argtypes = [_P, _PD, _PD, _I32, _P]                                                       # t, h_global, h_per_tensor, n_tensors, stream
    lib.eigen_trainer_adam_ex.argtypes = [_P, ctypes.POINTER(AdamSettings), ctypes.POINTER(AdamReport), _P]                # t, settings, h_report, stream
    lib.eigen_trainer_accumulate.argtypes = [_P, _I32, ctypes.c_double, _P]                                                # t, op, scale, stream
    lib._trainer_bound = True

HYPER = ("alpha", "beta1", "beta2", "eps")
OPTIM = ("clip_norm", "weight_decay", "skip_nonfinite")  # the optimiser controls; neutral: (None, 0.0, False)
ACC_CLEAR, ACC_ADD, ACC_LOAD = 0, 1, 2  # EIGEN_ACC_CLEAR, EIGEN_ACC_ADD, EIGEN_ACC_LOAD
SEQ_PARTS = ("h", "c", "P")
OBJECTIVES = {"mse": 0, "error": 1, "flow": 2}  # eigen_objective
FRAME_GRADS = (None, "frames", "tied")
FLOW_MAX_RADIUS = 16
FLOW_DIRECTIONS = ("tangent", "radial", "horizontal", "vertical")
FLOW_REFERENCES = ("constant", "moving")
FLOW_MOVING_REFERENCE = 1  # EIGEN_FLOW_MOVING_REFERENCE
FLOW_PAIRINGS = {"frame": 0, "prediction": 1}  # EIGEN_FLOW_PAIR_FRAME, EIGEN_FLOW_PAIR_PREDICTION
FLOW_MEMBERS_MASK, FLOW_MEMBERS_CORNERS = 0, 1  # EIGEN_FLOW_MEMBERS_MASK, EIGEN_FLOW_MEMBERS_CORNERS
CORNER_MAX, CORNER_MAX_BLOCK = 128, 9


class CornerMembers:
    """Membership of a score from the fitness's own corners ("The corner members"): the members of a term are the
    at most max_corners points ``goodFeaturesToTrack(quality_level, min_distance, block_size)`` picks on the term's own reference image,
    per sample, found on the device by the kernels of the fitness path; the score's geometric rule and its norm limits apply on top, and
    a shared [H, W] mask on the objective removes the corners it does not count.  The defaults are ``eigen_config``'s ``lk_*`` defaults.
    ValueError: max_corners outside 1 .. 128, block_size outside 1 .. 9, quality_level outside (0, 1], min_distance negative or not
    finite."""

    def __init__(self, max_corners=100, quality_level=0.3, min_distance=7.0, block_size=7):
        for name, v, hi in (("max_corners", max_corners, CORNER_MAX), ("block_size", block_size, CORNER_MAX_BLOCK)):
            if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= hi:
                raise ValueError("%s must be an integer in 1 .. %d, got %r" % (name, hi, v))
        quality_level, min_distance = float(quality_level), float(min_distance)
        if not 0 < quality_level <= 1:
            raise ValueError("quality_level must be in (0, 1], got %r" % (quality_level,))
        if not (np.isfinite(min_distance) and min_distance >= 0):
            raise ValueError("min_distance must be finite and >= 0, got %r" % (min_distance,))
        self.max_corners, self.quality_level, self.min_distance, self.block_size = int(max_corners), quality_level, min_distance, int(block_size)

    def settings(self):
        """eigen_flow_members of kind CORNERS"""
        return FlowMembersSettings(FLOW_MEMBERS_CORNERS, self.max_corners, self.block_size, 0, self.quality_level, self.min_distance, 0)


SCORE_STATS = ("N", "mean_rho", "mean_tau", "mean_abs_dx", "mean_norm", "var_rho", "var_tau", "var_norm", "score", "spare")  # one sample's record


class FlowScore:
    """The score mode of ``objective="flow"`` ("The score mode"): the value of a term is the reference's own
    ``Circles`` score on the dense field u of the stage's solve, per sample, and its mean over the samples.  A pixel is a member when
    the objective's mask counts it, its distance from (w / 2, h / 2) is not 0 and lies in `limits`, and min_norm <= |u| <= max_norm.
    Over the members: weights[0] times ``rotation_symmetry_score`` (the low variance of the normalised vectors' radial and tangential
    components) plus weights[1] times ``strength_number`` (mean |dx| / max_norm times one minus the variance of the norms, capped at
    1); a sample with fewer than min_count members scores 0 and passes no gradient.  Membership is a constant of the graph.

    The defaults are the reference's constants (fitness_calculator.py:522-533): max_norm 0.3 pixels, limits (0, h / 2) (None: resolved
    against the trainer's image), at least 25 vectors, weights (0.7, 0.3).  min_norm is this build's choice: the gradient carries
    1 / |u|, and the floor 1e-3 caps that factor at 1000; the reference has no such floor (it divides by the norm of whatever vector
    it was given).  ValueError: max_norm not finite or <= 0, min_norm outside [0, max_norm), limits not finite or not
    0 <= limits[0] <= limits[1], min_count < 2, a weight that is negative or not finite, both weights zero."""

    def __init__(self, max_norm=0.3, min_norm=1e-3, limits=None, min_count=25, weights=(0.7, 0.3)):
        max_norm, min_norm = float(max_norm), float(min_norm)
        if not (np.isfinite(max_norm) and max_norm > 0):
            raise ValueError("max_norm must be finite and > 0, got %r" % (max_norm,))
        if not 0 <= min_norm < max_norm:
            raise ValueError("min_norm must be in [0, max_norm = %r), got %r" % (max_norm, min_norm))
        if limits is not None:
            limits = tuple(float(v) for v in limits)
            if len(limits) != 2 or not all(np.isfinite(v) for v in limits) or not 0 <= limits[0] <= limits[1]:
                raise ValueError("limits must be finite with 0 <= limits[0] <= limits[1], got %r" % (limits,))
        if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 2:
            raise ValueError("min_count must be an integer >= 2, got %r" % (min_count,))
        weights = tuple(float(v) for v in weights)
        if len(weights) != 2 or not all(np.isfinite(v) and v >= 0 for v in weights) or not sum(weights) > 0:
            raise ValueError("weights must be two finite values >= 0, not both zero, got %r" % (weights,))
        self.max_norm, self.min_norm, self.limits, self.min_count, self.weights = max_norm, min_norm, limits, int(min_count), weights

    def settings(self, h):
        """eigen_flow_score against an image of height h"""
        lo, hi = self.limits if self.limits is not None else (0.0, h / 2.0)
        return FlowScoreSettings(self.max_norm, self.min_norm, lo, hi, self.weights[0], self.weights[1], self.min_count, 0)


BANDS_STATS = ("N", "mean_x", "mean_y", "var_x", "spare4", "spare5", "spare6", "spare7", "score", "spare")  # one sample's record under a BandsScore
FREE_STATS = ("N", "mean_abs_dx", "mean_norm", "var_norm", "swarm", "strength", "spare6", "spare7", "score", "spare")  # under a FreeScore


def _check_norms_and_count(max_norm, min_norm, min_count):
    """the rules the structure scores share -> (max_norm, min_norm, min_count)"""
    max_norm, min_norm = float(max_norm), float(min_norm)
    if not (np.isfinite(max_norm) and max_norm > 0):
        raise ValueError("max_norm must be finite and > 0, got %r" % (max_norm,))
    if not 0 <= min_norm < max_norm:
        raise ValueError("min_norm must be in [0, max_norm = %r), got %r" % (max_norm, min_norm))
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
        raise ValueError("min_count must be an integer >= 1, got %r" % (min_count,))
    return max_norm, min_norm, int(min_count)


class BandsScore:
    """The Bands structure's score as the value of a flow term ("The structure scores"): the fitness's own
    ``horizontal_symmetry_score`` on the dense field u of the stage's solve, per sample, and its mean over the samples.  A pixel is a
    member when the objective's mask counts it, limits[0] <= y <= limits[1] and min_norm <= |u| <= max_norm.  With middle =
    int(limits[1] / 2), a member above it stores (nx, nx) (the reference's quirk, kept) and one at or below it (-nx, ny), n = u / |u|;
    the score is ((1 - var mx) + |mean mx| + (1 - |mean my|)) / 3.  A sample with fewer than min_count members scores 0 and passes no
    gradient.  Membership is a constant of the graph.

    The defaults are the reference's constants: max_norm 0.15 pixels, limits (0, (h / 4) * 2) (None: resolved against the trainer's
    image), any vector at all (min_count 1).  min_norm is this build's floor, as ``FlowScore``'s.  ValueError: max_norm not finite or
    <= 0, min_norm outside [0, max_norm), limits not finite, limits[1] < limits[0] or |limits[1]| > 2e9 (the middle is an int), min_count < 1."""

    structure = 0
    stats = BANDS_STATS

    def __init__(self, max_norm=0.15, min_norm=1e-3, limits=None, min_count=1):
        self.max_norm, self.min_norm, self.min_count = _check_norms_and_count(max_norm, min_norm, min_count)
        if limits is not None:
            limits = tuple(float(v) for v in limits)
            if len(limits) != 2 or not all(np.isfinite(v) for v in limits) or not limits[0] <= limits[1] or abs(limits[1]) > 2e9:
                raise ValueError("limits must be finite with limits[0] <= limits[1] and |limits[1]| <= 2e9, got %r" % (limits,))
        self.limits = limits

    def settings(self, h):
        """eigen_flow_structure_score against an image of height h"""
        lo, hi = self.limits if self.limits is not None else (0.0, (h / 4.0) * 2.0)
        return FlowStructureSettings(self.structure, self.min_count, self.max_norm, self.min_norm, lo, hi, 0.0, (ctypes.c_double * 3)(0.0, 0.0, 0.0))


class FreeScore:
    """The Free structure's score as the value of a flow term ("The structure scores"): weights[0] times the
    fitness's own ``swarm_score`` (its quirks kept: ``% 2 * pi`` and the arccos of the x component alone) plus weights[1] times
    ``strength_number`` plus weights[2] times min(N, 15) / 15, on the dense field u of the stage's solve.  A pixel is a member when the
    objective's mask counts it and min_norm <= |u| <= max_norm.  ``swarm_score`` is a sum over all ordered pairs of members nearer than
    max_distance pixels, an N^2 pass per sample.  A sample with fewer than min_count members scores 0 and passes no gradient; the count
    term is a constant of the graph, as membership is.

    The defaults are the reference's constants: max_norm 0.4 pixels, max_distance 100, any vector at all (min_count 1), weights
    (0.5, 0.1, 0.4).  ValueError: max_norm not finite or <= 0, min_norm outside [0, max_norm), max_distance not finite or <= 0,
    min_count < 1, a weight that is negative or not finite, all weights zero."""

    structure = 2
    stats = FREE_STATS

    def __init__(self, max_norm=0.4, min_norm=1e-3, max_distance=100.0, min_count=1, weights=(0.5, 0.1, 0.4)):
        self.max_norm, self.min_norm, self.min_count = _check_norms_and_count(max_norm, min_norm, min_count)
        max_distance = float(max_distance)
        if not (np.isfinite(max_distance) and max_distance > 0 and np.isfinite(max_distance * max_distance) and max_distance * max_distance > 0):
            raise ValueError("max_distance must be finite and > 0, got %r" % (max_distance,))
        weights = tuple(float(v) for v in weights)
        if len(weights) != 3 or not all(np.isfinite(v) and v >= 0 for v in weights) or not sum(weights) > 0:
            raise ValueError("weights must be three finite values >= 0, not all zero, got %r" % (weights,))
        self.max_distance, self.weights = max_distance, weights

    def settings(self, h):
        """eigen_flow_structure_score (the image's height plays no part)"""
        return FlowStructureSettings(self.structure, self.min_count, self.max_norm, self.min_norm, 0.0, 0.0, self.max_distance, (ctypes.c_double * 3)(*self.weights))


FLOW_SCORES = (FlowScore, BandsScore, FreeScore)


def structure_score(structure, **kw):
    """The score of a structure of the fitness (``fitness.StructureType`` or its number), with the class's defaults unless `kw` states
    others: Bands -> ``BandsScore``, Free -> ``FreeScore``, Circles and CirclesFree -> ``FlowScore``.  ValueError: another structure."""
    if isinstance(structure, bool) or int(structure) != structure or int(structure) not in (0, 1, 2, 3):
        raise ValueError("structure must be 0 Bands, 1 Circles, 2 Free or 3 CirclesFree, got %r" % (structure,))
    return {0: BandsScore, 1: FlowScore, 2: FreeScore, 3: FlowScore}[int(structure)](**kw)


def flow_direction(kind, w, h):
    """A direction field for ``FlowObjective``: float32 [2, h, w], the x then the y component of a unit vector per pixel.
    "horizontal" is (1, 0) and "vertical" (0, 1) everywhere.  "radial" points away from the image centre ((w - 1) / 2, (h - 1) / 2):
    (dx, dy) / |(dx, dy)| with (dx, dy) the pixel's offset from it; "tangent" is that turned counter-clockwise in image coordinates,
    (-dy, dx) / |(dx, dy)|.  Both are zero at the centre pixel, where an odd-sized image has one."""
    if kind not in FLOW_DIRECTIONS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(FLOW_DIRECTIONS), kind))
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError("w and h must be >= 1")
    out = np.zeros((2, h, w), np.float64)
    if kind == "horizontal":
        out[0] = 1.0
    elif kind == "vertical":
        out[1] = 1.0
    else:
        dy, dx = np.mgrid[0:h, 0:w].astype(np.float64)
        dx -= (w - 1) / 2.0
        dy -= (h - 1) / 2.0
        norm = np.sqrt(dx * dx + dy * dy)
        norm[norm == 0] = 1.0
        out[0], out[1] = (dx / norm, dy / norm) if kind == "radial" else (-dy / norm, dx / norm)
    return out.astype(np.float32)


class FlowObjective:
    """The settings of ``objective="flow"`` ("The flow objective"): a dense, regularised Lucas-Kanade solve from
    the reference frame to the prediction over windows of Chebyshev radius `radius`, truncated at the border, with `eps` added to the
    diagonal of every 2x2 system.  direction None: the term is the mean squared displacement; direction float32 [2, H, W] (x then y
    component, ``flow_direction``): the mean displacement along it.  mask: [H, W], zero = the pixel is not counted (None: all are).
    reference: "constant", the reference frame of every term is a constant of the graph and a frame gradient is the input path alone;
    "moving", frame s + 1 is in the graph as the reference of term s, and the frame gradient of a training call (``forward_backward``,
    ``refine_stills``, ``refine_genomes``) also holds how every term moves with its reference ("The moving
    reference").  Loss, terms, weight gradients, predictions and state do not depend on it.
    score: None, or a ``FlowScore``: the term is then the fitness's own Circles score on the solved field ("The
    score mode"); it takes no direction (ValueError), the mask then selects the pixels that can be members.  ``scored(score)`` sets it
    on an objective that exists, which is how a ``PredictionFlow`` takes one.
    With a score the mask may also be [n, H, W], one plane per sample (n is checked against the batch of the call: ValueError), and
    members may be a ``CornerMembers``: the members of every term are then the corners the fitness would pick on the term's own
    reference, under the shared [H, W] mask if one is given ("The corner members"); ``with_members(m)`` sets them
    on an objective that exists.  ValueError: a per-sample mask or members without a score, or both together.

    The defaults are a design choice: radius 7 is a 15-pixel window, the fitness path's ``lk_win``; eps 1e-2 is in units of summed
    squared gradients of images in [0, 1] (a 15 x 15 window over an edge of contrast 0.1 sums to about 0.1), so it damps flat windows
    and leaves textured ones alone.  ValueError: radius outside 1 .. 16, eps not finite or <= 0, a direction that is not
    [2, H, W] or not finite, a mask that is not [H, W] or counts no pixel, a reference that is neither "constant" nor "moving".

    ``pairing`` is "frame": the reference of term s is frame s + 1.  For a repeated still that is "still -> extended prediction", what
    the single-image fitness path (``get_vectors``, ``PAIR_SINGLE``) scores.  ``PredictionFlow`` is the other pairing."""

    pairing = "frame"

    def __init__(self, radius=7, eps=1e-2, direction=None, mask=None, score=None, members=None, reference="constant"):
        if isinstance(members, str) and reference == "constant":
            members, reference = None, members      # `reference` was the sixth positional argument before `members` existed: such a call still means it
        if reference not in FLOW_REFERENCES:
            raise ValueError("reference must be one of %s, got %r" % (", ".join(FLOW_REFERENCES), reference))
        self.reference = reference
        if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= FLOW_MAX_RADIUS:
            raise ValueError("radius must be an integer in 1 .. %d, got %r" % (FLOW_MAX_RADIUS, radius))
        eps = float(eps)
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError("eps must be finite and > 0, got %r" % (eps,))
        self.radius, self.eps = int(radius), eps
        self.direction = self.mask = None
        if direction is not None:
            d = np.ascontiguousarray(direction, dtype=np.float32)
            if d.ndim != 3 or d.shape[0] != 2:
                raise ValueError("direction must be [2, H, W], got shape %s" % (d.shape,))
            if not np.isfinite(d).all():
                raise ValueError("direction must be finite")
            self.direction = d
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if m.ndim not in (2, 3):
                raise ValueError("mask must be [H, W] or, one plane per sample, [n, H, W]; got shape %s" % (m.shape,))
            if not m.any():
                raise ValueError("the mask counts no pixel")
            self.mask = m
        self._dev = {}
        self.score = self.members = None
        self.solve = None       # ``solved``: (levels, iters) of eigen_dense_solve; None is the single regularised step
        if score is not None:
            self.scored(score)
        self.with_members(members)
        if self.pairing == "frame":     # a PredictionFlow takes its score after construction (``scored``): checked at its first use
            self.check_members()

    def check_members(self):
        """ValueError: a per-sample mask without a score (``with_members`` refuses members without one)"""
        if self.score is None and (self.members is not None or self.per_sample):
            raise ValueError("a per-sample [n, H, W] mask and members need a score: the displacement modes divide by the shared mask's count")

    @property
    def per_sample(self):
        """whether the mask holds one plane per sample, [n, H, W]"""
        return self.mask is not None and self.mask.ndim == 3

    def with_members(self, members):
        """Set the membership of the score (a ``CornerMembers``; None: every pixel the mask counts) and return self.  ValueError: not a
        ``CornerMembers``, members on an objective without a score, or together with a per-sample [n, H, W] mask (a shared [H, W] mask
        is what combines with corners)."""
        if members is not None:
            if not isinstance(members, CornerMembers):
                raise ValueError("members must be a CornerMembers or None, got %r" % (members,))
            if self.score is None:
                raise ValueError("members need a score: the displacement modes divide by the shared mask's count")
            if self.per_sample:
                raise ValueError("a per-sample [n, H, W] mask does not go with CornerMembers: a shared [H, W] mask is what combines with corners")
        self.members = members
        return self

    def members_settings(self, n, h, w):
        """eigen_flow_members of a call of batch n on [h, w] images, or None where the objective has neither a per-sample mask nor members.
        ValueError: a per-sample mask that is not [n, h, w]."""
        if self.members is not None:
            return self.members.settings()
        if not self.per_sample:
            return None
        if tuple(self.mask.shape) != (n, h, w):
            raise ValueError("the per-sample mask is %s, the call is [%d, %d, %d]" % (self.mask.shape, n, h, w))
        return FlowMembersSettings(FLOW_MEMBERS_MASK, 0, 0, 0, 0.0, 0.0, h * w)

    def scored(self, score):
        """Set the score mode (a ``FlowScore``, or a structure score: ``BandsScore``, ``FreeScore``; None: the displacement modes) and return
        self.  ValueError: none of these, or a score on an objective with a direction field."""
        if score is not None and not isinstance(score, FLOW_SCORES):
            raise ValueError("score must be a FlowScore, a BandsScore, a FreeScore or None, got %r" % (score,))
        if score is not None and self.direction is not None:
            raise ValueError("a score takes no direction field")
        if score is None and (getattr(self, "members", None) is not None or self.per_sample):
            raise ValueError("a per-sample mask and members need a score")
        self.score = score
        return self

    def solved(self, levels=1, iters=1):
        """Set the solve of the stage (eigen_dense_solve; DESIGN.md section 13, "The iterated solve's gradient") and return self: the
        term's field is then Lucas-Kanade over `levels` pyramid levels with `iters` window iterations per level, what
        ``fitness.DenseFitness(levels=, iters=)`` scores, and the seed and the reference gradient are the exact gradient through every
        iteration and level.  (1, 1) is the single regularised step and leaves the objective on today's entries.  ValueError: levels
        outside 1 .. 6, iters outside 1 .. 32; a coarsest level below 4 pixels is refused by the call that knows the image
        (``solve_on``)."""
        for name, v, top in (("levels", levels, SOLVE_MAX_LEVELS), ("iters", iters, SOLVE_MAX_ITERS)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= top:
                raise ValueError("%s %r outside 1 .. %d" % (name, v, top))
        self.solve = (int(levels), int(iters))
        return self

    @property
    def real_solve(self):
        """whether the objective carries a solve other than the single step's (1, 1)"""
        return self.solve is not None and self.solve != (1, 1)

    def solve_on(self, w, h):
        """eigen_dense_solve of the objective against a w x h image, or None for the single step.  ValueError: the coarsest level would
        be below 4 pixels on its shorter side."""
        if not self.real_solve:
            return None
        cw, ch = int(w), int(h)
        for _ in range(self.solve[0] - 1):
            cw, ch = (cw + 1) // 2, (ch + 1) // 2
        if min(cw, ch) < SOLVE_MIN_COARSE:
            raise ValueError("levels %d: the coarsest level of a %d x %d image is %d x %d, below %d pixels" % (self.solve[0], w, h, cw, ch, SOLVE_MIN_COARSE))
        return engine.DenseSolveC(*self.solve)

    def settings(self, stage_alone=False):
        """eigen_flow_settings; the stage-alone entries take no flags (the reference gradient is asked for by the entry called)"""
        return FlowSettings(self.radius, FLOW_MOVING_REFERENCE if self.reference == "moving" and not stage_alone else 0, self.eps)

    def on_device(self, torch, device, h, w):
        """(direction, mask) as device tensors (None where not set), uploaded once per device; ValueError if they are not [.., h, w]"""
        self.check_members()
        for name, a in (("direction", self.direction), ("mask", self.mask)):
            if a is not None and tuple(a.shape[-2:]) != (h, w):
                raise ValueError("%s is %s, the trainer's image is [%d, %d]" % (name, a.shape, h, w))
        if device not in self._dev:
            up = lambda a: None if a is None else torch.from_numpy(a).cuda(device)
            self._dev[device] = (up(self.direction), up(self.mask))
        return self._dev[device]


class PredictionFlow(FlowObjective):
    """``objective="flow"`` with the pairing of the population fitness ("The prediction pairing"): the reference of
    term s is the previous PREDICTION P0_{s-1}, a float image that is itself part of the graph, in place of frame s + 1; for s = 0 it
    is the start state's P of layer 0 (zeros after a reset, the kept P of a continued call), a constant.  Term s is then the flow from
    P0_{s-1} to P0_s, and its gradient enters the backward pass twice: by P0_s as before, and by P0_{s-1} one step earlier.  With the
    weight on the term "prediction after the last fed frame -> first extended prediction" alone (``refine_stills``' default under this
    class) the loss is the dense stand-in for what ``get_fitnesses_neat`` / ``eval_images(pairing=PAIR_POPULATION)`` score.  Frames are no
    references here: a frame gradient is the input path alone, which is the whole gradient, and there is no `reference` argument.
    radius, eps, direction, mask: as ``FlowObjective``; the score mode is set by ``PredictionFlow(...).scored(FlowScore(...))`` or by
    ``make_flow("prediction", score=...)``, corner members by ``.with_members(CornerMembers(...))`` behind it or by ``make_flow``'s
    `members`.  A per-sample [n, H, W] mask needs a score by the first call that uses the objective (ValueError there)."""

    pairing = "prediction"

    def __init__(self, radius=7, eps=1e-2, direction=None, mask=None):
        super().__init__(radius, eps, direction, mask)


def make_flow(pairing="frame", radius=7, eps=1e-2, direction=None, mask=None, reference="constant", score=None, members=None, levels=1, iters=1):
    """The flow objective of a command line: a ``FlowObjective`` (pairing "frame", with its `reference`) or a ``PredictionFlow``
    (pairing "prediction"; it has no frame as a reference, so reference="moving" is a ValueError).  levels, iters: the solve
    (``FlowObjective.solved``); 1 and 1, the default, is the single step and leaves the objective as it was without them."""
    if pairing not in FLOW_PAIRINGS:
        raise ValueError("pairing must be one of %s, got %r" % (", ".join(FLOW_PAIRINGS), pairing))
    if pairing == "frame":
        flow = FlowObjective(radius, eps, direction, mask, reference=reference, score=score, members=members)
    else:
        if reference != "constant":
            raise ValueError("the prediction pairing has no frame as a reference: reference=%r does not go with it" % (reference,))
        flow = PredictionFlow(radius, eps, direction, mask).scored(score).with_members(members)
        flow.check_members()
    return flow if (levels, iters) == (1, 1) else flow.solved(levels, iters)


def _entry_key(flow, target=None, joint=False):
    """the key of _ENTRIES of a flow objective: "joint" for a call with a frame weight or validity planes; "target" for a call with a
    target field; "iter" under a real solve; else its pairing, the kind of its score, or "members" with a per-sample mask or corner members"""
    if joint:
        return "joint"
    if target is not None:
        return "target"
    if flow.real_solve:
        return "iter"
    if flow.score is None:
        return flow.pairing
    if flow.members is not None or flow.per_sample:
        return "members"
    return "score" if isinstance(flow.score, FlowScore) else "structure"


def _check_flow(objective, flow):
    """`flow` goes with objective="flow" and with nothing else"""
    if objective == "flow":
        if not isinstance(flow, FlowObjective):
            raise ValueError("objective='flow' needs flow=FlowObjective(...), got %r" % (flow,))
    elif flow is not None:
        raise ValueError("flow is given but the objective is %r" % (objective,))


def check_flow_target(objective, flow, target, shape):
    """The rules of a target field (``forward_backward(flow_target=)``, ``flow_term(target=)``) against the `shape` the call expects,
    [n, T - 1, 2, H, W] or, for the stage alone, [n, 2, H, W]: -> None without a target, else its leading strides in doubles (one per
    leading dimension).  The target is a float64 numpy array or torch tensor whose last three dimensions are contiguous.  ValueError: a
    target without objective="flow"; under an objective that carries a direction, a score, members or a per-sample mask (the target is a
    displacement mode of its own, and these modes divide by the shared mask's count); a wrong dtype or shape; last dimensions that are
    not contiguous."""
    if target is None:
        return None
    if objective != "flow" or not isinstance(flow, FlowObjective):
        raise ValueError("flow_target goes with objective='flow' and a FlowObjective, got objective %r" % (objective,))
    if flow.direction is not None or flow.score is not None or flow.members is not None or flow.per_sample:
        raise ValueError("a flow target takes no direction, score, members or per-sample mask")
    by_numpy = isinstance(target, np.ndarray)
    if not by_numpy and not (hasattr(target, "data_ptr") and hasattr(target, "stride")):
        raise ValueError("the flow target must be a float64 numpy array or torch tensor, got %r" % (type(target),))
    if (target.dtype != np.float64) if by_numpy else (str(target.dtype) != "torch.float64"):
        raise ValueError("the flow target must be float64, got %s" % (target.dtype,))
    shape = tuple(int(v) for v in shape)
    if tuple(target.shape) != shape:
        raise ValueError("the flow target must be %s, got %s" % (list(shape), list(target.shape)))
    strides = [int(v) // 8 for v in target.strides] if by_numpy else [int(v) for v in target.stride()]
    h, w = shape[-2:]
    if strides[-3:] != [h * w, w, 1]:
        raise ValueError("the last three dimensions of the flow target must be contiguous, got strides %s" % (strides,))
    return strides[:-3]


def check_frame_weight(objective, frame_weight):
    """The rules of ``forward_backward(frame_weight=)``: -> None without one, else the weight as a float.  ValueError: a weight that is no
    number, not finite or not > 0 (None is "no frame term"); a weight under an objective other than "flow" (the joint objective is the
    flow objective plus frame_weight times the squared error; the error-unit objective as the frame term is not offered)."""
    if frame_weight is None:
        return None
    if isinstance(frame_weight, (bool, np.bool_)) or not isinstance(frame_weight, (int, float, np.integer, np.floating)):
        raise ValueError("frame_weight must be a number, got %r" % (frame_weight,))
    mu = float(frame_weight)
    if not (np.isfinite(mu) and mu > 0):
        raise ValueError("frame_weight must be None (no frame term) or finite and > 0, got %r" % (frame_weight,))
    if objective != "flow":
        raise ValueError("frame_weight goes with objective='flow', got objective %r" % (objective,))
    return mu


def check_flow_valid(objective, flow, target, valid, shape):
    """The rules of validity planes (``forward_backward(flow_valid=)``, ``flow_term_valid``) against the `shape` the call expects,
    [n, T - 1, H, W] or, for the stage alone, [n, H, W]: -> None without planes, else their leading strides in bytes (one per leading
    dimension).  The planes are a uint8 or bool numpy array or torch tensor whose last two dimensions are contiguous; a pixel counts
    where its byte is not zero.  ValueError: planes without a target field (they weigh a target's endpoint error; `target` None) or
    without objective="flow"; a wrong dtype or shape; last dimensions that are not contiguous."""
    if valid is None:
        return None
    if objective != "flow" or not isinstance(flow, FlowObjective) or target is None:
        raise ValueError("flow_valid goes with objective='flow' and a flow target, got objective %r and %s target" % (objective, "no" if target is None else "a"))
    by_numpy = isinstance(valid, np.ndarray)
    if not by_numpy and not (hasattr(valid, "data_ptr") and hasattr(valid, "stride")):
        raise ValueError("the validity planes must be a uint8 or bool numpy array or torch tensor, got %r" % (type(valid),))
    if str(valid.dtype) not in ("uint8", "bool", "torch.uint8", "torch.bool"):
        raise ValueError("the validity planes must be uint8 or bool, got %s" % (valid.dtype,))
    shape = tuple(int(v) for v in shape)
    if tuple(valid.shape) != shape:
        raise ValueError("the validity planes must be %s, got %s" % (list(shape), list(valid.shape)))
    strides = [int(v) for v in (valid.strides if by_numpy else valid.stride())]
    h, w = shape[-2:]
    if strides[-2:] != [w, 1]:
        raise ValueError("the last two dimensions of the validity planes must be contiguous, got strides %s" % (strides,))
    return strides[:-2]


def check_layer_weights(layer_weights, n_layers):
    """layer_weights as a contiguous float64 [n_layers] array, or None (L_0: [1, 0, ...]).  ValueError on another length; the
    value rules (>= 0, finite, not all zero) are the library's."""
    if layer_weights is None:
        return None
    lam = np.ascontiguousarray(layer_weights, dtype=np.float64)
    if lam.shape != (n_layers,):
        raise ValueError("layer_weights must have one entry per layer (%d), got shape %s" % (n_layers, lam.shape))
    return lam


def check_optim(clip_norm=None, weight_decay=0.0, skip_nonfinite=False):
    """The optimiser controls of ``PredNetTrainer`` as (clip_norm: None or float > 0, weight_decay: float >= 0, skip_nonfinite: bool).
    ValueError: a clip_norm that is not None and not finite or <= 0 (None is "no clipping"), a weight_decay that is negative or not
    finite, a skip_nonfinite that is not a bool, a bool or a non-number where a number goes."""
    def number(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s must be a number, got %r" % (name, v))
        return float(v)
    if clip_norm is not None:
        clip_norm = number("clip_norm", clip_norm)
        if not (np.isfinite(clip_norm) and clip_norm > 0):
            raise ValueError("clip_norm must be None (no clipping) or finite and > 0, got %r" % (clip_norm,))
    weight_decay = number("weight_decay", weight_decay)
    if not (np.isfinite(weight_decay) and weight_decay >= 0):
        raise ValueError("weight_decay must be finite and >= 0, got %r" % (weight_decay,))
    if not isinstance(skip_nonfinite, (bool, np.bool_)):
        raise ValueError("skip_nonfinite must be True or False, got %r" % (skip_nonfinite,))
    return clip_norm, weight_decay, bool(skip_nonfinite)


def optim_is_neutral(clip_norm, weight_decay, skip_nonfinite):
    """whether the three controls leave ``adam()`` on the plain entry"""
    return clip_norm is None and weight_decay == 0.0 and not skip_nonfinite


def check_micro_batches(n, micro_batches, batch, reset=True, flow=None):
    """The rules of ``PredNetTrainer.step(micro_batches=k)`` for n sequences on a handle of `batch`: -> n / k, the sequences per chunk.
    ValueError: k not an integer >= 1; and for k > 1: n not a multiple of k, n / k above the handle's batch, reset=False (the handle
    keeps one sequence state per batch, not one per chunk), a flow objective with a per-sample [n, H, W] mask (not sliced here)."""
    k = micro_batches
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("micro_batches must be an integer >= 1, got %r" % (k,))
    k = int(k)
    if k == 1:
        return int(n)
    if n % k:
        raise ValueError("%d sequences do not divide into %d micro-batches" % (n, k))
    if n // k > batch:
        raise ValueError("a micro-batch of %d sequences exceeds the trainer's batch %d" % (n // k, batch))
    if not reset:
        raise ValueError("micro_batches > 1 needs reset=True: the handle keeps one sequence state per batch, not one per micro-batch")
    if flow is not None and getattr(flow, "per_sample", False):
        raise ValueError("a per-sample [n, H, W] flow mask is not sliced across micro-batches")
    return n // k


def combine_terms(table, layer_weights=None, step_weights=None):
    """The loss of the error-unit objective from the table err[s][l] (float64 [T - 1, L]), as the library forms it: in double,
    sum_s w_s (sum_l lambda_l err[s][l]) / sum_s w_s, added in (step, layer) order.  layer_weights None: L_0, [1, 0, ...];
    step_weights None: all one.  An empty table (T = 1) gives 0."""
    table = np.asarray(table, np.float64)
    if table.ndim != 2:
        raise ValueError("table must be [T - 1, L], got shape %s" % (table.shape,))
    n, L = table.shape
    lam = check_layer_weights(layer_weights, L)
    lam = [1.0] + [0.0] * (L - 1) if lam is None else [float(v) for v in lam]
    if step_weights is None:
        w = [1.0] * n
    else:
        w = [float(v) for v in np.asarray(step_weights, np.float64).ravel()]
        if len(w) != n:
            raise ValueError("step_weights must have T - 1 = %d entries, got %d" % (n, len(w)))
    bad = [v for v in lam + w if not (v >= 0.0 and np.isfinite(v))]
    if bad or not sum(lam) > 0.0 or (n and not sum(w) > 0.0):
        raise ValueError("weights must be finite, >= 0 and not all zero")
    if n == 0:
        return 0.0
    acc, tot = 0.0, 0.0
    for s in range(n):
        row = 0.0
        for l in range(L):
            row += lam[l] * float(table[s, l])
        acc += w[s] * row
        tot += w[s]
    return acc / tot


def seq_state_shapes(channels, w, h, batch):
    """Shapes of the kept sequence state: [(batch, C_l, H_l, W_l) for each layer]."""
    return [(int(batch), int(c), int(h) >> l, int(w) >> l) for l, c in enumerate(channels)]


def check_state(state, channels, w, h, max_batch=None):
    """Validate a ``PredNetTrainer.state_dict()``-shaped dict against a network; returns it with every array float32 and
    contiguous.  Raises ValueError on a missing or extra tensor, a wrong shape or a non-float dtype."""
    shapes = tensor_shapes(channels, w, h)
    out = {"adam_t": int(state["adam_t"]), "hyper": {k: float(v) for k, v in dict(state.get("hyper") or {}).items()}}
    if out["adam_t"] < 0:
        raise ValueError("adam_t must be >= 0, got %d" % out["adam_t"])
    if state.get("optim") is not None:      # the optimiser controls travel only when one of them is not neutral
        opt = dict(state["optim"])
        if set(opt) - set(OPTIM):
            raise ValueError("optim holds unknown settings %s" % sorted(set(opt) - set(OPTIM)))
        out["optim"] = dict(zip(OPTIM, check_optim(**opt)))
    for key in ("adam_m", "adam_v"):
        tab = state[key]
        if sorted(tab) != sorted(shapes):
            raise ValueError("%s holds %d tensors, expected the %d of %d layers" % (key, len(tab), len(shapes), len(channels)))
        out[key] = {}
        for n, shp in shapes.items():
            a = np.asarray(tab[n])
            if a.dtype.kind != "f" or a.shape != shp:
                raise ValueError("%s[%r] is %s %s, expected float32 %s" % (key, n, a.dtype, a.shape, shp))
            out[key][n] = np.ascontiguousarray(a, dtype=np.float32)
    seq = state.get("seq")
    out["seq"] = None
    if seq is not None:
        if sorted(seq) != sorted(SEQ_PARTS) or any(len(seq[k]) != len(channels) for k in SEQ_PARTS):
            raise ValueError("seq must hold h, c and P with one array per layer (%d)" % len(channels))
        batch = int(np.asarray(seq["h"][0]).shape[0]) if np.asarray(seq["h"][0]).ndim == 4 else -1
        if batch < 1 or (max_batch is not None and batch > max_batch):
            raise ValueError("sequence state of batch %d does not fit this trainer (batch %s)" % (batch, max_batch))
        want = seq_state_shapes(channels, w, h, batch)
        out["seq"] = {}
        for k in SEQ_PARTS:
            out["seq"][k] = []
            for l, shp in enumerate(want):
                a = np.asarray(seq[k][l])
                if a.dtype.kind != "f" or a.shape != shp:
                    raise ValueError("seq[%r][%d] is %s %s, expected float32 %s" % (k, l, a.dtype, a.shape, shp))
                out["seq"][k].append(np.ascontiguousarray(a, dtype=np.float32))
    return out


def write_checkpoint(path, weights, state):
    """ONE npz: the weights under the ``predictor/<name>`` keys of ``weights.save_chainer_npz`` (so ``weights.load_chainer_npz``
    reads the file), plus ``adam/m/<name>``, ``adam/v/<name>``, ``adam/t``, ``hyper/<alpha|beta1|beta2|eps>``, when a sequence
    state is kept ``seq/<h|c|P>/<layer>``, and, when state["optim"] holds a control that is not neutral,
    ``optim/<clip_norm|weight_decay|skip_nonfinite>`` (clip_norm 0: none).  A neutral trainer's file has no ``optim/*`` entry."""
    arrs = {"predictor/" + k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weights.items()}
    for k, v in state["adam_m"].items():
        arrs["adam/m/" + k] = np.ascontiguousarray(v, dtype=np.float32)
    for k, v in state["adam_v"].items():
        arrs["adam/v/" + k] = np.ascontiguousarray(v, dtype=np.float32)
    arrs["adam/t"] = np.asarray(int(state["adam_t"]), np.int64)
    for k, v in (state.get("hyper") or {}).items():
        arrs["hyper/" + k] = np.asarray(float(v), np.float64)
    if state.get("optim") is not None and not optim_is_neutral(*check_optim(**state["optim"])):
        clip, wd, skip = check_optim(**state["optim"])
        arrs["optim/clip_norm"] = np.asarray(0.0 if clip is None else clip, np.float64)     # 0: no clipping, as eigen_adam_settings spells it
        arrs["optim/weight_decay"] = np.asarray(wd, np.float64)
        arrs["optim/skip_nonfinite"] = np.asarray(int(skip), np.int64)
    if state.get("seq") is not None:
        for part in SEQ_PARTS:
            for l, a in enumerate(state["seq"][part]):
                arrs["seq/%s/%d" % (part, l)] = np.ascontiguousarray(a, dtype=np.float32)
    with open(path, "wb") as f:   # (a file object: np.savez would append .npz to a bare name)
        np.savez(f, **arrs)


def read_checkpoint(path, channels, w, h):
    """-> (weights, state) of a ``write_checkpoint`` file, every shape checked against the network (ValueError / KeyError)."""
    from .weights import load_chainer_npz
    wts = load_chainer_npz(path, channels, w, h)
    with np.load(path) as z:
        files = set(z.files)
        for n in wts:
            for mv in "mv":
                if "adam/%s/%s" % (mv, n) not in files:
                    raise KeyError("checkpoint %s lacks adam/%s/%s" % (path, mv, n))
        if "adam/t" not in files:
            raise KeyError("checkpoint %s lacks adam/t" % path)
        state = {"adam_m": {n: z["adam/m/" + n] for n in wts}, "adam_v": {n: z["adam/v/" + n] for n in wts}, "adam_t": int(z["adam/t"]),
                 "hyper": {k: float(z["hyper/" + k]) for k in HYPER if "hyper/" + k in files}, "seq": None}
        if any(("optim/" + k) in files for k in OPTIM):     # a file without them (a neutral or an earlier trainer's) loads as neutral
            clip = float(z["optim/clip_norm"]) if "optim/clip_norm" in files else 0.0
            state["optim"] = {"clip_norm": clip if clip != 0.0 else None,
                              "weight_decay": float(z["optim/weight_decay"]) if "optim/weight_decay" in files else 0.0,
                              "skip_nonfinite": bool(int(z["optim/skip_nonfinite"])) if "optim/skip_nonfinite" in files else False}
        if "seq/h/0" in files:
            try:
                state["seq"] = {part: [z["seq/%s/%d" % (part, l)] for l in range(len(channels))] for part in SEQ_PARTS}
            except KeyError as e:
                raise KeyError("checkpoint %s: incomplete sequence state (%s)" % (path, e))
    return wts, check_state(state, channels, w, h)


class PredNetTrainer:
    """One trainer handle on the current HIP device.  batch and max_steps size the tape (``tape_bytes``).

    model_name: anything ``fitness._resolve_weights`` takes (a weight dict, ``"synthetic[:seed]"`` or a chainer npz path): the
    starting weights.  alpha, beta1, beta2, eps: Adam (chainer's defaults).

    The optimiser controls ("Optimiser controls"; ``check_optim`` states their rules, ValueError): clip_norm, None
    or the global L2 norm above which the gradient of a step is scaled down to it (chainer's GradientClipping); weight_decay, the
    weight_decay_rate of chainer's AdamRule, p -= lr_t m / (sqrt(v) + eps) + weight_decay p; skip_nonfinite, a step whose gradient
    norm is not finite is not taken.  They are plain attributes and may be changed between steps.  With all three neutral (the
    defaults) ``adam()`` is the plain entry and its bits; otherwise it leaves what it did in ``last_update``."""

    def __init__(self, model_name, channels, w, h, batch, max_steps, alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, device=None, clip_norm=None,
                 weight_decay=0.0, skip_nonfinite=False):
        import torch
        from .fitness import _local_device, _resolve_weights
        self.clip_norm, self.weight_decay, self.skip_nonfinite = check_optim(clip_norm, weight_decay, skip_nonfinite)
        self.last_update = {"norm": None, "rate": None, "applied": None}
        self.last_loss_parts = None  # (L_flow, L_mse) of the last call with a frame_weight
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
        """Load a weight table; clears the Adam moments and step count, any kept sequence state and what was accumulated."""
        arrs = []
        for n in self._names:
            a = np.ascontiguousarray(weights[n], dtype=np.float32)
            if a.shape != self._shapes[n]:
                raise ValueError("tensor %r has shape %s, expected %s" % (n, a.shape, self._shapes[n]))
            arrs.append(a)
        _check(self.lib.eigen_trainer_set_weights(self._h, self._table(arrs), ctypes.c_int32(len(arrs))))

    @staticmethod
    def _table(arrays):
        """the ctypes table of the data pointers of a list of arrays (which the caller keeps alive)"""
        return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])

    def _empty(self):
        return {n: np.empty(self._shapes[n], np.float32) for n in self._names}

    def _read(self, fn):
        out = self._empty()
        _check(fn(self._h, self._table([out[n] for n in self._names]), ctypes.c_int32(len(self._names))))
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

    def _call_args(self, frames, n_fed):
        """What forward_backward and evaluate pass alike: the frames on the device, (n, T), n_fed (None: T; the range rules are the
        library's: EngineError -1) and the byte stride between sequences."""
        d = self._frames(frames)
        n, T = int(d.shape[0]), int(d.shape[1])
        return d, n, T, T if n_fed is None else int(n_fed), ctypes.c_int64(T * int(np.prod(d.shape[2:])))

    def _outputs(self, d, table, pred):
        """The outputs a call asked for, None where not wanted: the float64 [max(T - 1, 1), L] table of error-unit means and the
        device tensor of predictions.  Made once every argument has passed its checks."""
        tab = np.zeros((max(int(d.shape[1]) - 1, 1), len(self.channels)), np.float64) if table else None
        return tab, self._torch.empty(tuple(d.shape), dtype=self._torch.float32, device=d.device) if pred else None

    def _target(self, objective, flow, target, shape):
        """A target field on the device and its leading strides as c_int64 (``check_flow_target`` states the rules), or (None, [])"""
        if target is None:
            return None, []
        torch = self._torch
        if isinstance(target, np.ndarray) or not target.is_cuda:
            check_flow_target(objective, flow, target if isinstance(target, np.ndarray) else target.contiguous(), shape)
            target = (torch.from_numpy(np.ascontiguousarray(target)) if isinstance(target, np.ndarray) else target.contiguous()).cuda(self.device)
        return target, [ctypes.c_int64(v) for v in check_flow_target(objective, flow, target, shape)]

    def _valid(self, objective, flow, target, valid, shape):
        """Validity planes on the device and their leading strides in bytes as c_int64 (``check_flow_valid`` states the rules), or (None, [])"""
        if valid is None:
            return None, []
        torch = self._torch
        if isinstance(valid, np.ndarray) or not valid.is_cuda:
            check_flow_valid(objective, flow, target, valid if isinstance(valid, np.ndarray) else valid.contiguous(), shape)
            valid = (torch.from_numpy(np.ascontiguousarray(valid)) if isinstance(valid, np.ndarray) else valid.contiguous()).cuda(self.device)
        return valid, [ctypes.c_int64(v) for v in check_flow_valid(objective, flow, target, valid, shape)]

    def _loss_grad(self, d, n, T, n_fed, bstride, reset, pred, stream, requant, step_weights, objective, layer_weights, layer_errors, frame_grads,
                   flow_target=None, frame_weight=None, flow_valid=None, flow=None):
        """The call behind forward_backward, on frames already on the device: (loss, table or None, d_pred or None, d_grad or None), the
        last two device tensors.  Every argument is checked before anything is launched.  Under objective="flow" the float64 [T - 1]
        terms of the call are left in ``self.last_flow_terms``; under a per-sample mask or corner members the float64 [T - 1, n, 10] records
        of the samples of every computed term (zeros for the others) are left in ``self.last_flow_stats``, which any other call leaves as it is.
        A call with a frame_weight leaves (L_flow, L_mse) in ``self.last_loss_parts``, which any other call leaves as it is."""
        torch = self._torch
        if isinstance(flow_target, FlowObjective) and flow is None:     # `flow` was the positional argument here before `flow_target` existed
            flow_target, flow = None, flow_target
        if objective not in OBJECTIVES:
            raise ValueError("objective must be one of %s, got %r" % (sorted(OBJECTIVES), objective))
        _check_flow(objective, flow)
        by_flow = objective == "flow"
        mu = check_frame_weight(objective, frame_weight)
        d_target, t_strides = self._target(objective, flow, flow_target, (n, max(T - 1, 0), 2, self.h, self.w))
        d_valid, v_strides = self._valid(objective, flow, d_target, flow_valid, (n, max(T - 1, 0), self.h, self.w))
        joint = mu is not None or d_valid is not None
        d_dir, d_mask = flow.on_device(torch, self.device, self.h, self.w) if by_flow else (None, None)
        lam = check_layer_weights(layer_weights, len(self.channels))
        w_arr = None
        if step_weights is not None:
            w_arr = np.ascontiguousarray(step_weights, dtype=np.float64)
            if w_arr.shape != (T - 1,):
                raise ValueError("step_weights must have T - 1 = %d entries, got shape %s" % (T - 1, w_arr.shape))
        loss = ctypes.c_double(0.0)
        by_error = objective == "error"
        table, d_pred = self._outputs(d, layer_errors or by_error, pred)
        args = [self._h, _ptr(d), bstride, ctypes.c_int32(n), ctypes.c_int32(T), ctypes.c_int32(n_fed), ctypes.c_int32(int(bool(requant))),
                ctypes.c_int32(int(bool(reset))), ctypes.c_void_p(w_arr.ctypes.data if w_arr is not None and w_arr.size else None),
                ctypes.c_int32(OBJECTIVES[objective]), _ptr(lam), ctypes.byref(loss), _ptr(table), _ptr(d_pred)]
        d_grad, g_b, g_t = None, 0, 0
        if frame_grads is not None:
            img = tuple(d.shape[2:])
            d_grad = torch.empty((n,) + (() if frame_grads == "tied" else (T,)) + img, dtype=torch.float32, device=d.device)
            per = int(np.prod(img))
            g_b, g_t = (per, 0) if frame_grads == "tied" else (T * per, per)
        tails = {"frame_grad": [_ptr(d_grad), ctypes.c_int64(g_b), ctypes.c_int64(g_t)]}
        after_stream = []   # what an entry takes behind its stream: the solve of eigen_trainer_loss_grad_flow_iter
        if by_flow:
            terms = np.zeros(max(T - 1, 1), np.float64)
            cfg = flow.settings()
            tails["flow"] = [ctypes.byref(cfg), _ptr(d_dir), _ptr(d_mask), _ptr(terms)]
            tails["pairing"] = [ctypes.c_int32(FLOW_PAIRINGS[flow.pairing])]
            stats = None
            solve = flow.solve_on(self.w, self.h)      # the coarsest-level rule, before any call
            if solve is not None:
                tails["members"] = [None, None, None, None]    # the displacement modes; a score fills it in below
                after_stream = [ctypes.byref(solve)]
            if flow.score is not None:
                sc = flow.score.settings(self.h)
                tails["score"] = [ctypes.byref(sc)]
                mem = flow.members_settings(n, self.h, self.w)
                by_circles = isinstance(flow.score, FlowScore)
                if mem is not None:
                    # the widest entry: both scores (one of them NULL), the members and the records of every computed term
                    stats = np.zeros((max(T - 1, 1), n, len(SCORE_STATS)), np.float64)
                    tails["members"] = [ctypes.byref(sc) if by_circles else None, None if by_circles else ctypes.byref(sc), ctypes.byref(mem), _ptr(stats)]
                elif solve is not None:
                    tails["members"] = [ctypes.byref(sc) if by_circles else None, None if by_circles else ctypes.byref(sc), None, None]
            if d_target is not None:
                # eigen_trainer_loss_grad_flow_target: no score or members go with a target; the solve (NULL: the single step), then the target
                tails["members"] = [None, None, None, None]
                after_stream = [ctypes.byref(solve) if solve is not None else None, _ptr(d_target)] + t_strides
            if joint:
                # eigen_trainer_loss_grad_flow_joint: the target entry's arguments whatever the mode (a score or members fill theirs in, the
                # direction is in the flow group, the target may be NULL), then the record
                parts = np.zeros(2, np.float64)
                v_b, v_t = [v.value for v in v_strides] if v_strides else (0, 0)
                rec = FlowJointSettings(0.0 if mu is None else mu, d_valid.data_ptr() if d_valid is not None else None, v_b, v_t, parts.ctypes.data)
                if "members" not in tails:
                    tails["members"] = [None, None, None, None]
                    if flow.score is not None:
                        tails["members"] = [ctypes.byref(sc) if by_circles else None, None if by_circles else ctypes.byref(sc), None, None]
                if d_target is None:
                    after_stream = [ctypes.byref(solve) if solve is not None else None, None, ctypes.c_int64(0), ctypes.c_int64(0)]
                after_stream = after_stream + [ctypes.byref(rec)]
        entry, groups = _ENTRIES[by_flow, _entry_key(flow, d_target, joint) if by_flow else frame_grads is not None]
        _check(getattr(self.lib, entry)(*args, *[a for g in groups for a in tails[g]], _stream_arg(stream), *after_stream))
        if by_flow:
            self.last_flow_terms = terms[:T - 1]
            if mu is not None:
                self.last_loss_parts = (float(parts[0]), float(parts[1]))
            if stats is not None:       # the members entry alone returns records: any other call leaves what an earlier one left
                self.last_flow_stats = stats[:T - 1]
        if table is not None:
            table = table[:T - 1]
        value = combine_terms(table, lam, w_arr if w_arr is not None and w_arr.size else None) if by_error else loss.value
        return value, table, d_pred, d_grad

    def forward_backward(self, frames, reset=True, pred=False, stream=None, n_fed=None, requant=False, step_weights=None, objective="mse",
                         layer_weights=None, layer_errors=False, frame_grads=None, flow_terms=False, flow_target=None, frame_weight=None, flow_valid=None,
                         flow=None):
        """Loss of frames uint8 [n, T, C, H, W] (numpy or a device tensor, n <= batch) and the gradients, kept on the device
        (``grads()``).  reset=False continues from the state the previous call left (the same n), as a constant.
        pred=True also returns the float predictions P0 [n, T, C, H, W] (numpy).

        n_fed: the first n_fed steps read their frame, the rest are fed the previous prediction (None: all T read theirs);
        requant: feed the prediction back through the byte the inference engine emits, as a constant; step_weights: T - 1
        weights >= 0 of the loss terms (term s: prediction s against frame s + 1), None: all one.

        objective: "mse", the squared error of the image-layer prediction, or "error", PredNet's own objective: the means of
        the error units err[s][l] (layer 0 against the true next frame, half the mean absolute error; layers above as the
        network computed them at step s + 1) weighted by layer_weights, one weight >= 0 per layer: None is L_0, [1, 0, ...];
        L_all is [1, 0.1, ...].  The loss is ``combine_terms`` of the table.  layer_errors=True appends the float64 [T - 1, L]
        table to the return value, under either objective.

        frame_grads: None, or the gradient of the loss by the frames (as floats, byte / 255), appended last as a float32 numpy
        array: "frames" gives d loss / d frame t, [n, T, C, H, W] (the input path of every step that read its frame plus the
        target path of every frame but the first); "tied" gives their sum over t, [n, C, H, W], the gradient by a still that
        is repeated T times.  Nothing else the call returns or leaves on the device changes.

        objective "flow" with flow=FlowObjective(...) (required then, refused otherwise): term s is the displacement a dense
        Lucas-Kanade solve finds from frame s + 1, a constant of the graph, to prediction s: its mean square, or its mean along the
        direction field ("The flow objective").  The frame gradient is then the input path alone, unless the
        FlowObjective has reference="moving": frame s + 1 is then in the graph as the reference of term s, and g_t = fl(input path of
        step t + reference path of term t - 1); "tied" starts from zero and for s = T - 1 .. 0 adds the reference path of term s, then
        the input path of step s.  Nothing else the call returns depends on that setting.
        With flow=PredictionFlow(...) term s runs from the previous prediction P0_{s-1} (for s = 0 the start state's P0: zeros after a
        reset) to prediction s, both in the graph ("The prediction pairing"); loss and terms are those of that
        pairing and the frame gradient is the input path alone.
        flow_terms=True (flow only) appends the float64 [T - 1] terms last; a term of weight zero is not computed and reads 0.

        flow_target: None, or the field every term's flow shall equal ("The target field"): float64
        [n, T - 1, 2, H, W], numpy or a device tensor (the last three dimensions contiguous, the strides of the first two are passed
        through), in the solve's own convention (content at x in the reference is at x + u in the prediction), which is how
        ``MovingTextures.batch(k, n, flow=True)[1]`` states its flow.  Term s is then the mean squared endpoint error of the solved
        field against flow_target[:, s], and takes the place of the mean squared displacement.  Under a ``FlowObjective`` term s runs
        from frame s + 1 to P0_s.  Under ``PredictionFlow`` term s runs from P0_{s-1} to P0_s, the predictions of frames s and
        s + 1: its truth is the motion from frame s to frame s + 1, which is flow[:, s] of a video's flow [n, T - 1, 2, H, W], so that
        array is passed as it is.  ``check_flow_target`` states the rules (ValueError).

        flow_valid: None, or the validity planes of the target ("The joint objective and the valid pixels"): uint8 or
        bool [n, T - 1, H, W], numpy or a device tensor (the last two dimensions contiguous, the strides of the first two are passed
        through), as ``MovingTextures.batch(k, n, flow=True, valid=True)[3]`` states them.  A pixel of sample b counts in term s where the
        objective's shared mask counts it and flow_valid[b, s] is not zero; the term is the mean over the samples of each sample's mean
        squared endpoint error over its own counted pixels, and a sample that counts none contributes 0.  Only together with
        flow_target (``check_flow_valid``, ValueError).

        frame_weight: None, or mu > 0 (objective "flow" only, with any FlowObjective): the loss is L_flow + mu L_mse, the flow
        objective's loss plus mu times the squared error of the predictions against the next frames under the same step_weights, in
        one backward pass.  ``self.last_loss_parts`` is then (L_flow, L_mse): the losses of the same call without frame_weight and of
        the "mse" call with the same step_weights, to the bit.  A frame gradient holds the input path, the flow terms' reference
        paths under reference="moving" and mu times the squared error's target path.  ``check_frame_weight`` states the rules."""
        if isinstance(flow_target, FlowObjective) and flow is None:     # `flow` was the positional argument here before `flow_target` existed
            flow_target, flow = None, flow_target
        if frame_grads not in FRAME_GRADS:
            raise ValueError("frame_grads must be None, 'frames' or 'tied', got %r" % (frame_grads,))
        if flow_terms and objective != "flow":
            raise ValueError("flow_terms goes with objective='flow'")
        _check_flow(objective, flow)
        d, n, T, n_fed, bstride = self._call_args(frames, n_fed)
        value, table, d_pred, d_grad = self._loss_grad(d, n, T, n_fed, bstride, reset, pred, stream, requant, step_weights, objective, layer_weights,
                                                       layer_errors, frame_grads, flow=flow, flow_target=flow_target, frame_weight=frame_weight,
                                                       flow_valid=flow_valid)
        out = (value,) + ((d_pred.cpu().numpy(),) if pred else ()) + ((table,) if layer_errors else ()) + ((d_grad.cpu().numpy(),) if frame_grads else ())
        out += (self.last_flow_terms,) if flow_terms else ()
        return out[0] if len(out) == 1 else out

    def flow_members(self, ref, members, mask=None):
        """The membership stage alone (eigen_trainer_flow_members): ref uint8 or float32 [n, C, H, W], the references (a float one is
        clamped to [0, 1] and quantised as a self-fed step's byte is); members a ``CornerMembers``; mask [H, W], the shared plane
        (None: every pixel counts).  -> (uint8 [n, H, W], 1 at every corner the mask counts; int32 [n], the corners picked per
        sample, before the mask)."""
        torch = self._torch
        if not isinstance(members, CornerMembers):
            raise ValueError("members must be a CornerMembers, got %r" % (members,))
        shp = (self.channels[0], self.h, self.w)
        dev = "cuda:%d" % self.device
        r = (ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref))).to(dev).contiguous()
        if r.dtype not in (torch.uint8, torch.float32) or r.dim() != 4 or tuple(r.shape[1:]) != shp or not 1 <= int(r.shape[0]) <= self.batch:
            raise ValueError("ref must be uint8 or float32 [n, %d, %d, %d] with n <= %d; got %s %s" % (shp + (self.batch, r.dtype, tuple(r.shape))))
        d_mask = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if m.shape != (self.h, self.w):
                raise ValueError("mask must be [%d, %d], got %s" % (self.h, self.w, m.shape))
            d_mask = torch.from_numpy(m).to(dev)
        n = int(r.shape[0])
        planes, counts = np.zeros((n, self.h, self.w), np.uint8), np.zeros(n, np.int32)
        mem = members.settings()
        by_float = r.dtype == torch.float32
        _check(self.lib.eigen_trainer_flow_members(self._h, None if by_float else _ptr(r), _ptr(r) if by_float else None, ctypes.c_int64(int(np.prod(shp))),
                                                   ctypes.c_int32(n), ctypes.byref(mem), _ptr(d_mask), _ptr(planes), _ptr(counts), None))
        return planes, counts

    def flow_term(self, pred, ref, flow, scale=1.0, reference_grad=False, stats=False, target=None):
        """The flow stage alone (eigen_trainer_flow_term), with the kernels a training call runs: pred float32 [n, C, H, W], the
        prediction; ref uint8 [n, C, H, W], the reference frame; n <= batch.  -> (value, u, seed): the term, the flow float64
        [n, 2, H, W] in pixels per frame (x then y) and scale * d value / d pred as float32 [n, C, H, W].  reference_grad=True
        (eigen_trainer_flow_term_ref) appends scale * d value / d ref, by the reference as floats (byte / 255), float32
        [n, C, H, W]: what a training call adds to the frame gradient under reference="moving".  The FlowObjective's own `reference`
        plays no part here.  With a ``FlowScore`` on `flow` the stage runs in the score mode (eigen_trainer_flow_term_score), and
        stats=True (score only) appends the float64 [n, 10] record of the samples, ``SCORE_STATS``; either way a score-mode call
        leaves it in ``self.last_flow_stats`` (None after a call without a score).
        target: None, or float64 [n, 2, H, W] (eigen_trainer_flow_term_target): the value is then the mean squared endpoint error of u
        against it (``check_flow_target``)."""
        return self._flow_stage(pred, ref, False, flow, scale, reference_grad, stats, target)

    def flow_term_pair(self, pred, prev, flow, scale=1.0, reference_grad=False):
        """The flow stage alone on a pair of float images (eigen_trainer_flow_term_pair), with the kernels a training call runs under a
        ``PredictionFlow``: pred float32 [n, C, H, W], the prediction; prev float32 [n, C, H, W], the reference (the previous
        prediction); n <= batch.  -> (value, u, seed) as ``flow_term``; reference_grad=True appends scale * d value / d prev, float32
        [n, C, H, W]: what a training call adds to d loss / d P0_{s-1}.  The radius, eps, direction and mask of `flow` are used; its
        pairing and `reference` play no part here.  With a score on `flow` the stage runs in the score mode and leaves the float64
        [n, 10] record of the samples in ``self.last_flow_stats``.  ``flow_term_pair_target`` is this stage against a target field."""
        return self._flow_stage(pred, prev, True, flow, scale, reference_grad)

    def flow_term_pair_target(self, pred, prev, flow, target, scale=1.0, reference_grad=False):
        """``flow_term_pair`` against a target field (eigen_trainer_flow_term_target with a float reference), the stage a training call
        runs under a ``PredictionFlow`` and ``flow_target=``: target float64 [n, 2, H, W] as ``flow_term``'s; the value is the mean
        squared endpoint error of u against it.  (``flow_term_pair`` keeps its parameter list; ``flow_term`` takes `target` itself.)"""
        if target is None:
            raise ValueError("flow_term_pair_target needs a target field; flow_term_pair is the stage without one")
        return self._flow_stage(pred, prev, True, flow, scale, reference_grad, target=target)

    def flow_term_valid(self, pred, ref, flow, target, valid, scale=1.0, reference_grad=False):
        """``flow_term(target=)`` under validity planes (eigen_trainer_flow_term_valid): valid uint8 or bool [n, H, W], numpy or a device
        tensor; a pixel of sample b counts where the objective's shared mask counts it and valid[b] is not zero.  The value is the
        mean over the samples of each sample's mean squared endpoint error over its own counted pixels (0 for a sample that counts
        none); all-ones planes give the bytes of ``flow_term(target=)``.  ``check_flow_valid`` states the rules (ValueError)."""
        if target is None or valid is None:
            raise ValueError("flow_term_valid needs a target field and validity planes; flow_term is the stage without them")
        return self._flow_stage(pred, ref, False, flow, scale, reference_grad, target=target, valid=valid)

    def flow_term_pair_valid(self, pred, prev, flow, target, valid, scale=1.0, reference_grad=False):
        """``flow_term_pair_target`` under validity planes (eigen_trainer_flow_term_valid with a float reference), as ``flow_term_valid``."""
        if target is None or valid is None:
            raise ValueError("flow_term_pair_valid needs a target field and validity planes; flow_term_pair is the stage without them")
        return self._flow_stage(pred, prev, True, flow, scale, reference_grad, target=target, valid=valid)

    def _flow_stage(self, pred, ref, float_ref, flow, scale, reference_grad, stats=False, target=None, valid=None):
        """flow_term (float_ref False: a uint8 reference) and flow_term_pair (True: a float32 one): the upload, the checks, the buffers,
        the one call and the result tuple"""
        torch = self._torch
        if not isinstance(flow, FlowObjective):
            raise ValueError("flow must be a FlowObjective, got %r" % (flow,))
        if not np.isfinite(scale):
            raise ValueError("scale must be finite, got %r" % (scale,))
        if stats and flow.score is None:
            raise ValueError("stats goes with a FlowObjective that has a score")
        shp = (self.channels[0], self.h, self.w)
        dev = "cuda:%d" % self.device
        up = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt))).to(dev).contiguous()
        p, r = up(pred, np.float32), up(ref, np.float32 if float_ref else None)
        if p.dtype != torch.float32 or r.dtype != (torch.float32 if float_ref else torch.uint8) or p.dim() != 4 or tuple(p.shape[1:]) != shp or tuple(r.shape) != tuple(p.shape):
            raise ValueError(("pred and prev must be float32, both" if float_ref else "pred must be float32 and ref uint8, both") + " [n, %d, %d, %d]; got %s %s and %s %s"
                             % (shp + (p.dtype, tuple(p.shape), r.dtype, tuple(r.shape))))
        n, per = int(p.shape[0]), int(np.prod(shp))
        d_target, t_strides = self._target("flow", flow, target, (n, 2, self.h, self.w))
        d_valid, v_strides = self._valid("flow", flow, d_target, valid, (n, self.h, self.w))
        d_dir, d_mask = flow.on_device(torch, self.device, self.h, self.w)
        value = ctypes.c_double(0.0)
        u = torch.empty((n, 2, self.h, self.w), dtype=torch.float64, device=dev)
        seed = torch.empty((n,) + shp, dtype=torch.float32, device=dev)
        rg = torch.empty((n,) + shp, dtype=torch.float32, device=dev) if reference_grad else None
        cfg = flow.settings(stage_alone=True)
        self.last_flow_stats = None
        solve = flow.solve_on(self.w, self.h)       # the coarsest-level rule, before the call
        if d_target is not None:
            # eigen_trainer_flow_term_target: the iter entry's arguments (no score or members go with a target), the solve (NULL: the single
            # step), then the target
            # under validity planes eigen_trainer_flow_term_valid: the same arguments, then the planes and their stride
            entry, tail = (self.lib.eigen_trainer_flow_term_target, []) if d_valid is None else (self.lib.eigen_trainer_flow_term_valid, [_ptr(d_valid)] + v_strides)
            _check(entry(
                self._h, _ptr(p), ctypes.c_int64(per), None if float_ref else _ptr(r), _ptr(r) if float_ref else None, ctypes.c_int64(per), ctypes.c_int32(n),
                ctypes.byref(cfg), _ptr(d_mask), None, None, None, ctypes.c_double(float(scale)), ctypes.byref(value), None, _ptr(u), _ptr(seed), ctypes.c_int64(per),
                _ptr(rg), ctypes.c_int64(per if reference_grad else 0), None, None, ctypes.byref(solve) if solve is not None else None, _ptr(d_target), *t_strides, *tail))
            out = (value.value, u.cpu().numpy(), seed.cpu().numpy())
            return out + (rg.cpu().numpy(),) if reference_grad else out
        if solve is not None:
            # eigen_trainer_flow_term_iter: every mode through one entry, the solve behind the stream
            sc = flow.score.settings(self.h) if flow.score is not None else None
            by_circles = isinstance(flow.score, FlowScore)
            mem = flow.members_settings(n, self.h, self.w) if flow.score is not None else None
            rec = np.zeros((n, len(SCORE_STATS)), np.float64) if flow.score is not None else None
            ref_of = lambda x: None if x is None else ctypes.byref(x)
            _check(self.lib.eigen_trainer_flow_term_iter(
                self._h, _ptr(p), ctypes.c_int64(per), None if float_ref else _ptr(r), _ptr(r) if float_ref else None, ctypes.c_int64(per), ctypes.c_int32(n),
                ctypes.byref(cfg), _ptr(d_mask), ref_of(sc if by_circles else None), ref_of(None if by_circles else sc), ref_of(mem), ctypes.c_double(float(scale)),
                ctypes.byref(value), _ptr(rec), _ptr(u), _ptr(seed), ctypes.c_int64(per), _ptr(rg), ctypes.c_int64(per if reference_grad else 0), None, _ptr(d_dir),
                ctypes.byref(solve)))
            self.last_flow_stats = rec
            out = (value.value, u.cpu().numpy(), seed.cpu().numpy()) + ((rg.cpu().numpy(),) if reference_grad else ())
            return out + (rec,) if stats else out
        if flow.score is not None:
            sc = flow.score.settings(self.h)
            rec = np.zeros((n, len(SCORE_STATS)), np.float64)
            by_circles = isinstance(flow.score, FlowScore)
            mem = flow.members_settings(n, self.h, self.w)
            if mem is not None:
                entry, scores = self.lib.eigen_trainer_flow_term_members, [ctypes.byref(sc) if by_circles else None, None if by_circles else ctypes.byref(sc), ctypes.byref(mem)]
            else:
                entry, scores = self.lib.eigen_trainer_flow_term_score if by_circles else self.lib.eigen_trainer_flow_term_structure, [ctypes.byref(sc)]
            _check(entry(self._h, _ptr(p), ctypes.c_int64(per), None if float_ref else _ptr(r), _ptr(r) if float_ref else None,
                         ctypes.c_int64(per), ctypes.c_int32(n), ctypes.byref(cfg), _ptr(d_mask), *scores,
                         ctypes.c_double(float(scale)), ctypes.byref(value), _ptr(rec), _ptr(u), _ptr(seed), ctypes.c_int64(per),
                         _ptr(rg), ctypes.c_int64(per if reference_grad else 0), None))
            self.last_flow_stats = rec
            out = (value.value, u.cpu().numpy(), seed.cpu().numpy()) + ((rg.cpu().numpy(),) if reference_grad else ())
            return out + (rec,) if stats else out
        args = [self._h, _ptr(p), ctypes.c_int64(per), _ptr(r), ctypes.c_int64(per), ctypes.c_int32(n), ctypes.byref(cfg), _ptr(d_dir), _ptr(d_mask),
                ctypes.c_double(float(scale)), ctypes.byref(value), _ptr(u), _ptr(seed), ctypes.c_int64(per)]
        if float_ref:
            _check(self.lib.eigen_trainer_flow_term_pair(*args, _ptr(rg), ctypes.c_int64(per if reference_grad else 0), None))
        elif reference_grad:
            _check(self.lib.eigen_trainer_flow_term_ref(*args, _ptr(rg), ctypes.c_int64(per), None))
        else:
            _check(self.lib.eigen_trainer_flow_term(*args, None))
        out = (value.value, u.cpu().numpy(), seed.cpu().numpy())
        return out + (rg.cpu().numpy(),) if reference_grad else out

    def free_planes(self, n):
        """Debug (eigen_trainer_debug_free_planes): what the last stage under a ``FreeScore`` left of its pair pass, for the first n samples:
        {"theta", "L": float64 [n, H, W]; "rowS", "colS": int32 [n, H, W]; "member": bool [n, H, W]}."""
        shp = (int(n), self.h, self.w)
        out = {"theta": np.zeros(shp, np.float64), "L": np.zeros(shp, np.float64), "rowS": np.zeros(shp, np.int32), "colS": np.zeros(shp, np.int32),
               "member": np.zeros(shp, np.uint8)}
        _check(self.lib.eigen_trainer_debug_free_planes(self._h, ctypes.c_int32(int(n)), *[_ptr(out[k]) for k in ("theta", "L", "rowS", "colS", "member")], None))
        out["member"] = out["member"] != 0
        return out

    def debug_flow_iter(self, force=None):
        """Test hook (eigen_trainer_debug_flow_iter): force True / False sets whether a flow call without a real solve goes through the
        iterated stage and its backward too, on this handle.  -> the bytes of the iterated workspace the handle holds (0 before its first
        iterated call)."""
        n = ctypes.c_int64(0)
        _check(self.lib.eigen_trainer_debug_flow_iter(self._h, ctypes.c_int32(-1 if force is None else int(bool(force))), ctypes.byref(n)))
        return int(n.value)

    def evaluate(self, frames, reset=True, n_fed=None, requant=False, pred=False, layer_errors=False):
        """Forward only, no tape: the mean squared error of every step of frames uint8 [n, T, C, H, W], T of any length, as
        float64 [T - 1] (entry s: prediction s against frame s + 1).  Gradients and Adam state are untouched; the kept sequence
        state is shared with forward_backward (reset=False of either continues the last call of either).  pred=True also
        returns the float predictions [n, T, C, H, W]; layer_errors=True appends the float64 [T - 1, L] table of error-unit
        means, the one forward_backward returns."""
        d, n, T, n_fed, bstride = self._call_args(frames, n_fed)
        out = np.zeros(max(T - 1, 1), np.float64)
        table, d_pred = self._outputs(d, layer_errors, pred)
        _check(self.lib.eigen_trainer_evaluate_err(self._h, _ptr(d), bstride, ctypes.c_int32(n), ctypes.c_int32(T), ctypes.c_int32(n_fed),
                                                   ctypes.c_int32(int(bool(requant))), ctypes.c_int32(int(bool(reset))),
                                                   ctypes.c_void_p(out.ctypes.data), _ptr(table), _ptr(d_pred), None))
        res = (out[:T - 1],) + ((d_pred.cpu().numpy(),) if pred else ()) + ((table[:T - 1],) if layer_errors else ())
        return res[0] if len(res) == 1 else res

    def loss_and_grad(self, frames, reset=True):
        """(loss, {name: gradient}) of frames uint8 [n, T, C, H, W]; overwrites the gradients."""
        loss = self.forward_backward(frames, reset)
        return loss, self.grads()

    def grad_norms(self, stream=None):
        """The L2 norms of the current gradients, computed on the device in float64 (eigen_trainer_grad_norms): (global, {name: norm}).
        A norm that is not finite is returned as it is."""
        total, per = ctypes.c_double(0.0), np.zeros(len(self._names), np.float64)
        _check(self.lib.eigen_trainer_grad_norms(self._h, ctypes.byref(total), per.ctypes.data_as(_PD), ctypes.c_int32(len(self._names)), _stream_arg(stream)))
        return total.value, {n: float(v) for n, v in zip(self._names, per)}

    def accumulate(self, scale=1.0, stream=None):
        """Add scale times the current gradients to the accumulator, on the device: acc = acc + float32(scale) * g, each rounded once;
        the first addition after ``clear_accumulated`` (or ``set_weights``, or the trainer's start) starts from zero.  ValueError: a
        scale that is not finite."""
        scale = float(scale)
        if not np.isfinite(scale):
            raise ValueError("scale must be finite, got %r" % (scale,))
        _check(self.lib.eigen_trainer_accumulate(self._h, ctypes.c_int32(ACC_ADD), ctypes.c_double(scale), _stream_arg(stream)))

    def clear_accumulated(self, stream=None):
        """Empty the accumulator."""
        _check(self.lib.eigen_trainer_accumulate(self._h, ctypes.c_int32(ACC_CLEAR), ctypes.c_double(0.0), _stream_arg(stream)))

    def load_accumulated(self, stream=None):
        """Make the accumulated sum the current gradients (``grads()``, ``grad_norms()`` and ``adam()`` then see it); the accumulator keeps
        its contents.  EngineError -3: nothing was accumulated."""
        _check(self.lib.eigen_trainer_accumulate(self._h, ctypes.c_int32(ACC_LOAD), ctypes.c_double(0.0), _stream_arg(stream)))

    def adam(self, stream=None):
        """One Adam step on the current gradients.  Under neutral controls this is eigen_trainer_adam and ``last_update`` holds None
        thrice: nothing is read back.  Otherwise eigen_trainer_adam_ex clips, decays and, under skip_nonfinite, leaves out a step whose
        norm is not finite; ``last_update`` = {"norm": the global gradient norm, "rate": the factor the gradient was scaled by, "applied":
        1, or 0 for a step that was left out}.  Without skip_nonfinite a gradient that is not finite is applied."""
        clip, wd, skip = check_optim(self.clip_norm, self.weight_decay, self.skip_nonfinite)
        if optim_is_neutral(clip, wd, skip):
            _check(self.lib.eigen_trainer_adam(self._h, self.alpha, self.beta1, self.beta2, self.eps, _stream_arg(stream)))
            self.last_update = {"norm": None, "rate": None, "applied": None}
            return
        cfg = AdamSettings(self.alpha, self.beta1, self.beta2, self.eps, wd, 0.0 if clip is None else clip, int(skip), 0)
        rep = AdamReport()
        _check(self.lib.eigen_trainer_adam_ex(self._h, ctypes.byref(cfg), ctypes.byref(rep), _stream_arg(stream)))
        self.last_update = {"norm": rep.norm, "rate": rep.rate, "applied": int(rep.applied)}

    def step(self, frames, reset=True, n_fed=None, requant=False, step_weights=None, objective="mse", layer_weights=None, micro_batches=1, flow_target=None,
             frame_weight=None, flow_valid=None, flow=None):
        """Gradient and one Adam step; returns the loss before the step.  (`flow` stays the last argument, as in every call that takes
        one; it was the eighth positional one before `micro_batches` existed, and such a call still means it.)

        micro_batches = k > 1: the n sequences are cut into k equal chunks in order, each runs ``forward_backward`` with reset=True and is
        added to the accumulator with scale 1 / k, the sum becomes the gradient and ONE Adam step is taken.  Every objective is a mean
        over the samples, so in real arithmetic that is the full batch's gradient: a handle of batch n / k trains a logical batch of n.
        The loss returned is sum_j loss_j / k, formed in double in chunk order.  ``check_micro_batches`` states the rules (ValueError).
        flow_target, flow_valid: ``forward_backward``'s; with micro_batches = k they are sliced along n with the frames.  frame_weight:
        ``forward_backward``'s."""
        if isinstance(micro_batches, FlowObjective) and flow is None:
            micro_batches, flow = 1, micro_batches
        if isinstance(flow_target, FlowObjective) and flow is None:
            flow_target, flow = None, flow_target
        kw = dict(n_fed=n_fed, requant=requant, step_weights=step_weights, objective=objective, layer_weights=layer_weights, flow=flow)
        for key, v in (("flow_target", flow_target), ("frame_weight", frame_weight), ("flow_valid", flow_valid)):
            if v is not None:
                kw[key] = v
        if micro_batches == 1 and not isinstance(micro_batches, bool):     # the call as it always was: the accumulator is not touched
            loss = self.forward_backward(frames, reset, **kw)
            self.adam()
            return loss
        loss = self.accumulate_micro_batches(frames, micro_batches, reset=reset, **kw)
        self.load_accumulated()
        self.adam()
        return loss

    def accumulate_micro_batches(self, frames, micro_batches, reset=True, **kw):
        """The gradient half of ``step(micro_batches=k)``: empties the accumulator, runs the k chunks of `frames` and adds each with scale
        1 / k; -> sum_j loss_j / k.  ``load_accumulated()`` then makes the sum the gradient.  kw: ``forward_backward``'s n_fed, requant,
        step_weights, objective, layer_weights, flow, frame_weight, and flow_target and flow_valid (both sliced along n with the frames).
        Under validity planes every chunk's term is the mean over ITS samples of their own means, and the chunks are averaged."""
        kw = dict(kw)
        target, valid = kw.pop("flow_target", None), kw.pop("flow_valid", None)
        d = self._frames(frames)
        m = check_micro_batches(int(d.shape[0]), micro_batches, self.batch, reset, kw.get("flow"))
        k = int(micro_batches)
        self.clear_accumulated()
        total = 0.0
        for j in range(k):
            chunk = {} if target is None else {"flow_target": target[j * m:(j + 1) * m]}
            if valid is not None:
                chunk["flow_valid"] = valid[j * m:(j + 1) * m]
            total += float(self.forward_backward(d[j * m:(j + 1) * m], True, **kw, **chunk))
            self.accumulate(1.0 / k)
        return total / k

    # -- state in and out ------------------------------------------------------------------------------
    def state_dict(self):
        """Everything a continued run needs besides ``weights()``: {"adam_m", "adam_v": {name: float32 array}, "adam_t": int,
        "hyper": {alpha, beta1, beta2, eps}, "seq": None or {"h", "c", "P": [one float32 [n, C_l, H_l, W_l] per layer]}} and, when
        one of the optimiser controls is not neutral, "optim": {clip_norm, weight_decay, skip_nonfinite}."""
        m, v = self._empty(), self._empty()
        t, nb = ctypes.c_int32(0), ctypes.c_int32(0)
        _check(self.lib.eigen_trainer_get_state(self._h, self._table([m[n] for n in self._names]), self._table([v[n] for n in self._names]),
                                                ctypes.c_int32(len(self._names)), ctypes.byref(t), ctypes.byref(nb), None, ctypes.c_int32(0)))
        seq = None
        if nb.value > 0:
            shp = seq_state_shapes(self.channels, self.w, self.h, nb.value)
            seq = {k: [np.empty(s, np.float32) for s in shp] for k in SEQ_PARTS}
            flat = [seq[k][l] for l in range(len(shp)) for k in SEQ_PARTS]
            _check(self.lib.eigen_trainer_get_state(self._h, None, None, ctypes.c_int32(0), None, None, self._table(flat), ctypes.c_int32(len(flat))))
        out = {"adam_m": m, "adam_v": v, "adam_t": int(t.value), "hyper": {k: float(getattr(self, k)) for k in HYPER}, "seq": seq}
        optim = check_optim(self.clip_norm, self.weight_decay, self.skip_nonfinite)
        if not optim_is_neutral(*optim):    # "optim": the controls, present only when one is not neutral; the accumulator is no part of the state
            out["optim"] = dict(zip(OPTIM, optim))
        return out

    def load_state_dict(self, state):
        """Restore a ``state_dict()`` (after ``set_weights``, which clears all of it).  Shapes and dtypes are checked before
        anything reaches the device (ValueError); the hyper-parameters, when present, replace this trainer's, and so do the optimiser
        controls: a state without "optim" sets them neutral."""
        st = check_state(state, self.channels, self.w, self.h, self.batch)
        tm, tv = (self._table([st[key][n] for n in self._names]) for key in ("adam_m", "adam_v"))
        flat = [] if st["seq"] is None else [st["seq"][k][l] for l in range(len(self.channels)) for k in SEQ_PARTS]
        _check(self.lib.eigen_trainer_set_state(self._h, tm, tv, ctypes.c_int32(len(self._names)), ctypes.c_int32(st["adam_t"]),
                                                ctypes.c_int32(flat[0].shape[0] if flat else 0), self._table(flat) if flat else None, ctypes.c_int32(len(flat))))
        for k, v in st["hyper"].items():
            if k in HYPER:
                setattr(self, k, v)
        # the optimiser controls: the state's, and neutral where it carries none (a state of a neutral or an earlier trainer)
        self.clip_norm, self.weight_decay, self.skip_nonfinite = check_optim(**st.get("optim", {}))

    def save_checkpoint(self, path):
        """weights(), state_dict() and the hyper-parameters as one npz (``write_checkpoint``)."""
        write_checkpoint(path, self.weights(), self.state_dict())

    def load_checkpoint(self, path):
        """Continue the run ``save_checkpoint`` wrote: the following steps give the bits the saved trainer would have given."""
        wts, state = read_checkpoint(path, self.channels, self.w, self.h)
        if state["seq"] is not None and state["seq"]["h"][0].shape[0] > self.batch:
            raise ValueError("checkpoint keeps a sequence state of batch %d, this trainer holds %d" % (state["seq"]["h"][0].shape[0], self.batch))
        self.set_weights(wts)
        self.load_state_dict(state)

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


def flow_epe(trainer, pred, prev_or_ref, flow, target, valid=None):
    """The mean squared endpoint error of the flow `flow` solves from prev_or_ref to pred against `target`, on the device: the value of
    the stage alone under a target field (``PredNetTrainer.flow_term`` for a uint8 reference, ``flow_term_pair_target`` for a float32 one; float64
    target [n, 2, H, W]), the metric form of what ``forward_backward(flow_target=)`` trains on.  The mean runs over the samples and the
    pixels the objective's shared mask counts.  valid: None, or validity planes [n, H, W] (``flow_term_valid``): the mean over the
    samples of each sample's mean over its own counted pixels."""
    if target is None:
        raise ValueError("flow_epe needs a target field")
    by_float = str(getattr(prev_or_ref, "dtype", "")) in ("float32", "torch.float32")
    if valid is not None:
        return (trainer.flow_term_pair_valid if by_float else trainer.flow_term_valid)(pred, prev_or_ref, flow, target, valid)[0]
    if by_float:
        return trainer.flow_term_pair_target(pred, prev_or_ref, flow, target)[0]
    return trainer.flow_term(pred, prev_or_ref, flow, target=target)[0]


def _still_call(trainer, n_repeat, n_ext, iters, requant, objective, layer_weights, flow):
    """What refine_stills and refine_genomes share.  Checks the objective and the lengths at once; -> weigh(step_weights), which settles the
    step weights (``_still_weights``, checked then) and -> loss_of(img, frame_grads): the loss of the stills img uint8 [n, C, H, W] on the
    device, repeated n_repeat + n_ext times with the first n_repeat fed, and its frame gradient as a device tensor (None if not asked)."""
    T = int(n_repeat) + int(n_ext)
    _check_flow(objective, flow)
    if n_repeat < 1 or n_ext < 1 or iters < 0:
        raise ValueError("n_repeat >= 1, n_ext >= 1 and iters >= 0 required")
    if T > trainer.max_steps:
        raise ValueError("n_repeat + n_ext = %d frames exceed the trainer's max_steps %d" % (T, trainer.max_steps))

    def weigh(step_weights):
        step_weights = _still_weights(step_weights, n_repeat, n_ext, flow)

        def loss_of(img, frame_grads):
            n, per = int(img.shape[0]), int(np.prod(img.shape[1:]))
            d = img[:, None].expand(n, T, *img.shape[1:]).contiguous()
            value, _, _, d_grad = trainer._loss_grad(d, n, T, n_repeat, ctypes.c_int64(T * per), True, False, None, requant, step_weights, objective,
                                                     layer_weights, False, frame_grads, flow=flow)
            return value, d_grad
        return loss_of
    return weigh


def refine_stills(trainer, images, n_repeat=20, n_ext=2, iters=10, step=2.0, requant=True, objective="mse", layer_weights=None, step_weights=None,
                  mask=None, flow=None):
    """Gradient ascent on stills: raise how far PredNet's extended prediction leaves a still, the differentiable stand-in for the
    fitness (which scores the flow between the still and that prediction).  -> (uint8 [n, C, H, W] numpy, float64 [iters + 1]).

    images: uint8 [n, C, H, W] (numpy or a device tensor, n <= the trainer's batch); they are not modified.  Per iteration the
    frames are the image repeated T = n_repeat + n_ext times, the first n_repeat steps read it and the last n_ext are self-fed
    (requant: through the byte, as the fitness path feeds them), the targets are the still on every step, and the loss is
    `objective` under step_weights (None: 0 for the terms s < n_repeat - 1, 1 for the n_ext terms of the extension).  One call
    with reset=True gives the loss and its tied frame gradient; ``eigen_trainer_still_step`` then moves every free pixel by at
    most `step` bytes along the gradient, normalised by the image's largest |g| over the free pixels.  mask: [H, W], zero keeps
    a pixel as it is (None: every pixel is free).  Everything stays on the device between iterations.  objective "flow" with
    flow=FlowObjective(...) climbs the displacement between the still and the extended prediction itself, which is what the fitness
    scores; the FlowObjective's own mask selects the pixels that are counted, `mask` the pixels that move.  The still is also the
    reference frame of every flow term: with FlowObjective(reference="constant") the step follows the input path alone and ignores how the
    term moves with its reference, with reference="moving" it follows the whole gradient.

    Which fitness path the loss stands in for: a ``FlowObjective`` pairs the still with the extended predictions, the pairing of the
    single-image path (``get_vectors``, ``PAIR_SINGLE``).  flow=PredictionFlow(...) pairs consecutive predictions, as the population path
    does (``get_fitnesses_neat``, ``eval_images(pairing=PAIR_POPULATION)``): the default step_weights are then 0 for the terms s < n_repeat
    and 1 for the n_ext - 1 terms between extended predictions and their predecessors, at n_ext = 2 exactly the term "prediction after
    the last fed frame -> first extended prediction" that fitness scores; n_ext < 2 leaves no such term and is a ValueError.
    With requant=True the byte a self-fed step reads is a constant of the graph, so the gradient does not hold how that byte follows the
    prediction; under a PredictionFlow every weighted term passes through such a step, and at 160 x 120 that gradient was measured
    not to predict the change of the loss, while with requant=False it does ("The prediction pairing").
    The objective's solve is followed: with ``flow.solved(levels, iters)``, or ``DenseFitness.solve_objective()``, every term's field is
    the pyramidal, iterated solve's and the step follows the exact gradient through it ("The iterated solve's
    gradient"); ValueError before any call if the coarsest level of the trainer's image would be below 4 pixels.

    history[i] is the loss of the images as they entered iteration i, history[iters] that of the returned images.  The calls
    OVERWRITE the trainer's weight gradients and its kept sequence state."""
    weigh = _still_call(trainer, n_repeat, n_ext, iters, requant, objective, layer_weights, flow)
    if not (np.isfinite(step) and step > 0):
        raise ValueError("step must be finite and > 0, got %r" % (step,))
    loss_of = weigh(step_weights)
    torch = trainer._torch
    if isinstance(images, torch.Tensor):
        img = images.detach().to("cuda:%d" % trainer.device).clone()
    else:
        img = torch.from_numpy(np.ascontiguousarray(images)).cuda(trainer.device)
    if img.dtype != torch.uint8 or img.dim() != 4 or tuple(img.shape[1:]) != (trainer.channels[0], trainer.h, trainer.w):
        raise ValueError("images must be uint8 [n, %d, %d, %d], got %s %s" % (trainer.channels[0], trainer.h, trainer.w, img.dtype, tuple(img.shape)))
    img = img.contiguous()
    n, per = int(img.shape[0]), int(np.prod(img.shape[1:]))
    d_mask = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != (trainer.h, trainer.w):
            raise ValueError("mask must be [%d, %d], got %s" % (trainer.h, trainer.w, m.shape))
        d_mask = torch.from_numpy(m).cuda(trainer.device)

    history = np.zeros(iters + 1, np.float64)
    for i in range(iters):
        history[i], d_grad = loss_of(img, "tied")
        _check(trainer.lib.eigen_trainer_still_step(trainer._h, _ptr(img), _ptr(d_grad), ctypes.c_int64(per), _ptr(d_mask), ctypes.c_double(float(step)),
                                                    ctypes.c_int32(n), None))
    history[iters], _ = loss_of(img, None)
    return img.cpu().numpy(), history


def _still_weights(step_weights, n_repeat, n_ext, flow):
    """the step weights of refine_stills / refine_genomes: as given, else the extension's terms under the pairing of `flow`.  Under a
    PredictionFlow the first of them, P0_{n_repeat - 1} -> P0_{n_repeat}, is term n_repeat; n_ext < 2 has none (ValueError)."""
    by_pred = flow is not None and flow.pairing == "prediction"
    if by_pred and n_ext < 2:
        raise ValueError("a PredictionFlow needs n_ext >= 2: its first term between two predictions of the extension is term n_repeat, got n_ext = %d" % n_ext)
    if step_weights is not None:
        return step_weights
    return [0.0] * n_repeat + [1.0] * (n_ext - 1) if by_pred else [0.0] * (n_repeat - 1) + [1.0] * n_ext


PARAM_KINDS = ("weight", "bias", "response")


def _genome_bounds(config, bounds):
    """{kind: (lo, hi)} of refine_genomes: `bounds` as given, else the <kind>_min_value / <kind>_max_value the genome config carries; a
    kind without both is not clipped."""
    if bounds is not None:
        out = {}
        for k, v in dict(bounds).items():
            if k not in PARAM_KINDS or len(v) != 2 or not float(v[0]) <= float(v[1]):
                raise ValueError("bounds must map %s to (lo, hi) with lo <= hi, got %r: %r" % (", ".join(PARAM_KINDS), k, v))
            out[k] = (float(v[0]), float(v[1]))
        return out
    gc = getattr(config, "genome_config", None)
    out = {}
    for k in PARAM_KINDS:
        lo, hi = getattr(gc, k + "_min_value", None), getattr(gc, k + "_max_value", None)
        if lo is not None and hi is not None:
            out[k] = (float(lo), float(hi))
    return out


def genome_update(genome, gmap, g_bias, g_resp, g_w, lr, params=PARAM_KINDS, bounds=None):
    """One normalised ascent step of refine_genomes on ONE genome, in place, in float64.  gmap: ``genome.flatten_genome_map`` of it;
    g_bias, g_resp, g_w: the gradients of its flat parameters.  The trainable parameters are those of the selected kinds whose map
    entry is a gene (not None); m = max |g| over them; m zero or not finite leaves the genome as it is, otherwise every one moves
    by lr * g / m and is then clipped to bounds[kind] where that is given.  Returns whether the genome moved."""
    todo = []   # (gene, attribute, kind, gradient)
    if "bias" in params or "response" in params:
        for n, key in enumerate(gmap["node_key"]):
            if key is None:
                continue
            if "bias" in params:
                todo.append((genome.nodes[key], "bias", "bias", float(g_bias[n])))
            if "response" in params:
                todo.append((genome.nodes[key], "response", "response", float(g_resp[n])))
    if "weight" in params:
        for k, key in enumerate(gmap["edge_key"]):
            if key is not None:
                todo.append((genome.connections[key], "weight", "weight", float(g_w[k])))
    if not todo:
        return False
    m = float(np.max(np.abs(np.asarray([t[3] for t in todo], np.float64))))
    if not (np.isfinite(m) and m > 0):
        return False
    bounds = bounds or {}
    for gene, attr, kind, g in todo:
        v = float(getattr(gene, attr)) + float(lr) * (g / m)
        if kind in bounds:
            v = min(max(v, bounds[kind][0]), bounds[kind][1])
        setattr(gene, attr, v)
    return True


def refine_genomes(trainer, genomes, config, structure, n_repeat=20, n_ext=2, iters=10, lr=0.02, requant=True, objective="mse", layer_weights=None,
                   step_weights=None, bg=1, params=PARAM_KINDS, bounds=None, flow=None):
    """Gradient ascent on the genomes' own parameters: ``refine_stills``' loss (how far PredNet's extended prediction leaves the still),
    climbed through the CPPN render instead of in pixel space, so that what comes back can be mutated, crossed and rendered at any
    size.  -> (genomes', float64 [iters + 1] history, uint8 [n, C, H, W] images).

    genomes: a list of n <= the trainer's batch NEAT genomes of `config`; they are never modified: genomes' are deep copies that
    keep keys, structure, `enabled` flags and `fitness`.  structure: the grid (``fitness.leaf_planes``) at the trainer's w, h.
    Per iteration the copies are rendered on the device (gradient = 1 render, background `bg`), one trainer call exactly as
    ``refine_stills`` makes it gives the loss and its tied frame gradient, ``Engine.cppn_param_grads`` turns that into the gradient by
    every flat parameter (straight through the uint8 quantisation; DESIGN.md section 13, "CPPN parameter gradients"), and the host
    updates every genome in float64 (``genome_update``): theta += lr * g / max |g| over its trainable parameters of the kinds in
    `params`, then clipped to `bounds` ({kind: (lo, hi)}; None: the <kind>_min_value / _max_value of the genome config, where it has
    them).  FROZEN, i.e. never updated: folded float32 constants (``genome.flatten_genome_map``'s None entries and everything inside a
    folded sub-graph), disabled connections and whatever the outputs do not depend on.

    objective "flow" takes flow=FlowObjective(...) as ``refine_stills`` does, its `reference` setting included: that loss pairs the
    still with the extended predictions and stands in for the single-image fitness path (``get_vectors``, ``PAIR_SINGLE``).
    flow=PredictionFlow(...) pairs consecutive predictions and stands in for the population path (``get_fitnesses_neat``,
    ``eval_images(pairing=PAIR_POPULATION)``); the default step_weights and the n_ext >= 2 rule are ``refine_stills``'.

    history[i] is the loss of the images as they entered iteration i, history[iters] that of the returned images, which are the
    render of genomes'.  The objective's solve is followed as ``refine_stills`` follows it: ``DenseFitness.solve_objective()`` climbs the
    score of the field the dense fitness itself scores.  The calls OVERWRITE the trainer's weight gradients and its kept sequence state."""
    import copy
    from . import fitness
    from .genome import GenomeBatch, flatten_genome_map
    weigh = _still_call(trainer, n_repeat, n_ext, iters, requant, objective, layer_weights, flow)
    genomes = list(genomes)
    n = len(genomes)
    if not 1 <= n <= trainer.batch:
        raise ValueError("%d genomes: 1 .. the trainer's batch %d required" % (n, trainer.batch))
    if not (np.isfinite(lr) and lr > 0):
        raise ValueError("lr must be finite and > 0, got %r" % (lr,))
    params = (params,) if isinstance(params, str) else tuple(params)
    if not params or any(k not in PARAM_KINDS for k in params):
        raise ValueError("params must be a non-empty selection of %s, got %r" % (", ".join(PARAM_KINDS), params))
    limits = _genome_bounds(config, bounds)
    loss_of = weigh(step_weights)
    torch = trainer._torch
    C0, h, w = trainer.channels[0], trainer.h, trainer.w
    n_in = len(config.genome_config.input_keys)
    out = [copy.deepcopy(g) for g in genomes]
    maps = [flatten_genome_map(g, config, n_in) for g in out]   # values change below, the structure (and so the map) does not
    with torch.cuda.device(trainer.device):
        eng = engine.Engine(w, h, [C0], n, device=trainer.device)   # weight-free: it renders and differentiates the render
        try:
            eng.set_grid(fitness.leaf_planes(structure, w, h, n_in))
            img = torch.empty((n, C0, h, w), dtype=torch.uint8, device="cuda:%d" % trainer.device)

            def render():
                gb = GenomeBatch(out, config, C0, n_leaves=n_in)
                eng.render_cppn(gb, img, bg=bg, gradient=1)
                return gb

            history = np.zeros(iters + 1, np.float64)
            for i in range(iters):
                gb = render()
                history[i], d_grad = loss_of(img, "tied")
                g_bias, g_resp, g_w = eng.cppn_param_grads(gb, d_grad, bg=bg, gradient=1)
                for j, (g, m) in enumerate(zip(out, maps)):
                    n0, n1 = int(gb.node_off[j]), int(gb.node_off[j + 1])
                    e0, e1 = int(gb.edge_off[n0]), int(gb.edge_off[n1])
                    if n1 - n0 != len(m["node_key"]) or e1 - e0 != len(m["edge_key"]):
                        raise RuntimeError("genome %r: the batch holds %d nodes / %d edges, its map %d / %d" % (getattr(g, "key", None), n1 - n0, e1 - e0,
                                                                                                              len(m["node_key"]), len(m["edge_key"])))
                    genome_update(g, m, g_bias[n0:n1], g_resp[n0:n1], g_w[e0:e1], lr, params, limits)
            render()
            history[iters], _ = loss_of(img, None)
            torch.cuda.synchronize(trainer.device)
            images = img.cpu().numpy()
        finally:
            eng.close()
    return out, history, images


# ---- moving CPPN textures: a seeded, device-resident frame source with its exact flow ("Moving textures")
def similarity_affines(c, o, m, d, n_frames):
    """One layer's affines of a constant similarity per frame, in closed form.  Pixels and texture points are complex numbers
    (z = px + i py about the image centre, w = u + i v): the texture sits at w = c z + o in frame 0 and every frame moves the surface
    by g(z) = m z + d (m = zoom * exp(i turn), d the shift).  g^t(z) = m^t z + D_t with D_t = d (1 + m + ... + m^(t - 1)), so
      A_t  = A_0 o g^-t :  w = (c / m^t) z + (o - (c / m^t) D_t)
      A_t^-1            :  z = (m^t / c) w + (D_t - (m^t / c) o)
    with m^t = zoom^t exp(i t turn) from pow, cos and sin, never from a product of t factors or a numerical inverse.
    -> (affine, affine_inv), float64 [n_frames, 6]: rows (a0 .. a5) of u = a0 px + a1 py + a2, v = a3 px + a4 py + a5."""
    c, o, m, d = complex(c), complex(o), complex(m), complex(d)
    zoom, turn = abs(m), np.arctan2(m.imag, m.real)
    A, Ainv = np.zeros((n_frames, 6), np.float64), np.zeros((n_frames, 6), np.float64)
    geo = 0j   # 1 + m + ... + m^(t - 1)
    for t in range(n_frames):
        mt = (zoom ** t) * complex(np.cos(t * turn), np.sin(t * turn))
        ct, it = c / mt, mt / c
        ot, pt = o - ct * (d * geo), d * geo - it * o
        A[t] = (ct.real, -ct.imag, ot.real, ct.imag, ct.real, ot.imag)
        Ainv[t] = (it.real, -it.imag, pt.real, it.imag, it.real, pt.imag)
        geo += mt
    return A, Ainv


def flat_genome_batch(flats, c_out):
    """The ``GenomeBatch`` of a list of ``genome.flatten_genome`` dicts, c_out outputs of each."""
    from .genome import GenomeBatch
    e0 = np.cumsum([0] + [len(f["edge_w"]) for f in flats])
    arrays = (np.cumsum([0] + [len(f["act"]) for f in flats]), np.concatenate([[0]] + [f["edge_off"][1:] + e for f, e in zip(flats, e0)]),
              np.concatenate([f["act"] for f in flats]), np.concatenate([f["bias"] for f in flats]), np.concatenate([f["resp"] for f in flats]),
              np.concatenate([f["edge_src"] for f in flats]), np.concatenate([f["edge_w"] for f in flats]),
              np.concatenate([f["out_node"][:c_out] for f in flats]))
    return GenomeBatch._from_arrays(len(flats), c_out, arrays)


def check_moving_textures(w, h, c_dim, seq, seed=0, layers=1, max_shift=1.5, max_turn=0.02, max_zoom=0.01, texture_scale=None, num_hidden=20):
    """The arguments of ``MovingTextures`` as (w, h, c_dim, seq, seed, layers, max_shift, max_turn, max_zoom, texture_scale,
    num_hidden), texture_scale filled in (3 / max(w, h): the longer side spans three texture units).  ValueError: w, h, seq or
    num_hidden not an integer >= 1, c_dim not 1 or 3, layers not 1 or 2, a seed that is not an integer >= 0, max_shift or max_turn
    negative or not finite, max_zoom outside [0, 1), a texture_scale that is not finite and > 0, a bool or a non-number where a
    number goes."""
    def integer(name, v, lo):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, v))
        return int(v)

    def number(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
        return float(v)
    w, h, seq, num_hidden = integer("w", w, 1), integer("h", h, 1), integer("seq", seq, 1), integer("num_hidden", num_hidden, 1)
    seed = integer("seed", seed, 0)
    if isinstance(c_dim, (bool, np.bool_)) or c_dim not in (1, 3):
        raise ValueError("c_dim must be 1 or 3, got %r" % (c_dim,))
    if isinstance(layers, (bool, np.bool_)) or layers not in (1, 2):
        raise ValueError("layers must be 1 or 2, got %r" % (layers,))
    max_shift, max_turn, max_zoom = number("max_shift", max_shift), number("max_turn", max_turn), number("max_zoom", max_zoom)
    if max_shift < 0 or max_turn < 0:
        raise ValueError("max_shift and max_turn must be >= 0, got %r and %r" % (max_shift, max_turn))
    if not 0 <= max_zoom < 1:
        raise ValueError("max_zoom must be in [0, 1), got %r" % (max_zoom,))
    texture_scale = 3.0 / max(w, h) if texture_scale is None else number("texture_scale", texture_scale)
    if not texture_scale > 0:
        raise ValueError("texture_scale must be > 0, got %r" % (texture_scale,))
    return w, h, int(c_dim), seq, seed, int(layers), max_shift, max_turn, max_zoom, texture_scale, num_hidden


class MovingTextures:
    """An unlimited, seeded stream of uint8 [n, seq, C, H, W] sequences of moving CPPN textures, rendered on the device with the
    exact flow of every pixel (``Engine.render_moving_cppn``; DESIGN.md section 13, "Moving textures").

    Batch index k holds the samples drawn from ``numpy.random.default_rng((seed, k))``: per sample and layer a ``synth.make_genome``
    texture with num_hidden hidden nodes and a constant similarity per frame about the image centre (a shift of at most max_shift
    pixels, a turn of at most max_turn radians, a zoom factor within 1 +- max_zoom), composed in closed form
    (``similarity_affines``).  Layer 0 fills the image, texture_scale texture units per pixel; with layers=2 layer 1 is a disc (an
    ellipse once it zooms) with a texture and a motion of its own in front of it: an occlusion boundary with two motions.
    ``check_moving_textures`` states the argument rules (ValueError).  engine: an ``Engine`` of this size and c_dim to render
    with; without one the object creates a one-layer engine of max_batch 1 (the entry does not depend on it) and closes it with
    itself."""

    def __init__(self, w, h, c_dim, seq, seed=0, layers=1, max_shift=1.5, max_turn=0.02, max_zoom=0.01, texture_scale=None, num_hidden=20, engine=None,
                 device=None):
        (self.w, self.h, self.c_dim, self.seq, self.seed, self.layers, self.max_shift, self.max_turn, self.max_zoom, self.texture_scale,
         self.num_hidden) = check_moving_textures(w, h, c_dim, seq, seed, layers, max_shift, max_turn, max_zoom, texture_scale, num_hidden)
        if engine is not None and (engine.width, engine.height, engine.c_dim) != (self.w, self.h, self.c_dim):
            raise ValueError("the engine renders (%d, %d, %d), the textures are (%d, %d, %d) (w, h, c_dim)"
                             % (engine.width, engine.height, engine.c_dim, self.w, self.h, self.c_dim))
        self.engine, self._own, self.device = engine, False, device
        from . import synth
        self.config = synth.make_config(2, self.c_dim)

    def describe(self, k, n):
        """Host only: the n samples of batch index k as a dict -- w, h, c_dim, n, T, L; genomes (n * L ``synth`` genomes, sample-major)
        and config; gb, their ``GenomeBatch`` (``genome.flatten_genome`` of each); affine and affine_inv, float64 [n, T, L, 6];
        motion, float64 [n, L, 4]: the drawn (shift x, shift y, turn, zoom) of every layer."""
        from . import synth
        from .genome import flatten_genome
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError("the batch index must be an integer >= 0, got %r" % (k,))
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("n must be an integer >= 1, got %r" % (n,))
        rng = np.random.default_rng((self.seed, int(k)))
        T, L = self.seq, self.layers
        genomes, flats = [], []
        affine, affine_inv, motion = np.zeros((n, T, L, 6)), np.zeros((n, T, L, 6)), np.zeros((n, L, 4))
        for b in range(n):
            for l in range(L):
                g = synth.make_genome(b * L + l + 1, self.config, int(rng.integers(1 << 31)), num_hidden=self.num_hidden)
                genomes.append(g)
                flats.append(flatten_genome(g, self.config))
                r, ang = rng.uniform(0.0, self.max_shift), rng.uniform(0.0, 2 * np.pi)
                turn, zoom = rng.uniform(-self.max_turn, self.max_turn), rng.uniform(1 - self.max_zoom, 1 + self.max_zoom)
                d, m = r * complex(np.cos(ang), np.sin(ang)), zoom * complex(np.cos(turn), np.sin(turn))
                phi = rng.uniform(0.0, 2 * np.pi)
                rot = complex(np.cos(phi), np.sin(phi))
                if l == 0:   # the texture under the whole image, at a seeded offset
                    c, o = self.texture_scale * rot, complex(rng.uniform(-1, 1), rng.uniform(-1, 1))
                else:        # a disc of 0.2 .. 0.35 of the shorter side, its centre in the middle half of the image
                    radius = rng.uniform(0.2, 0.35) * min(self.w, self.h)
                    zc = complex(rng.uniform(-0.25, 0.25) * self.w, rng.uniform(-0.25, 0.25) * self.h)
                    c = rot / radius
                    o = -c * zc
                affine[b, :, l], affine_inv[b, :, l] = similarity_affines(c, o, m, d, T)
                motion[b, l] = (d.real, d.imag, turn, zoom)
        gb = flat_genome_batch(flats, self.c_dim)
        return dict(w=self.w, h=self.h, c_dim=self.c_dim, n=int(n), T=T, L=L, genomes=genomes, config=self.config, gb=gb, affine=affine,
                    affine_inv=affine_inv, motion=motion)

    def _engine(self):
        if self.engine is None:
            from .fitness import _local_device
            self.engine = engine.Engine(self.w, self.h, [self.c_dim], 1, device=_local_device() if self.device is None else int(self.device))
            self._own = True
        return self.engine

    def batch(self, k, n, flow=False, stream=None, valid=False):
        """The device uint8 [n, seq, C, H, W] tensor of batch index k; flow=True: (frames, flow float64 [n, seq - 1, 2, H, W], layer
        uint8 [n, seq, H, W]).  The same (seed, k, n) always gives the same bytes.  valid=True (with flow=True; ValueError without)
        appends the validity planes, uint8 [n, seq - 1, H, W] (``Engine.moving_cppn_valid``): 1 where the surface a pixel of frame t
        shows is inside the image and uncovered in frame t + 1, so that its flow can be recovered from the two frames at all."""
        if valid and not flow:
            raise ValueError("valid=True states the validity of the flow: it needs flow=True")
        d = self.describe(k, n)
        frames, fl, layer = self._engine().render_moving_cppn(d["gb"], d["affine"], d["affine_inv"] if flow else None, flow=flow, layer=flow, stream=stream)
        if valid:
            return frames, fl, layer, self._engine().moving_cppn_valid(d["affine"], d["affine_inv"], stream=stream)
        return (frames, fl, layer) if flow else frames

    def close(self):
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine, self._own = None, False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


__all__ = ["PredNetTrainer", "EngineError", "check_state", "write_checkpoint", "read_checkpoint", "combine_terms", "refine_stills", "refine_genomes", "genome_update", "FlowObjective",
           "check_flow_valid", "check_frame_weight", "PredictionFlow", "make_flow", "flow_direction", "FlowScore", "BandsScore", "FreeScore", "structure_score", "CornerMembers", "check_optim",
           "check_micro_batches", "MovingTextures", "check_moving_textures", "similarity_affines", "flat_genome_batch"]
