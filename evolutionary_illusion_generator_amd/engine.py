"""ctypes binding of the C-ABI engine library (include/eigen_engine.h -> libeigen_hip.so).

The library is the ONLY compute path of this package: if it is missing or cannot be loaded the import of
:class:`Engine` users fails loudly -- there is no PyTorch/CPU fallback.  torch is used by callers for device
memory and streams only; this module passes raw pointers.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EIGEN_HIP_LIB") or os.path.join(_HERE, "libeigen_hip.so")  # EIGEN_HIP_LIB: A/B builds (scripts/)
ABI_VERSION = 4  # include/eigen_engine.h: EIGEN_ABI_VERSION
MAX_LAYERS = 8

PAIR_POPULATION, PAIR_SINGLE = 0, 1

EXPORTS = ["eigen_abi_version", "eigen_gate_order", "eigen_winograd_mask", "eigen_last_error", "eigen_config_defaults", "eigen_create", "eigen_destroy",
           "eigen_set_prednet_weights", "eigen_set_grid", "eigen_render_cppn", "eigen_eval_cppn_nodes", "eigen_prednet_rollout", "eigen_prednet_sequence", "eigen_flow",
           "eigen_score", "eigen_eval_population", "eigen_eval_images", "eigen_test_conv", "eigen_time_conv", "eigen_test_det_math",
           "eigen_get_timings", "eigen_conv_profile", "eigen_debug_corners", "eigen_debug_dense_flow", "eigen_debug_state", "eigen_prednet_flops_per_step", "eigen_flatten_genomes", "eigen_plan_text", "eigen_plan_text_sw",
           "eigen_trainer_create", "eigen_trainer_destroy", "eigen_trainer_set_weights", "eigen_trainer_get_weights", "eigen_trainer_loss_grad",
           "eigen_trainer_get_grads", "eigen_trainer_adam", "eigen_trainer_tape_bytes", "eigen_trainer_loss_grad_ext", "eigen_trainer_evaluate",
           "eigen_trainer_get_state", "eigen_trainer_set_state", "eigen_trainer_loss_grad_obj", "eigen_trainer_evaluate_err",
           "eigen_trainer_loss_grad_frames", "eigen_trainer_still_step", "eigen_cppn_param_grads", "eigen_trainer_flow_term",
           "eigen_trainer_loss_grad_flow", "eigen_trainer_flow_term_ref", "eigen_trainer_loss_grad_flow_pair", "eigen_trainer_flow_term_pair",
           "eigen_trainer_flow_term_score", "eigen_trainer_loss_grad_flow_score", "eigen_trainer_flow_term_structure",
           "eigen_trainer_loss_grad_flow_structure", "eigen_trainer_debug_free_planes", "eigen_trainer_flow_members",
           "eigen_trainer_flow_term_members", "eigen_trainer_loss_grad_flow_members", "eigen_trainer_grad_norms", "eigen_trainer_adam_ex",
           "eigen_trainer_accumulate", "eigen_dense_score", "eigen_eval_population_dense", "eigen_eval_images_dense",
           "eigen_render_moving_cppn", "eigen_dense_score_iter", "eigen_eval_population_dense_iter", "eigen_eval_images_dense_iter",
           "eigen_debug_dense_solve", "eigen_trainer_flow_term_iter", "eigen_trainer_loss_grad_flow_iter", "eigen_trainer_debug_flow_iter",
           "eigen_trainer_flow_term_target", "eigen_trainer_loss_grad_flow_target", "eigen_moving_cppn_valid", "eigen_trainer_flow_term_valid",
           "eigen_trainer_loss_grad_flow_joint", "eigen_dense_score_members", "eigen_eval_population_dense_members", "eigen_eval_images_dense_members",
           "eigen_dense_score_float", "eigen_debug_dense_gray"]


class EigenConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("n_layers", ctypes.c_int32), ("channels", ctypes.c_int32 * MAX_LAYERS), ("max_batch", ctypes.c_int32),
                ("n_repeat", ctypes.c_int32), ("n_ext", ctypes.c_int32), ("requant_feedback", ctypes.c_int32),
                ("lk_max_corners", ctypes.c_int32), ("lk_block_size", ctypes.c_int32), ("lk_win", ctypes.c_int32),
                ("lk_max_level", ctypes.c_int32), ("lk_max_iter", ctypes.c_int32), ("flow_method", ctypes.c_int32),
                ("lk_quality_level", ctypes.c_double), ("lk_min_distance", ctypes.c_double),
                ("lk_epsilon", ctypes.c_double), ("lk_min_eig_thr", ctypes.c_double),
                ("fb_levels", ctypes.c_int32), ("fb_winsize", ctypes.c_int32), ("fb_iterations", ctypes.c_int32),
                ("fb_poly_n", ctypes.c_int32), ("fb_step", ctypes.c_int32), ("reserved1", ctypes.c_int32),
                ("fb_poly_sigma", ctypes.c_double)]


class GenomeBatchC(ctypes.Structure):
    _fields_ = [("n_genomes", ctypes.c_int32), ("c_out", ctypes.c_int32),
                ("node_off", ctypes.c_void_p), ("edge_off", ctypes.c_void_p), ("node_act", ctypes.c_void_p),
                ("node_bias", ctypes.c_void_p), ("node_resp", ctypes.c_void_p), ("edge_src", ctypes.c_void_p),
                ("edge_w", ctypes.c_void_p), ("out_node", ctypes.c_void_p)]


class FlowSettingsC(ctypes.Structure):
    """eigen_flow_settings (train.FlowSettings is the same layout)"""
    _fields_ = [("radius", ctypes.c_int32), ("flags", ctypes.c_int32), ("eps", ctypes.c_double)]


class DenseSettingsC(ctypes.Structure):
    """eigen_dense_settings: the window and exactly one of the two scores"""
    _fields_ = [("flow", FlowSettingsC), ("score", ctypes.c_void_p), ("sscore", ctypes.c_void_p)]


class DenseSolveC(ctypes.Structure):
    """eigen_dense_solve: the pyramid levels and the iterations per level of the dense stage's solve"""
    _fields_ = [("levels", ctypes.c_int32), ("iters", ctypes.c_int32)]


FLOW_METHODS = {"lk": 0, "farneback": 1}  # eigen_flow_method
DENSE_FLOAT_FRAMES = 2  # EIGEN_DENSE_FLOAT_FRAMES: bit 1 of eigen_dense_settings.flow.flags
DENSE_REC = 10  # doubles of one sample's record (train.SCORE_STATS / BANDS_STATS / FREE_STATS)


class EngineError(RuntimeError):
    pass


_lib = None


def load_library(path=None):
    """dlopen libeigen_hip.so (built by ``__graft_entry__.build()``); raises if it is absent."""
    global _lib
    if _lib is None or path is not None:
        p = path or LIB_PATH
        # PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime of the process (device tensors and
        # streams come from torch), so make sure it is loaded before this library's dependency is resolved.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(p):
            raise EngineError("HIP engine library %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % p)
        lib = ctypes.CDLL(p)
        lib.eigen_last_error.restype = ctypes.c_char_p
        lib.eigen_prednet_flops_per_step.restype = ctypes.c_double
        lib.eigen_prednet_flops_per_step.argtypes = [ctypes.c_void_p]
        for name in EXPORTS:
            getattr(lib, name)  # AttributeError if the ABI drifted
        if lib.eigen_abi_version() != ABI_VERSION:  # EigenConfig below mirrors eigen_config of exactly this version
            raise EngineError("%s has ABI version %d, this package binds version %d: rebuild it" % (p, lib.eigen_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def _check(rc):
    if rc != 0:
        raise EngineError("eigen engine error %d: %s" % (rc, load_library().eigen_last_error().decode()))


def _ptr(x):
    """Raw address of a numpy array / torch tensor / int."""
    if x is None:
        return None
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    return ctypes.c_void_p(x.data_ptr())  # torch tensor


def _stream_arg(stream):
    if stream is None:
        return None
    return ctypes.c_void_p(int(getattr(stream, "cuda_stream", stream)))


W4_SWITCHES = ("w4_tall", "w4_half", "w4_pack", "w4_parts")   # csrc/conv_plan.h: Switches (EIGEN_W4_TALL / _HALF / _PACK / _PARTS)
W4_DEFAULTS = {"w4_tall": -1, "w4_half": -1, "w4_pack": -1, "w4_parts": 0}


def plan_text(channels, width, height, batch, n_cu=256, wino_mask=-1, step0=False, switches=W4_DEFAULTS):
    """The launches of one PredNet step as the library plans them (host-only): one dict per launch, in launch order -- op, kernel, shape as strings, every
    other field an int.  switches: the Winograd shape switches, a dict over W4_DEFAULTS (the default: eigen_plan_text, the environment is not read; wino_mask < 0:
    the built-in default), or None: what THIS process launches -- its EIGEN_* environment, and wino_mask < 0 its effective mask (eigen_plan_text_sw)."""
    lib = load_library()
    ch = (ctypes.c_int32 * len(channels))(*channels)
    buf = ctypes.create_string_buffer(1 << 16)
    head = (ctypes.c_int32(len(channels)), ch, ctypes.c_int32(width), ctypes.c_int32(height), ctypes.c_int32(batch), ctypes.c_int32(n_cu),
            ctypes.c_int32(wino_mask), ctypes.c_int32(int(step0)))
    if switches is W4_DEFAULTS:
        n = lib.eigen_plan_text(*head, buf, ctypes.c_int32(len(buf)))
    else:
        if switches is not None and set(switches) - set(W4_SWITCHES):
            raise ValueError("plan_text: unknown switches %s" % sorted(set(switches) - set(W4_SWITCHES)))
        w4 = None if switches is None else (ctypes.c_int32 * 4)(*[int(switches.get(k, W4_DEFAULTS[k])) for k in W4_SWITCHES])
        n = lib.eigen_plan_text_sw(*head, w4, buf, ctypes.c_int32(len(buf)))
    _check(min(n, 0))
    if n >= len(buf):
        raise EngineError("eigen_plan_text: the plan has %d characters, the buffer %d" % (n, len(buf)))
    rows = []
    for ln in buf.value.decode().splitlines():
        op, *fields = ln.split()
        row = {"op": op}
        for f in fields:
            k, v = f.split("=")
            row[k] = v if k in ("kernel", "shape") else int(v)
        rows.append(row)
    return rows


def check_moving_affines(affine, affine_inv, n_genomes, flow):
    """The affines of ``Engine.render_moving_cppn`` as contiguous float64 arrays (affine, affine_inv or None).  ValueError: an affine
    that is not [n >= 1, T >= 1, L in (1, 2), 6], n * L not the batch's genome count, flow without an inverse or with fewer than two
    frames, an inverse of another shape."""
    a = np.ascontiguousarray(affine, dtype=np.float64)
    if a.ndim != 4 or a.shape[0] < 1 or a.shape[1] < 1 or a.shape[2] not in (1, 2) or a.shape[3] != 6:
        raise ValueError("affine must be float64 [n, T, L in (1, 2), 6], got shape %s" % (a.shape,))
    if a.shape[0] * a.shape[2] != n_genomes:
        raise ValueError("%d samples of %d layers need %d genomes, the batch has %d" % (a.shape[0], a.shape[2], a.shape[0] * a.shape[2], n_genomes))
    if not flow:
        return a, None
    if affine_inv is None:
        raise ValueError("flow=True needs affine_inv")
    if a.shape[1] < 2:
        raise ValueError("flow=True needs at least two frames, affine has %d" % a.shape[1])
    i = np.ascontiguousarray(affine_inv, dtype=np.float64)
    if i.shape != a.shape:
        raise ValueError("affine_inv has shape %s, affine %s" % (i.shape, a.shape))
    return a, i


class Engine:
    """One engine handle = one GPU rank.  Sizes are fixed at creation (workspaces live in HBM)."""

    def __init__(self, width, height, channels, max_batch, device=0, n_repeat=20, n_ext=2, requant_feedback=False, flow="lk", **lk):
        self.lib = load_library()
        cfg = EigenConfig()
        self.lib.eigen_config_defaults(ctypes.byref(cfg))
        cfg.device, cfg.width, cfg.height, cfg.n_layers, cfg.max_batch = device, width, height, len(channels), max_batch
        for i, c in enumerate(channels):
            cfg.channels[i] = c
        cfg.n_repeat, cfg.n_ext, cfg.requant_feedback = n_repeat, n_ext, int(requant_feedback)
        if flow not in FLOW_METHODS:
            raise ValueError("flow must be one of %s" % sorted(FLOW_METHODS))
        cfg.flow_method = FLOW_METHODS[flow]
        for k, v in lk.items():  # lk_* (Lucas-Kanade) or fb_* (Farneback) parameters, prefix optional for lk
            name = k if k.startswith("fb_") else "lk_" + k
            if not hasattr(cfg, name):
                raise TypeError("unknown flow parameter %r" % k)
            setattr(cfg, name, v)
        self.cfg = cfg
        self.width, self.height, self.channels, self.max_batch = width, height, list(channels), max_batch
        self.c_dim, self.K = channels[0], cfg.lk_max_corners
        self.last_dense_stats = None  # float64 [n, 10]: the records of the last dense call (dense_score, eval_*(dense=...))
        self._h = ctypes.c_void_p()
        _check(self.lib.eigen_create(ctypes.byref(cfg), ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.eigen_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------------------------------
    def set_weights(self, weights):
        from .weights import tensor_names, tensor_shapes
        names = tensor_names(len(self.channels))
        shapes = tensor_shapes(self.channels, self.width, self.height)
        arrs = []
        for n in names:
            a = np.ascontiguousarray(weights[n], dtype=np.float32)
            if a.shape != shapes[n]:
                raise ValueError("tensor %r has shape %s, expected %s" % (n, a.shape, shapes[n]))
            arrs.append(a)
        tab = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        _check(self.lib.eigen_set_prednet_weights(self._h, tab, ctypes.c_int32(len(arrs))))

    def set_grid(self, planes):
        planes = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64).reshape(-1) for p in planes]))
        if planes.shape[1] != self.width * self.height:
            raise ValueError("grid planes must have H*W = %d values" % (self.width * self.height))
        self.n_planes = planes.shape[0]
        _check(self.lib.eigen_set_grid(self._h, _ptr(planes), ctypes.c_int32(planes.shape[0])))

    @staticmethod
    def _genome_struct(gb):
        s = GenomeBatchC(gb.n_genomes, gb.c_out, gb.node_off.ctypes.data, gb.edge_off.ctypes.data, gb.node_act.ctypes.data,
                         gb.node_bias.ctypes.data, gb.node_resp.ctypes.data, gb.edge_src.ctypes.data, gb.edge_w.ctypes.data,
                         gb.out_node.ctypes.data)
        return s

    # -- stages --------------------------------------------------------------------------------------
    def render_cppn(self, gb, d_images, bg=1, gradient=1, stream=None):
        s = self._genome_struct(gb)
        _check(self.lib.eigen_render_cppn(self._h, ctypes.byref(s), ctypes.c_int32(bg), ctypes.c_int32(gradient), _ptr(d_images), _stream_arg(stream)))

    def eval_cppn_nodes(self, gb, d_nodes, stream=None):
        """float64 [n, c_out, H*W] raw output-node values (create_cppn node calls, generate_illusion.py:395)."""
        s = self._genome_struct(gb)
        _check(self.lib.eigen_eval_cppn_nodes(self._h, ctypes.byref(s), _ptr(d_nodes), _stream_arg(stream)))

    def render_moving_cppn(self, gb, affine, affine_inv=None, flow=False, layer=False, out=None, stream=None):
        """eigen_render_moving_cppn ("Moving textures"): n sequences of T frames of one or two CPPN layers on affine
        coordinates.  affine: float64 [n, T, L, 6], pixel -> texture, genome b * L + l of `gb` being layer l of sample b; affine_inv: the
        same shape, texture -> pixel, needed with flow=True.  out: a uint8 device tensor [n, T, C, H, W] to render into, contiguous but
        for its stride between samples (default: a fresh one).
        -> (frames uint8 [n, T, C, H, W], flow float64 [n, T - 1, 2, H, W] or None, layer uint8 [n, T, H, W] or None), device tensors."""
        import torch
        affine = check_moving_affines(affine, affine_inv if flow else None, gb.n_genomes, flow)
        n, T, L = affine[0].shape[:3]
        shape = (n, T, self.c_dim, self.height, self.width)
        seq = int(np.prod(shape[1:]))
        dev = torch.device("cuda", self.cfg.device)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_cuda or (n > 1 and out.stride(0) < seq) \
                or tuple(out.stride()[1:]) != (seq // T, self.height * self.width, self.width, 1):
            raise ValueError("out must be a uint8 device tensor %s, every sequence contiguous" % (shape,))
        bstride = int(out.stride(0)) if n > 1 else seq
        d_flow = torch.empty((n, T - 1, 2, self.height, self.width), dtype=torch.float64, device=dev) if flow else None
        d_layer = torch.empty((n, T, self.height, self.width), dtype=torch.uint8, device=dev) if layer else None
        s = self._genome_struct(gb)
        _check(self.lib.eigen_render_moving_cppn(self._h, ctypes.byref(s), ctypes.c_int32(n), ctypes.c_int32(T), ctypes.c_int32(L), _ptr(affine[0]),
                                                 _ptr(affine[1]) if flow else None, _ptr(out), ctypes.c_int64(bstride), _ptr(d_flow), _ptr(d_layer),
                                                 _stream_arg(stream)))
        return out, d_flow, d_layer

    def moving_cppn_valid(self, affine, affine_inv, stream=None):
        """eigen_moving_cppn_valid ("The joint objective and the valid pixels"): the validity planes of the flow
        ``render_moving_cppn`` states for the same affines, float64 [n, T >= 2, L, 6] each.  -> uint8 device tensor [n, T - 1, H, W]: 1
        where the surface a pixel of frame t shows lies inside the image in frame t + 1 and, if it is on layer 0, is not covered there
        by layer 1; else 0.  From the affines alone: no genome is read."""
        import torch
        a = np.ascontiguousarray(affine, dtype=np.float64)
        if a.ndim != 4 or a.shape[0] < 1 or a.shape[1] < 2 or a.shape[2] not in (1, 2) or a.shape[3] != 6:
            raise ValueError("affine must be float64 [n, T >= 2, L in (1, 2), 6], got shape %s" % (a.shape,))
        if affine_inv is None:
            raise ValueError("the validity planes need affine_inv")
        i = np.ascontiguousarray(affine_inv, dtype=np.float64)
        if i.shape != a.shape:
            raise ValueError("affine_inv has shape %s, affine %s" % (i.shape, a.shape))
        n, T, L = a.shape[:3]
        d_valid = torch.empty((n, T - 1, self.height, self.width), dtype=torch.uint8, device=torch.device("cuda", self.cfg.device))
        _check(self.lib.eigen_moving_cppn_valid(self._h, ctypes.c_int32(n), ctypes.c_int32(T), ctypes.c_int32(L), _ptr(a), _ptr(i), _ptr(d_valid), _stream_arg(stream)))
        return d_valid

    def cppn_param_grads(self, gb, d_image_grad, bg=1, gradient=1, stream=None):
        """The gradient of a loss by the parameters of the genomes of `gb`, from its gradient by their gradient = 1 renders (DESIGN.md
        section 13, "CPPN parameter gradients").  d_image_grad: a float32 device tensor [n, C, H, W], d loss / d (byte / 255), as
        ``PredNetTrainer`` returns its tied frame gradient; a stride between the images above C*H*W is taken from the tensor.
        -> (g_bias [total_nodes], g_resp [total_nodes], g_w [total_edges]) float64 numpy arrays in the batch's own layout."""
        per = self.c_dim * self.height * self.width
        shape, dtype = tuple(getattr(d_image_grad, "shape", ())), str(getattr(d_image_grad, "dtype", ""))
        if "float32" not in dtype or len(shape) != 4 or shape[0] < gb.n_genomes or int(np.prod(shape[1:])) != per:
            raise ValueError("d_image_grad must be float32 [>= %d, %d, %d, %d], got %s %s" % (gb.n_genomes, self.c_dim, self.height, self.width, dtype, shape))
        stride = getattr(d_image_grad, "stride", None)
        bstride = int(stride(0)) if callable(stride) and shape[0] > 1 else per
        if callable(stride) and tuple(stride()[1:]) != (shape[2] * shape[3], shape[3], 1):
            raise ValueError("every image of d_image_grad must be contiguous")
        n_nodes = int(gb.node_off[gb.n_genomes])
        g_bias, g_resp, g_w = np.zeros(n_nodes, np.float64), np.zeros(n_nodes, np.float64), np.zeros(max(int(gb.edge_off[n_nodes]), 1), np.float64)
        s = self._genome_struct(gb)
        _check(self.lib.eigen_cppn_param_grads(self._h, ctypes.byref(s), ctypes.c_int32(bg), ctypes.c_int32(gradient), _ptr(d_image_grad), ctypes.c_int64(bstride),
                                               _ptr(g_bias), _ptr(g_resp), _ptr(g_w), _stream_arg(stream)))
        return g_bias, g_resp, g_w[:int(gb.edge_off[n_nodes])]

    def _check_images(self, d_images, batch):
        """The C side reads batch * C0 * H * W bytes from the raw pointer: refuse anything smaller."""
        if not 1 <= int(batch) <= self.max_batch:
            return  # the library reports capacity errors itself (EIGEN_ERR_CAPACITY)
        need = int(batch) * self.c_dim * self.height * self.width
        have = getattr(d_images, "numel", None)
        have = have() if callable(have) else getattr(d_images, "size", None)
        if isinstance(have, int) and have < need:
            raise ValueError("image buffer holds %d bytes, %d images of (%d, %d, %d) need %d"
                             % (have, batch, self.c_dim, self.height, self.width, need))

    def prednet_rollout(self, d_images, batch, n_steps, first_out_step, d_frames, stream=None):
        self._check_images(d_images, batch)
        _check(self.lib.eigen_prednet_rollout(self._h, _ptr(d_images), ctypes.c_int32(batch), ctypes.c_int32(n_steps),
                                              ctypes.c_int32(first_out_step), _ptr(d_frames), _stream_arg(stream)))

    @staticmethod
    def _buffer_bytes(buf):
        """Bytes reachable from the first element of a torch tensor (its storage: a strided view reaches past its own elements) or of a
        C-contiguous numpy array; None for a raw address."""
        if isinstance(buf, np.ndarray):
            return int(buf.nbytes) if buf.flags.c_contiguous else None
        if hasattr(buf, "untyped_storage"):
            st = buf.untyped_storage()
            return int(st.nbytes()) - (int(buf.data_ptr()) - int(st.data_ptr()))
        return None

    def prednet_sequence(self, d_in, in_bstride, batch, n_in, n_ext, reset, first_out_step, d_out, stream=None):
        """eigen_prednet_sequence: frame t of sequence b at byte d_in + b * in_bstride + t * C*H*W; predictions of the steps
        from first_out_step on into d_out [batch][n_in + n_ext - first_out_step][C][H][W].  reset=False continues from the state
        the previous call with the same batch left."""
        frame = self.c_dim * self.height * self.width
        if 1 <= int(batch) <= self.max_batch and int(n_in) >= 0 and int(n_ext) >= 0 and 0 <= int(first_out_step) < int(n_in) + int(n_ext):
            # the C side reads and writes through raw pointers: refuse buffers smaller than what it touches
            checks = [(d_out, int(batch) * (int(n_in) + int(n_ext) - int(first_out_step)) * frame, "output")]
            if int(n_in) > 0 and d_in is not None:
                checks.append((d_in, (int(batch) - 1) * int(in_bstride) + int(n_in) * frame, "input"))
            for buf, need, what in checks:
                have = self._buffer_bytes(buf)
                if have is not None and have < need:
                    raise ValueError("%s buffer holds %d bytes, %d are needed" % (what, have, need))
        _check(self.lib.eigen_prednet_sequence(self._h, _ptr(d_in), ctypes.c_int64(int(in_bstride)), ctypes.c_int32(batch), ctypes.c_int32(n_in),
                                               ctypes.c_int32(n_ext), ctypes.c_int32(int(reset)), ctypes.c_int32(first_out_step), _ptr(d_out),
                                               _stream_arg(stream)))

    def flow(self, d_img0, stride0, d_img1, stride1, batch, d_vectors, d_counts, stream=None):
        _check(self.lib.eigen_flow(self._h, _ptr(d_img0), ctypes.c_int64(stride0), _ptr(d_img1), ctypes.c_int64(stride1),
                                   ctypes.c_int32(batch), _ptr(d_vectors), _ptr(d_counts), _stream_arg(stream)))

    def score(self, structure, d_vectors, d_counts, batch, d_fitness, stream=None, width=0, height=0):
        _check(self.lib.eigen_score(self._h, ctypes.c_int32(int(structure)), ctypes.c_int32(width), ctypes.c_int32(height), _ptr(d_vectors),
                                    _ptr(d_counts), ctypes.c_int32(batch), _ptr(d_fitness), _stream_arg(stream)))

    # -- the dense fitness (include/eigen_engine.h "dense fitness") --------------
    def _dense_args(self, dense):
        """`dense`: anything with ``dense_settings(h)`` -> (radius, eps, the ctypes settings of its score, True for a Circles score)
        and ``mask_on(torch, device, h, w)`` -> the shared mask on the device or None (``fitness.DenseFitness``).
        -> (DenseSettingsC, what must stay alive during the call, the mask's pointer).  A `dense` whose ``frames`` is "float" sets
        EIGEN_DENSE_FLOAT_FRAMES: the eval entries then score PredNet's float predictions, the byte stage refuses it."""
        radius, eps, sc, by_circles = dense.dense_settings(self.height)
        addr = ctypes.addressof(sc)
        flags = DENSE_FLOAT_FRAMES if getattr(dense, "frames", "byte") == "float" else 0
        cfg = DenseSettingsC(FlowSettingsC(int(radius), flags, float(eps)), addr if by_circles else None, None if by_circles else addr)
        import torch
        mask = dense.mask_on(torch, self.cfg.device, self.height, self.width)
        return cfg, (sc, mask), _ptr(mask)

    @staticmethod
    def _dense_solve(dense):
        """the eigen_dense_solve of a `dense` argument (its ``levels`` and ``iters``, 1 where it has none), or None for the single step:
        such a call goes to the plain entry, as it always did"""
        levels, iters = int(getattr(dense, "levels", 1)), int(getattr(dense, "iters", 1))
        return None if (levels, iters) == (1, 1) else DenseSolveC(levels, iters)

    def _dense_members(self, dense, batch):
        """The members of a `dense` argument (its ``members``, None where it has none) for a call of `batch` samples -> None, or
        (the eigen_flow_members, the per-sample planes [batch, H, W] on the device, which take d_mask's place, or None under corner
        members, which keep the shared mask).  ``dense.members_on`` makes both (ValueError: planes of another shape)."""
        if getattr(dense, "members", None) is None:
            return None
        import torch
        return dense.members_on(torch, self.cfg.device, int(batch), self.height, self.width)

    def debug_dense_solve(self, force=None):
        """Test hook (eigen_debug_dense_solve): force True / False sets whether the single step goes through the iteration kernel too.
        -> the bytes of the pyramid this handle holds, 0 before its first iterated call"""
        n = ctypes.c_int64(-1)
        _check(self.lib.eigen_debug_dense_solve(self._h, ctypes.c_int32(-1 if force is None else int(bool(force))), ctypes.byref(n)))
        return int(n.value)

    def dense_score(self, d_img0, stride0, d_img1, stride1, batch, dense, stats=False, flow=False, stream=None, members_out=False):
        """The dense stage alone on two batches of uint8 device images (eigen_dense_score): image b of either at its pointer + b * its
        stride (bytes).  -> the float64 [batch] fitness, S_b of every sample; stats=True appends the float64 [batch, 10] records,
        flow=True the field u, float64 [batch, 2, H, W] (numpy).  The records are also left in ``last_dense_stats``.  A `dense` with
        ``levels`` or ``iters`` above 1 runs the pyramidal, iterated solve (eigen_dense_score_iter), one with ``members`` counts those
        alone (eigen_dense_score_members; per-sample planes must be [batch, H, W]).  members_out=True (corner members) appends
        (the member planes uint8 [batch, H, W], the corner counts int32 [batch], before the mask)."""
        cfg, keep, d_mask = self._dense_args(dense)
        solve = self._dense_solve(dense)
        batch = int(batch)
        mem = self._dense_members(dense, batch)
        if members_out and (mem is None or mem[1] is not None):
            raise ValueError("members_out needs a dense fitness with corner members")
        fit, rec = np.zeros(max(batch, 0), np.float64), np.zeros((max(batch, 0), DENSE_REC), np.float64)
        u = None
        if flow:
            import torch
            u = torch.empty((max(batch, 1), 2, self.height, self.width), dtype=torch.float64, device="cuda:%d" % self.cfg.device)
        if 1 <= batch <= self.max_batch:   # the C side reads through raw pointers: refuse buffers smaller than what it touches
            per = self.c_dim * self.height * self.width
            for buf, stride, what in ((d_img0, stride0, "img0"), (d_img1, stride1, "img1")):
                have = self._buffer_bytes(buf)
                if have is not None and int(stride) >= per and have < (batch - 1) * int(stride) + per:
                    raise ValueError("%s buffer holds %d bytes, %d are needed" % (what, have, (batch - 1) * int(stride) + per))
        args = (self._h, _ptr(d_img0), ctypes.c_int64(int(stride0)), _ptr(d_img1), ctypes.c_int64(int(stride1)), ctypes.c_int32(batch), ctypes.byref(cfg), d_mask,
                _ptr(fit), _ptr(rec), _ptr(u), _stream_arg(stream))
        planes = counts = None
        if mem is None:
            _check(self.lib.eigen_dense_score(*args) if solve is None else self.lib.eigen_dense_score_iter(*args, ctypes.byref(solve)))
        else:
            if members_out:
                planes, counts = np.zeros((max(batch, 0), self.height, self.width), np.uint8), np.zeros(max(batch, 0), np.int32)
            args = args[:7] + (d_mask if mem[1] is None else _ptr(mem[1]),) + args[8:]
            _check(self.lib.eigen_dense_score_members(*args, None if solve is None else ctypes.byref(solve), ctypes.byref(mem[0]), _ptr(planes), _ptr(counts)))
        self.last_dense_stats = rec
        out = (fit,) + ((rec,) if stats else ()) + ((u[:batch].cpu().numpy(),) if flow else ()) + (((planes, counts),) if members_out else ())
        return out[0] if len(out) == 1 else out

    def dense_score_float(self, img0, stride0, img1, stride1, batch, dense, stats=False, flow=False, stream=None):
        """The dense stage alone on float images (eigen_dense_score_float): `img0` a uint8 or float32 device tensor, `img1` a float32
        one, image b of either at its pointer + b * its stride (elements).  Results as ``dense_score``; the two gray planes the stage
        started from are then ``last_dense_gray()``.  `dense` may carry either ``frames``.  There is no ``members_out``: the entry
        returns no member planes; the corners are picked on the byte image of img0, where ``dense_score(members_out=True)`` returns them."""
        import torch
        if not (torch.is_tensor(img0) and img0.dtype in (torch.uint8, torch.float32)) or not (torch.is_tensor(img1) and img1.dtype == torch.float32):
            raise ValueError("img0 must be a uint8 or float32 device tensor and img1 a float32 one")
        cfg, keep, d_mask = self._dense_args(dense)
        solve = self._dense_solve(dense)
        batch = int(batch)
        mem = self._dense_members(dense, batch)
        fit, rec = np.zeros(max(batch, 0), np.float64), np.zeros((max(batch, 0), DENSE_REC), np.float64)
        u = torch.empty((max(batch, 1), 2, self.height, self.width), dtype=torch.float64, device="cuda:%d" % self.cfg.device) if flow else None
        if 1 <= batch <= self.max_batch:   # the C side reads through raw pointers: refuse buffers smaller than what it touches
            per = self.c_dim * self.height * self.width
            for buf, stride, what in ((img0, stride0, "img0"), (img1, stride1, "img1")):
                have = buf.numel()
                if int(stride) >= per and have < (batch - 1) * int(stride) + per:
                    raise ValueError("%s buffer holds %d elements, %d are needed" % (what, have, (batch - 1) * int(stride) + per))
        as_float = img0.dtype == torch.float32
        _check(self.lib.eigen_dense_score_float(
            self._h, None if as_float else _ptr(img0), _ptr(img0) if as_float else None, ctypes.c_int64(int(stride0)), _ptr(img1), ctypes.c_int64(int(stride1)),
            ctypes.c_int32(batch), ctypes.byref(cfg), None if solve is None else ctypes.byref(solve), None if mem is None else ctypes.byref(mem[0]),
            d_mask if mem is None or mem[1] is None else _ptr(mem[1]), _ptr(fit), _ptr(rec), _ptr(u), _stream_arg(stream)))
        self.last_dense_stats = rec
        out = (fit,) + ((rec,) if stats else ()) + ((u[:batch].cpu().numpy(),) if flow else ())
        return out[0] if len(out) == 1 else out

    def last_dense_gray(self, batch, stream=None):
        """(I0, I1), float64 [batch, H, W] each: the gray planes the last float dense call on this engine started from
        (eigen_debug_dense_gray).  EngineError: there was none, or it was of another batch."""
        I0, I1 = (np.zeros((max(int(batch), 0), self.height, self.width), np.float64) for _ in range(2))
        _check(self.lib.eigen_debug_dense_gray(self._h, ctypes.c_int32(int(batch)), _ptr(I0), _ptr(I1), _stream_arg(stream)))
        return I0, I1

    def eval_population(self, gb, structure, bg=1, gradient=1, pairing=PAIR_POPULATION, stream=None, dense=None):
        """dense None: the corner fitness (eigen_eval_population).  dense: a ``fitness.DenseFitness`` resolved for `structure`: the dense
        motion score (eigen_eval_population_dense); the records of the call are then left in ``last_dense_stats``.  A `dense` with
        ``members`` counts those alone (eigen_eval_population_dense_members); per-sample planes must be [n_genomes, H, W]."""
        fit = np.zeros(gb.n_genomes, dtype=np.float64)
        s = self._genome_struct(gb)
        if dense is not None:
            cfg, keep, d_mask = self._dense_args(dense)
            rec = np.zeros((gb.n_genomes, DENSE_REC), np.float64)
            solve = self._dense_solve(dense)
            args = (self._h, ctypes.byref(s), ctypes.c_int32(int(structure)), ctypes.c_int32(bg), ctypes.c_int32(gradient), ctypes.c_int32(pairing), ctypes.byref(cfg),
                    d_mask, _ptr(fit), _ptr(rec), _stream_arg(stream))
            mem = self._dense_members(dense, gb.n_genomes)
            if mem is None:
                _check(self.lib.eigen_eval_population_dense(*args) if solve is None else self.lib.eigen_eval_population_dense_iter(*args, ctypes.byref(solve)))
            else:
                args = args[:7] + (d_mask if mem[1] is None else _ptr(mem[1]),) + args[8:]
                _check(self.lib.eigen_eval_population_dense_members(*args, None if solve is None else ctypes.byref(solve), ctypes.byref(mem[0])))
            self.last_dense_stats = rec
            return fit
        _check(self.lib.eigen_eval_population(self._h, ctypes.byref(s), ctypes.c_int32(int(structure)), ctypes.c_int32(bg),
                                              ctypes.c_int32(gradient), ctypes.c_int32(pairing), _ptr(fit), _stream_arg(stream)))
        return fit

    def eval_images(self, d_images, batch, structure, pairing=PAIR_SINGLE, stream=None, dense=None):
        """dense None: the corner fitness and its vectors (eigen_eval_images).  dense: as ``eval_population``; there are no vectors, the
        second result is an empty list per image."""
        self._check_images(d_images, batch)
        if dense is not None:
            cfg, keep, d_mask = self._dense_args(dense)
            fit, rec = np.zeros(max(int(batch), 0), np.float64), np.zeros((max(int(batch), 0), DENSE_REC), np.float64)
            solve = self._dense_solve(dense)
            args = (self._h, _ptr(d_images), ctypes.c_int32(batch), ctypes.c_int32(int(structure)), ctypes.c_int32(pairing), ctypes.byref(cfg), d_mask, _ptr(fit),
                    _ptr(rec), _stream_arg(stream))
            mem = self._dense_members(dense, batch)
            if mem is None:
                _check(self.lib.eigen_eval_images_dense(*args) if solve is None else self.lib.eigen_eval_images_dense_iter(*args, ctypes.byref(solve)))
            else:
                args = args[:6] + (d_mask if mem[1] is None else _ptr(mem[1]),) + args[7:]
                _check(self.lib.eigen_eval_images_dense_members(*args, None if solve is None else ctypes.byref(solve), ctypes.byref(mem[0])))
            self.last_dense_stats = rec
            return fit, [np.zeros((0, 4), np.float32) for _ in range(int(batch))]
        fit = np.zeros(batch, dtype=np.float64)
        vec = np.zeros((batch, self.K, 4), dtype=np.float32)
        cnt = np.zeros(batch, dtype=np.int32)
        _check(self.lib.eigen_eval_images(self._h, _ptr(d_images), ctypes.c_int32(batch), ctypes.c_int32(int(structure)),
                                          ctypes.c_int32(pairing), _ptr(fit), _ptr(vec), _ptr(cnt), _stream_arg(stream)))
        return fit, [vec[i, :cnt[i]].copy() for i in range(batch)]

    # -- test / measurement hooks --------------------------------------------------------------------
    def test_conv(self, d_srcs, cins, ups, h_weights, cout, H, W, batch, d_out, stream=None):
        n = len(d_srcs)
        st = (ctypes.c_void_p * n)(*[int(s.data_ptr()) for s in d_srcs])
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w in h_weights]
        wt = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        ci = (ctypes.c_int32 * n)(*cins)
        up = (ctypes.c_int32 * n)(*ups)
        _check(self.lib.eigen_test_conv(self._h, ctypes.c_int32(n), st, ci, up, wt, ctypes.c_int32(cout), ctypes.c_int32(H),
                                        ctypes.c_int32(W), ctypes.c_int32(batch), _ptr(d_out), _stream_arg(stream)))

    def time_conv(self, d_srcs, cins, ups, h_weights, cout, H, W, batch, d_out, iters=5, stream=None):
        n = len(d_srcs)
        st = (ctypes.c_void_p * n)(*[int(s.data_ptr()) for s in d_srcs])
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w in h_weights]
        wt = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        ci = (ctypes.c_int32 * n)(*cins)
        up = (ctypes.c_int32 * n)(*ups)
        ms = ctypes.c_double(0)
        _check(self.lib.eigen_time_conv(self._h, ctypes.c_int32(n), st, ci, up, wt, ctypes.c_int32(cout), ctypes.c_int32(H),
                                        ctypes.c_int32(W), ctypes.c_int32(batch), _ptr(d_out), ctypes.c_int32(iters), ctypes.byref(ms),
                                        _stream_arg(stream)))
        return ms.value

    def test_det_math(self, d_x, n, d_exp, d_sig, d_tanh, stream=None):
        _check(self.lib.eigen_test_det_math(self._h, _ptr(d_x), ctypes.c_int32(n), _ptr(d_exp), _ptr(d_sig), _ptr(d_tanh), _stream_arg(stream)))

    def timings(self):
        ms = np.zeros(6, dtype=np.float64)
        _check(self.lib.eigen_get_timings(self._h, _ptr(ms)))
        return dict(render_ms=ms[0], prednet_ms=ms[1], flow_ms=ms[2], score_ms=ms[3], conv_ms=ms[4], conv_launches=int(ms[5]))

    def conv_profile(self, enable, reset=True):
        out = np.zeros((6 * MAX_LAYERS, 8), dtype=np.float64)
        n = ctypes.c_int32(0)
        _check(self.lib.eigen_conv_profile(self._h, ctypes.c_int32(int(enable)), ctypes.c_int32(int(reset)), _ptr(out),
                                           ctypes.c_int32(out.shape[0]), ctypes.byref(n)))
        rows = []
        for r in out[:n.value]:
            rows.append(dict(layer=int(r[0]), epi={1: "lstm", 2: "convA", 3: "convP", 4: "lstm", 5: "up4", 6: "up4"}.get(int(r[1]) & 15, "raw"), step0=bool((int(r[1]) >> 4) & 1),
                             wino=bool(int(r[1]) & 32),  # Winograd form (csrc/conv_wino4.h): flops_per_image counts ITS multiply-adds
                             NI=int(r[2]), TW=int(r[3]),
                             launches=int(r[4]), ms=float(r[5]), flops_per_image=float(r[6]), n_nblk=int(r[7])))
        return rows

    def debug_dense_flow(self, batch, stream=None):
        """float32 [batch, 2, H, W]: the dense Farneback field of the last flow call (engines created with flow="farneback")."""
        f = np.zeros((batch, 2, self.height, self.width), np.float32)
        _check(self.lib.eigen_debug_dense_flow(self._h, ctypes.c_int32(batch), _ptr(f), _stream_arg(stream)))
        return f

    def debug_state(self, batch, stream=None):
        """The float32 layer state the last prednet_sequence call left (eigen_debug_state): one dict per layer, "R", "c", "P" of
        [batch, C_l, H_l, W_l] and "E" of [batch, 2 C_l, H_l, W_l] (E_0: the error units the last executed step consumed)."""
        out = []
        for l, C in enumerate(self.channels):
            d = {}
            for which, k in enumerate(("R", "c", "P", "E")):
                d[k] = np.zeros((batch, (2 if k == "E" else 1) * C, self.height >> l, self.width >> l), np.float32)
                _check(self.lib.eigen_debug_state(self._h, ctypes.c_int32(batch), ctypes.c_int32(l), ctypes.c_int32(which), _ptr(d[k]), _stream_arg(stream)))
            out.append(d)
        return out

    def debug_corners(self, batch, stream=None):
        c = np.zeros((batch, self.K, 2), np.float32); n = np.zeros(batch, np.int32)
        nx = np.zeros((batch, self.K, 2), np.float32); st = np.zeros((batch, self.K), np.uint8)
        _check(self.lib.eigen_debug_corners(self._h, ctypes.c_int32(batch), _ptr(c), _ptr(n), _ptr(nx), _ptr(st), _stream_arg(stream)))
        return c, n, nx, st

    def flops_per_step(self):
        return float(self.lib.eigen_prednet_flops_per_step(self._h))
