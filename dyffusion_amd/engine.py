"""Thin object wrapper over the C ABI (one HipEngine = one dyf_engine).  PyTorch is only used for device memory
and streams here: every tensor crosses the boundary as a raw device pointer (`tensor.data_ptr()`)."""
import ctypes as C
import operator
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L


class EngineError(RuntimeError):
    pass


def _raise(status: int, msg: str):
    if status == L.DYF_ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    if status == L.DYF_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise EngineError(msg)


def net_config(*, in_channels: int, cond_channels: int, out_channels: int, dim: int, with_time_emb: bool = True,
               upsample_dims: Optional[Sequence[int]] = (256, 256), dropout: float = 0.0,
               input_dropout: float = 0.0, outer_sample_mode: str = "bilinear") -> L.NetConfig:
    uh, uw = (0, 0) if upsample_dims is None else (int(upsample_dims[0]), int(upsample_dims[1]))
    cfg = L.NetConfig()
    cfg.arch, cfg.in_channels, cfg.cond_channels, cfg.out_channels = L.ARCH_UNET_SIMPLE, in_channels, cond_channels, out_channels
    cfg.dim, cfg.with_time_emb, cfg.upsample_h, cfg.upsample_w = dim, int(bool(with_time_emb)), uh, uw
    cfg.dropout, cfg.input_dropout = float(dropout), float(input_dropout)
    if outer_sample_mode not in ("bilinear", "nearest"):
        raise NotImplementedError(f"outer_sample_mode={outer_sample_mode!r}: the HIP engine implements 'bilinear' and 'nearest'")
    cfg.outer_nearest = int(outer_sample_mode == "nearest")
    return cfg


def resnet_net_config(*, in_channels: int, cond_channels: int, out_channels: int, dim: int, dim_mults=(1, 2, 4),
                      with_time_emb: bool = True, block_dropout: float = 0.0, block_dropout1: float = 0.0,
                      attn_dropout: float = 0.0, input_dropout: float = 0.0, groups: int = 8, init_kernel_size: int = 7,
                      init_padding: int = 3, keep_spatial_dims: bool = False, double_conv_layer: bool = True,
                      learned_sinusoidal_dim: int = 0) -> L.NetConfig:
    """dyf_net_config for src.models.unet.Unet (no outer resampling)."""
    cfg = L.NetConfig()
    cfg.arch, cfg.in_channels, cfg.cond_channels, cfg.out_channels = L.ARCH_UNET_RESNET, in_channels, cond_channels, out_channels
    cfg.dim, cfg.with_time_emb = dim, int(bool(with_time_emb))
    cfg.dropout, cfg.input_dropout = float(block_dropout), float(input_dropout)
    cfg.n_mults = len(dim_mults)
    for i, m in enumerate(dim_mults):
        cfg.dim_mults[i] = int(m)
    cfg.block_dropout1, cfg.attn_dropout, cfg.groups = float(block_dropout1), float(attn_dropout), int(groups)
    cfg.init_kernel_size, cfg.init_padding = int(init_kernel_size), int(init_padding)
    cfg.keep_spatial_dims, cfg.single_conv_layer = int(bool(keep_spatial_dims)), int(not double_conv_layer)
    cfg.learned_sinusoidal_dim = int(learned_sinusoidal_dim)
    return cfg


def default_dtype_for(net) -> str:
    """16-bit storage / MFMA operand format an engine is built with when the caller names none: "bf16" for the unet_simple /
    SimpleConvNet backbones (BASELINE configs[1]: "bf16"), "fp16" for the ResNet-UNet `unet.Unet` (OISST, 512^2: ~60 16-bit
    roundings per forward and 93 chained forwards per rollout -- bf16's 8 mantissa bits give 4e-2 .. 5e-2 per field over the
    OISST rollout, fp16's 11 bits 6e-3 at the same MFMA rate and the same bytes).  A network class states
    its default as `default_engine_dtype`; `net.engine_dtype = "bf16" | "fp16" | "fp32" | "bf16x3"` or `DYffusion(dtype=...)` override it
    ("fp32": reference-precision sampling, dyf_set_sample_precision(32); "bf16x3": the same forward with (hi, lo) bf16 conv operands on
    the bf16 matrix cores, dyf_set_sample_precision(48))."""
    return getattr(net, "engine_dtype", None) or getattr(net, "default_engine_dtype", "bf16")


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); the HIP engine has no CPU path")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def parse_train_precision(precision) -> int:
    """Lightning-style precision value -> bits for dyf_train_set_precision (0 = not set)."""
    if precision is None:
        return 0
    key = str(precision).lower()
    if key in ("32", "32-true", "fp32", "float32"):
        return 32
    if key in ("bf16x3", "48"):
        # fp32-grade convs on the 16-bit matrix cores: each operand a (hi, lo) pair of bf16, three MFMAs per product; all else as under 32
        return L.DYF_TRAIN_PRECISION_BF16X3
    if key in ("16", "16-mixed", "bf16", "bf16-mixed", "fp16", "fp16-mixed"):
        # every 16-bit request runs as bf16-mixed (csrc/train_internal.h): the engine has no GradScaler, and fp16 gradient operands
        # without one lose the gradient at real batch sizes (dL/dout ~ 1 / numel).  An explicit fp16 request is told so once.
        if key in ("fp16", "fp16-mixed"):
            import warnings
            warnings.warn("train precision 'fp16-mixed' runs as bf16-mixed: the engine rounds its training conv operands to bf16 "
                          "(no loss scaling needed); fp16 operands are not offered", stacklevel=2)
        return 16
    raise ValueError(f"train precision {precision!r}: expected 32 / '32-true', 16 / '16-mixed' / 'bf16-mixed' or 48 / 'bf16x3'")


def resolve_train_deterministic(setting) -> bool:
    """The deterministic training mode a `train_deterministic` setting asks for right now (dyf_train_set_deterministic; the reference's
    `trainer.deterministic`): True / False fix it; None follows `torch.are_deterministic_algorithms_enabled()` -- what Lightning's
    `Trainer(deterministic=True)` sets -- and is read again at every training forward.  Anything else is a ValueError."""
    if setting is None:
        return bool(torch.are_deterministic_algorithms_enabled())
    if isinstance(setting, bool):
        return setting
    raise ValueError(f"train_deterministic {setting!r}: expected True, False or None (None follows torch.use_deterministic_algorithms)")


class HipEngine:
    def __init__(self, forecaster: L.NetConfig, interpolator: L.NetConfig, height: int, width: int, max_batch: int,
                 device: Optional[int] = None, use_graph: bool = True, enable_mfma: bool = True, dtype: str = "bf16",
                 batch_invariant: bool = False, row_groups: Optional[int] = None, train_precision=None,
                 attention_dropout: str = "fast", train_deterministic=None):
        attn_mode = L.attention_dropout_mode(attention_dropout)  # ValueError before anything is created
        resolve_train_deterministic(train_deterministic)
        self._train_deterministic = train_deterministic  # True / False / None (follow torch): applied before every training call
        if not torch.cuda.is_available():
            raise EngineError("no GPU visible: the DYffusion HIP engine needs an MI355X (gfx950); there is no CPU fallback")
        # "fp32" / "float32" / "32": the default (bf16) build with dyf_set_sample_precision(32) -- every sampling forward in fp32
        # "bf16x3" / "48": the same with dyf_set_sample_precision(48) -- that forward with (hi, lo) bf16 conv operands on the bf16 matrix cores
        self.dtype = L.canonical_dtype(dtype)
        storage = L.storage_dtype(dtype)
        self._lib = L.lib(storage)
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.height, self.width, self.max_batch = int(height), int(width), int(max_batch)
        cfg = L.EngineConfig(L.DYF_ABI_VERSION, self.device, self.height, self.width, self.max_batch, int(use_graph),
                             int(enable_mfma), L.DTYPES[storage], int(batch_invariant),
                             (L.NetConfig * 2)(forecaster, interpolator))
        self.cfg = cfg
        h = C.c_void_p()
        st = self._lib.dyf_engine_create(C.byref(cfg), C.byref(h))
        if st != L.DYF_OK:
            _raise(st, self._lib.dyf_last_error(None).decode())
        self._h = h
        if self.dtype in L.SAMPLE_PRECISION_BITS:
            try:
                self.set_sample_precision(L.SAMPLE_PRECISION_BITS[self.dtype])
            except Exception:
                self.close()
                raise
        if row_groups is not None:  # None: the engine's own default (dyf_engine_create, DYF_ROW_GROUPS)
            self._check(self._lib.dyf_set_row_groups(self._h, int(row_groups)))
        if attn_mode != L.ATTN_DROPOUT_FAST:
            try:
                self.set_attention_dropout(attention_dropout)
            except Exception:
                self.close()
                raise
        if train_precision is not None:
            self.train_set_precision(train_precision)
        self._sync_train_deterministic()
        self._plan_keepalive = None
        self.n_out_slots = 0
        self._tape_net = {}       # tape slot -> network of the recorded training forward
        self._tape_nb = {}        # tape slot -> batch rows of the recorded forward (train_backward validates dout against it)
        self.comm_rank, self.comm_world = 0, 1
        self.synchronize_errors = True  # poll_errors() after every call waits for the call's stream (ResNet-UNet engines only)
        self.train_step_id = 0    # bumped by every p_losses / get_loss training forward: a loss of an older step cannot run backward
        self.plan_valid = False   # cleared by load_weights: the plan's FiLM tables are functions of the weights
        self.weights_version = 0
        self._before_close = []   # callbacks run by close() while the engine is still alive (optim.EngineAdamW)

    # ------------------------------------------------------------------ plumbing
    def _check(self, st: int):
        if st != L.DYF_OK:
            _raise(st, self._lib.dyf_last_error(self._h).decode())

    def poll_errors(self, synchronize: Optional[bool] = None):
        """dyf_poll_errors: asynchronous failures of the work just submitted (a fused GroupNorm convolution whose wait for its
        sample's statistics timed out; csrc/gn_fused.h) fail THIS call instead of the next one.  Engines without a live fused form
        (unet_simple, SimpleConvNet, after a downgrade) return at once; ResNet-UNet engines first wait for the STREAM the call was
        enqueued on (never for the device: other streams keep running; a stream under capture is not waited for).  A caller that
        wants net_forward / sample / sample_gather to stay asynchronous sets `engine.synchronize_errors = False`: a failure is then
        reported by the next entry point instead."""
        if synchronize is None:
            synchronize = self.synchronize_errors
        self._check(self._lib.dyf_poll_errors(self._h, int(synchronize)))

    def gn_fuse_state(self):
        """(live, downgrades): the fused GroupNorm form is in use / how often this engine left it (dyf_gn_fuse_state)."""
        live, down = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.dyf_gn_fuse_state(self._h, C.byref(live), C.byref(down)))
        return bool(live.value), down.value

    def debug_gn_fuse(self, timeout_ticks: int = 0, force_timeout: bool = False):
        """Test hook (dyf_debug_gn_fuse): sweep bound in 100 MHz ticks, forced time-out of every granule sweep."""
        self._check(self._lib.dyf_debug_gn_fuse(self._h, int(timeout_ticks), int(force_timeout)))

    def set_sample_precision(self, bits: int) -> None:
        """dyf_set_sample_precision: 16 = the library's 16-bit path, 32 = fp32 forwards for net_forward / sample / sample_gather,
        48 = those forwards with bf16x3 conv operands (hi / lo bf16 pairs, three MFMAs per product: reference precision on the bf16
        matrix cores).  The first switch to 32 or 48 allocates the engine's fp32 arena; ValueError for any other value."""
        self._check(self._lib.dyf_set_sample_precision(self._h, int(bits)))

    @property
    def sample_precision(self) -> int:
        return int(self._lib.dyf_sample_precision(self._h))

    def set_attention_dropout(self, mode: str) -> None:
        """dyf_set_attention_dropout: how the 16-bit path draws the dropout of unet.Unet's Attention probabilities under the engine's
        generator.  "fast" (default): the quad form, keep probability floor((1 - p) * 256) / 256 on a stream of its own; "exact":
        nn.Dropout(p) on the keep bits of the fp32 / training path (at most 32 767 bottleneck tokens: NotImplementedError beyond).
        Applies to every 16-bit forward that follows, `op_attention(p_drop=...)` included; ValueError for any other string."""
        self._check(self._lib.dyf_set_attention_dropout(self._h, L.attention_dropout_mode(mode)))

    @property
    def attention_dropout(self) -> str:
        return "exact" if int(self._lib.dyf_attention_dropout(self._h)) == L.ATTN_DROPOUT_EXACT else "fast"

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            try:
                for cb in list(getattr(self, "_before_close", ())):  # an EngineAdamW moves its resident state to the host first
                    cb(self)
            finally:  # whatever a callback raised, the engine goes
                self._lib.dyf_engine_destroy(self._h)
                self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream() -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ------------------------------------------------------------------ weights
    @staticmethod
    def _marshal_state_dict(state_dict: Dict[str, torch.Tensor]):
        items = [(k, v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")]
        arrs = [np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy()) for _, v in items]
        n = len(items)
        names = (C.c_char_p * n)(*[k.encode() for k, _ in items])
        data = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        shp_store = [(C.c_int64 * max(1, a.ndim))(*a.shape) for a in arrs]
        shapes = (C.c_void_p * n)(*[C.addressof(s) for s in shp_store])
        ndims = (C.c_int32 * n)(*[a.ndim for a in arrs])
        return n, names, data, shapes, ndims, (arrs, shp_store)  # the last element keeps the buffers alive

    def load_weights(self, net: int, state_dict: Dict[str, torch.Tensor]):
        """state_dict: the reference's `UNet.state_dict()` (same key names)."""
        n, names, data, shapes, ndims, _keep = self._marshal_state_dict(state_dict)
        self.plan_valid = False
        self.weights_version += 1
        self._check(self._lib.dyf_load_weights(self._h, net, n, names, data, shapes, ndims))

    def train_load_weights(self, net: int, state_dict: Dict[str, torch.Tensor]):
        """Refresh only the training copy of `net`'s parameters (after optimizer.step()); the sampling copy keeps the weights of
        the last `load_weights` until that is called again.  Tensors that all live on this engine's GPU are read in place
        (dyf_train_load_weights_dev)."""
        items = [(k, v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")]
        if items and all(v.is_cuda and v.device.index == self.device for _, v in items):
            ts = [v.detach().to(torch.float32).contiguous() for _, v in items]
            n = len(items)
            names = (C.c_char_p * n)(*[k.encode() for k, _ in items])
            data = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
            shp_store = [(C.c_int64 * max(1, t.dim()))(*t.shape) for t in ts]
            shapes = (C.c_void_p * n)(*[C.addressof(s_) for s_ in shp_store])
            ndims = (C.c_int32 * n)(*[t.dim() for t in ts])
            torch.cuda.current_stream().synchronize()  # the optimizer's kernels have written these tensors
            self._check(self._lib.dyf_train_load_weights_dev(self._h, net, n, names, data, shapes, ndims))
            return
        n, names, data, shapes, ndims, _keep = self._marshal_state_dict(state_dict)
        self._check(self._lib.dyf_train_load_weights(self._h, net, n, names, data, shapes, ndims))

    # ------------------------------------------------------------------ per-network seam
    def net_forward(self, net: int, inputs: torch.Tensor, time: Optional[torch.Tensor] = None,
                    condition: Optional[torch.Tensor] = None, dropout_mode: int = 0,
                    masks: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
        inputs = _f32c(inputs, "inputs")
        nb = inputs.shape[0]
        ncfg = self.cfg.net[net]
        if inputs.dim() != 4 or inputs.shape[1] != ncfg.in_channels or tuple(inputs.shape[2:]) != (self.height, self.width):
            raise ValueError(f"inputs must be (NB, {ncfg.in_channels}, {self.height}, {self.width}), got {tuple(inputs.shape)}")
        if condition is not None:
            condition = _f32c(condition, "condition")
            if tuple(condition.shape) != (nb, ncfg.cond_channels, self.height, self.width):
                raise ValueError(f"condition has shape {tuple(condition.shape)}")
        if time is not None:
            time = _f32c(time.reshape(-1), "time")
            if time.numel() != nb:
                raise ValueError("time must have one entry per batch row")
        out = torch.empty((nb, ncfg.out_channels, self.height, self.width), dtype=torch.float32, device=inputs.device)
        mptr = None
        if masks is not None:
            keep = [m.contiguous() for m in masks]
            mptr = (C.c_void_p * len(keep))(*[m.data_ptr() for m in keep])
        self._check(self._lib.dyf_net_forward(
            self._h, net, inputs.data_ptr(), None if time is None else time.data_ptr(),
            None if condition is None else condition.data_ptr(), out.data_ptr(), nb, dropout_mode, mptr, self._stream()))
        self.poll_errors()
        return out

    # ------------------------------------------------------------------ sampler seam
    def set_plan(self, steps: List[dict], *, sampling_cold: bool, cold_for_last_step: bool, forward_conditioning: str,
                 refine: Sequence[tuple], n_out_slots: int, interpolator_dropout: bool, forecaster_dropout: bool):
        n = len(steps)
        arr = (L.PlanStep * n)()
        for i, s in enumerate(steps):
            arr[i] = L.PlanStep(float(s["forecaster_time"]), float(s["tau"]),
                                -1.0 if s["i_next"] is None else float(s["i_next"]),
                                -1.0 if s["i_cur"] is None else float(s["i_cur"]), int(s["is_last"]),
                                -1 if s["out_slot"] is None else int(s["out_slot"]))
        nr = len(refine)
        rt = (C.c_float * max(1, nr))(*[float(t) for t, _ in refine])
        rs = (C.c_int32 * max(1, nr))(*[int(sl) for _, sl in refine])
        plan = L.Plan(n, arr, int(sampling_cold), int(cold_for_last_step), L.FCOND[forward_conditioning], nr, rt, rs,
                      int(n_out_slots), int(interpolator_dropout), int(forecaster_dropout))
        self._plan_keepalive = (arr, rt, rs, plan)
        self._check(self._lib.dyf_set_plan(self._h, C.byref(plan)))
        self.n_out_slots = int(n_out_slots)
        self.plan_valid = True

    def sample(self, initial: torch.Tensor, static: Optional[torch.Tensor] = None,
               masks: Optional[Sequence[torch.Tensor]] = None, noise: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Returns the forecast stack (n_out_slots, NB, C, H, W); slot i = t{i+1}_preds."""
        initial = _f32c(initial, "initial_condition")
        if initial.dim() != 4:
            raise AssertionError(f"condition.shape: {tuple(initial.shape)} (should be 4D)")
        nb = initial.shape[0]
        # the C ABI copies nb * channels * H * W floats from raw pointers: validate the shapes here
        icfg = self.cfg.net[L.NET_INTERPOLATOR]
        c_out = self.cfg.net[L.NET_FORECASTER].out_channels
        if tuple(initial.shape[2:]) != (self.height, self.width) or initial.shape[1] != icfg.in_channels - c_out:
            raise ValueError(f"initial_condition must be (NB, {icfg.in_channels - c_out}, {self.height}, {self.width}), "
                             f"got {tuple(initial.shape)}")
        if (static is None) != (icfg.cond_channels == 0):
            raise ValueError("static_condition must be given iff the networks take conditional channels")
        if static is not None:
            static = _f32c(static, "static_condition")
            if tuple(static.shape) != (nb, icfg.cond_channels, self.height, self.width):
                raise ValueError(f"static_condition must be ({nb}, {icfg.cond_channels}, {self.height}, {self.width}), "
                                 f"got {tuple(static.shape)}")
        if out is None:
            out = torch.empty((self.n_out_slots, nb, c_out, self.height, self.width), dtype=torch.float32,
                              device=initial.device)
        mptr = None
        if masks is not None:
            keep = [m.contiguous() for m in masks]
            mptr = (C.c_void_p * len(keep))(*[m.data_ptr() for m in keep])
        if noise is not None:
            noise = _f32c(noise, "noise")
        if tuple(out.shape) != (self.n_out_slots, nb, c_out, self.height, self.width) or not out.is_contiguous() \
                or out.dtype != torch.float32:
            raise ValueError("out must be a contiguous fp32 (n_out_slots, NB, C, H, W) tensor")
        self._check(self._lib.dyf_sample(self._h, initial.data_ptr(), None if static is None else static.data_ptr(),
                                         out.data_ptr(), nb, mptr, None if noise is None else noise.data_ptr(),
                                         self._stream()))
        self.poll_errors()
        return out

    # ------------------------------------------------------------------ engine-owned exchange (ensemble sharding over GPUs)
    @staticmethod
    def comm_unique_id(dtype: str = "bf16") -> bytes:
        """128-byte RCCL unique id (dyf_comm_unique_id): created on ONE rank, handed to every rank's `comm_init`."""
        lib = L.lib(dtype)
        buf = (C.c_uint8 * L.COMM_ID_BYTES)()
        st = lib.dyf_comm_unique_id(buf)
        if st != L.DYF_OK:
            _raise(st, lib.dyf_last_error(None).decode())
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """This engine's RCCL communicator over `world` ranks (dyf_comm_init); needed by `sample_gather`."""
        if len(unique_id) != L.COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {L.COMM_ID_BYTES} bytes")
        buf = (C.c_uint8 * L.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.dyf_comm_init(self._h, buf, int(rank), int(world)))
        self.comm_rank, self.comm_world = int(rank), int(world)

    def comm_destroy(self):
        self._check(self._lib.dyf_comm_destroy(self._h))
        self.comm_world = 1

    def comm_count(self) -> int:
        """Ranks of this engine's communicator as RCCL reports them (ncclCommCount); 0 when it owns none."""
        n = C.c_int32(0)
        self._check(self._lib.dyf_comm_count(self._h, C.byref(n)))
        return n.value

    def sample_gather(self, initial: torch.Tensor, static: Optional[torch.Tensor], total_rows: int) -> torch.Tensor:
        """dyf_sample_gather: rollout of this rank's rows, ONE all-gather of the forecast stack, unpack -> (n_out_slots, total_rows,
        C, H, W) with every rank's rows in global order."""
        initial = _f32c(initial, "initial_condition")
        nb = initial.shape[0]
        icfg = self.cfg.net[L.NET_INTERPOLATOR]
        c_out = self.cfg.net[L.NET_FORECASTER].out_channels
        if initial.dim() != 4 or tuple(initial.shape[2:]) != (self.height, self.width) or initial.shape[1] != icfg.in_channels - c_out:
            raise ValueError(f"initial_condition must be (NB, {icfg.in_channels - c_out}, {self.height}, {self.width}), got {tuple(initial.shape)}")
        if (static is None) != (icfg.cond_channels == 0):
            raise ValueError("static_condition must be given iff the networks take conditional channels")
        if static is not None:
            static = _f32c(static, "static_condition")
            if tuple(static.shape) != (nb, icfg.cond_channels, self.height, self.width):
                raise ValueError(f"static_condition has shape {tuple(static.shape)}")
        out = torch.empty((self.n_out_slots, int(total_rows), c_out, self.height, self.width), dtype=torch.float32, device=initial.device)
        self._check(self._lib.dyf_sample_gather(self._h, initial.data_ptr(), None if static is None else static.data_ptr(),
                                                out.data_ptr(), nb, int(total_rows), self._stream()))
        self.poll_errors()
        return out

    def sampler_state(self, what: int, nb: int) -> torch.Tensor:
        """what: 0 = last x0_hat, 1 = x_s, 2 = x_interpolated_s_next of the final step (dyf_sampler_state)."""
        c_out = self.cfg.net[L.NET_FORECASTER].out_channels
        out = torch.empty((nb, c_out, self.height, self.width), dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self._lib.dyf_get_sampler_state(self._h, what, out.data_ptr(), nb, self._stream()))
        return out

    def last_x0hat(self, nb: int) -> torch.Tensor:
        return self.sampler_state(0, nb)

    def seed(self, seed: int):
        """Re-seed the dropout / noise generator; forward and noise counters restart at 0."""
        self._check(self._lib.dyf_seed(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1))))

    def set_log_intermediates(self, enable: bool):
        """log_every_t: keep x0_hat / x_interpolated_s_next / x_interpolated_s of every sampling step of the next `sample` calls."""
        self._check(self._lib.dyf_set_log_intermediates(self._h, int(bool(enable))))

    def get_log(self, step: int, what: int, nb: int) -> torch.Tensor:
        c_out = self.cfg.net[L.NET_FORECASTER].out_channels
        out = torch.empty((nb, c_out, self.height, self.width), dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self._lib.dyf_get_log(self._h, int(step), int(what), out.data_ptr(), nb, self._stream()))
        return out

    @property
    def row_groups(self) -> int:
        """Number of concurrent row groups a large enough sampling call is split over (dyf_set_row_groups; 1 = none)."""
        return int(self._lib.dyf_row_groups(self._h))

    def set_row_offset(self, first_row: int):
        """Global index of this engine's batch row 0 (ensemble sharding): rows draw the masks of the un-sharded batch."""
        self._check(self._lib.dyf_set_row_offset(self._h, C.c_uint32(int(first_row))))

    def read_block_output(self, net: int, layer: int, nb: int) -> torch.Tensor:
        """Test seam: output of UNetBlock `layer` (0..11) of the most recent unet_simple forward, fp32 NCHW."""
        d = self.cfg.net[net].dim
        ch = [2 * d, 2 * d, 4 * d, 8 * d, 8 * d, 8 * d, 8 * d, 8 * d, 4 * d, 2 * d, 2 * d, d][layer]
        uh = self.cfg.net[net].upsample_h or self.height
        uw = self.cfg.net[net].upsample_w or self.width
        sh = layer + 1 if layer < 6 else 11 - layer   # log2 of the block output's down-sampling factor
        shape = (nb, ch, uh >> sh, uw >> sh)
        out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self._lib.dyf_debug_read_block_output(self._h, net, layer, nb, out.data_ptr(), self._stream()))
        return out

    def form_log(self, enable: bool) -> None:
        """Test seam: clear and enable (or disable) the process-wide kernel-form log (dyf_debug_form_log)."""
        self._lib.dyf_debug_form_log(int(bool(enable)))

    def form_log_read(self) -> Dict[str, Dict[int, int]]:
        """{kernel form: {batch rows of the launch: launches noted}} since the log was enabled."""
        n = self._lib.dyf_debug_form_log_read(None, 0)
        buf = C.create_string_buffer(n + 1)
        self._lib.dyf_debug_form_log_read(buf, n + 1)
        out: Dict[str, Dict[int, int]] = {}
        for item in buf.value.decode().split(";"):
            if item:
                key, cnt = item.rsplit("=", 1)
                form, rows = key.rsplit("@", 1)
                out.setdefault(form, {})[int(rows)] = int(cnt)
        return out

    # ------------------------------------------------------------------ introspection
    def forward_counts(self):
        a, b = C.c_int32(), C.c_int32()
        self._check(self._lib.dyf_plan_forward_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def net_flops(self, net: int) -> float:
        f = C.c_double()
        self._check(self._lib.dyf_net_flops(self._h, net, C.byref(f)))
        return f.value

    def net_flops_executed(self, net: int) -> float:
        f = C.c_double()
        self._check(self._lib.dyf_net_flops_executed(self._h, net, C.byref(f)))
        return f.value

    def time_conv_layer(self, net: int, layer: int, nb: int, iters: int = 20):
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.dyf_time_conv_layer(self._h, net, layer, nb, iters, self._stream(), C.byref(ms),
                                                  C.byref(fl), C.byref(by)))
        return ms.value, fl.value, by.value

    def ensemble_metrics(self, preds: torch.Tensor, targets: torch.Tensor):
        """preds (N, B, ...) fp32 on the GPU, targets (B, ...) -> (mse, ssr, crps) floats (dyf_ensemble_metrics)."""
        n = preds.shape[0]
        preds = preds.contiguous().float()
        targets = targets.contiguous().float()
        if preds.shape[1:] != targets.shape:
            raise ValueError(f"predictions.shape[1:] ({tuple(preds.shape[1:])}) != targets.shape ({tuple(targets.shape)})")
        out = (C.c_double * 3)()
        self._check(self._lib.dyf_ensemble_metrics(self._h, preds.data_ptr(), targets.data_ptr(), n, targets.numel(), out,
                                                   self._stream()))
        return out[0], out[1], out[2]

    @staticmethod
    def _segments(preds, targets, what: str):
        """The two input forms of the segment-wise metrics -> (n_members, n_segments, points, member_stride, prediction pointers,
        target pointers, the tensors to keep alive until the launches are enqueued, device)."""
        if torch.is_tensor(preds) != torch.is_tensor(targets):
            raise ValueError("preds and targets must both be lists or both be tensors")
        if torch.is_tensor(preds):
            if preds.dim() < 2 or preds.shape[1:] != targets.shape:
                raise ValueError(f"predictions.shape[1:] ({tuple(preds.shape[1:])}) != targets.shape ({tuple(targets.shape)})")
            preds, targets = preds.contiguous().float(), targets.contiguous().float()
            n, nseg = preds.shape[0], preds.shape[1]
            if n < 1 or nseg < 1 or targets.numel() < 1:
                raise ValueError("empty predictions")
            points = targets.numel() // nseg
            stride = nseg * points
            p_ptrs = [preds.data_ptr() + 4 * s * points for s in range(nseg)]
            t_ptrs = [targets.data_ptr() + 4 * s * points for s in range(nseg)]
            keep = (preds, targets)
        else:
            preds, targets = list(preds), list(targets)
            if len(preds) != len(targets):
                raise ValueError(f"{len(preds)} prediction segments but {len(targets)} target segments")
            nseg = len(preds)
            if nseg < 1:
                raise ValueError("no segments")
            for p, t in zip(preds, targets):
                if p.dim() < 1 or p.shape[1:] != t.shape:
                    raise ValueError(f"predictions.shape[1:] ({tuple(p.shape[1:])}) != targets.shape ({tuple(t.shape)})")
                if p.shape != preds[0].shape:
                    raise ValueError(f"segments differ in shape: {tuple(p.shape)} and {tuple(preds[0].shape)}")
            preds = [p.contiguous().float() for p in preds]
            targets = [t.contiguous().float() for t in targets]
            n, points = preds[0].shape[0], targets[0].numel()
            stride = points
            p_ptrs, t_ptrs = [p.data_ptr() for p in preds], [t.data_ptr() for t in targets]
            keep = (preds, targets)
        dev = keep[0].device if torch.is_tensor(keep[0]) else keep[0][0].device
        if dev.type != "cuda":
            raise ValueError(f"{what} works on GPU tensors (the HIP engine computes them)")
        return n, nseg, points, stride, p_ptrs, t_ptrs, keep, dev

    @staticmethod
    def _accum_ptr(accum: Optional[torch.Tensor], shape: tuple, dev):
        if accum is None:
            return None
        if accum.dtype != torch.float64 or tuple(accum.shape) != shape or not accum.is_contiguous() or accum.device != dev:
            raise ValueError(f"accum must be a contiguous float64 {shape} tensor on {dev}")
        return accum.data_ptr()

    @staticmethod
    def _group_shape(group_shape: Optional[Sequence[int]], points: int):
        """(outer, groups, inner) of one segment's `points`; None pools the segment."""
        if group_shape is None:
            group_shape = (1, 1, points)
        try:
            outer, groups, inner = (operator.index(v) for v in group_shape)
        except (TypeError, ValueError):
            raise ValueError(f"group_shape must be (outer, groups, inner) integers, not {group_shape!r}") from None
        if min(outer, groups, inner) < 1 or outer * groups * inner != points:
            raise ValueError(f"group_shape {(outer, groups, inner)} must be positive with product {points}, a segment's points")
        return outer, groups, inner

    def trajectory_metrics(self, preds, targets, accum: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-segment (mse, ssr, crps) on the device (dyf_trajectory_metrics): the curves of the reference's
        `evaluate_ensemble_prediction(..., mean_over_samples=False)`.  `preds` is a list of T contiguous (N, ...) tensors with
        `targets` the list of the T matching (...) tensors, or one (N, S, ...) tensor with `targets` (S, ...): that form is read in
        place, member stride S * points.  Non-contiguous or non-fp32 inputs are made contiguous fp32 first.  Returns a float64
        device tensor (3, T), rows mse / ssr / crps; `accum` (float64, (3, T), on the device) += it.  No synchronisation: the
        two launches are enqueued on the current stream."""
        n, nseg, points, stride, p_ptrs, t_ptrs, keep, dev = self._segments(preds, targets, "trajectory_metrics")
        accum_ptr = self._accum_ptr(accum, (3, nseg), dev)
        out = torch.empty(3, nseg, dtype=torch.float64, device=dev)
        self._check(self._lib.dyf_trajectory_metrics(self._h, nseg, (C.c_void_p * nseg)(*p_ptrs), (C.c_void_p * nseg)(*t_ptrs), n,
                                                     points, stride, out.data_ptr(), accum_ptr, self._stream()))
        del keep  # held until the launches were enqueued; the caching allocator orders any reuse behind them on this stream
        return out

    def ensemble_size_metrics(self, preds, targets, accum: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The metrics as a function of the ensemble size, one pass on the device (dyf_ensemble_size_metrics): for every segment
        and n = 1..N the mse / ssr / crps of `preds[:n]` (the reference's `evaluate_ensemble_prediction_for_varying_members`)
        and every member's own mse.  Inputs as `trajectory_metrics`: a list of T (N, ...) tensors with T (...) targets, or one
        (N, S, ...) tensor with (S, ...) targets, read in place.  Returns a float64 device tensor (4, T, N), planes mse / ssr /
        crps (entry n - 1 = the first n members) / mse_per_mem; `accum` (float64, (4, T, N), on the device) += it.  At most 256
        members (NotImplementedError beyond).  No synchronisation."""
        n, nseg, points, stride, p_ptrs, t_ptrs, keep, dev = self._segments(preds, targets, "ensemble_size_metrics")
        accum_ptr = self._accum_ptr(accum, (4, nseg, n), dev)
        out = torch.empty(4, nseg, n, dtype=torch.float64, device=dev)
        self._check(self._lib.dyf_ensemble_size_metrics(self._h, nseg, (C.c_void_p * nseg)(*p_ptrs), (C.c_void_p * nseg)(*t_ptrs), n,
                                                        points, stride, out.data_ptr(), accum_ptr, self._stream()))
        del keep  # as in trajectory_metrics
        return out

    def ensemble_scores(self, preds, targets, group_shape: Optional[Sequence[int]] = None,
                        accum: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Five scores per (segment, group), one pass on the device (dyf_ensemble_scores).  Inputs as `trajectory_metrics`: a list
        of T (N, ...) tensors with T (...) targets, or one (N, S, ...) tensor with (S, ...) targets, read in place.  `group_shape`
        = (outer, groups, inner) views one segment's points as row-major (outer, groups, inner), point p in group
        (p // inner) % groups; None pools the segment, (1, 1, points).  Returns a float64 device tensor (5, T, G), planes mse / ssr
        / crps / nll / corr (`dyffusion_amd.metrics.SCORE_ROWS`); `accum` (float64, (5, T, G), on the device) += it.  IEEE
        behaviour as numpy: one member gives a NaN nll, a group with constant ensemble means or targets a NaN corr.  No
        synchronisation."""
        n, nseg, points, stride, p_ptrs, t_ptrs, keep, dev = self._segments(preds, targets, "ensemble_scores")
        outer, groups, inner = self._group_shape(group_shape, points)
        accum_ptr = self._accum_ptr(accum, (5, nseg, groups), dev)
        out = torch.empty(5, nseg, groups, dtype=torch.float64, device=dev)
        self._check(self._lib.dyf_ensemble_scores(self._h, nseg, (C.c_void_p * nseg)(*p_ptrs), (C.c_void_p * nseg)(*t_ptrs), n, points,
                                                  stride, outer, groups, inner, out.data_ptr(), accum_ptr, self._stream()))
        del keep  # as in trajectory_metrics
        return out

    def ensemble_products(self, preds, mean: bool = True, std: bool = True, min: bool = False, max: bool = False,
                          quantiles: Sequence[float] = (), exceed: Sequence[float] = ()):
        """Forecast fields per grid point, reduced over the members on the device (dyf_ensemble_products): the ensemble mean, the
        population standard deviation, min / max, the `quantiles` (probabilities in [0, 1], numpy's "linear" method) and the
        exceedance probabilities P(x > t) for t in `exceed`.  `preds` is one (N, ...) fp32 device tensor -> `fields` (K, ...), or a
        list of T equally shaped (N, ...) tensors, read in place as the segments of one call -> (T, K, ...).  Returns (fields,
        names): fp32 on the device, the K planes in the order of `names`, e.g. ["mean", "std", "q0.05", "q0.5", "q0.95", "gt0.5"].
        Non-contiguous or non-fp32 inputs are made contiguous fp32 first.  A point with a NaN member is NaN in every plane but the
        exceedances.  At most 16 quantiles and 16 thresholds.  No synchronisation: one launch on the current stream."""
        one = torch.is_tensor(preds)
        plist = [preds] if one else list(preds)
        if not plist:
            raise ValueError("no segments")
        for p in plist:
            if not torch.is_tensor(p) or p.dim() < 1 or p.shape[0] < 1 or p.numel() < 1:
                raise ValueError("ensemble_products takes (N, ...) tensors with at least one member and one point")
            if p.shape != plist[0].shape:
                raise ValueError(f"segments differ in shape: {tuple(p.shape)} and {tuple(plist[0].shape)}")
        for p in plist:
            if p.device.type != "cuda":
                raise ValueError("ensemble_products works on GPU tensors (the HIP engine computes them)")
        try:
            qs, ts = [float(q) for q in quantiles], [float(t) for t in exceed]
        except (TypeError, ValueError):
            raise ValueError(f"quantiles and exceed must be sequences of numbers, not {quantiles!r} / {exceed!r}") from None
        if len(qs) > L.MAX_PRODUCT_QUANTILES or len(ts) > L.MAX_PRODUCT_THRESHOLDS:
            raise ValueError(f"at most {L.MAX_PRODUCT_QUANTILES} quantiles and {L.MAX_PRODUCT_THRESHOLDS} thresholds")
        spec = L.ProductsSpec(mean=int(bool(mean)), std=int(bool(std)), min=int(bool(min)), max=int(bool(max)),
                                 n_quantiles=len(qs), n_thresholds=len(ts))
        for k, q in enumerate(qs):
            spec.quantiles[k] = q
        for k, t in enumerate(ts):
            spec.thresholds[k] = t
        names = [m for m, on in (("mean", mean), ("std", std), ("min", min), ("max", max)) if on]
        names += [f"q{q:g}" for q in qs] + [f"gt{t:g}" for t in ts]
        keep = [p.contiguous().float() for p in plist]
        n, nseg, shape = keep[0].shape[0], len(keep), tuple(keep[0].shape[1:])
        points = keep[0].numel() // n
        out = torch.empty(nseg, len(names), *shape, dtype=torch.float32, device=keep[0].device)
        self._check(self._lib.dyf_ensemble_products(self._h, nseg, (C.c_void_p * nseg)(*[p.data_ptr() for p in keep]), n, points, points,
                                                    C.byref(spec), out.data_ptr(), self._stream()))
        del keep  # as in trajectory_metrics
        return (out[0] if one else out), names

    def rank_histogram(self, preds, targets, group_shape: Optional[Sequence[int]] = None,
                       accum: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The rank histogram (Talagrand diagram) per (segment, group) on the device (dyf_rank_histogram).  Inputs and `group_shape`
        as `ensemble_scores`.  Returns a float64 device tensor (T, G, N + 1): bin r counts the points whose target has r members
        below it; a target tied with e members gives 1 / (e + 1) to each of the e + 1 bins it could fall in; points with a NaN
        target or member are left out.  `accum` (float64, (T, G, N + 1), on the device) += it.  At most 1024 members
        (NotImplementedError beyond).  No synchronisation."""
        n, nseg, points, stride, p_ptrs, t_ptrs, keep, dev = self._segments(preds, targets, "rank_histogram")
        outer, groups, inner = self._group_shape(group_shape, points)
        accum_ptr = self._accum_ptr(accum, (nseg, groups, n + 1), dev)
        out = torch.empty(nseg, groups, n + 1, dtype=torch.float64, device=dev)
        self._check(self._lib.dyf_rank_histogram(self._h, nseg, (C.c_void_p * nseg)(*p_ptrs), (C.c_void_p * nseg)(*t_ptrs), n, points,
                                                 stride, outer, groups, inner, out.data_ptr(), accum_ptr, self._stream()))
        del keep  # as in trajectory_metrics
        return out

    def energy_score(self, preds, targets, group_shape: Optional[Sequence[int]] = None, accum: Optional[torch.Tensor] = None,
                     members: bool = False, pairs: bool = False):
        """The energy score per (segment, group) on the device (dyf_energy_score): the CRPS with |.| replaced by the Euclidean norm
        over a whole vector of points.  Inputs and `group_shape` as `ensemble_scores`; a vector is one (outer, group) slab of `inner`
        contiguous points, and a group's values are the means over `outer`: (B, 1, C * H * W) on (B, C, H, W) targets scores whole
        fields, (B, C, H * W) every channel; None is one vector per segment.  Returns a float64 device tensor (4, T, G), planes es /
        es_fair / dist_target / dist_pair (`dyffusion_amd.metrics.ENERGY_ROWS`); `accum` (float64, (4, T, G), on the device) += it.
        With `members` / `pairs` it returns (scores, {"member_dist": (T, G, N) every member's distance to the target, "pair_dist":
        (T, G, N, N) the symmetric member-distance matrix with a zero diagonal}).  One member gives NaN in es_fair and dist_pair.
        At most 256 members (NotImplementedError beyond).  No synchronisation."""
        n, nseg, points, stride, p_ptrs, t_ptrs, keep, dev = self._segments(preds, targets, "energy_score")
        outer, groups, inner = self._group_shape(group_shape, points)
        accum_ptr = self._accum_ptr(accum, (4, nseg, groups), dev)
        out = torch.empty(4, nseg, groups, dtype=torch.float64, device=dev)
        extra = {}
        if members:
            extra["member_dist"] = torch.empty(nseg, groups, n, dtype=torch.float64, device=dev)
        if pairs:
            extra["pair_dist"] = torch.empty(nseg, groups, n, n, dtype=torch.float64, device=dev)
        self._check(self._lib.dyf_energy_score(self._h, nseg, (C.c_void_p * nseg)(*p_ptrs), (C.c_void_p * nseg)(*t_ptrs), n, points,
                                               stride, outer, groups, inner, out.data_ptr(),
                                               extra["member_dist"].data_ptr() if members else None,
                                               extra["pair_dist"].data_ptr() if pairs else None, accum_ptr, self._stream()))
        del keep  # as in trajectory_metrics
        return (out, extra) if extra else out

    SPECTRUM_WINDOWS = {"none": 0, "hann": 1}

    def power_spectrum(self, preds, targets, window: str = "none", accum: Optional[torch.Tensor] = None) -> dict:
        """Radially binned power spectra per (segment, channel) on the device (dyf_power_spectrum).  `preds` is one (N, B, C, H, W)
        tensor with `targets` (B, C, H, W), or lists of such tensors (the segments of one call, all of one shape).  A prediction
        tensor whose members are each contiguous is read in place through its member stride (a slice of a larger stack is not
        copied); anything else is made contiguous fp32 first.  `window` "hann" tapers every field with the separable Hann window.
        Returns {"spread", "mean", "target", "error": float64 device tensors (S, C, n_bins), "total": (S, C, 4) the planes' sums over
        ALL coefficients, the dropped corners included, "n_bins": max(H, W) // 2 + 1, "planes": the (S, C, 4, n_bins + 1) tensor the
        others are views of}; `accum` (float64, the shape of "planes", on the device) += it.  The engine builds and keeps the
        twiddle, taper and shell tables per (H, W) on first use; after that nothing synchronises.  H, W in [2, 1024], at most 256
        members (NotImplementedError beyond)."""
        if window not in self.SPECTRUM_WINDOWS:
            raise ValueError(f"window must be one of {sorted(self.SPECTRUM_WINDOWS)}, not {window!r}")
        if torch.is_tensor(preds) != torch.is_tensor(targets):
            raise ValueError("preds and targets must both be lists or both be tensors")
        plist, tlist = ([preds], [targets]) if torch.is_tensor(preds) else (list(preds), list(targets))
        if len(plist) != len(tlist) or not plist:
            raise ValueError(f"{len(plist)} prediction segments but {len(tlist)} target segments")
        for p, t in zip(plist, tlist):
            if p.dim() != 5 or p.shape[1:] != t.shape:
                raise ValueError(f"predictions must be (N, B, C, H, W) with targets (B, C, H, W), not {tuple(p.shape)} and {tuple(t.shape)}")
            if p.shape != plist[0].shape:
                raise ValueError(f"segments differ in shape: {tuple(p.shape)} and {tuple(plist[0].shape)}")
            if not p.is_cuda or not t.is_cuda:
                raise ValueError("power_spectrum works on GPU tensors (the HIP engine computes them)")
        n, b, c, h, w = plist[0].shape
        if min(n, b, c) < 1:
            raise ValueError("empty predictions")
        points = b * c * h * w

        def in_place(p):  # fp32, every member contiguous, members a fixed stride apart
            return p.dtype == torch.float32 and p[0].is_contiguous() and (n == 1 or p.stride(0) >= points)
        strides = {p.stride(0) if n > 1 else points for p in plist}
        if not (all(in_place(p) for p in plist) and len(strides) == 1):
            plist = [p.contiguous().float() for p in plist]
            strides = {points}
        tlist = [t.contiguous().float() for t in tlist]
        nseg, dev = len(plist), plist[0].device
        n_bins = max(h, w) // 2 + 1
        accum_ptr = self._accum_ptr(accum, (nseg, c, 4, n_bins + 1), dev)
        out = torch.empty(nseg, c, 4, n_bins + 1, dtype=torch.float64, device=dev)
        self._check(self._lib.dyf_power_spectrum(self._h, nseg, (C.c_void_p * nseg)(*[p.data_ptr() for p in plist]),
                                                 (C.c_void_p * nseg)(*[t.data_ptr() for t in tlist]), n, strides.pop(), b, c, h, w,
                                                 self.SPECTRUM_WINDOWS[window], out.data_ptr(), accum_ptr, self._stream()))
        del plist, tlist  # as in trajectory_metrics
        res = {name: out[:, :, i, :n_bins] for i, name in enumerate(("spread", "mean", "target", "error"))}
        res.update(total=out[:, :, :, n_bins], n_bins=n_bins, planes=out)
        return res

    def time_layer_in_rollout(self, layer: int, nb: int):
        """(average ms, launches) of decoder block `layer`'s conv over one eagerly launched rollout of the current plan."""
        ms, cnt = C.c_double(), C.c_int32()
        self._check(self._lib.dyf_time_layer_in_rollout(self._h, layer, nb, self._stream(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def time_kernel_in_rollout(self, kind: int, nb: int):
        """ResNet-UNet pair: (average ms, launches, flops per launch, algorithmic bytes per launch) of kernel class `kind` (0 level-0
        3x3 convs, 1 bottleneck attention core, 2 level-0 GroupNorm chain) over one eagerly launched rollout of the current plan."""
        ms, cnt, fl, by = C.c_double(), C.c_int32(), C.c_double(), C.c_double()
        self._check(self._lib.dyf_time_kernel_in_rollout(self._h, kind, nb, self._stream(), C.byref(ms), C.byref(cnt), C.byref(fl),
                                                         C.byref(by)))
        return ms.value, cnt.value, fl.value, by.value

    def time_named_kernel_in_rollout(self, kernel: str, nb: int):
        """(total ms, launches, total algorithmic bytes) of every launch of `kernel` in one eager rollout (dyffusion_hip_testing.h)."""
        ms, by, n = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
        self._check(self._lib.dyf_time_named_kernel_in_rollout(self._h, kernel.encode(), nb, self._stream(), C.byref(ms), C.byref(n),
                                                               C.byref(by)))
        return ms.value, n.value, by.value

    def op_conv2d(self, x_nhwc_bf16: torch.Tensor, weight: torch.Tensor, stride: int, pad: int,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, act: int = 0,
                  path: int = 1) -> torch.Tensor:
        """Test seam: x (N,H,W,Cin) bf16 on the GPU, weight (Cout,Cin,kh,kw) fp32 (any device) -> (N,Ho,Wo,Cout) bf16."""
        assert x_nhwc_bf16.dtype == torch.bfloat16 and x_nhwc_bf16.is_cuda and x_nhwc_bf16.is_contiguous()
        n, h, w, cin = x_nhwc_bf16.shape
        cout, _, kh, kw = weight.shape
        wh = np.ascontiguousarray(weight.detach().to("cpu", torch.float32).numpy())
        ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
        y = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=x_nhwc_bf16.device)
        if scale is not None:
            scale, shift = _f32c(scale, "scale"), _f32c(shift, "shift")
        self._check(self._lib.dyf_op_conv2d(self._h, x_nhwc_bf16.data_ptr(), wh.ctypes.data, n, h, w, cin, cout, kh, kw,
                                            stride, pad, None if scale is None else scale.data_ptr(),
                                            None if shift is None else shift.data_ptr(), act, path, y.data_ptr(),
                                            self._stream()))
        return y

    def op_conv2d_ex(self, x: torch.Tensor, weight: torch.Tensor, stride: int, pad: int, scale: Optional[torch.Tensor] = None,
                     shift: Optional[torch.Tensor] = None, act: int = 0, path: int = 1, *, x1: Optional[torch.Tensor] = None,
                     residual: Optional[torch.Tensor] = None, out16: bool = True, out_f32: bool = False, coef_div: int = 0,
                     n_sel: int = 0, mask: Optional[torch.Tensor] = None, p: float = 0.0, rng_site: Optional[int] = None,
                     rng_row_offset: int = 0, rng_forward: int = 0):
        """Test seam (dyf_op_conv2d_ex): op_conv2d over the rest of the conv argument block.  x (N,H,W,c0) and x1 (N,H,W,c1) in the
        engine's 16-bit dtype, weight (Cout, c0 + c1, kh, kw); residual 16-bit of the output's shape; scale / shift of
        ceil(N / coef_div) rows; mask: uint8 NHWC keep mask (dropout mode 2); rng_site: dropout mode 1 from the engine's generator at
        that site, forward index and global row offset; act 0..4.  Returns the 16-bit output, the fp32 output, or (16-bit, fp32)."""
        dt = self.torch_dtype
        assert x.dtype == dt and x.is_cuda and x.is_contiguous() and (out16 or out_f32)
        n, h, w, c0 = x.shape
        c1 = 0
        if x1 is not None:
            assert x1.dtype == dt and x1.is_cuda and x1.is_contiguous() and x1.shape[:3] == x.shape[:3]
            c1 = x1.shape[3]
        cout, cin, kh, kw = weight.shape
        assert cin == c0 + c1 and not (mask is not None and rng_site is not None)
        wh = np.ascontiguousarray(weight.detach().to("cpu", torch.float32).numpy())
        ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
        y = torch.empty((n, ho, wo, cout), dtype=dt, device=x.device) if out16 else None
        y32 = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device) if out_f32 else None
        if scale is not None:
            rows = -(-n // coef_div) if coef_div > 1 else n
            scale, shift = _f32c(scale, "scale"), _f32c(shift, "shift")
            assert tuple(scale.shape) == (rows, cout) and tuple(shift.shape) == (rows, cout)
        ex = L.ConvEx()
        if x1 is not None:
            ex.x1_dev, ex.c1 = x1.data_ptr(), c1
        if residual is not None:
            assert residual.dtype == dt and residual.is_cuda and residual.is_contiguous() and tuple(residual.shape) == (n, ho, wo, cout)
            ex.residual_dev = residual.data_ptr()
        if y32 is not None:
            ex.y_f32_dev = y32.data_ptr()
        ex.coef_div, ex.n_sel, ex.drop_p = int(coef_div), int(n_sel), float(p)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and tuple(mask.shape) == (n, ho, wo, cout)
            ex.drop_mode, ex.mask_dev = 2, mask.data_ptr()
        elif rng_site is not None:
            ex.drop_mode, ex.drop_site, ex.drop_row_offset, ex.drop_forward = 1, int(rng_site), int(rng_row_offset), int(rng_forward)
        self._check(self._lib.dyf_op_conv2d_ex(self._h, x.data_ptr(), wh.ctypes.data, n, h, w, c0, cout, kh, kw, stride, pad,
                                               None if scale is None else scale.data_ptr(),
                                               None if shift is None else shift.data_ptr(), act, path,
                                               None if y is None else y.data_ptr(), C.byref(ex), self._stream()))
        return (y, y32) if out16 and out_f32 else y if out16 else y32

    def op_conv_gn(self, x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, gamma: Optional[torch.Tensor] = None,
                   beta: Optional[torch.Tensor] = None, *, groups: int = 0, want: str = "fused", x1: Optional[torch.Tensor] = None,
                   residual: Optional[torch.Tensor] = None, film_a: Optional[torch.Tensor] = None, film_c: Optional[torch.Tensor] = None,
                   coef_div: int = 0, n_sel: int = 0, invariant: bool = False, act: int = 3, gran: Optional[torch.Tensor] = None,
                   epoch: Optional[torch.Tensor] = None, conv_tag: int = 0, max_slots: int = 0, new_forward: bool = False,
                   part: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                   p: float = 0.0, rng_site: Optional[int] = None, rng_row_offset: int = 0, rng_forward: int = 0):
        """Test seam (dyf_op_conv_gn): one 3x3 conv in front of a GroupNorm through the entry point a ResnetBlock calls it by.
        want="fused": launch_conv_gn_fused -- conv + bias -> GroupNorm(groups, gamma, beta) -> FiLM rows (film_a, film_c: fp32 device
        (ceil(N / coef_div), stride >= cout)) -> SiLU -> Dropout -> + residual.  `gran` (int64 device, N * max_slots * (cout / 8) * 2
        words) and `epoch` (int32 device, one word) are the CALLER's: zeroed once, kept across calls; a (forward, conv_tag) pair must
        not repeat on one buffer, new_forward starts the next forward.  want="stats": launch_conv_stats -- y = conv + bias and the
        per-octet partials in `part` (fp32 device (N, slots, cout / 8, 2), sized for the largest slot count).  x / x1 / residual: 16-bit
        NHWC; weight (cout, c0 + c1, 3, 3) as it is (not standardised here); `y`: an output tensor to write into (else a new one).
        Returns (y, info) with info = dict(fused, slots, bm, slow_sweep); fused == 0: nothing was launched and y is untouched."""
        dt = self.torch_dtype
        if want not in ("fused", "stats"):
            raise ValueError(f"want: 'fused' or 'stats', not {want!r}")
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 4:
            raise ValueError(f"x: a contiguous NHWC device tensor of dtype {dt}")
        n, h, w, c0 = x.shape
        c1 = 0
        desc, tens, res = L.ConvGn(), L.ConvGnTensors(), L.ConvGnResult()
        if x1 is not None:
            if x1.dtype != dt or not x1.is_cuda or not x1.is_contiguous() or x1.shape[:3] != x.shape[:3]:
                raise ValueError("x1: a contiguous 16-bit device tensor over x's (N, H, W)")
            c1 = x1.shape[3]
            tens.x1 = x1.data_ptr()
        cout = weight.shape[0]
        if tuple(weight.shape) != (cout, c0 + c1, 3, 3):
            raise ValueError(f"weight must be ({cout}, {c0 + c1}, 3, 3)")
        host = lambda t_: None if t_ is None else np.ascontiguousarray(t_.detach().to("cpu", torch.float32).numpy()).reshape(-1)
        wh, bh, gh, beh = host(weight), host(bias), host(gamma), host(beta)
        if any(v is not None and v.size != cout for v in (bh, gh, beh)) or bh is None:
            raise ValueError(f"bias / gamma / beta hold {cout} values")
        if y is None:
            y = torch.empty((n, h, w, cout), dtype=dt, device=x.device)
        elif y.dtype != dt or not y.is_cuda or not y.is_contiguous() or tuple(y.shape) != (n, h, w, cout):
            raise ValueError("y: a contiguous 16-bit device tensor (N, H, W, cout)")
        desc.n, desc.h, desc.w, desc.c0, desc.c1, desc.cout = n, h, w, c0, c1, cout
        desc.want, desc.n_sel = (0 if want == "fused" else 1), int(n_sel)
        tens.x0, tens.y = x.data_ptr(), y.data_ptr()
        keep = []  # tensors the call reads: alive until it returns
        if want == "fused":
            desc.groups, desc.act, desc.coef_div, desc.invariant = int(groups), int(act), int(coef_div), int(bool(invariant))
            desc.conv_tag, desc.max_slots, desc.new_forward = int(conv_tag), int(max_slots), int(bool(new_forward))
            if gran is None or epoch is None or gran.dtype != torch.int64 or epoch.dtype != torch.int32 or not gran.is_cuda or not epoch.is_cuda \
                    or not gran.is_contiguous() or epoch.numel() < 1:
                raise ValueError("gran: int64 device words, epoch: an int32 device word, both owned by the caller")
            tens.gran, tens.epoch, tens.gran_granules = gran.data_ptr(), epoch.data_ptr(), gran.numel()
            if (film_a is None) != (film_c is None):
                raise ValueError("film_a and film_c go together")
            if film_a is not None:
                film_a, film_c = _f32c(film_a, "film_a"), _f32c(film_c, "film_c")
                rows = -(-n // coef_div) if coef_div > 1 else n
                if film_a.dim() != 2 or film_a.shape != film_c.shape or film_a.shape[0] != rows:
                    raise ValueError(f"film rows must be ({rows}, stride) fp32")
                desc.film_stride = film_a.shape[1]
                tens.film_a, tens.film_c = film_a.data_ptr(), film_c.data_ptr()
                keep += [film_a, film_c]
            if residual is not None:
                if residual.dtype != dt or not residual.is_cuda or not residual.is_contiguous() or tuple(residual.shape) != (n, h, w, cout):
                    raise ValueError("residual: a contiguous 16-bit device tensor of the output's shape")
                tens.residual = residual.data_ptr()
            desc.drop_p = float(p)
            if mask is not None and rng_site is not None:
                raise ValueError("mask or rng_site, not both")
            if mask is not None:
                if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != (n, h, w, cout):
                    raise ValueError("mask: a contiguous uint8 device tensor of the output's shape")
                desc.drop_mode, tens.mask = 2, mask.data_ptr()
            elif rng_site is not None:
                desc.drop_mode, desc.drop_site, desc.drop_row_offset, desc.drop_forward = 1, int(rng_site), int(rng_row_offset), int(rng_forward)
        else:
            if part is None or part.dtype != torch.float32 or not part.is_cuda or not part.is_contiguous():
                raise ValueError("want='stats' needs part: a contiguous fp32 device tensor")
            if any(v is not None for v in (gamma, beta, residual, film_a, film_c, gran, epoch, mask, rng_site)) or groups or coef_div or invariant \
                    or conv_tag or max_slots or new_forward or p:
                raise ValueError("want='stats' takes the sources, weight, bias, n_sel, part and y")
            tens.part, tens.part_floats = part.data_ptr(), part.numel()
        fp = lambda a_: None if a_ is None else a_.ctypes.data
        self._check(self._lib.dyf_op_conv_gn(self._h, C.byref(desc), C.byref(tens), fp(wh), fp(bh), fp(gh), fp(beh), C.byref(res), self._stream()))
        del keep
        return y, dict(fused=res.fused, slots=res.slots, bm=res.bm, slow_sweep=res.slow_sweep)

    def criterion(self, pred: torch.Tensor, target: torch.Tensor, kind: str = "l1") -> float:
        """Mean L1 / MSE / smooth-L1 between two fp32 device tensors (get_loss, src/utilities/utils.py:201-212)."""
        name = kind.lower().strip().replace("-", "_")
        code = 0 if name in ("l1", "mae", "mean_absolute_error") else 1 if name in ("l2", "mse", "mean_squared_error") else \
            2 if name in ("smoothl1", "smooth") else None
        if code is None:
            raise ValueError(f"Unknown loss function {kind}")
        pred, target = _f32c(pred, "pred"), _f32c(target, "target")
        # the kernel reads 16 bytes per lane: a contiguous view at an odd element offset is copied to an aligned buffer
        if pred.data_ptr() % 16:
            pred = pred.clone()
        if target.data_ptr() % 16:
            target = target.clone()
        if pred.shape != target.shape:
            raise ValueError(f"shape mismatch: {tuple(pred.shape)} vs {tuple(target.shape)}")
        out = C.c_double(0.0)
        self._sync_train_deterministic()
        self._check(self._lib.dyf_criterion(self._h, pred.data_ptr(), target.data_ptr(), pred.numel(), code, C.byref(out),
                                            self._stream()))
        return out.value

    # ------------------------------------------------------------------ training step (every arch, fp32 tensors)
    def train_forward(self, net: int, slot: int, inputs: torch.Tensor, time: Optional[torch.Tensor],
                      condition: Optional[torch.Tensor], batch_stats: bool, dropout: bool) -> torch.Tensor:
        """One RECORDED forward (tape `slot`, 0..3): batch-statistics BatchNorm iff `batch_stats`, Dropout iff `dropout`."""
        inputs = _f32c(inputs, "inputs")
        nb = inputs.shape[0]
        ncfg = self.cfg.net[net]
        if inputs.dim() != 4 or inputs.shape[1] != ncfg.in_channels or tuple(inputs.shape[2:]) != (self.height, self.width):
            raise ValueError(f"inputs must be (NB, {ncfg.in_channels}, {self.height}, {self.width}), got {tuple(inputs.shape)}")
        if condition is not None:
            condition = _f32c(condition, "condition")
            if tuple(condition.shape) != (nb, ncfg.cond_channels, self.height, self.width):
                raise ValueError(f"condition has shape {tuple(condition.shape)}")
        if time is not None:
            time = _f32c(time.reshape(-1), "time")
        out = torch.empty((nb, ncfg.out_channels, self.height, self.width), dtype=torch.float32, device=inputs.device)
        flags = (L.TRAIN_BATCH_STATS if batch_stats else 0) | (L.TRAIN_DROPOUT if dropout else 0)
        self._tape_net[slot] = net
        self._tape_nb[slot] = nb
        self._sync_train_deterministic()
        self._check(self._lib.dyf_train_forward(self._h, net, slot, inputs.data_ptr(), None if time is None else time.data_ptr(),
                                                None if condition is None else condition.data_ptr(), out.data_ptr(), nb, flags,
                                                self._stream()))
        return out

    def train_backward(self, slot: int, dout: torch.Tensor, want_dinputs: bool, param_grads: bool) -> Optional[torch.Tensor]:
        dout = _f32c(dout, "dout")
        if slot not in self._tape_net:
            raise EngineError(f"tape slot {slot} holds no recorded forward")
        net = self._tape_net[slot]
        want = (self._tape_nb[slot], self.cfg.net[net].out_channels, self.height, self.width)
        if tuple(dout.shape) != want:  # the C ABI reads / writes nb rows from raw pointers
            raise ValueError(f"dout must have the recorded forward's output shape {want}, got {tuple(dout.shape)}")
        din = None
        if want_dinputs:
            din = torch.empty((dout.shape[0], self.cfg.net[net].in_channels, self.height, self.width), dtype=torch.float32,
                              device=dout.device)
        self._check(self._lib.dyf_train_backward(self._h, slot, dout.data_ptr(), None if din is None else din.data_ptr(),
                                                 int(param_grads), self._stream()))
        return din

    def train_set_precision(self, precision) -> None:
        """Operand precision of the training convolutions (dyf_train_set_precision; the reference's Lightning `trainer.precision`):
        32 / "32" / "32-true" = fp32 operands (default), 16 / "16-mixed" / "bf16-mixed" = operands rounded to bf16 while staged (fp32
        tensors, master weights and accumulation) -- bf16 on fp16 engines too: the reference's precision=16 is fp16 + GradScaler, and
        fp16 gradient operands without a loss scale underflow at real batch sizes (`parse_train_precision`); 48 / "bf16x3" = fp32-grade convs on the 16-bit matrix cores: the convs the 16-bit
        dispatch takes split each operand into a (hi, lo) pair of bf16 and sum three MFMA terms, everything else exactly as under 32
        (SimpleConvNet keeps fp32 operands); None = not set (fp32)."""
        self._check(self._lib.dyf_train_set_precision(self._h, parse_train_precision(precision)))

    @property
    def train_precision(self) -> int:
        return int(self._lib.dyf_train_precision(self._h))

    def train_set_deterministic(self, value) -> None:
        """Deterministic training mode (dyf_train_set_deterministic; the reference's `trainer.deterministic`): True = no sum of the
        recorded forward, its backward or the criterion is merged with atomics, so identical steps are bitwise equal; False = the
        default atomic forms; None = follow `torch.are_deterministic_algorithms_enabled()`, read at every training forward
        (`resolve_train_deterministic`).  Sampling never reads it."""
        resolve_train_deterministic(value)
        self._train_deterministic = value
        self._sync_train_deterministic()

    def _sync_train_deterministic(self) -> None:
        want = int(resolve_train_deterministic(self._train_deterministic))
        if int(self._lib.dyf_train_deterministic(self._h)) != want:
            self._check(self._lib.dyf_train_set_deterministic(self._h, want))

    @property
    def train_deterministic(self) -> bool:
        self._sync_train_deterministic()
        return bool(self._lib.dyf_train_deterministic(self._h))

    def train_zero_grads(self, net: int):
        self._check(self._lib.dyf_train_zero_grads(self._h, net))

    def train_export(self, net: int, names_shapes: Dict[str, tuple], device: Optional[torch.device] = None) -> Dict[str, torch.Tensor]:
        """Gradients (or updated BatchNorm running statistics) by state_dict name -> fp32 tensors: on the CPU, or -- `device` =
        this engine's GPU -- written there directly (device-to-device, dyf_train_export_dev)."""
        names = list(names_shapes)
        if device is not None and device.type == "cuda":
            outs = [torch.empty(names_shapes[k], dtype=torch.float32, device=device) for k in names]
            cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
            cp = (C.c_void_p * len(names))(*[o.data_ptr() for o in outs])
            torch.cuda.current_stream().synchronize()
            self._check(self._lib.dyf_train_export_dev(self._h, net, len(names), cn, cp))
            return dict(zip(names, outs))
        bufs = [np.empty(names_shapes[k], dtype=np.float32) for k in names]
        cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
        cp = (C.c_void_p * len(names))(*[b.ctypes.data for b in bufs])
        self._check(self._lib.dyf_train_export(self._h, net, len(names), cn, cp))
        return {k: torch.from_numpy(b) for k, b in zip(names, bufs)}

    # ------------------------------------------------------------------ engine-resident optimizer (csrc/train_optim.hip)
    def optim_create(self, net: int, *, beta1: float, beta2: float, eps: float, weight_decay: float, max_grad_norm: float, ema: bool):
        """dyf_optim_create: AdamW state (zero) and, with `ema`, a shadow copy of the current weights for network `net`."""
        cfg = L.OptimConfig(float(beta1), float(beta2), float(eps), float(weight_decay), float(max_grad_norm), int(bool(ema)))
        self._check(self._lib.dyf_optim_create(self._h, net, C.byref(cfg)))

    def optim_destroy(self, net: int):
        self._check(self._lib.dyf_optim_destroy(self._h, net))

    def optim_step(self, net: int, lr: float, ema_decay_now: float = 0.0):
        """dyf_optim_step: two launches on the current stream.  Nothing launched here is waited for; the call first reads the
        PREVIOUS step's outcome (its status copy was queued behind that step), so the host runs at most one step ahead."""
        self._check(self._lib.dyf_optim_step(self._h, net, float(lr), float(ema_decay_now), self._stream()))

    def optim_last(self, net: int):
        """(gradient norm before clipping, skipped) of the most recent step; waits for that step."""
        norm, skipped = C.c_double(0.0), C.c_int32(0)
        self._check(self._lib.dyf_optim_last(self._h, net, C.byref(norm), C.byref(skipped)))
        return norm.value, bool(skipped.value)

    def optim_get_step(self, net: int) -> int:
        n = C.c_int64(0)
        self._check(self._lib.dyf_optim_get_step(self._h, net, C.byref(n)))
        return int(n.value)

    def optim_set_step(self, net: int, step: int):
        self._check(self._lib.dyf_optim_set_step(self._h, net, C.c_int64(int(step))))

    def optim_export(self, net: int, kind: int, names_shapes: Dict[str, tuple], device: Optional[torch.device] = None) -> Dict[str, torch.Tensor]:
        """dyf_optim_export: tensors of `kind` (L.OPTIM_*) by state_dict name in PyTorch layouts -> fp32 tensors on the CPU, or --
        `device` = this engine's GPU -- written there device-to-device."""
        names = list(names_shapes)
        if not names:
            return {}
        cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
        if device is not None and torch.device(device).type == "cuda":
            outs = [torch.empty(names_shapes[k], dtype=torch.float32, device=device) for k in names]
            cp = (C.c_void_p * len(names))(*[o.data_ptr() for o in outs])
            torch.cuda.current_stream().synchronize()
            self._check(self._lib.dyf_optim_export(self._h, net, int(kind), len(names), cn, cp, 1))
            return dict(zip(names, outs))
        bufs = [np.empty(names_shapes[k], dtype=np.float32) for k in names]
        cp = (C.c_void_p * len(names))(*[b.ctypes.data for b in bufs])
        self._check(self._lib.dyf_optim_export(self._h, net, int(kind), len(names), cn, cp, 0))
        return {k: torch.from_numpy(b) for k, b in zip(names, bufs)}

    def optim_import(self, net: int, kind: int, tensors: Dict[str, torch.Tensor]):
        """dyf_optim_import: the reverse of `optim_export`; tensors that all live on this engine's GPU are read in place.  Shapes are
        the caller's responsibility as far as the element count goes: each tensor must have its parameter's number of elements."""
        names = list(tensors)
        if not names:
            return
        cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
        vals = [tensors[k].detach() for k in names]
        if all(v.is_cuda and v.device.index == self.device for v in vals):
            keep = [v.to(torch.float32).contiguous() for v in vals]
            cp = (C.c_void_p * len(names))(*[t.data_ptr() for t in keep])
            torch.cuda.current_stream().synchronize()
            self._check(self._lib.dyf_optim_import(self._h, net, int(kind), len(names), cn, cp, 1))
            return
        keep = [np.ascontiguousarray(v.to("cpu", torch.float32).numpy()) for v in vals]
        cp = (C.c_void_p * len(names))(*[a.ctypes.data for a in keep])
        self._check(self._lib.dyf_optim_import(self._h, net, int(kind), len(names), cn, cp, 0))

    def optim_swap_ema(self, net: int):
        """dyf_optim_swap_ema: weights <-> EMA shadow in place (both conv layouts), on the current stream."""
        self._check(self._lib.dyf_optim_swap_ema(self._h, net, self._stream()))

    def criterion_grad(self, pred: torch.Tensor, target: torch.Tensor, kind: str, scale: float) -> torch.Tensor:
        name = kind.lower().strip().replace("-", "_")
        code = 0 if name in ("l1", "mae", "mean_absolute_error") else 1 if name in ("l2", "mse", "mean_squared_error") else 2
        pred, target = _f32c(pred, "pred"), _f32c(target, "target")
        d = torch.empty_like(pred)
        self._check(self._lib.dyf_criterion_grad(self._h, pred.data_ptr(), target.data_ptr(), pred.numel(), code, float(scale),
                                                 d.data_ptr(), self._stream()))
        return d

    def train_conv_check(self, kind: int, n: int, h: int, w: int, cin: int, cout: int, k: int, s: int, p: int, seed: int = 1):
        """Test seam: one training convolution (0 forward, 1 dgrad, 2 wgrad on the matrix-core launchers; 3 wgrad, 4 forward through the
        step's dispatchers) vs the plain VALU kernel.
        Returns (relative max error with split-K workspace, without, whether the matrix-core form took the shape)."""
        out = (C.c_float * 3)()
        self._check(self._lib.dyf_train_conv_check(self._h, kind, n, h, w, cin, cout, k, s, p, C.c_uint32(seed), out))
        return float(out[0]), float(out[1]), bool(out[2])

    def op_linear_attention(self, qkv_bf16: torch.Tensor) -> torch.Tensor:
        """Test seam: LinearAttention core.  qkv (N,HW,384) bf16 (to_qkv output, 4 heads x 32) -> (N,HW,128) bf16."""
        assert qkv_bf16.dtype == self.torch_dtype and qkv_bf16.is_cuda and qkv_bf16.is_contiguous()
        n, hw, c3 = qkv_bf16.shape
        assert c3 == 384
        y = torch.empty((n, hw, 128), dtype=qkv_bf16.dtype, device=qkv_bf16.device)
        self._check(self._lib.dyf_op_linear_attention(self._h, qkv_bf16.data_ptr(), n, hw, y.data_ptr(), self._stream()))
        return y

    def op_linear_attention_fused(self, xn: torch.Tensor, xres: torch.Tensor, wqkv: torch.Tensor, wout: torch.Tensor,
                                  bout: torch.Tensor) -> torch.Tensor:
        """Test seam: the fused LinearAttention block (to_qkv + core + to_out + bias + residual).  xn, xres (N,HW,C) in the engine's
        16-bit dtype on the device, C in {64, 128}; wqkv (384,C), wout (C,128), bout (C) fp32 on the host -> (N,HW,C)."""
        assert xn.dtype == self.torch_dtype and xn.is_cuda and xn.is_contiguous() and xres.shape == xn.shape and xres.is_contiguous()
        n, hw, c = xn.shape
        wq, wo, bo = (t.detach().to(torch.float32).cpu().contiguous() for t in (wqkv, wout, bout))
        assert wq.shape == (384, c) and wo.shape == (c, 128) and bo.shape == (c,)
        y = torch.empty_like(xn)
        self._check(self._lib.dyf_op_linear_attention_fused(self._h, xn.data_ptr(), xres.data_ptr(), n, hw, c, wq.data_ptr(),
                                                            wo.data_ptr(), bo.data_ptr(), y.data_ptr(), self._stream()))
        return y

    @property
    def torch_dtype(self) -> torch.dtype:
        return torch.float16 if L.DTYPES[L.storage_dtype(self.dtype)] else torch.bfloat16

    def op_attention(self, qkv: torch.Tensor, p_drop: float = 0.0, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Test seam: Attention core.  qkv (N,HW,384) in the engine's 16-bit dtype (to_qkv output) -> (N,HW,128); p_drop > 0:
        dropout on the probabilities from the engine's generator, in the engine's `attention_dropout` mode -- or, with `mask`
        (N,4,HW,HW) uint8, on the caller's keep mask (dyf_op_attention_mask: survivors scaled by 1 / (1 - p_drop))."""
        assert qkv.dtype == self.torch_dtype and qkv.is_cuda and qkv.is_contiguous() and qkv.shape[2] == 384
        n, hw, _ = qkv.shape
        y = torch.empty((n, hw, 128), dtype=qkv.dtype, device=qkv.device)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and tuple(mask.shape) == (n, 4, hw, hw)
            self._check(self._lib.dyf_op_attention_mask(self._h, qkv.data_ptr(), n, hw, float(p_drop), mask.data_ptr(), y.data_ptr(), self._stream()))
            return y
        self._check(self._lib.dyf_op_attention_dropout(self._h, qkv.data_ptr(), n, hw, float(p_drop), y.data_ptr(), self._stream()))
        return y

    def op_attention_f32(self, qkv: torch.Tensor, p_drop: float = 0.0, mask: Optional[torch.Tensor] = None, form: int = 1) -> torch.Tensor:
        """Test seam: the fp32 Attention core.  qkv (N,HW,384) fp32 -> (N,HW,128) fp32.  form 0: the kernel that keeps its
        probabilities (HW <= 4096), form 1: the streaming kernel.  p_drop > 0: dropout on the probabilities, from `mask`
        (N,4,HW,HW) uint8 if given, else from the engine's generator."""
        assert qkv.dtype == torch.float32 and qkv.is_cuda and qkv.is_contiguous() and qkv.shape[2] == 384
        n, hw, _ = qkv.shape
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and tuple(mask.shape) == (n, 4, hw, hw)
        y = torch.empty((n, hw, 128), dtype=torch.float32, device=qkv.device)
        self._check(self._lib.dyf_op_attention_f32(self._h, qkv.data_ptr(), n, hw, float(p_drop), None if mask is None else mask.data_ptr(),
                                                   int(form), y.data_ptr(), self._stream()))
        return y

    def op_train(self, op: str, inputs, params=(), dout: Optional[torch.Tensor] = None, grads_in=None, *, k: int = 0, stride: int = 0,
                 pad: int = 0, groups: int = 0, p: float = 0.0, ws: bool = False, pre: bool = False, act: str = "silu", running: bool = False,
                 mask: Optional[torch.Tensor] = None, size=None, nearest: bool = False, skip_grad: Optional[torch.Tensor] = None,
                 residual: Optional[torch.Tensor] = None, sample: bool = False) -> Dict[str, object]:
        """Test seam (dyf_op_train_f32): ONE recorded op of the training step (either backbone) and its adjoint, through the training
        step's own launch code.  `inputs`: fp32 tensors on the device, activations NHWC (nb, h, w, c) -- rows (nb, c) for "linear", times (nb,)
        for "learned_sinu"; "add" with one input is add(a, a).  `params`: fp32 tensors in PyTorch layouts, in the header's order (conv:
        weight (c2, c, k, k) [, bias]; gn_act: weight, bias -- a second input is the FiLM (nb, 2c); layernorm: g; linear: weight (c2, c),
        bias; learned_sinu: weights).  `dout`: gradient of the output (its shape).  `grads_in`: what the parameter-gradient buffers hold
        before the op runs (default zeros): the kernels accumulate.  Returns {"y", "dinputs": [...], "dparams": [...]} (dparams on the
        CPU).  p > 0 draws from the engine's generator: a new forward, site 0, rows row offset .. + nb - 1.
        unet_simple's ops: "norm_act" (gn_act's inputs; params weight, bias and -- groups = 0, BatchNorm2d -- running_mean, running_var, whose
        "dparams" entries return the UPDATED statistics; `running`: normalise by them; `act` "silu" | "leaky" | "relu"; `mask`: a uint8 keep
        mask (nb, h, w, c) instead of the generator -- forward only, "dinputs" is None), "up2_bilinear" (one source, or two standing for
        their concatenation; `skip_grad`: the gradient the second source already has), "resize" (`size` = (oh, ow), which travels in the
        descriptor's k and stride fields; `nearest`), "convt"
        (ConvTranspose2d(c, c2, 4, 2, 1): weight (c, c2, 4, 4), bias).
        "attention_stream": "attention" in the streaming form a recorded forward takes past 4096 tokens, at any h * w <= 32 767.
        SimpleConvNet's block: "norm_act" with `act` "gelu" and `residual` (nb, h, w, c), added behind activation and dropout in the same
        launch; its gradient is the last entry of "dinputs".
        `sample` ("conv" only): the forward alone, launched the way a sampling forward launches it -- operands from `sample_precision`,
        the forms only sampling takes; "dinputs" and "dparams" are None."""
        if sample and op != "conv":
            raise NotImplementedError("sample=True: conv only")
        ins = [_f32c(t, "input") for t in inputs]
        n_plain = len(ins)  # inputs without the residual, which follows them in the pointer array
        if residual is not None:
            if op != "norm_act":
                raise ValueError("residual: norm_act only")
            ins.append(_f32c(residual, "residual"))
        x = ins[0]
        nb = x.shape[0]
        if op in ("linear", "learned_sinu"):
            h = w = 1
            c = x.shape[1] if op == "linear" else params[0].numel()
        else:
            if x.dim() != 4:
                raise ValueError(f"{op}: inputs are NHWC (nb, h, w, c), got {tuple(x.shape)}")
            _, h, w, c = x.shape
        c2, flags = 0, 0
        ps = [t.detach().to("cpu", torch.float32).contiguous() for t in params]
        if op == "conv":
            c2 = ps[0].shape[0]
            if tuple(ps[0].shape) != (c2, c, k, k):
                raise ValueError(f"conv weight must be (c2, {c}, {k}, {k}), got {tuple(ps[0].shape)}")
            flags = (L.TOP_WS if ws else 0) | (L.TOP_BIAS if len(ps) > 1 else 0) | (L.TOP_SAMPLE if sample else 0)
            out_shape = (nb, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1, c2)
        elif op == "gn_act":
            flags = L.TOP_FILM if len(ins) > 1 else 0
            out_shape = tuple(x.shape)
        elif op in ("linattn", "attention", "attention_stream"):
            out_shape = (nb, h, w, 128)
        elif op == "linear":
            c2, flags = ps[0].shape[0], (L.TOP_PRE if pre else 0)
            out_shape = (nb, c2)
        elif op == "learned_sinu":
            out_shape = (nb, 2 * c + 1)
        elif op == "add":
            flags = L.TOP_SAME if len(ins) == 1 else 0
            out_shape = tuple(x.shape)
        elif op == "cat":
            c2 = ins[1].shape[3]
            out_shape = (nb, h, w, c + c2)
        elif op == "up2_nearest":
            out_shape = (nb, 2 * h, 2 * w, c)
        elif op in ("layernorm", "dropout", "gelu"):
            out_shape = tuple(x.shape)
        elif op == "norm_act":
            flags = ((L.TOP_FILM if n_plain > 1 else 0) | (L.TOP_RUNNING if running else 0) | (L.TOP_MASK if mask is not None else 0)
                     | (L.TOP_RESIDUAL if residual is not None else 0)
                     | {"silu": 0, "leaky": L.TOP_LEAKY, "relu": L.TOP_RELU, "gelu": L.TOP_ACT_GELU}[act])
            out_shape = tuple(x.shape)
        elif op == "up2_bilinear":
            c2 = ins[1].shape[3] if len(ins) > 1 else 0
            flags = L.TOP_GRAD_IN if skip_grad is not None else 0
            out_shape = (nb, 2 * h, 2 * w, c + c2)
        elif op == "resize":
            k, stride = int(size[0]), int(size[1])  # the descriptor has no size fields: a resize carries (oh, ow) in k and stride
            flags = L.TOP_NEAREST if nearest else 0
            out_shape = (nb, k, stride, c)
        elif op == "convt":
            c2 = ps[0].shape[1]
            out_shape = (nb, 2 * h, 2 * w, c2)
        else:
            raise ValueError(f"unknown training op {op!r}")
        want_in = {"gn_act": (1, 2), "norm_act": (1, 2), "up2_bilinear": (1, 2), "add": (1, 2), "cat": (2, 2)}.get(op, (1, 1))
        want_p = {"conv": (1, 2), "gn_act": (2, 2), "norm_act": (2, 2) if groups else (4, 4), "convt": (2, 2), "layernorm": (1, 1), "linear": (2, 2),
                  "learned_sinu": (1, 1)}.get(op, (0, 0))
        if not (want_in[0] <= n_plain <= want_in[1]) or not (want_p[0] <= len(ps) <= want_p[1]):
            raise ValueError(f"{op}: {len(ins)} inputs and {len(ps)} parameters")
        expect = {"conv": [(nb, h, w, c)], "gn_act": [(nb, h, w, c), (nb, 2 * c)], "norm_act": [(nb, h, w, c), (nb, 2 * c)],
                  "up2_bilinear": [(nb, h, w, c), (nb, h, w, c2)], "add": [tuple(x.shape)] * 2, "cat": [(nb, h, w, c), (nb, h, w, c2)],
                  "linear": [(nb, c)], "learned_sinu": [(nb,)]}.get(op, [tuple(x.shape)])
        if residual is not None:
            expect = expect[:n_plain] + [(nb, h, w, c)]
        for t, sh in zip(ins, expect):
            if tuple(t.shape) != sh:
                raise ValueError(f"{op}: an input has shape {tuple(t.shape)}, expected {sh}")
        pshape = {"conv": [(c2, c, k, k), (c2,)], "gn_act": [(c,), (c,)], "norm_act": [(c,)] * 4, "convt": [(c, c2, 4, 4), (c2,)], "layernorm": [(1, c, 1, 1)], "linear": [(c2, c), (c2,)],
                  "learned_sinu": [(c,)]}.get(op, [])
        for t, sh in zip(ps, pshape):
            if t.numel() != int(np.prod(sh)):
                raise ValueError(f"{op}: a parameter has shape {tuple(t.shape)}, expected {sh}")
        if (op in ("linattn", "attention", "attention_stream")) and c != 384:
            raise ValueError("the attention cores take qkv of 384 channels")
        dout = _f32c(dout, "dout")
        if tuple(dout.shape) != out_shape:  # the C ABI reads / writes raw pointers
            raise ValueError(f"dout must have the output's shape {out_shape}, got {tuple(dout.shape)}")
        gs = [torch.zeros_like(t) for t in ps] if grads_in is None else [g.detach().to("cpu", torch.float32).contiguous().clone() for g in grads_in]
        if [g.shape for g in gs] != [t.shape for t in ps]:
            raise ValueError("grads_in must match params")
        y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
        dins = [torch.empty_like(t) for t in ins]
        if skip_grad is not None:
            dins[1] = _f32c(skip_grad, "skip_grad").clone()
            if dins[1].shape != ins[1].shape:
                raise ValueError("skip_grad must have the second source's shape")
        if mask is not None:
            if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != tuple(x.shape):
                raise ValueError("mask: a contiguous uint8 tensor of the input's shape on the device")
            ins = ins + [mask]  # follows the inputs in the pointer array
        desc = L.TrainOp(L.TRAIN_OPS[op], nb, h, w, c, c2, k, stride, pad, groups, flags, float(p))
        arr = lambda ts: (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
        self._sync_train_deterministic()
        self._check(self._lib.dyf_op_train_f32(self._h, C.byref(desc), arr(ins), arr(ps), dout.data_ptr(), y.data_ptr(), arr(dins), arr(gs),
                                               self._stream()))
        if op == "learned_sinu":
            dins = [None]  # a time value has no gradient
        if mask is not None:
            dins = None    # forward only
        if sample:
            dins = gs = None
        return {"y": y, "dinputs": dins, "dparams": gs}

    def op_sample(self, op: str, xs, params=(), *, groups: int = 0, act: str = "none", k: int = 0, pad: int = 0,
                  film_a: Optional[torch.Tensor] = None, film_c: Optional[torch.Tensor] = None, film_div: int = 0,
                  residual: Optional[torch.Tensor] = None, part: Optional[torch.Tensor] = None, stats: bool = True,
                  mask: Optional[torch.Tensor] = None, p: float = 0.0, rng_site: Optional[int] = None, rng_row_offset: int = 0,
                  rng_forward: int = 0, **net):
        """Test seam (dyf_op_sample16): ONE 16-bit sampling kernel between the convs, through its launcher.  `op`: "gn_act",
        "layernorm_c", "head", "up2_nearest", "drop16", "stem_conv", "groupnorm_f32", "up2_bilinear", "up2_epilogue".  `xs`: the device
        tensor(s): NHWC (nb, h, w, c) in the engine's 16-bit dtype; fp32 NHWC for "groupnorm_f32" / "up2_epilogue"; up to four fp32 NCHW
        sources for "stem_conv"; two 16-bit sources for the "up2_bilinear" of a concatenation.  `params`: fp32 tensors in PyTorch
        layouts (gn_act / groupnorm_f32: gamma, beta; layernorm_c: g; head: weight (cout, c), bias; stem_conv: weight (dim, cin, k, k),
        bias).  film_a / film_c: fp32 device rows (rows, stride) with stride >= c (up2_epilogue: its coefficient rows), `film_div` samples
        per row; residual: 16-bit of x's shape; part: fp32 (nb, slots, c / 8, 2) conv-epilogue partials; stats=False: no statistics
        scratch; mask: uint8 keep mask of the output's shape, or rng_site: the engine's generator.  Returns the output: 16-bit NHWC, or
        fp32 NCHW for "head".  The launchers around the networks ("readout" .. "noisy_condition") take their own keywords:
        HipEngine._op_sample_net."""
        if op not in L.SAMPLE_OPS:
            raise ValueError(f"unknown sampling op {op!r}")
        xs = [xs] if torch.is_tensor(xs) else list(xs)
        if L.SAMPLE_OPS[op] >= L.SAMPLE_OPS["readout"]:
            return self._op_sample_net(op, xs, params, mask=mask, p=p, rng_site=rng_site, rng_row_offset=rng_row_offset, rng_forward=rng_forward, **net)
        if net:
            raise ValueError(f"{op}: unknown arguments {sorted(net)}")
        dt = self.torch_dtype
        f32_in = op in ("stem_conv", "groupnorm_f32", "up2_epilogue")
        for t in xs:
            if t.dtype != (torch.float32 if f32_in else dt) or not t.is_cuda or not t.is_contiguous() or t.dim() != 4:
                raise ValueError(f"{op}: inputs are contiguous 4-d device tensors of dtype {torch.float32 if f32_in else dt}")
        if not 1 <= len(xs) <= (4 if op == "stem_conv" else 2 if op == "up2_bilinear" else 1):
            raise ValueError(f"{op}: {len(xs)} inputs")
        x = xs[0]
        ps = [np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy()) for t in params]
        desc, tens = L.SampleOp(), L.SampleTensors()
        desc.op, desc.groups, desc.act, desc.film_div = L.SAMPLE_OPS[op], int(groups), L.ACTS[act], int(film_div)
        desc.flags = 0 if stats else L.SOP_NO_STATS
        if op == "stem_conv":
            nb, _, h, w = x.shape
            c = sum(t.shape[1] for t in xs)
            desc.nsrc, desc.k, desc.pad = len(xs), int(k), int(pad)
            for i, t in enumerate(xs):
                if (t.shape[0], t.shape[2], t.shape[3]) != (nb, h, w):
                    raise ValueError("stem_conv: the sources share (nb, h, w)")
                desc.ch[i] = t.shape[1]
            if len(ps) != 2 or ps[0].shape[1:] != (c, k, k) or ps[1].shape != (ps[0].shape[0],):
                raise ValueError("stem_conv: params are weight (dim, cin, k, k) and bias (dim)")
            desc.c2 = ps[0].shape[0]
            out_shape, out_dt = (nb, h, w, desc.c2), dt
        else:
            nb, h, w, c = x.shape
            want = {"gn_act": [(c,), (c,)], "groupnorm_f32": [(c,), (c,)], "layernorm_c": [(c,)]}.get(op, [])
            out_shape, out_dt = (nb, h, w, c), dt
            if op == "head":
                if len(ps) != 2 or ps[0].ndim != 2 or ps[0].shape[1] != c:
                    raise ValueError("head: params are weight (cout, c) and bias (cout)")
                desc.c2 = ps[0].shape[0]
                want = [(desc.c2, c), (desc.c2,)]
                out_shape, out_dt = (nb, desc.c2, h, w), torch.float32
            elif op == "up2_bilinear":
                if len(xs) == 2:
                    if xs[1].shape[:3] != x.shape[:3]:
                        raise ValueError("up2_bilinear: the sources share (nb, h, w)")
                    desc.c2 = xs[1].shape[3]
                out_shape = (nb, 2 * h, 2 * w, c + desc.c2)
            elif op in ("up2_nearest", "up2_epilogue"):
                out_shape = (nb, 2 * h, 2 * w, c)
            if len(ps) != len(want) or any(t.size != int(np.prod(sh)) for t, sh in zip(ps, want)):
                raise ValueError(f"{op}: parameters must have the shapes {want}")
        desc.nb, desc.h, desc.w, desc.c = nb, h, w, c
        for i, t in enumerate(xs):
            tens.x[i] = t.data_ptr()
        keep = []  # tensors the call reads: alive until it returns
        if (film_a is None) != (film_c is None):
            raise ValueError("film_a and film_c go together")
        if film_a is not None:
            film_a, film_c = _f32c(film_a, "film_a"), _f32c(film_c, "film_c")
            rows = -(-nb // film_div) if film_div > 1 else nb
            if film_a.dim() != 2 or film_a.shape != film_c.shape or film_a.shape[0] != rows or film_a.shape[1] < c:
                raise ValueError(f"film rows must be ({rows}, >= {c}) fp32")
            desc.film_stride = film_a.shape[1]
            tens.film_a, tens.film_c = film_a.data_ptr(), film_c.data_ptr()
            keep += [film_a, film_c]
        if residual is not None:
            if residual.dtype != dt or not residual.is_cuda or not residual.is_contiguous() or tuple(residual.shape) != tuple(x.shape):
                raise ValueError("residual: a contiguous 16-bit device tensor of the input's shape")
            tens.residual = residual.data_ptr()
        if part is not None:
            part = _f32c(part, "part")
            if part.dim() != 4 or part.shape[0] != nb or part.shape[2] * 8 != c or part.shape[3] != 2:
                raise ValueError("part: fp32 (nb, slots, c / 8, 2)")
            desc.part_slots = part.shape[1]
            tens.part = part.data_ptr()
            keep.append(part)
        desc.drop_p = float(p)
        if mask is not None and rng_site is not None:
            raise ValueError("mask or rng_site, not both")
        if mask is not None:
            if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != out_shape:
                raise ValueError("mask: a contiguous uint8 device tensor of the output's shape")
            desc.drop_mode, tens.mask = 2, mask.data_ptr()
        elif rng_site is not None:
            desc.drop_mode, desc.drop_site, desc.drop_row_offset, desc.drop_forward = 1, int(rng_site), int(rng_row_offset), int(rng_forward)
        y = torch.empty(out_shape, dtype=out_dt, device=x.device)
        tens.y = y.data_ptr()
        arr = (C.c_void_p * max(len(ps), 1))(*[t.ctypes.data for t in ps])
        self._check(self._lib.dyf_op_sample16(self._h, C.byref(desc), C.byref(tens), arr, self._stream()))
        return y

    def _op_sample_net(self, op, xs, params, *, mask=None, p=0.0, rng_site=None, rng_row_offset=0, rng_forward=0, out_hw=None, in_hw=None,
                       nearest=False, src_rows=0, nb=None, col_map=None, tables=True, fold_rng=False, counters_only=False, dst=None, tau=0.0,
                       blocks=(), copy=False, iw_store=None, pair_once=False, pitch=16):
        """dyf_op_sample16 for the launchers around the networks (csrc/kernels.hip).  Device tensors, parameters fp32 in PyTorch layouts.
          readout         xs = [x 16-bit (nb, ih, iw_store, cin)], params = [weight (cin, cout, 4, 4), bias]; out_hw = the native grid;
                          col_map: int16 device tensor (iw,) of a compact input; tables=False: launch without the tap tables -> fp32 NCHW
          readout_tables  in_hw, out_hw, nearest, col_map with iw_store = the compact width -> (row_tab, col_tab) int32 (oh | ow, 8): four
                          byte offsets, four weight bit patterns
          stem / stem16   xs = 1..4 fp32 NCHW sources of src_rows (or nb) rows; out_hw = (uh, uw); params = [weight (dim, cin), bias] for
                          stem; nb: output rows (default: the sources'); stem: mask / rng_site dropout -> 16-bit NHWC; stem16:
                          (nb, uh + 2, uw + 2, 16), with fold_rng also the row-key table (nb, 2) and the generator state (8,), int32 bit patterns;
                          pair_once (needs src_rows): only the src_rows distinct rows are written -> (src_rows, uh + 2, uw + 2, 16);
                          pitch=8 (at most 8 channels): 8-channel pixels without the bias slot -> (rows, uh + 2, uw + 2, 8)
          rng_begin       nb rows, src_rows per forward, rng_forward, rng_row_offset -> (row-key table, state)
          rng_clone       xs = [source state int32 (8,)], dst = destination state (not modified), rng_row_offset = row_add -> the new destination
          time_mlp        xs = [times fp32 (rows,)], params = [w1, b1, w2, b2 (, learned weights)] -> fp32 (rows, 2 dim)
          film            xs = [SiLU rows fp32 (rows, tdim)] or [] with nb = rows; params = [wf, bf, norm_a, norm_c]; blocks = cout per block
                          -> (coef_a, coef_c)
          cold_update     xs = [x_s, x_cur, x_next] fp32 of one shape (nb, ...); copy -> (new x_s, copy or None)
          noisy_condition xs = [cond (nb, c, h, w)] or [cond, noise]; tau; rng_row_offset -> fp32"""
        given = {k for k, v, d in (("mask", mask, None), ("p", p, 0.0), ("rng_site", rng_site, None), ("rng_row_offset", rng_row_offset, 0),
                                   ("rng_forward", rng_forward, 0), ("out_hw", out_hw, None), ("in_hw", in_hw, None), ("nearest", nearest, False),
                                   ("src_rows", src_rows, 0), ("nb", nb, None), ("col_map", col_map, None), ("tables", tables, True),
                                   ("fold_rng", fold_rng, False), ("counters_only", counters_only, False), ("dst", dst, None), ("tau", tau, 0.0),
                                   ("blocks", blocks, ()), ("copy", copy, False), ("iw_store", iw_store, None),
                                   ("pair_once", pair_once, False), ("pitch", pitch, 16)) if v is not d and v != d}
        takes = {"readout": {"out_hw", "nearest", "col_map", "tables"}, "readout_tables": {"in_hw", "out_hw", "nearest", "col_map", "iw_store"},
                 "stem": {"out_hw", "nearest", "src_rows", "nb", "mask", "p", "rng_site", "rng_row_offset", "rng_forward"},
                 "stem16": {"out_hw", "nearest", "src_rows", "nb", "fold_rng", "rng_row_offset", "rng_forward", "pair_once", "pitch"},
                 "rng_begin": {"nb", "src_rows", "rng_row_offset", "rng_forward"}, "rng_clone": {"dst", "rng_row_offset", "counters_only"},
                 "time_mlp": set(), "film": {"blocks", "nb"}, "cold_update": {"copy"}, "noisy_condition": {"tau", "rng_row_offset"}}[op]
        if given - takes:
            raise ValueError(f"{op}: does not take {sorted(given - takes)}")
        dev = torch.device("cuda", self.device)
        ps = [np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy()) for t in params]
        desc, tens = L.SampleOp(), L.SampleTensors()
        desc.op = L.SAMPLE_OPS[op]
        for t in xs:
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{op}: inputs are contiguous device tensors")
        dt = self.torch_dtype
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        want = lambda t, d, n: t.dtype == d and t.dim() == n
        outs = None
        if op in ("readout", "readout_tables"):
            desc.oh, desc.ow, desc.nearest = int(out_hw[0]), int(out_hw[1]), int(bool(nearest))
            if col_map is not None:
                if col_map.dtype != torch.int16 or not col_map.is_cuda or not col_map.is_contiguous() or col_map.dim() != 1:
                    raise ValueError(f"{op}: col_map is a contiguous int16 device vector")
                tens.col_map = col_map.data_ptr()
            if op == "readout":
                if len(xs) != 1 or not want(xs[0], dt, 4) or len(ps) != 2 or ps[0].ndim != 4 or ps[0].shape[0] != xs[0].shape[3] or ps[0].shape[2:] != (4, 4):
                    raise ValueError("readout: x 16-bit (nb, ih, iw_store, cin), weight (cin, cout, 4, 4), bias (cout)")
                desc.nb, desc.h, iws, desc.c = xs[0].shape
                desc.c2 = ps[0].shape[1]
                desc.w = iws if col_map is None else col_map.numel()
                desc.iw_store = 0 if col_map is None else iws
                desc.flags = 0 if tables else L.SOP_NO_TABLES
                outs = [f32(desc.nb, desc.c2, desc.oh, desc.ow)]
            else:
                desc.nb, desc.h, desc.w = 1, int(in_hw[0]), int(in_hw[1])
                desc.iw_store = 0 if col_map is None else int(iw_store)
                outs = [i32(desc.oh, 8), i32(desc.ow, 8)]
        elif op in ("stem", "stem16"):
            if not 1 <= len(xs) <= 4 or any(not want(t, torch.float32, 4) or t.shape[0] != xs[0].shape[0] or t.shape[2:] != xs[0].shape[2:] for t in xs):
                raise ValueError(f"{op}: 1..4 fp32 NCHW sources of one (rows, h, w)")
            rows, _, desc.h, desc.w = xs[0].shape
            desc.nb = rows if nb is None else int(nb)
            desc.src_rows = int(src_rows)
            if (desc.src_rows if desc.src_rows > 0 else desc.nb) != rows:
                raise ValueError(f"{op}: the sources hold src_rows (or nb) rows")
            desc.nsrc, desc.c = len(xs), sum(t.shape[1] for t in xs)
            for i, t in enumerate(xs):
                desc.ch[i] = t.shape[1]
            desc.oh, desc.ow, desc.nearest = int(out_hw[0]), int(out_hw[1]), int(bool(nearest))
            if op == "stem":
                if len(ps) != 2 or ps[0].ndim != 2 or ps[0].shape[1] != desc.c or ps[1].shape != (ps[0].shape[0],):
                    raise ValueError("stem: params are weight (dim, cin) and bias (dim)")
                desc.c2 = ps[0].shape[0]
                outs = [torch.empty((desc.nb, desc.oh, desc.ow, desc.c2), dtype=dt, device=dev)]
                desc.drop_p = float(p)
                if mask is not None and rng_site is not None:
                    raise ValueError("mask or rng_site, not both")
                if mask is not None:
                    if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != tuple(outs[0].shape):
                        raise ValueError("mask: a contiguous uint8 device tensor of the output's shape")
                    desc.drop_mode, tens.mask = 2, mask.data_ptr()
                elif rng_site is not None:
                    desc.drop_mode, desc.drop_site, desc.drop_row_offset, desc.drop_forward = 1, int(rng_site), int(rng_row_offset), int(rng_forward)
            else:
                if pair_once and desc.src_rows < 1:
                    raise ValueError("stem16: pair_once writes the src_rows distinct rows: give src_rows")
                if pitch not in (8, 16) or (pitch == 8 and desc.c > 8):
                    raise ValueError("stem16: pitch is 16, or 8 for at most 8 channels")
                outs = [torch.empty((desc.src_rows if pair_once else desc.nb, desc.oh + 2, desc.ow + 2, int(pitch)), dtype=dt, device=dev)]
                desc.flags = (L.SOP_PAIR_ONCE if pair_once else 0) | (L.SOP_STEM_PITCH8 if pitch == 8 else 0)
                if fold_rng:
                    desc.flags, desc.drop_row_offset, desc.drop_forward = desc.flags | L.SOP_FOLD_RNG, int(rng_row_offset), int(rng_forward)
                    outs += [i32(desc.nb, 2), i32(L.RNG_STATE_WORDS)]
        elif op == "rng_begin":
            desc.nb, desc.src_rows, desc.drop_row_offset, desc.drop_forward = int(nb), int(src_rows), int(rng_row_offset), int(rng_forward)
            outs = [i32(desc.nb, 2), i32(L.RNG_STATE_WORDS)]
        elif op == "rng_clone":
            if len(xs) != 1 or dst is None or any(t.dtype != torch.int32 or tuple(t.shape) != (L.RNG_STATE_WORDS,) for t in (xs[0], dst)):
                raise ValueError("rng_clone: source and destination states are int32 (8,)")
            desc.nb, desc.drop_row_offset, desc.flags = 1, int(rng_row_offset), L.SOP_COUNTERS_ONLY if counters_only else 0
            outs = [dst.clone()]
        elif op == "time_mlp":
            if len(xs) != 1 or not want(xs[0], torch.float32, 1) or len(ps) not in (4, 5) or ps[2].ndim != 2:
                raise ValueError("time_mlp: times fp32 (rows,), params w1, b1, w2, b2 (, learned weights)")
            desc.nb, desc.c = xs[0].shape[0], ps[2].shape[0] // 2
            desc.c2 = ps[4].size if len(ps) == 5 else 0
            nfeat = 2 * desc.c2 + 1 if desc.c2 else desc.c
            if [t.shape for t in ps[:4]] != [(2 * desc.c, nfeat), (2 * desc.c,), (2 * desc.c, 2 * desc.c), (2 * desc.c,)]:
                raise ValueError("time_mlp: parameter shapes")
            outs = [f32(desc.nb, 2 * desc.c)]
        elif op == "film":
            total = sum(blocks)
            if len(ps) != 4 or ps[0].ndim != 2 or [t.shape for t in ps] != [(2 * total, ps[0].shape[1]), (2 * total,), (total,), (total,)] or not 1 <= len(blocks) <= 4:
                raise ValueError("film: params wf (2 total, tdim), bf, norm_a, norm_c; 1..4 blocks")
            desc.c = ps[0].shape[1]
            if xs and (len(xs) != 1 or not want(xs[0], torch.float32, 2) or xs[0].shape[1] != desc.c):
                raise ValueError("film: SiLU rows fp32 (rows, tdim)")
            desc.nb = xs[0].shape[0] if xs else int(nb)
            desc.nsrc = len(blocks)
            for i, c in enumerate(blocks):
                desc.ch[i] = int(c)
            outs = [f32(desc.nb, total), f32(desc.nb, total)]
        elif op == "cold_update":
            if len(xs) != 3 or any(not want(t, torch.float32, 4) or t.shape != xs[0].shape for t in xs):
                raise ValueError("cold_update: x_s, x_cur, x_next fp32 of one 4-d shape")
            desc.nb, desc.c, desc.h, desc.w = xs[0].shape
            outs = [xs[0].clone()] + ([torch.empty_like(xs[0])] if copy else [])
            xs = xs[1:]
        elif op == "noisy_condition":
            if not 1 <= len(xs) <= 2 or any(not want(t, torch.float32, 4) or t.shape != xs[0].shape for t in xs):
                raise ValueError("noisy_condition: cond (and noise) fp32 (nb, c, h, w)")
            desc.nb, desc.c, desc.h, desc.w = xs[0].shape
            desc.tau, desc.drop_row_offset = float(tau), int(rng_row_offset)
            outs = [torch.empty_like(xs[0])]
        for i, t in enumerate(xs):
            tens.x[i] = t.data_ptr()
        tens.y = outs[0].data_ptr()
        if len(outs) > 1:
            tens.y2 = outs[1].data_ptr()
        if len(outs) > 2:
            tens.y3 = outs[2].data_ptr()
        arr = (C.c_void_p * max(len(ps), 1))(*[t.ctypes.data for t in ps])
        self._check(self._lib.dyf_op_sample16(self._h, C.byref(desc), C.byref(tens), arr, self._stream()))
        if op == "cold_update":
            return outs[0], (outs[1] if copy else None)
        return outs[0] if len(outs) == 1 else tuple(outs)

    def op_upconv2d(self, x_nhwc_bf16: torch.Tensor, weight: torch.Tensor, scale: Optional[torch.Tensor] = None,
                    shift: Optional[torch.Tensor] = None, act: int = 0) -> torch.Tensor:
        """Test seam: fused Upsample(x2, bilinear) + Conv2d(3x3, pad 1).  x (N,H,W,Cin) bf16 -> (N,2H,2W,Cout) bf16."""
        assert x_nhwc_bf16.dtype == torch.bfloat16 and x_nhwc_bf16.is_cuda and x_nhwc_bf16.is_contiguous()
        n, h, w, cin = x_nhwc_bf16.shape
        cout = weight.shape[0]
        wh = np.ascontiguousarray(weight.detach().to("cpu", torch.float32).numpy())
        y = torch.empty((n, 2 * h, 2 * w, cout), dtype=torch.bfloat16, device=x_nhwc_bf16.device)
        if scale is not None:
            scale, shift = _f32c(scale, "scale"), _f32c(shift, "shift")
        self._check(self._lib.dyf_op_upconv2d(self._h, x_nhwc_bf16.data_ptr(), wh.ctypes.data, n, h, w, cin, cout,
                                              None if scale is None else scale.data_ptr(),
                                              None if shift is None else shift.data_ptr(), act, y.data_ptr(),
                                              self._stream()))
        return y

    def op_upconv2d_ex(self, x: torch.Tensor, weight: torch.Tensor, scale: Optional[torch.Tensor] = None,
                       shift: Optional[torch.Tensor] = None, act: int = 0, *, x1: Optional[torch.Tensor] = None, coef_div: int = 0,
                       n_sel: int = 0, mask: Optional[torch.Tensor] = None, p: float = 0.0, rng_site: Optional[int] = None,
                       rng_row_offset: int = 0, rng_forward: int = 0, residual: Optional[torch.Tensor] = None, out_f32: bool = False,
                       needed: Optional[torch.Tensor] = None, fill: Optional[float] = None):
        """Test seam (dyf_op_upconv2d_ex): the fused Upsample(x2, bilinear) + Conv2d(3x3, pad 1) with the argument block of a decoder
        block, through the ladder.  x (N,H,W,c0) and x1 (N,H,W,c1: the skip) in the engine's 16-bit dtype, weight (Cout, c0 + c1, 3, 3),
        scale / shift of ceil(N / coef_div) rows, mask: uint8 keep mask of the DENSE output shape (dropout mode 2), rng_site: dropout
        mode 1.  needed: uint8 / bool over the 2W output columns -> the seam plans the sparse column lists and the result is
        (y, plan): plan["planned"] == 1: y is the compact (N,2H,wo_store,Cout) tensor and plan["col_map"] its int16 column map;
        0: the planner declined and y is dense.  fill: the output buffer holds this value before the launch.  Without `needed` the
        result is y, or (y, y_f32) with out_f32."""
        dt = self.torch_dtype
        assert x.dtype == dt and x.is_cuda and x.is_contiguous()
        n, h, w, c0 = x.shape
        c1 = 0
        if x1 is not None:
            assert x1.dtype == dt and x1.is_cuda and x1.is_contiguous() and x1.shape[:3] == x.shape[:3]
            c1 = x1.shape[3]
        cout, cin, kh, kw = weight.shape
        assert cin == c0 + c1 and (kh, kw) == (3, 3) and not (mask is not None and rng_site is not None)
        wh = np.ascontiguousarray(weight.detach().to("cpu", torch.float32).numpy())
        shape = (n, 2 * h, 2 * w, cout)
        y = torch.empty(shape, dtype=dt, device=x.device)
        y32 = torch.empty(shape, dtype=torch.float32, device=x.device) if out_f32 else None
        if fill is not None:
            y.fill_(fill)
        if scale is not None:
            rows = -(-n // coef_div) if coef_div > 1 else n
            scale, shift = _f32c(scale, "scale"), _f32c(shift, "shift")
            assert tuple(scale.shape) == (rows, cout) and tuple(shift.shape) == (rows, cout)
        ex = L.ConvEx()
        if x1 is not None:
            ex.x1_dev, ex.c1 = x1.data_ptr(), c1
        if residual is not None:
            assert residual.dtype == dt and residual.is_cuda and residual.is_contiguous() and tuple(residual.shape) == shape
            ex.residual_dev = residual.data_ptr()
        if y32 is not None:
            ex.y_f32_dev = y32.data_ptr()
        ex.coef_div, ex.n_sel, ex.drop_p = int(coef_div), int(n_sel), float(p)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and tuple(mask.shape) == shape
            ex.drop_mode, ex.mask_dev = 2, mask.data_ptr()
        elif rng_site is not None:
            ex.drop_mode, ex.drop_site, ex.drop_row_offset, ex.drop_forward = 1, int(rng_site), int(rng_row_offset), int(rng_forward)
        sp = None
        if needed is not None:
            need = np.ascontiguousarray(needed.detach().to("cpu").numpy().astype(np.uint8))
            assert need.shape == (2 * w,)
            cmap = np.full(2 * w, -1, dtype=np.int16)
            sp = L.UpconvSparse()
            sp.needed_host, sp.col_map_host = need.ctypes.data, cmap.ctypes.data
        self._check(self._lib.dyf_op_upconv2d_ex(self._h, x.data_ptr(), wh.ctypes.data, n, h, w, c0, cout,
                                                 None if scale is None else scale.data_ptr(), None if shift is None else shift.data_ptr(),
                                                 act, y.data_ptr(), C.byref(ex), None if sp is None else C.byref(sp), self._stream()))
        if sp is None:
            return (y, y32) if out_f32 else y
        plan = dict(planned=int(sp.planned), ntiles=int(sp.ntiles), npad=int(sp.npad), nvalid0=int(sp.nvalid0), nvalid1=int(sp.nvalid1),
                    wo_store=int(sp.wo_store), mix=[int(v) for v in sp.mix], col_map=torch.from_numpy(cmap.copy()))
        if plan["planned"]:
            ws = plan["wo_store"]
            return y.reshape(-1)[:n * 2 * h * ws * cout].reshape(n, 2 * h, ws, cout), plan
        return y, plan


class EngineLoss(torch.autograd.Function):
    """Scalar loss whose backward is the engine's backward pass: `owner._train_backward(upstream)` runs dyf_train_backward and
    accumulates into `param.grad` (so `loss.backward()` / torch.optim / Lightning's training_step work unchanged)."""

    @staticmethod
    def forward(ctx, anchor, owner, value):
        ctx.owner = owner
        ctx.step_id = owner._train_state["step_id"]  # the engine's tapes are single-slot: they belong to the LATEST forward
        return anchor.new_tensor(value)

    @staticmethod
    def backward(ctx, grad_out):
        st = getattr(ctx.owner, "_train_state", None)
        # the owner's own record AND the engine-wide counter: two owners can share one engine (a DYffusion and its attached
        # forecaster's get_loss both record into the same tape slots), and a training forward by EITHER overwrites the tapes
        eng = None if st is None else st.get("eng")
        if st is None or st.get("step_id") != ctx.step_id or st.get("consumed") or \
                (eng is not None and eng.train_step_id != ctx.step_id):
            raise RuntimeError("this loss belongs to an earlier training forward (or has already been back-propagated): the "
                               "engine records one step at a time -- call .backward() on a loss before the next p_losses() / "
                               "get_loss() of the same engine, and only once")
        st["consumed"] = True
        ctx.owner._train_backward(float(grad_out))
        return None, None, None


def state_version(net) -> int:
    """Identifies the state of a module's parameters and buffers: the sum of their in-place modification counters
    (`Tensor._version`: optimizer steps, `p.mul_()`, `load_state_dict`, ...) and of their storage addresses (`p.data = other`
    swaps).  NOT visible to it: in-place writes through an alias, e.g. `p.data.copy_(...)` -- call `mark_weights_modified()`
    on the module (or `load_state_dict`) after such an edit.  The tensor list is cached on the module (the mirrors drop it in
    `_apply`, i.e. on .cuda() / .to() / .float(), which replace buffer objects): ~20 us per call."""
    vt = net.__dict__.get("_version_tensors")
    if vt is None:
        vt = list(net.parameters()) + list(net.buffers())
        net.__dict__["_version_tensors"] = vt
    v = net.__dict__.get("_manual_version", 0)
    for t in vt:
        v += t._version + t.data_ptr()
    return v


def mark_weights_modified(net) -> None:
    """Force the next engine use of `net` to re-upload its weights (after edits the version counters cannot see)."""
    net.__dict__["_manual_version"] = net.__dict__.get("_manual_version", 0) + 1
    net.__dict__.pop("_version_tensors", None)


def upload_weights(net, eng: "HipEngine", slot: int) -> None:
    """dyf_load_weights of `net`'s state_dict (sampling copy AND training copy), remembering which version of the parameters
    the engine now holds."""
    eng.load_weights(slot, net.state_dict())
    net._uploaded_version = net._train_version = (id(eng), state_version(net))


def resident_optimizer(net):
    """The `optim.EngineAdamW` attached to `net` (its weights are updated on the engine), or None."""
    return net.__dict__.get("_engine_optim")


def sync_weights(net, eng: "HipEngine", slot: int) -> None:
    """Before SAMPLING / inference: re-upload a network whose parameters or buffers were modified since the last full upload
    (optimizer.step(), `p.data = ...` swaps; see `state_version` for what is detected).  With an engine-resident optimizer the
    module is first brought up to date from the engine (`EngineAdamW.pull`), which changes its version marks: the sampling copy
    is then refreshed by the same mechanism."""
    opt = resident_optimizer(net)
    if opt is not None:
        opt.pull()
    if getattr(net, "_uploaded_version", None) != (id(eng), state_version(net)):
        upload_weights(net, eng, slot)


def sync_train_weights(net, eng: "HipEngine", slot: int) -> None:
    """Before a TRAINING step: refresh only the engine's fp32 training copy (dyf_train_load_weights, ~10x cheaper than the full
    upload, which re-derives every packed 16-bit layout of the sampling path); the sampling copy is brought up to date by
    `sync_weights` when the network is next sampled."""
    opt = resident_optimizer(net)
    if opt is not None and opt.engine_is_ahead(eng):
        return  # the engine's training copy IS the current state (resident steps / BatchNorm updates the module has not pulled yet)
    ver = (id(eng), state_version(net))
    if getattr(net, "_train_version", None) == ver:
        return
    if getattr(net, "_uploaded_version", None) is None or net._uploaded_version[0] != id(eng):
        upload_weights(net, eng, slot)  # this engine has never seen the network: full load first
    else:
        eng.train_load_weights(slot, net.state_dict())
        net._train_version = ver


def collect_train_results(net, eng: "HipEngine", slot: int, n_forwards: int) -> None:
    """After dyf_train_backward: add the engine's parameter gradients of network `slot` to `param.grad`, clear them in the
    engine, and bring the BatchNorm buffers to what module.train() leaves (running statistics after `n_forwards` momentum
    updates, num_batches_tracked).  With an engine-resident optimizer attached (`optim.EngineAdamW`) nothing is exported: the
    gradients stay, and accumulate, in the engine; the optimizer books the BatchNorm updates for its next `pull()`."""
    opt = resident_optimizer(net)
    if opt is not None:
        opt.after_backward(eng, slot, n_forwards)
        return
    sd = net.state_dict(keep_vars=True)
    shapes = {k: tuple(v.shape) for k, v in sd.items() if isinstance(v, torch.nn.Parameter)}
    on_gpu = all(v.is_cuda and v.device.index == eng.device for v in sd.values() if torch.is_tensor(v) and v.is_floating_point())
    dev = next(iter(sd.values())).device if on_gpu else None
    for k, g in eng.train_export(slot, shapes, device=dev).items():
        p = sd[k]
        g = g.to(device=p.device, dtype=p.dtype)
        p.grad = g if p.grad is None else p.grad + g
    eng.train_zero_grads(slot)
    bufs = {k: tuple(v.shape) for k, v in sd.items() if k.endswith("running_mean") or k.endswith("running_var")}
    with torch.no_grad():
        for k, v in eng.train_export(slot, bufs, device=dev).items():
            sd[k].copy_(v)
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                v += n_forwards
    # the engine's TRAINING copy holds exactly these buffers; its sampling copy still has the old running statistics folded in
    net._train_version = (id(eng), state_version(net))

