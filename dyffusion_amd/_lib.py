"""ctypes binding of libdyffusion_hip.so (C ABI: include/dyffusion_hip.h).

The library is built in-tree by `__graft_entry__.build()` (hipcc --offload-arch=gfx950).  There is deliberately NO
fallback: if the shared object is missing or a symbol cannot be resolved, importing this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DYF_LIB") or os.path.join(_HERE, "lib", "libdyffusion_hip.so")  # DYF_LIB: experiment builds
# the fp16 build of the same sources (-DDYF_F16=1): same ABI, fp16 storage + v_mfma_*_f16 (BASELINE configs[4])
LIB_PATH_F16 = os.environ.get("DYF_LIB_F16") or os.path.join(_HERE, "lib", "libdyffusion_hip_f16.so")
DTYPES = {"bf16": 0, "bfloat16": 0, "fp16": 1, "float16": 1, "half": 1}
# fp32 sampling (dyf_set_sample_precision(32)) is a mode of an engine, not a build of the library: such engines load the bf16 build
FP32_NAMES = ("fp32", "float32", "32")
# bf16x3 sampling (dyf_set_sample_precision(48)): the fp32 forward with (hi, lo) bf16 conv operands -- likewise a mode of a bf16-build engine
BF16X3_NAMES = ("bf16x3", "48")


def canonical_dtype(dtype) -> str:
    """"bf16" | "fp16" | "fp32" | "bf16x3" for every accepted spelling; ValueError for anything else."""
    key = str(dtype).lower()
    if key in FP32_NAMES:
        return "fp32"
    if key in BF16X3_NAMES:
        return "bf16x3"
    if key not in DTYPES:
        raise ValueError(f"dtype {dtype!r}: expected one of {sorted(DTYPES) + list(FP32_NAMES) + list(BF16X3_NAMES)}")
    return "fp16" if DTYPES[key] else "bf16"


def storage_dtype(dtype) -> str:
    """The 16-bit build an engine of `dtype` is served by ("fp32" and "bf16x3" engines: the default bf16 build)."""
    d = canonical_dtype(dtype)
    return "bf16" if d in ("fp32", "bf16x3") else d


# dyf_set_sample_precision: bits an engine of a canonical dtype is switched to at creation (absent: it stays at 16)
SAMPLE_PRECISION_BITS = {"fp32": 32, "bf16x3": 48}


# dyf_set_attention_dropout: how a 16-bit engine draws the dropout of unet.Unet's Attention probabilities (include/dyffusion_hip.h)
ATTN_DROPOUT_FAST, ATTN_DROPOUT_EXACT = 0, 1
ATTN_DROPOUT_MODES = {"fast": ATTN_DROPOUT_FAST, "exact": ATTN_DROPOUT_EXACT}


def attention_dropout_mode(mode) -> int:
    """"fast" | "exact" -> DYF_ATTN_DROPOUT_FAST / DYF_ATTN_DROPOUT_EXACT; ValueError for anything else."""
    if not isinstance(mode, str) or mode not in ATTN_DROPOUT_MODES:
        raise ValueError(f"attention_dropout {mode!r}: expected one of {sorted(ATTN_DROPOUT_MODES)}")
    return ATTN_DROPOUT_MODES[mode]


DYF_ABI_VERSION = 9
DYF_TRAIN_PRECISION_BF16X3 = 48  # dyf_train_set_precision: bf16x3 (hi/lo bf16 operand pairs, three MFMAs per product)
DYF_SAMPLE_PRECISION_BF16X3 = 48  # dyf_set_sample_precision: the fp32 sampling forward with those conv operands
DYF_OK, DYF_ERR_INVALID_ARGUMENT, DYF_ERR_UNSUPPORTED, DYF_ERR_HIP, DYF_ERR_STATE = range(5)
NET_FORECASTER, NET_INTERPOLATOR = 0, 1
ARCH_UNET_SIMPLE, ARCH_UNET_RESNET = 0, 1
ARCH_SIMPLE_CONV_NET = 2
FCOND = {"none": 0, "data": 1, "data+noise": 2}


class NetConfig(C.Structure):
    _fields_ = [("arch", C.c_int32), ("in_channels", C.c_int32), ("cond_channels", C.c_int32),
                ("out_channels", C.c_int32), ("dim", C.c_int32), ("with_time_emb", C.c_int32),
                ("upsample_h", C.c_int32), ("upsample_w", C.c_int32), ("dropout", C.c_float),
                ("input_dropout", C.c_float), ("n_mults", C.c_int32), ("dim_mults", C.c_int32 * 6),
                ("block_dropout1", C.c_float), ("attn_dropout", C.c_float), ("groups", C.c_int32),
                ("init_kernel_size", C.c_int32), ("init_padding", C.c_int32), ("outer_nearest", C.c_int32),
                ("keep_spatial_dims", C.c_int32), ("single_conv_layer", C.c_int32), ("learned_sinusoidal_dim", C.c_int32)]


class EngineConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("max_batch", C.c_int32), ("use_graph", C.c_int32), ("enable_mfma", C.c_int32), ("dtype", C.c_int32),
                ("batch_invariant", C.c_int32), ("net", NetConfig * 2)]


class PlanStep(C.Structure):
    _fields_ = [("forecaster_time", C.c_float), ("tau", C.c_float), ("i_next", C.c_float), ("i_cur", C.c_float),
                ("is_last", C.c_int32), ("out_slot", C.c_int32)]


class Plan(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("steps", C.POINTER(PlanStep)), ("sampling_cold", C.c_int32),
                ("cold_for_last_step", C.c_int32), ("forward_conditioning", C.c_int32), ("n_refine", C.c_int32),
                ("refine_times", C.POINTER(C.c_float)), ("refine_slots", C.POINTER(C.c_int32)),
                ("n_out_slots", C.c_int32), ("interpolator_dropout", C.c_int32), ("forecaster_dropout", C.c_int32)]


class BcArgs(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_fields", C.c_int32), ("rows", C.c_int32), ("channels", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("n_meta", C.c_int32), ("row_meta_dev", C.c_void_p),
                ("time_factor_dev", C.c_void_p), ("times_per_meta", C.c_int32), ("fixed_mask_dev", C.c_void_p),
                ("in_velocity_dev", C.c_void_p), ("vertex_y_dev", C.c_void_p), ("boundary_dev", C.c_void_p)]


class ConvEx(C.Structure):
    """dyf_conv_ex (include/dyffusion_hip_testing.h): the optional arguments of dyf_op_conv2d_ex; zero / NULL = absent."""
    _fields_ = [("x1_dev", C.c_void_p), ("residual_dev", C.c_void_p), ("y_f32_dev", C.c_void_p), ("mask_dev", C.c_void_p),
                ("c1", C.c_int32), ("coef_div", C.c_int32), ("n_sel", C.c_int32), ("drop_mode", C.c_int32),
                ("drop_p", C.c_float), ("drop_site", C.c_int32), ("drop_row_offset", C.c_uint32), ("drop_forward", C.c_uint32)]


class UpconvSparse(C.Structure):
    """dyf_upconv_sparse (include/dyffusion_hip_testing.h): the needed-column mask of dyf_op_upconv2d_ex and the plan it reports."""
    _fields_ = [("needed_host", C.c_void_p), ("col_map_host", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("planned", "ntiles", "npad", "nvalid0", "nvalid1", "wo_store")] + [("mix", C.c_int32 * 3)]


class ConvGn(C.Structure):
    """dyf_conv_gn (include/dyffusion_hip_testing.h): one 3x3 conv in front of a GroupNorm for dyf_op_conv_gn."""
    _fields_ = [(k, C.c_int32) for k in ("n", "h", "w", "c0", "c1", "cout", "groups", "want", "act", "coef_div", "n_sel", "invariant",
                                         "film_stride", "drop_mode")] + \
               [("drop_p", C.c_float), ("drop_site", C.c_int32), ("drop_row_offset", C.c_uint32), ("drop_forward", C.c_uint32)] + \
               [(k, C.c_int32) for k in ("conv_tag", "max_slots", "new_forward")]


class ConvGnTensors(C.Structure):
    """dyf_conv_gn_tensors: the device pointers of one dyf_op_conv_gn call; NULL = absent."""
    _fields_ = [(k, C.c_void_p) for k in ("x0", "x1", "residual", "film_a", "film_c", "mask", "y", "gran", "epoch", "part")] + \
               [("gran_granules", C.c_int64), ("part_floats", C.c_int64)]


class ConvGnResult(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("fused", "slots", "bm", "slow_sweep")]


class ProductsSpec(C.Structure):
    """dyf_products_spec (include/dyffusion_hip.h): the planes dyf_ensemble_products writes, in this order."""
    _fields_ = [("mean", C.c_int32), ("std", C.c_int32), ("min", C.c_int32), ("max", C.c_int32),
                ("n_quantiles", C.c_int32), ("quantiles", C.c_double * 16), ("n_thresholds", C.c_int32), ("thresholds", C.c_float * 16)]


MAX_PRODUCT_QUANTILES = MAX_PRODUCT_THRESHOLDS = 16  # DYF_MAX_PRODUCT_QUANTILES / DYF_MAX_PRODUCT_THRESHOLDS
ENERGY_TILE_POINTS = 64  # DYF_ENERGY_TILE_POINTS: the fp32 accumulation length of dyf_energy_score
ENERGY_MAX_MEMBERS = 256  # DYF_ENERGY_MAX_MEMBERS
ENERGY_MAX_WORKSPACE_DOUBLES = 1 << 27  # DYF_ENERGY_MAX_WORKSPACE_DOUBLES
SPECTRUM_MAX_DIM = 1024  # DYF_SPECTRUM_MAX_DIM: the largest transform length of dyf_power_spectrum
SPECTRUM_MAX_MEMBERS = 256  # DYF_SPECTRUM_MAX_MEMBERS
BC_NAVIER_STOKES, BC_SPRING_MESH = 0, 1
COMM_ID_BYTES = 128  # DYF_COMM_ID_BYTES (ncclUniqueId)
TRAIN_BATCH_STATS, TRAIN_DROPOUT = 1, 2


class TrainOp(C.Structure):
    """dyf_train_op (include/dyffusion_hip_testing.h): one recorded op of the training step for dyf_op_train_f32."""
    _fields_ = [(k, C.c_int32) for k in ("op", "nb", "h", "w", "c", "c2", "k", "stride", "pad", "groups", "flags")] + [("p", C.c_float)]


TRAIN_OPS = {"conv": 0, "gn_act": 1, "layernorm": 2, "linattn": 3, "attention": 4, "linear": 5, "learned_sinu": 6, "dropout": 7,
             "gelu": 8, "add": 9, "cat": 10, "up2_nearest": 11, "norm_act": 12, "up2_bilinear": 13, "resize": 14, "convt": 15,
             "attention_stream": 16}
TOP_WS, TOP_BIAS, TOP_PRE, TOP_FILM, TOP_SAME = 1, 2, 4, 8, 16
TOP_RUNNING, TOP_MASK, TOP_LEAKY, TOP_RELU, TOP_NEAREST, TOP_GRAD_IN = 32, 64, 128, 256, 512, 1024
TOP_ACT_GELU, TOP_RESIDUAL = 2048, 4096
TOP_SAMPLE = 8192  # conv: the forward alone, launched as a sampling forward launches it


class SampleOp(C.Structure):
    """dyf_sample_op (include/dyffusion_hip_testing.h): one 16-bit sampling kernel's launch for dyf_op_sample16."""
    _fields_ = [(k, C.c_int32) for k in ("op", "nb", "h", "w", "c", "c2", "k", "pad", "groups", "act", "flags", "film_stride", "film_div",
                                         "part_slots", "nsrc")] + [("ch", C.c_int32 * 4), ("drop_mode", C.c_int32), ("drop_p", C.c_float),
                                                                   ("drop_site", C.c_int32), ("drop_row_offset", C.c_uint32), ("drop_forward", C.c_uint32)] + \
               [(k, C.c_int32) for k in ("oh", "ow", "nearest", "src_rows", "iw_store")] + [("tau", C.c_float)]


class SampleTensors(C.Structure):
    """dyf_sample_tensors: the device pointers of one dyf_op_sample16 call; NULL = absent."""
    _fields_ = [("x", C.c_void_p * 4), ("residual", C.c_void_p), ("film_a", C.c_void_p), ("film_c", C.c_void_p), ("part", C.c_void_p),
                ("mask", C.c_void_p), ("y", C.c_void_p), ("col_map", C.c_void_p), ("y2", C.c_void_p), ("y3", C.c_void_p)]


SAMPLE_OPS = {"gn_act": 0, "layernorm_c": 1, "head": 2, "up2_nearest": 3, "drop16": 4, "stem_conv": 5, "groupnorm_f32": 6, "up2_bilinear": 7,
              "up2_epilogue": 8, "readout": 9, "readout_tables": 10, "stem": 11, "stem16": 12, "rng_begin": 13, "rng_clone": 14, "time_mlp": 15,
              "film": 16, "cold_update": 17, "noisy_condition": 18}
SOP_NO_STATS, SOP_NO_TABLES, SOP_FOLD_RNG, SOP_COUNTERS_ONLY, SOP_PAIR_ONCE, SOP_STEM_PITCH8 = 1, 2, 4, 8, 16, 32
RNG_STATE_WORDS = 8  # DYF_RNG_STATE_WORDS (csrc/kernels.h)
ACTS = {"none": 0, "relu": 1, "leaky": 2, "silu": 3, "gelu": 4}


class OptimConfig(C.Structure):
    """dyf_optim_config (include/dyffusion_hip.h): the engine-resident AdamW / EMA step."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_grad_norm", C.c_double), ("ema", C.c_int32)]


OPTIM_WEIGHT, OPTIM_GRAD, OPTIM_EXP_AVG, OPTIM_EXP_AVG_SQ, OPTIM_EMA, OPTIM_WEIGHT_FWD = range(6)

# every symbol include/dyffusion_hip.h and include/dyffusion_hip_testing.h declare: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("dyf_engine_create", C.c_int, [C.POINTER(EngineConfig), C.POINTER(_P)]),
    ("dyf_engine_destroy", None, [_P]),
    ("dyf_last_error", C.c_char_p, [_P]),
    ("dyf_abi_version", C.c_int32, []),
    ("dyf_dtype", C.c_int32, []),
    ("dyf_load_weights", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_P),
                                   C.POINTER(C.c_int32)]),
    ("dyf_train_load_weights", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_P),
                                         C.POINTER(C.c_int32)]),
    ("dyf_train_load_weights_dev", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_P),
                                             C.POINTER(C.c_int32)]),
    ("dyf_train_export_dev", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_P)]),
    ("dyf_net_forward", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(_P), _P]),
    ("dyf_set_plan", C.c_int, [_P, C.POINTER(Plan)]),
    ("dyf_sample", C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(_P), _P, _P]),
    ("dyf_seed", C.c_int, [_P, C.c_uint64]),
    ("dyf_set_row_offset", C.c_int, [_P, C.c_uint32]),
    ("dyf_set_log_intermediates", C.c_int, [_P, C.c_int32]),
    ("dyf_get_log", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    ("dyf_set_row_groups", C.c_int, [_P, C.c_int32]),
    ("dyf_row_groups", C.c_int32, [_P]),
    ("dyf_comm_unique_id", C.c_int, [_P]),
    ("dyf_comm_init", C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    ("dyf_comm_destroy", C.c_int, [_P]),
    ("dyf_comm_count", C.c_int, [_P, _P]),
    ("dyf_sample_gather", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    ("dyf_get_sampler_state", C.c_int, [_P, C.c_int32, _P, C.c_int32, _P]),
    ("dyf_plan_forward_counts", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("dyf_net_flops", C.c_int, [_P, C.c_int32, C.POINTER(C.c_double)]),
    ("dyf_net_flops_executed", C.c_int, [_P, C.c_int32, C.POINTER(C.c_double)]),
    ("dyf_time_conv_layer", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("dyf_ensemble_metrics", C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_double), _P]),
    ("dyf_trajectory_metrics", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.c_int32, C.c_int64, C.c_int64, _P, _P, _P]),
    ("dyf_ensemble_size_metrics", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.c_int32, C.c_int64, C.c_int64, _P, _P, _P]),
    ("dyf_ensemble_scores", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                      C.c_int64, _P, _P, _P]),
    ("dyf_ensemble_products", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.c_int32, C.c_int64, C.c_int64, C.POINTER(ProductsSpec), _P, _P]),
    ("dyf_rank_histogram", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                     C.c_int64, _P, _P, _P]),
    ("dyf_energy_score", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                   C.c_int64, _P, _P, _P, _P, _P]),
    ("dyf_power_spectrum", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, _P, _P, _P]),
    ("dyf_time_layer_in_rollout", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("dyf_time_kernel_in_rollout", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("dyf_op_conv2d", C.c_int, [_P, _P, _P] + [C.c_int32] * 9 + [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    ("dyf_op_conv2d_ex", C.c_int, [_P, _P, _P] + [C.c_int32] * 9 + [_P, _P, C.c_int32, C.c_int32, _P, C.POINTER(ConvEx), _P]),
    ("dyf_op_conv_gn", C.c_int, [_P, C.POINTER(ConvGn), C.POINTER(ConvGnTensors), _P, _P, _P, _P, C.POINTER(ConvGnResult), _P]),
    ("dyf_op_upconv2d", C.c_int, [_P, _P, _P] + [C.c_int32] * 5 + [_P, _P, C.c_int32, _P, _P]),
    ("dyf_op_upconv2d_ex", C.c_int, [_P, _P, _P] + [C.c_int32] * 5 + [_P, _P, C.c_int32, _P, C.POINTER(ConvEx), C.POINTER(UpconvSparse), _P]),
    ("dyf_op_linear_attention", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    ("dyf_op_linear_attention_fused", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("dyf_op_attention", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    ("dyf_op_attention_dropout", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P]),
    ("dyf_op_attention_mask", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P]),
    ("dyf_op_attention_f32", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P, C.c_int32, _P, _P]),
    ("dyf_op_train_f32", C.c_int, [_P, C.POINTER(TrainOp), C.POINTER(_P), C.POINTER(_P), _P, _P, C.POINTER(_P), C.POINTER(_P), _P]),
    ("dyf_op_sample16", C.c_int, [_P, C.POINTER(SampleOp), C.POINTER(SampleTensors), C.POINTER(_P), _P]),
    ("dyf_criterion", C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P, _P]),
    ("dyf_train_forward", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    ("dyf_train_backward", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P]),
    ("dyf_train_zero_grads", C.c_int, [_P, C.c_int32]),
    ("dyf_train_set_precision", C.c_int, [_P, C.c_int32]),
    ("dyf_train_precision", C.c_int32, [_P]),
    ("dyf_train_set_deterministic", C.c_int, [_P, C.c_int32]),
    ("dyf_train_deterministic", C.c_int32, [_P]),
    ("dyf_set_sample_precision", C.c_int, [_P, C.c_int32]),
    ("dyf_sample_precision", C.c_int32, [_P]),
    ("dyf_set_attention_dropout", C.c_int, [_P, C.c_int32]),
    ("dyf_attention_dropout", C.c_int32, [_P]),
    ("dyf_train_export", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_P)]),
    ("dyf_optim_create", C.c_int, [_P, C.c_int32, C.POINTER(OptimConfig)]),
    ("dyf_optim_destroy", C.c_int, [_P, C.c_int32]),
    ("dyf_optim_step", C.c_int, [_P, C.c_int32, C.c_double, C.c_double, _P]),
    ("dyf_optim_last", C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("dyf_optim_get_step", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64)]),
    ("dyf_optim_set_step", C.c_int, [_P, C.c_int32, C.c_int64]),
    ("dyf_optim_export", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_P), C.c_int32]),
    ("dyf_optim_import", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_P), C.c_int32]),
    ("dyf_optim_swap_ema", C.c_int, [_P, C.c_int32, _P]),
    ("dyf_criterion_grad", C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P, _P]),
    ("dyf_train_conv_check", C.c_int, [_P] + [C.c_int32] * 9 + [C.c_uint32, C.POINTER(C.c_float)]),
    ("dyf_apply_boundary_conditions", C.c_int, [_P, C.POINTER(BcArgs), _P, _P]),
    ("dyf_debug_read_block_output", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("dyf_poll_errors", C.c_int, [_P, C.c_int32]),
    ("dyf_gn_fuse_state", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("dyf_debug_gn_fuse", C.c_int, [_P, C.c_uint32, C.c_int32]),
    ("dyf_debug_form_log", None, [C.c_int32]),
    ("dyf_debug_form_log_read", C.c_int32, [C.c_char_p, C.c_int32]),
    ("dyf_time_named_kernel_in_rollout", C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_double)]),
    ("dyf_debug_set_form", None, [C.c_char_p, C.c_char_p]),
    ("dyf_debug_forms", C.c_int32, [C.c_char_p, C.c_int32]),
]


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: the DYffusion HIP engine has not been built.  Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` from the repository root (needs hipcc).  There is no CPU fallback for the product path.")
    lib = C.CDLL(path)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.dyf_abi_version() != DYF_ABI_VERSION:
        raise ImportError(f"ABI mismatch: library {lib.dyf_abi_version()} vs binding {DYF_ABI_VERSION}")
    return lib


_LIBS = {}


def lib(dtype: str = "bf16") -> C.CDLL:
    """The C-ABI library for `dtype`: "bf16" (and "fp32", "bf16x3") -> libdyffusion_hip.so, "fp16" -> libdyffusion_hip_f16.so."""
    code = DTYPES[storage_dtype(dtype)]
    if code not in _LIBS:
        l = load_library(LIB_PATH_F16 if code else LIB_PATH)
        if l.dyf_dtype() != code:
            raise ImportError(f"library for dtype {dtype} reports dyf_dtype() = {l.dyf_dtype()}")
        for k, v in _FORMS.items():  # switches set before this build of the library was loaded
            l.dyf_debug_set_form(k.encode(), v.encode())
        _LIBS[code] = l
    return _LIBS[code]


_FORMS = {}


def set_form(key=None, value=None) -> None:
    """Test / tool seam (include/dyffusion_hip_testing.h dyf_debug_set_form): set kernel-form switch `key` to `value` in every loaded
    build of the library (and in builds loaded later); value None removes the key, key None removes all.  The product never calls
    this, and the library reads no such switch from the environment."""
    if key is None:
        _FORMS.clear()
    elif value is None:
        _FORMS.pop(key, None)
    else:
        _FORMS[key] = str(value)
    for l in _LIBS.values():
        l.dyf_debug_set_form(None if key is None else key.encode(), None if value is None else str(value).encode())


def forms() -> dict:
    return dict(_FORMS)
