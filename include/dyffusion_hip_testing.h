/*
 * dyffusion_hip_testing.h -- test / benchmark seams of libdyffusion_hip.so.  NOT part of the drop-in boundary
 * (include/dyffusion_hip.h): op-level entry points for the kernel parity tests, per-layer timers for bench.py's roofline
 * object, and activation read-back for per-layer parity analysis.  Same conventions as the public header.
 */
#ifndef DYFFUSION_HIP_TESTING_H
#define DYFFUSION_HIP_TESTING_H

#include "dyffusion_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Time the dominant conv kernel: average HIP-event duration (ms) of the conv layer `layer` (0..11, encoder then
 * decoder blocks) of `net` at batch nb over `iters` launches on `stream`; also returns its 2*MAC count. */
dyf_status dyf_time_conv_layer(dyf_engine* engine, int32_t net, int32_t layer, int32_t nb, int32_t iters,
                               void* stream, double* avg_ms, double* flops, double* algorithmic_bytes);

/* Benchmark introspection: average duration (HIP events on `stream`) of the conv launch of decoder block `layer` (6..11)
 * over ONE eagerly launched rollout of the current plan (all forecaster + interpolator forwards, MC dropout as configured),
 * re-using the inputs of the last dyf_sample call.  `launches` receives the number of launches averaged. */
dyf_status dyf_time_layer_in_rollout(dyf_engine* engine, int32_t layer, int32_t nb, void* stream, double* avg_ms,
                                     int32_t* launches);

/* The same for a ResNet-UNet pair (arch unet.Unet: BASELINE configs[2] OISST, configs[4] 512^2): kind 0 = the 3x3 weight-
 * standardised convs of the full-resolution level with cin == cout == dim (the largest share of an OISST forward), 1 = the
 * bottleneck Attention core (flash kernel), 2 = the GroupNorm(+FiLM+SiLU+dropout(+residual)) chain of the full-resolution level
 * (dim channels; all kernels of one Block's normalisation count as ONE launch).  avg_ms is per launch over nb rows; flops = 2*MAC
 * of one launch (0 for kind 2), algorithmic_bytes = 16-bit operands once each (kind 2: one read + one write of the tensor). */
dyf_status dyf_time_kernel_in_rollout(dyf_engine* engine, int32_t kind, int32_t nb, void* stream, double* avg_ms,
                                      int32_t* launches, double* flops, double* algorithmic_bytes);

/* The HBM-bound kernels (bench.py `hbm_kernels`; north_star: "HBM GB/s for the norm/activation kernels"): over ONE eagerly launched
 * rollout of the current plan at nb rows, HIP events on `stream` around every launch of the kernel called `kernel` --
 * "layernorm_c_vec_kernel", "up2x_quad_kernel", "up2x_epilogue_kernel", "stem16_rows_kernel", "readout_dma_kernel",
 * "up2x_nearest_vec_kernel", "gn_apply_walk_kernel", "gn_apply_part_kernel" (the launchers that open a KernelProf scope, csrc/common.h).
 * total_ms = sum of the launch durations, total_bytes = sum of their ALGORITHMIC bytes (every operand once, 16-bit activations),
 * launches = how many (0: the rollout does not launch that kernel).  GB/s = total_bytes / total_ms / 1e6. */
dyf_status dyf_time_named_kernel_in_rollout(dyf_engine* engine, const char* kernel, int32_t nb, void* stream, double* total_ms,
                                            int32_t* launches, double* total_bytes);

/* ---- op-level seam (tests only): one Conv2d + fused epilogue on NHWC bf16 tensors ---------------------------- */
/* x_dev (N,H,W,Cin) bf16 bits; w (Cout,Cin,kh,kw) host fp32; scale/shift (N,Cout) device fp32 or NULL;
 * y_dev (N,Ho,Wo,Cout) bf16 bits.  act: 0 none, 1 relu, 2 leaky(0.2).  path: 0 direct, 1 MFMA implicit GEMM. */
dyf_status dyf_op_conv2d(dyf_engine* engine, const uint16_t* x_dev, const float* w_host, int32_t n, int32_t h,
                         int32_t w, int32_t cin, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                         const float* scale_dev, const float* shift_dev, int32_t act, int32_t path, uint16_t* y_dev,
                         void* stream);

/* The same seam over the rest of the conv argument block (csrc/conv.h ConvArgs); dyf_op_conv2d is this call with ex = NULL.  A zero /
 * NULL field of `ex` means "absent" and gives dyf_op_conv2d's behaviour.  16-bit tensors are bf16 or fp16 as the engine's build.
 *   x1_dev, c1     second NHWC source (N,H,W,c1), concatenated on channels behind x_dev's `cin`: w_host is (Cout, cin + c1, kh, kw)
 *   residual_dev   16-bit (N,Ho,Wo,Cout), added after activation and dropout
 *   y_f32_dev      fp32 (N,Ho,Wo,Cout) output, instead of y_dev (which may then be NULL) or as well
 *   coef_div       samples per row of scale / shift, which then hold ceil(N / coef_div) rows (0 / 1: one row per sample)
 *   n_sel          batch rows the kernel FORM is chosen for (0: this launch's N)
 *   drop_mode      0 none; 2: mask_dev = uint8 NHWC keep mask of the whole launch; 1: the engine's generator (dyf_seed) at dropout
 *                  site drop_site, forward index drop_forward, global batch rows drop_row_offset .. + N - 1 (N <= 2 max_batch) -- sets
 *                  the engine's forward counter and row offset, and advances the counter by one like a network forward.  Survivors are
 *                  scaled by 1 / (1 - drop_p).
 * act: 0 none, 1 relu, 2 leaky(0.2), 3 SiLU, 4 GELU (erf).  What the argument block cannot express is refused
 * (DYF_ERR_INVALID_ARGUMENT / DYF_ERR_UNSUPPORTED), never truncated. */
typedef struct {
    const uint16_t* x1_dev;
    const uint16_t* residual_dev;
    float* y_f32_dev;
    const uint8_t* mask_dev;
    int32_t c1;
    int32_t coef_div;
    int32_t n_sel;
    int32_t drop_mode;
    float drop_p;
    int32_t drop_site;
    uint32_t drop_row_offset;
    uint32_t drop_forward;
} dyf_conv_ex;
dyf_status dyf_op_conv2d_ex(dyf_engine* engine, const uint16_t* x_dev, const float* w_host, int32_t n, int32_t h,
                            int32_t w, int32_t cin, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                            const float* scale_dev, const float* shift_dev, int32_t act, int32_t path, uint16_t* y_dev,
                            const dyf_conv_ex* ex, void* stream);

/* The 3x3 convs that feed a GroupNorm, through the two entry points a ResnetBlock calls them by (csrc/conv.h): want 0 =
 * launch_conv_gn_fused -- conv + bias -> GroupNorm -> FiLM -> SiLU -> Dropout (-> + residual) in ONE launch (csrc/gn_fused.h), want 1 =
 * launch_conv_stats -- y = conv + bias, 16 bit, and the per-octet (sum, sum of squares) partials its epilogue leaves for GN_ACT.  The
 * seam fills the ConvArgs as the ResNet-UNet forward fills them (3x3, stride 1, pad 1; coef_a = ones, coef_c = bias), uploads the weights
 * with the engine's own upload (every fragment order a layer of this shape gets) and calls the ENTRY POINT, never a form's launcher:
 * form choice, slots per sample and the tile height are the ladder's.  The weights are taken as they are (a caller that wants
 * weight standardisation passes standardised weights, as the weight upload would).
 *   desc      n, h, w, c0, c1 (second source behind the first, 0 = none), cout, groups; act (3 = SiLU, what the forward asks with: any
 *             other value is handed to the ladder, which then fuses nothing); coef_div (samples per FiLM row), n_sel, invariant
 *             (GnFuse::invariant), film_stride (floats per FiLM row, >= cout); dropout fields as dyf_conv_ex's -- mode 2 is handed to the
 *             ladder: the fused forms take no injected mask; conv_tag 1..255 and max_slots (slot stride of `gran`); new_forward != 0 bumps
 *             the epoch word first, as the head of a forward does.  want 1 uses n .. cout and n_sel; every other field must be 0
 *   t         device tensors, 16-bit NHWC: x0 (n,h,w,c0), x1 (n,h,w,c1), residual and y (n,h,w,cout); film_a / film_c fp32
 *             (ceil(n / coef_div) rows of film_stride); mask uint8 (n,h,w,cout) for mode 2.  gran: n * max_slots * (cout / 8) * 2
 *             8-byte granules and epoch: one 32-bit word, both allocated by the CALLER, zeroed once and kept across calls -- the caller
 *             owns the tag protocol (a (forward, conv_tag) pair must not repeat on one buffer); gran_granules = the buffer's capacity.
 *             part (want 1): fp32 [n][slots][cout / 8][2], part_floats = its capacity (the seam refuses a buffer the launch could overrun)
 *   host      weight (cout, c0 + c1, 3, 3), bias, gamma, beta (cout) fp32 (gamma / beta NULL for want 1)
 *   out       fused: 0 = NOTHING was launched (want 1: always 1, the conv ran); slots: GnFuse::slots / the partial-sum slots per sample
 *             (0: the form wrote no statistics); bm: GnFuse::bm (128 / 256 on the implicit-GEMM forms, else 0); slow_sweep: a sweep
 *             needed more than 1 024 passes (the result is still correct)
 * The sweeps' error words are the CALL's own (pinned, mapped, freed on return), never the engine's: a test cannot downgrade a live
 * engine.  A sweep that timed out makes the call fail with DYF_ERR_STATE (its output is NaN-poisoned).  What the descriptor cannot
 * express is refused (DYF_ERR_INVALID_ARGUMENT / DYF_ERR_UNSUPPORTED), never truncated.  Synchronises. */
typedef struct dyf_conv_gn {
    int32_t n, h, w, c0, c1, cout, groups;
    int32_t want, act;
    int32_t coef_div, n_sel, invariant, film_stride;
    int32_t drop_mode;
    float drop_p;
    int32_t drop_site;
    uint32_t drop_row_offset, drop_forward;
    int32_t conv_tag, max_slots, new_forward;
} dyf_conv_gn;
typedef struct dyf_conv_gn_tensors {
    const uint16_t* x0;
    const uint16_t* x1;
    const uint16_t* residual;
    const float* film_a;
    const float* film_c;
    const uint8_t* mask;
    uint16_t* y;
    unsigned long long* gran;
    uint32_t* epoch;
    float* part;
    int64_t gran_granules, part_floats;
} dyf_conv_gn_tensors;
typedef struct dyf_conv_gn_result {
    int32_t fused, slots, bm, slow_sweep;
} dyf_conv_gn_result;
dyf_status dyf_op_conv_gn(dyf_engine* engine, const dyf_conv_gn* desc, const dyf_conv_gn_tensors* t, const float* weight_host,
                          const float* bias_host, const float* gamma_host, const float* beta_host, dyf_conv_gn_result* out, void* stream);

/* Upsample(x2, bilinear, align_corners=False) + Conv2d(3x3, pad 1) + epilogue in one kernel (phase-decomposed MFMA
 * implicit GEMM; unet_simple.py:40-52).  x_dev (N,H,W,Cin) bf16 -> y_dev (N,2H,2W,Cout) bf16. */
dyf_status dyf_op_upconv2d(dyf_engine* engine, const uint16_t* x_dev, const float* w_host, int32_t n, int32_t h,
                           int32_t w, int32_t cin, int32_t cout, const float* scale_dev, const float* shift_dev,
                           int32_t act, uint16_t* y_dev, void* stream);

/* The same fused conv with the argument block of a decoder block of the network forward (csrc/engine.hip net_forward): up2x = 1, the
 * phase-decomposed weights (pack_up2x_weights) and their fragment order (pack_up2x_frag), the engine's split-K workspace and a border
 * scratch of the call's own, pre-filled with 0xFF bytes (fp32 NaN: a ring pixel the border kernel leaves out reaches the output) --
 * through launch_conv, never a form's launcher: the form is the ladder's.  16-bit tensors are bf16 or fp16 as the engine's build.
 *   x_dev (N,H,W,c0), w_host (Cout, c0 + c1, 3, 3), scale / shift (ceil(N / coef_div), Cout) device fp32 or both NULL, act 0..3
 *   ex       dyf_conv_ex: x1_dev / c1 (the skip tensor, behind x_dev's channels), coef_div, n_sel, dropout modes 1 and 2 (mask_dev: uint8
 *            (N,2H,2W,Cout), the DENSE shape also for a sparse launch); residual_dev and y_f32_dev are handed to the ladder as they are
 *   sparse   NULL: every column.  Else needed_host = uint8 [2W], the output columns somebody reads: the seam plans the column lists with
 *            the code the weight upload plans the last decoder block with (same planner order, same switches) and reports the plan:
 *            planned (0: the planner declined, or the sparse form does not take the launch -- the launch is DENSE, as in the engine),
 *            ntiles, npad, mix[3], nvalid0 / nvalid1, wo_store, and col_map_host = int16 [2W] (output column -> column of the compact
 *            tensor, -1 = not stored; written only when planned).  A sparse call takes no residual and no fp32 output.
 *   y_dev    room for (N,2H,2W,Cout); with planned != 0 the launch writes the compact (N,2H,wo_store,Cout) tensor at its start.
 * What the arguments cannot express is refused (DYF_ERR_INVALID_ARGUMENT / DYF_ERR_UNSUPPORTED), never truncated; tensors past the
 * kernels' 32-bit element indices are refused.  Synchronises and frees what it allocated. */
typedef struct dyf_upconv_sparse {
    const uint8_t* needed_host;
    int16_t* col_map_host;
    int32_t planned, ntiles, npad, nvalid0, nvalid1, wo_store;
    int32_t mix[3];
} dyf_upconv_sparse;
dyf_status dyf_op_upconv2d_ex(dyf_engine* engine, const uint16_t* x_dev, const float* w_host, int32_t n, int32_t h, int32_t w,
                              int32_t c0, int32_t cout, const float* scale_dev, const float* shift_dev, int32_t act, uint16_t* y_dev,
                              const dyf_conv_ex* ex, dyf_upconv_sparse* sparse, void* stream);

/* LinearAttention core (attention.py:28-49, 4 heads of 32 channels): qkv_dev (N,HW,384) bf16 = to_qkv output ->
 * out_dev (N,HW,128) bf16 = softmax_d(q)*scale . (softmax_n(k) . v^T / HW), the input of to_out.  Runs the pixel-parallel
 * MFMA kernels the ResNet-UNet uses. */
dyf_status dyf_op_linear_attention(dyf_engine* engine, const uint16_t* qkv_dev, int32_t n, int32_t hw, uint16_t* out_dev,
                                   void* stream);

/* The fused LinearAttention block the ResNet-UNet runs for dim 64 / 128 (csrc/unet_kernels.hip linattn_fused_*): xn_dev
 * (N,HW,C) 16-bit = the PreNorm LayerNorm output, xres_dev (N,HW,C) = the block input (residual); wqkv_host (384,C),
 * wout_host (C,128), bout_host (C) fp32 = to_qkv / to_out parameters -> y_dev (N,HW,C) = to_out(core(to_qkv(xn))) + xres.
 * The to_qkv and core outputs are never written to memory. */
dyf_status dyf_op_linear_attention_fused(dyf_engine* engine, const uint16_t* xn_dev, const uint16_t* xres_dev, int32_t n,
                                         int32_t hw, int32_t c, const float* wqkv_host, const float* wout_host,
                                         const float* bout_host, uint16_t* y_dev, void* stream);

/* Attention core (attention.py:62-72, 4 heads of 32 channels, no dropout): qkv_dev (N,HW,384) 16-bit = to_qkv output ->
 * out_dev (N,HW,128) = softmax_j(q_i . k_j / sqrt(32)) . v_j, the input of to_out.  Runs the MFMA flash kernel the bottleneck
 * of the ResNet-UNet uses (HW up to 65 535: 16 384 tokens for the 512^2 synthetic configuration). */
dyf_status dyf_op_attention(dyf_engine* engine, const uint16_t* qkv_dev, int32_t n, int32_t hw, uint16_t* out_dev,
                            void* stream);
/* ... with nn.Dropout(p) on the softmax probabilities (attention.py:70), masks from the engine's generator: the form the
 * interpolator's bottleneck runs under MC dropout (n <= 2 max_batch rows).  Follows the engine's dyf_set_attention_dropout mode; in
 * the exact mode more than 32 767 tokens are refused with DYF_ERR_UNSUPPORTED before anything is launched. */
dyf_status dyf_op_attention_dropout(dyf_engine* engine, const uint16_t* qkv_dev, int32_t n, int32_t hw, float p, uint16_t* out_dev,
                                    void* stream);
/* ... with the CALLER's keep mask (DropSpec mode 2, what dyf_net_forward's dropout_mode 2 hands the bottleneck): mask_dev
 * (N,4,HW,HW) uint8, nonzero = keep, indexed ((row * 4 + head) * HW + query) * HW + key; survivors scaled by 1 / (1 - p), 0 < p < 1.
 * The engine's generator and its attention-dropout mode are not involved.  What the call cannot express is refused with
 * DYF_ERR_INVALID_ARGUMENT: a missing mask (the generator's masks: dyf_op_attention_dropout) and p outside (0, 1) (p = 0 is the
 * dropout-free core: dyf_op_attention).  A mask of more than 2^32 - 1 bytes is DYF_ERR_UNSUPPORTED. */
dyf_status dyf_op_attention_mask(dyf_engine* engine, const uint16_t* qkv_dev, int32_t n, int32_t hw, float p, const uint8_t* mask_dev,
                                 uint16_t* out_dev, void* stream);
/* The fp32 Attention core of fp32 sampling and the training step: qkv_dev (N,HW,384) fp32 -> out_dev (N,HW,128) fp32.  form 0: the
 * kernel that keeps its (tokens x tokens) probabilities, in scratch memory here (HW <= 4096, else DYF_ERR_UNSUPPORTED); form 1: the
 * streaming matrix-core kernel a sampling forward takes past 4096 tokens, at any HW <= 32 767.  p > 0 with mask_dev == NULL: dropout
 * on the probabilities from the engine's generator, armed as dyf_op_attention_dropout arms it; mask_dev (N,4,HW,HW) uint8: the
 * caller's keep mask, survivors scaled by 1 / (1 - p). */
dyf_status dyf_op_attention_f32(dyf_engine* engine, const float* qkv_dev, int32_t n, int32_t hw, float p, const uint8_t* mask_dev,
                                int32_t form, float* out_dev, void* stream);

/* One training convolution (csrc/train_gemm.hip: fp32 matrix-core forward / dgrad / wgrad of nn.Conv2d on NHWC fp32 tensors) on
 * hash-random data against the plain VALU kernel of csrc/train.hip.  kind 0 forward, 1 data gradient, 2 weight gradient (the
 * matrix-core launchers of train_gemm.hip / train_halo16.hip), 3 weight gradient and 4 forward through the step's own dispatchers
 * (conv_wgrad / conv_fwd: reaches the small-channel forms); with 16-bit operands selected the inputs are rounded to 16 bit first; geometry
 * as nn.Conv2d(cin, cout, k, stride s, padding p) on (n, h, w).  out_host[0] = max |mfma - valu| / max |valu| with the split-K
 * workspace, [1] = the same for the unsplit launch, [2] = 1 if the matrix-core form took the shape. */
dyf_status dyf_train_conv_check(dyf_engine* engine, int32_t kind, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                int32_t k, int32_t s, int32_t p, uint32_t seed, float* out_host);

/* ONE recorded op of the training step of either backbone (csrc/train_resnet.inc RCtx) and its adjoint, for float64 parity tests of the
 * fp32 kernels.  The seam calls the RCtx member function itself on a scratch tape and then runs the recorded closures in reverse with
 * the loop dyf_train_backward runs, so grid sizes, chunk counts and kernel choices are the training step's own.  Convs take their
 * operand precision from dyf_train_set_precision like the step does.  Tensors are fp32, activations NHWC.
 *   inputs_dev   device pointers of the op's inputs, dout_dev the gradient of its output, y_dev receives the output, dinputs_dev[i]
 *                the gradient of input i (entries may be NULL; a time input has no gradient)
 *   params_host  host pointers of the parameters in PyTorch layouts (packed by the code dyf_load_weights packs the training copy with)
 *   dparams_host host pointers, IN/OUT: the gradient buffers start from these contents and the kernels accumulate into them (as the
 *                two forecaster passes of a step meet in one buffer); conv weights in PyTorch layout through dyf_train_export's unpack
 * op (inputs; parameters), hw = h * w:
 *   CONV        x (nb,h,w,c); weight (c2,c,k,k) [, bias (c2) with DYF_TOP_BIAS] -> (nb,ho,wo,c2); DYF_TOP_WS = weight-standardised
 *               DYF_TOP_SAMPLE: the forward alone, launched the way a sampling forward launches it -- operand precision from
 *               dyf_sample_precision (48: bf16x3; 16 and 32: fp32 operands), the default kernel forms, the sampling-forward scope of
 *               csrc/train_internal.h set (the forms only sampling takes); no adjoint runs and no gradient is written.  Every other op
 *               refuses the flag (DYF_ERR_UNSUPPORTED)
 *   GN_ACT      z (nb,hw,c) [, ss (nb,2c) = FiLM (scale | shift) with DYF_TOP_FILM]; weight (c), bias (c); `groups`; dropout p
 *   LAYERNORM   x (nb,hw,c); g (1,c,1,1); dropout p
 *   LINATTN     qkv (nb,hw,384) -> (nb,hw,128)
 *   ATTENTION   qkv (nb,hw,384) -> (nb,hw,128), the form that keeps its probabilities (hw <= 4096); dropout p on the probabilities
 *   ATTENTION_STREAM the same op, always in the streaming form a recorded forward takes past 4096 tokens (t_at_stream_fwd keeping the
 *               softmax statistics, t_at_stream_bwd_dq / _dkv recomputing the scores per tile), at any hw <= 32 767; dropout p
 *   LINEAR      x (nb,c); weight (c2,c), bias (c2) -> (nb,c2); DYF_TOP_PRE = SiLU on the input first
 *   LEARNED_SINU time (nb); weights (c) -> (nb, 2c + 1)
 *   DROPOUT     x (nb,h,w,c); p          GELU  x (nb,h,w,c)
 *   ADD         a, b (nb,h,w,c); DYF_TOP_SAME = add(a, a): one input, one gradient
 *   CAT         a (nb,h,w,c), b (nb,h,w,c2) -> (nb,h,w,c+c2)          UP2_NEAREST x (nb,h,w,c) -> (nb,2h,2w,c)
 *   NORM_ACT    unet_simple's UNetBlock norm: GN_ACT's inputs; weight (c), bias (c) and, with groups = 0 (BatchNorm2d), running_mean (c),
 *               running_var (c), whose dparams entries RECEIVE the statistics as the forward left them.  groups > 0: GroupNorm; groups = 0:
 *               batch statistics (running statistics updated, momentum 0.1), DYF_TOP_RUNNING: normalise by the running statistics.  SiLU, or
 *               DYF_TOP_LEAKY (slope 0.2) / DYF_TOP_RELU; dropout p from the generator, or with DYF_TOP_MASK from a uint8 keep mask (nb,h,w,c)
 *               that follows the inputs in inputs_dev -- the sampling path's injected masks: the forward alone runs, no gradient is written.
 *               Sum kernels on unet_simple's grid (GN_ACT: the ResNet-UNet's).  SimpleConvNet's block: DYF_TOP_ACT_GELU = exact (erf) GELU as the
 *               activation; DYF_TOP_RESIDUAL = one more input r (nb,h,w,c) behind the FiLM (in front of a mask), y = keep * act(..) + r in the
 *               same launch, and one more returned gradient (dinputs_dev entry of r)
 *   UP2_BILINEAR x (nb,h,w,c) [, x2 (nb,h,w,c2): the upsample of cat([x, x2]) without the concat] -> (nb,2h,2w,c+c2), bilinear
 *               align_corners=False; DYF_TOP_GRAD_IN: dinputs_dev[1] is IN/OUT, the gradient x2 already has from another consumer
 *   RESIZE      x (nb,h,w,c) -> (nb,k,stride,c): F.interpolate(size=(k, stride)), bilinear align_corners=False or DYF_TOP_NEAREST
 *   CONVT       x (nb,h,w,c); weight (c,c2,4,4), bias (c2) -> (nb,2h,2w,c2): ConvTranspose2d(c, c2, 4, stride 2, padding 1)
 * p > 0 draws from the engine's generator armed as dyf_op_attention_f32 arms it: a new forward (dyf_seed resets the counter), site 0,
 * global rows row offset .. + nb - 1, nb <= 2 max_batch; element index = the NHWC index inside the row ((h * N + i) * N + j for the
 * Attention probabilities).  Fields an op does not use must be 0.  What the descriptor cannot express is refused
 * (DYF_ERR_INVALID_ARGUMENT / DYF_ERR_UNSUPPORTED), never truncated.  Synchronises; everything allocated goes back to the engine. */
typedef enum dyf_train_op_kind {
    DYF_TOP_CONV = 0, DYF_TOP_GN_ACT = 1, DYF_TOP_LAYERNORM = 2, DYF_TOP_LINATTN = 3, DYF_TOP_ATTENTION = 4, DYF_TOP_LINEAR = 5,
    DYF_TOP_LEARNED_SINU = 6, DYF_TOP_DROPOUT = 7, DYF_TOP_GELU = 8, DYF_TOP_ADD = 9, DYF_TOP_CAT = 10, DYF_TOP_UP2_NEAREST = 11,
    DYF_TOP_NORM_ACT = 12, DYF_TOP_UP2_BILINEAR = 13, DYF_TOP_RESIZE = 14, DYF_TOP_CONVT = 15, DYF_TOP_ATTENTION_STREAM = 16
} dyf_train_op_kind;
#define DYF_TOP_WS 1
#define DYF_TOP_BIAS 2
#define DYF_TOP_PRE 4
#define DYF_TOP_FILM 8
#define DYF_TOP_SAME 16
#define DYF_TOP_RUNNING 32
#define DYF_TOP_MASK 64
#define DYF_TOP_LEAKY 128
#define DYF_TOP_RELU 256
#define DYF_TOP_NEAREST 512
#define DYF_TOP_GRAD_IN 1024
#define DYF_TOP_ACT_GELU 2048
#define DYF_TOP_RESIDUAL 4096
#define DYF_TOP_SAMPLE 8192
typedef struct dyf_train_op {
    int32_t op, nb, h, w, c, c2, k, stride, pad, groups, flags;
    float p;
} dyf_train_op;
dyf_status dyf_op_train_f32(dyf_engine* engine, const dyf_train_op* desc, const float* const* inputs_dev, const float* const* params_host,
                            const float* dout_dev, float* y_dev, float* const* dinputs_dev, float* const* dparams_host, void* stream);

/* ONE 16-bit sampling kernel between the convs (csrc/unet_kernels.hip, csrc/kernels.hip), for float64 parity tests.  The seam fills the
 * launcher's own argument struct and calls the LAUNCHER, never a kernel: form choice, grid sizes and the DYF_* form switches are the
 * engine's.  Scratch is provided as a forward provides it (GnActArgs::stats: gn_stats_doubles(nb, groups) doubles).  hw = h * w.
 *   desc        op kind, geometry, flags; fields an op does not use must be 0
 *   t           device pointers.  16-bit tensors are bit patterns of the build's element type (bf16 or fp16), NHWC; a NULL entry = absent
 *   params_host host pointers of the parameters, fp32, PyTorch layouts
 * op (tensors; parameters):
 *   GN_ACT        launch_gn_act: x[0] 16-bit (nb,hw,c); gamma (c), beta (c); `groups`; act 0..3.  Optional: film_a / film_c fp32 rows of
 *                 film_stride >= c floats per sample (y * film_a + film_c); residual 16-bit (nb,hw,c), added after the dropout; part fp32
 *                 [nb][part_slots][c / 8][2] = the (sum, sum of squares) partials a conv epilogue leaves per 8-channel octet, in place of
 *                 a statistics pass (shapes gn_part_supported rejects: DYF_ERR_UNSUPPORTED); DYF_SOP_NO_STATS: GnActArgs::stats = NULL
 *                 (reaches gn_act_kernel, or gn_apply_part_kernel at any slot count); dropout
 *   LAYERNORM_C   launch_layernorm_c: x[0] 16-bit (nb,hw,c); g (c); dropout
 *   HEAD          launch_head: x[0] 16-bit (nb,hw,c); weight (c2,c), bias (c2) -> y fp32 NCHW (nb,c2,h,w)
 *   UP2_NEAREST   launch_up2x_nearest: x[0] 16-bit (nb,h,w,c) -> (nb,2h,2w,c)
 *   DROP16        launch_drop16: x[0] 16-bit (nb,h,w,c), h * w * c even; dropout
 *   STEM_CONV     launch_stem_conv: x[0..nsrc-1] fp32 NCHW (nb,ch[i],h,w), c = sum of ch; weight (c2,c,k,k), bias (c2), packed by the code
 *                 the weight upload uses (pack_stem_frag included when stem_frag_steps takes the shape); taps reach from -pad to k-1-pad
 *                 -> y 16-bit (nb,h,w,c2)
 *   GROUPNORM_F32 launch_groupnorm: x[0] fp32 (nb,hw,c); gamma, beta; `groups`; act 0..4; film rows as GN_ACT with film_div samples per
 *                 row (absent: ones / zeros); dropout -> y 16-bit
 *   UP2_BILINEAR  launch_up2x: x[0] 16-bit (nb,h,w,c) [, x[1] (nb,h,w,c2): the upsample of the concatenation] -> (nb,2h,2w,c+c2)
 *   UP2_EPILOGUE  launch_up2x_epilogue: x[0] fp32 (nb,h,w,c), c % 4 == 0; film_a / film_c = the coefficient rows (stride film_stride,
 *                 film_div samples per row); act 0..3; dropout -> y 16-bit (nb,2h,2w,c) = drop(act(lerp(x) * a + c))
 * The launchers around the networks (csrc/kernels.hip), same rules; x[0] may be NULL where an op lists no input:
 *   READOUT       launch_readout: x[0] 16-bit (nb,h,iw_store,c) = the decoder output on the (h, w) grid; weight (c,c2,4,4), bias (c2),
 *                 packed by the code the weight upload uses (pack_readout_weights, and pack_readout_frag + the tap tables of
 *                 launch_readout_tables exactly when the upload builds them: c == 64, c2 <= 4); (oh, ow) = the native grid; `nearest`;
 *                 iw_store / col_map: compact columns (col_map device int16 [w]: column -> stored column, -1 = not stored), both or
 *                 neither; DYF_SOP_NO_TABLES: launch without the tap tables -> y fp32 NCHW (nb,c2,oh,ow)
 *   READOUT_TABLES launch_readout_tables for (h, w) -> (oh, ow), `nearest`, iw_store / col_map -> y = row_tab (oh entries of 8 words:
 *                 four byte offsets, four weights), y2 = col_tab (ow entries)
 *   STEM          launch_stem: x[0..nsrc-1] fp32 NCHW (src_rows or nb, ch[i], h, w), c = sum of ch, resampled to (oh, ow) (`nearest` or
 *                 bilinear; oh == h and ow == w: identity); weight (c2,c), bias (c2); src_rows: rows the sources hold (0: nb), output row
 *                 r reads source row r % src_rows; dropout as below -> y 16-bit (nb,oh,ow,c2)
 *   STEM16        launch_stem16, c <= 15, no parameters -> y 16-bit (nb,oh+2,ow+2,16); DYF_SOP_FOLD_RNG: the start of a forward folded
 *                 into the launch (StemArgs::rng_state / rng_row_keys of the engine, nb <= 2 max_batch rows, src_rows or nb rows per
 *                 forward) -> y2 = the row-key table (2 nb words), y3 = the generator state (DYF_RNG_STATE_WORDS words) afterwards;
 *                 DYF_SOP_PAIR_ONCE (src_rows > 0): StemArgs::distinct_only -> y holds the src_rows distinct rows only;
 *                 DYF_SOP_STEM_PITCH8 (c <= 8): StemArgs::out_pitch = 8 -> y 16-bit (rows,oh+2,ow+2,8), no bias slot
 *   RNG_BEGIN    launch_rng_begin_forward over nb rows, src_rows (0: nb) rows per forward, from forward index drop_forward and row
 *                 offset drop_row_offset (set as generator dropout sets them) -> y = the row-key table, y2 = the state afterwards
 *   RNG_CLONE     launch_rng_clone: x[0] = source state, y = destination state (IN/OUT), DYF_RNG_STATE_WORDS device words each; row_add =
 *                 drop_row_offset; DYF_SOP_COUNTERS_ONLY
 *   TIME_MLP      launch_time_mlp: x[0] fp32 (nb) times; c = dim; w1 (2c, c or 2 c2 + 1), b1, w2 (2c,2c), b2 [, learned weights (c2): c2 =
 *                 learned_half > 0] -> y fp32 (nb, 2c)
 *   FILM          launch_film: x[0] fp32 (nb, c) SiLU rows or NULL (no time embedding); nsrc blocks of ch[i] channels, total = their sum;
 *                 wf (2 total, c), bf (2 total), norm_a (total), norm_c (total); block tables built as the weight upload builds them
 *                 -> y = coef_a, y2 = coef_c, fp32 (nb, total)
 *   COLD_UPDATE   launch_cold_update over nb * h * w * c floats: y = x_s (IN/OUT), x[0] = x_cur, x[1] = x_next, y2 = copy or NULL
 *   NOISY_CONDITION launch_noisy_condition over nb rows of h * w * c floats: x[0] = cond, x[1] = noise or NULL (the engine's generator:
 *                 rows drop_row_offset .., the NEXT field of the stream -- dyf_seed resets the noise-call counter); `tau` -> y
 * Dropout (ops that end in one): drop_mode 2 = mask, a uint8 keep mask of the output's shape; 1 = the engine's generator at site
 * drop_site, forward index drop_forward, global rows drop_row_offset .. + nb - 1 (nb <= 2 max_batch), armed by the code dyf_conv_ex's
 * fields are armed by.  Survivors are scaled by 1 / (1 - drop_p).  Every tensor must stay below the kernels' 32-bit element indices.
 * What the descriptor cannot express is refused (DYF_ERR_INVALID_ARGUMENT / DYF_ERR_UNSUPPORTED), never truncated.  Synchronises;
 * everything allocated goes back to the engine. */
typedef enum dyf_sample_op_kind {
    DYF_SOP_GN_ACT = 0, DYF_SOP_LAYERNORM_C = 1, DYF_SOP_HEAD = 2, DYF_SOP_UP2_NEAREST = 3, DYF_SOP_DROP16 = 4, DYF_SOP_STEM_CONV = 5,
    DYF_SOP_GROUPNORM_F32 = 6, DYF_SOP_UP2_BILINEAR = 7, DYF_SOP_UP2_EPILOGUE = 8, DYF_SOP_READOUT = 9, DYF_SOP_READOUT_TABLES = 10,
    DYF_SOP_STEM = 11, DYF_SOP_STEM16 = 12, DYF_SOP_RNG_BEGIN = 13, DYF_SOP_RNG_CLONE = 14, DYF_SOP_TIME_MLP = 15, DYF_SOP_FILM = 16,
    DYF_SOP_COLD_UPDATE = 17, DYF_SOP_NOISY_CONDITION = 18
} dyf_sample_op_kind;
#define DYF_SOP_NO_STATS 1
#define DYF_SOP_NO_TABLES 2
#define DYF_SOP_FOLD_RNG 4
#define DYF_SOP_COUNTERS_ONLY 8
#define DYF_SOP_PAIR_ONCE 16
#define DYF_SOP_STEM_PITCH8 32
typedef struct dyf_sample_op {
    int32_t op, nb, h, w, c, c2, k, pad, groups, act, flags;
    int32_t film_stride, film_div, part_slots;
    int32_t nsrc, ch[4];
    int32_t drop_mode;
    float drop_p;
    int32_t drop_site;
    uint32_t drop_row_offset, drop_forward;
    int32_t oh, ow, nearest, src_rows, iw_store;
    float tau;
} dyf_sample_op;
typedef struct dyf_sample_tensors {
    const void* x[4];
    const uint16_t* residual;
    const float* film_a;
    const float* film_c;
    const float* part;
    const uint8_t* mask;
    void* y;
    const int16_t* col_map;
    void* y2;
    void* y3;
} dyf_sample_tensors;
dyf_status dyf_op_sample16(dyf_engine* engine, const dyf_sample_op* desc, const dyf_sample_tensors* t, const float* const* params_host,
                           void* stream);

/* Read back the output of UNetBlock `layer` (0..11: encoder then decoder blocks) of the most recent unet_simple forward
 * as fp32 NCHW (NB, cout, h, w) -- per-layer parity analysis against the oracle's taps (oracle/nets.py `taps=`).  The last
 * decoder block is returned dense; positions its sparse-column form did not compute are NaN. */
dyf_status dyf_debug_read_block_output(dyf_engine* engine, int32_t net, int32_t layer, int32_t nb, float* out_dev,
                                       void* stream);

/* Fused GroupNorm (csrc/gn_fused.h) failure drill: timeout_ticks = bound of a granule sweep in 100 MHz ticks (0 = the default, 2 s);
 * force_timeout != 0 makes every sweep wait for a tag nobody publishes, i.e. behave as if a workgroup of its sample never arrived.
 * Drops the captured graphs (both values travel as kernel arguments) after waiting for the device. */
dyf_status dyf_debug_gn_fuse(dyf_engine* engine, uint32_t timeout_ticks, int32_t force_timeout);

/* Kernel-form log: which kernel FORM every launcher took (conv_halo_rows_kernel<0/1/2>, conv_up_halo_kernel<3/4/5>,
 * conv_igemm2_kernel<1/2>, conv_igemm_kernel<..>(+splitk), conv_enc0_stem_kernel, stem16_rows_kernel, up2x_quad_kernel,
 * readout_dma_kernel, ...) and for how many batch rows.  Forms are chosen per launch from tile counts (csrc/conv_dispatch.hip
 * conv_choose_form), so a parity test at NB = 1 does not exercise the kernels a NB = 80 benchmark runs: tests enable the log, run the
 * engine (a hipGraph capture notes its launches once; replays launch nothing on the host) and assert the forms.  Process-wide.
 * dyf_debug_form_log(1) clears and enables, (0) disables; dyf_debug_form_log_read writes "form@rows=count;..." (sorted by name),
 * NUL-terminated and truncated to cap bytes, and returns the untruncated length. */
void dyf_debug_form_log(int32_t enable);
int32_t dyf_debug_form_log_read(char* buf, int32_t cap);

/* Kernel-form switches (tests/ and tools/ only).  The launchers choose between equivalent kernel forms from tile counts; the
 * parity tests force each form on small problems, the A/B tools flip one form at a time.  This call is the ONLY way to set them:
 * libdyffusion_hip.so reads none of them from the environment (the only environment variables it reads are DYF_VERBOSE -- print
 * the engine's form policy at creation -- and DYF_RCCL_LIB -- the librccl to dlopen).  Process-wide (per library: the bf16 and the fp16 build each hold their own table); read per launch / per engine
 * creation / per weight upload as DESIGN.md 7.1 lists.  key = the historic switch name ("DYF_IGEMM2_MIN_TILES", ...), value = its
 * text; value NULL removes the key, key NULL removes every key.  dyf_debug_forms writes "key=value;..." like
 * dyf_debug_form_log_read. */
void dyf_debug_set_form(const char* key, const char* value);
int32_t dyf_debug_forms(char* buf, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* DYFFUSION_HIP_TESTING_H */
