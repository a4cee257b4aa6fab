/*
 * dyffusion_hip.h -- C ABI of libdyffusion_hip.so: the MI355X (gfx950) DYffusion sampling engine.
 *
 * Drop-in boundary for the reference's hot path (all paths relative to the upstream repo root):
 *   - per-network seam   BaseModel.forward(inputs, time, condition)        src/models/unet_simple.py:181-197
 *   - sampler seam       DYffusion.sample(initial_condition, static_condition=..., num_predictions=N)
 *                                                                          src/diffusion/dyffusion.py:335-431
 *     reached from BaseDiffusion.predict_forward (src/diffusion/_base_diffusion.py:48-68) and
 *     BaseExperiment.predict (src/experiment_types/_base_experiment.py:315-356).
 *
 * Conventions
 *   - plain C types only; every pointer named *_dev is DEVICE memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()), everything else is HOST memory.  Tensors crossing the ABI are fp32, NCHW, contiguous -- the
 *     reference's layout.  Internally the engine keeps activations NHWC in a 16-bit format (bf16, or fp16 in the
 *     libdyffusion_hip_f16.so build) and accumulates in fp32; dyf_set_sample_precision(32) switches an engine to fp32 activations
 *     and weights (reference-precision rollouts, ABI 9).
 *   - the engine owns packed device weights, its workspace arena and captured hipGraphs; no allocation happens
 *     inside dyf_sample / dyf_net_forward after the first call for a given batch size.
 *   - one engine per (device, stream); calls on one engine are not re-entrant.
 *   - every function returns a dyf_status; dyf_last_error(engine) (or NULL for create-time failures) returns a
 *     message.  The Python shim re-raises ValueError / AssertionError / RuntimeError from these.
 *   - `stream` arguments are hipStream_t passed as void* (0 = the null stream).
 */
#ifndef DYFFUSION_HIP_H
#define DYFFUSION_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYF_ABI_VERSION 9

typedef struct dyf_engine dyf_engine;

typedef enum dyf_status {
    DYF_OK = 0,
    DYF_ERR_INVALID_ARGUMENT = 1, /* maps to ValueError / AssertionError in the shim */
    DYF_ERR_UNSUPPORTED = 2,      /* valid in the reference, not implemented by this engine (NotImplementedError) */
    DYF_ERR_HIP = 3,              /* a HIP runtime call failed (RuntimeError) */
    DYF_ERR_STATE = 4             /* call order violated, e.g. sampling before weights / plan are set */
} dyf_status;

/* Which network of the DYffusion pair a call refers to (dyffusion.py:448-468: self.model / self.interpolator). */
typedef enum dyf_net_id { DYF_NET_FORECASTER = 0, DYF_NET_INTERPOLATOR = 1 } dyf_net_id;

/* Backbone architectures (src/models/). */
typedef enum dyf_arch {
    DYF_ARCH_UNET_SIMPLE = 0, /* src/models/unet_simple.py:85-197 (Navier-Stokes / spring-mesh backbone) */
    DYF_ARCH_UNET_RESNET = 1, /* src/models/unet.py:112-315 (OISST / synthetic backbone: ResnetBlocks + attention) */
    DYF_ARCH_SIMPLE_CONV_NET = 2 /* src/models/simple_conv_net.py:58-131 (spring-mesh backbone); kernel_sizes travel in
                                  * n_mults / dim_mults, dropout in `dropout` */
} dyf_arch;

/* Hyper-parameters of one backbone: the kwargs of unet_simple.UNet.__init__ (unet_simple.py:86-95) plus the
 * channel bookkeeping of BaseModel (src/models/_base_model.py:43-66). */
typedef struct dyf_net_config {
    int32_t arch;             /* dyf_arch */
    int32_t in_channels;      /* num_input_channels (without the conditional channels) */
    int32_t cond_channels;    /* num_conditional_channels */
    int32_t out_channels;     /* num_output_channels */
    int32_t dim;              /* base width */
    int32_t with_time_emb;    /* 0/1 */
    int32_t upsample_h;       /* upsample_dims[0], 0 = no outer resampling */
    int32_t upsample_w;
    float dropout;            /* unet_simple: UNetBlock dropout p; unet: block_dropout (2nd Block of a ResnetBlock) */
    float input_dropout;      /* Dropout on init_conv's output: unet_simple.py:116,168 (one site, the first of a forward; the engine then
                               * runs the un-fused stem), unet.py:162-163,276-277 (two sites: residual copy, input); 0 in every shipped config */
    /* ---- unet.Unet only (kwargs of Unet.__init__, src/models/unet.py:113-135) ---- */
    int32_t n_mults;          /* len(dim_mults), <= 6 */
    int32_t dim_mults[6];
    float block_dropout1;     /* 1st Block of a ResnetBlock */
    float attn_dropout;       /* LinearAttention input dropout / Attention probability dropout */
    int32_t groups;           /* resnet_block_groups */
    int32_t init_kernel_size; /* 7 */
    int32_t init_padding;     /* 3 */
    int32_t outer_nearest;    /* unet_simple outer_sample_mode: 0 "bilinear", 1 "nearest" (upsampler + final F.interpolate,
                               * unet_simple.py:103,195) */
    /* ---- unet.Unet options no shipped config sets (unet.py:127-135); 0 = the shipped default ---- */
    int32_t keep_spatial_dims;      /* 1: no down / up sampling, plain 3x3 convs between the levels (unet.py:190,214) */
    int32_t single_conv_layer;      /* 1: double_conv_layer=False, a ResnetBlock's second Block is nn.Identity (unet.py:94) */
    int32_t learned_sinusoidal_dim; /* > 0: learned_sinusoidal_cond=True with this (even) dim: time features
                                     * [t, sin(2 pi t w), cos(2 pi t w)] with the parameter time_emb_mlp.0.weights (misc.py:35-59) */
} dyf_net_config;

typedef enum dyf_dtype_id { DYF_DTYPE_BF16 = 0, DYF_DTYPE_F16 = 1 } dyf_dtype_id;

typedef struct dyf_engine_config {
    int32_t abi_version;      /* DYF_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    int32_t height, width;    /* native grid (e.g. 221 x 42) */
    int32_t max_batch;        /* largest NB = N_ensemble * B the workspace is sized for */
    int32_t use_graph;        /* capture the rollout in a hipGraph (dyf_sample) */
    int32_t enable_mfma;      /* 1: implicit-GEMM MFMA conv where shapes allow; 0: direct conv everywhere (debug) */
    int32_t dtype;            /* dyf_dtype of activations / weights in HBM and of the MFMA operands; must equal dyf_dtype() of
                               * the library: libdyffusion_hip.so is the bf16 build, libdyffusion_hip_f16.so the fp16 build of the
                               * same sources (-DDYF_F16=1), same ABI */
    int32_t batch_invariant;  /* 1: the kernel form of every layer (implicit-GEMM variant, split-K factor, halo forms) is chosen for
                               * 2 * max_batch rows whatever the batch of a call, so a row's result is bit-identical under any
                               * batching / sharding served by engines of equal max_batch; 0: chosen per call (fastest) */
    dyf_net_config net[2];    /* indexed by dyf_net_id */
} dyf_engine_config;

/* One iteration of the sampling loop, resolved on the host (dyffusion.py:352-397). */
typedef struct dyf_plan_step {
    float forecaster_time;    /* enc(s): value fed to the forecaster's time embedding */
    float tau;                /* s/(T-1), used by forward_conditioning="data+noise" */
    float i_next;             /* interpolation time of s_next, < 0: none (x_next = x0_hat) */
    float i_cur;              /* interpolation time of s,      < 0: none (x_cur  = x_s)    */
    int32_t is_last;          /* s == T-1 */
    int32_t out_slot;         /* index into the forecast stack written after this step, -1: none */
} dyf_plan_step;

typedef enum dyf_fcond { DYF_FCOND_NONE = 0, DYF_FCOND_DATA = 1, DYF_FCOND_DATA_NOISE = 2 } dyf_fcond;

typedef struct dyf_plan {
    int32_t n_steps;
    const dyf_plan_step* steps;
    int32_t sampling_cold;            /* 1 = "cold", 0 = "naive" (dyffusion.py:381-391) */
    int32_t cold_for_last_step;       /* use_cold_sampling_for_last_step */
    int32_t forward_conditioning;     /* dyf_fcond */
    int32_t n_refine;                 /* refinement pass (dyffusion.py:408-422): number of re-predicted times */
    const float* refine_times;        /* [n_refine] interpolation times */
    const int32_t* refine_slots;      /* [n_refine] forecast-stack slots they overwrite */
    int32_t n_out_slots;              /* h: number of (NB,C,H,W) fields in the forecast stack */
    int32_t interpolator_dropout;     /* MC dropout active in the interpolator (enable_interpolator_dropout) */
    int32_t forecaster_dropout;       /* dropout active in the forecaster (module.enable_inference_dropout) */
} dyf_plan;

/* ---- lifetime ------------------------------------------------------------------------------------------ */
dyf_status dyf_engine_create(const dyf_engine_config* cfg, dyf_engine** out_engine);
void dyf_engine_destroy(dyf_engine* engine);
const char* dyf_last_error(const dyf_engine* engine);
int32_t dyf_abi_version(void);
int32_t dyf_dtype(void);   /* dyf_dtype_id this library was built for */

/* ---- weights: the reference's state_dict (names as in UNet.state_dict(), host fp32, contiguous) ---------- */
/* Replaces BaseExperiment.instantiate_model / load_state_dict (_base_experiment.py:173-199).  Folds eval-mode
 * BatchNorm into per-channel scale/shift, repacks conv weights to the MFMA layout and uploads as bf16. */
dyf_status dyf_load_weights(dyf_engine* engine, int32_t net, int32_t n_tensors, const char* const* names,
                            const float* const* data, const int64_t* const* shapes, const int32_t* ndims);

/* ---- per-network seam: BaseModel.forward(inputs, time, condition) (unet_simple.py:181-197) ------------------ */
/* inputs_dev (NB,in_channels,H,W), time_dev (NB) or NULL when with_time_emb == 0, condition_dev
 * (NB,cond_channels,H,W) or NULL, out_dev (NB,out_channels,H,W).  dropout_mode: 0 off (eval), 1 on (engine RNG),
 * 2 on with injected keep-masks: masks_dev[l] is the uint8 keep-mask of the l-th dropout site with p > 0 in
 * execution order (NHWC for activations, (NB,heads,N,N) for attention probabilities), used by the parity tests. */
dyf_status dyf_net_forward(dyf_engine* engine, int32_t net, const float* inputs_dev, const float* time_dev,
                           const float* condition_dev, float* out_dev, int32_t nb, int32_t dropout_mode,
                           const uint8_t* const* masks_dev, void* stream);

/* ---- sampler seam: DYffusion.sample / sample_loop (dyffusion.py:335-431) ------------------------------------- */
dyf_status dyf_set_plan(dyf_engine* engine, const dyf_plan* plan);
/* initial_dev (NB, window*C, H, W); static_dev (NB, Cs, H, W) or NULL; out_dev (n_out_slots, NB, C, H, W): slot i
 * holds t{i+1}_preds.  masks_dev: NULL, or one pointer per (interpolator/forecaster forward, dropout layer) in
 * execution order (12 per forward that has dropout on) for the mask-injection parity mode; noise_dev: NULL or
 * (n_steps, NB, window*C, H, W) standard-normal draws for forward_conditioning="data+noise" parity. */
dyf_status dyf_sample(dyf_engine* engine, const float* initial_dev, const float* static_dev, float* out_dev,
                      int32_t nb, const uint8_t* const* masks_dev, const float* noise_dev, void* stream);
/* Asynchronous failures (ABI 7).  Every entry point only ENQUEUES work on the caller's stream; the one thing that can go wrong
 * after that is a fused GroupNorm convolution of the ResNet-UNet (csrc/gn_fused.h: workgroups of one sample meet inside the launch)
 * whose wait for its sample's statistics times out -- its output is then NaN-poisoned and a host-visible word is raised.
 * dyf_poll_errors reports that: DYF_OK, or DYF_ERR_STATE naming it (the engine has then already dropped its captured graphs and
 * runs the un-fused GroupNorm kernels from now on: repeat the call).  synchronize != 0 first waits for the STREAM of the engine's last
 * dyf_sample / dyf_sample_gather / dyf_net_forward call (not for the device: other streams keep running; a stream under capture is not waited for), so a
 * caller that polls right after dyf_sample / dyf_sample_gather / dyf_net_forward gets the failure from the SAME call (the Python
 * wrappers do).  Engines without a live fused form (unet_simple, SimpleConvNet, after a downgrade) return
 * DYF_OK at once without waiting.  Un-polled failures are still reported at the head of the next entry point.
 * dyf_gn_fuse_state: *live = the fused form is in use, *downgrades = how often the engine left it (time-out, or sweeps slower than
 * 1 ms on a GPU shared with another process -- the latter is not an error; DYF_VERBOSE=1 logs either to stderr). */
dyf_status dyf_poll_errors(dyf_engine* engine, int32_t synchronize);
dyf_status dyf_gn_fuse_state(const dyf_engine* engine, int32_t* live, int32_t* downgrades);
/* log_every_t of sample_loop (dyffusion.py:339-344, 398-406): with logging enabled a dyf_sample call also keeps, per sampling step,
 * x0_hat (what = 0, the reference's `intermediate_{s}_x0hat`), x_interpolated_s_next (1: `xipol_{s}_dmodel`, and `t{k}_preds2` on
 * the steps that emit a forecast) and, for cold sampling, x_interpolated_s (2: `xipol_{s}_dmodel2`; as in the reference the last
 * step without cold sampling reports the previous step's value).  Logged calls run eagerly on the engine's own workspace (no
 * captured graph, no row groups).  dyf_get_log copies one (NB, C, H, W) tensor of the most recent logged call; `step` indexes the
 * plan's steps. */
dyf_status dyf_set_log_intermediates(dyf_engine* engine, int32_t enable);
dyf_status dyf_get_log(dyf_engine* engine, int32_t step, int32_t what, float* out_dev, int32_t nb, void* stream);
/* Re-seed the engine's counter-based dropout / noise generator (forward and noise counters reset to 0).  The keep bit of
 * an element is a function of (seed, forward index, GLOBAL batch row, dropout layer, element index inside the row), see
 * csrc/common.h: a rollout does not depend on how its rows are batched or sharded over GPUs.  dyf_seed and dyf_set_row_offset
 * wait for the device to go idle before they write the generator state (hipDeviceSynchronize), so they are ordered against
 * rollouts in flight on ANY stream. */
dyf_status dyf_seed(dyf_engine* engine, uint64_t seed);
/* Global index of this engine's batch row 0 (default 0).  A rank that samples rows [lo, hi) of an N*B-row ensemble
 * (_base_experiment.py:503-538 tiles them, row = n*B + b) sets lo: its rows then draw exactly the masks / noise they
 * would draw inside the un-sharded batch. */
dyf_status dyf_set_row_offset(dyf_engine* engine, uint32_t first_row);
/* Row groups (ABI 5).  The rows of a sampling call are independent for the whole rollout, so the engine may run them as n_groups
 * concurrent rollouts of ceil(NB / n_groups) rows each -- own workspace, own packed weights, own captured hipGraph, own HIP stream,
 * forked from and joined into the caller's stream -- so that under-filled launches, ragged last rounds of workgroups and launch
 * gaps of one group are covered by the kernels of the others.  Row g*per + i of the call is row i of group g and draws the
 * masks / noise of global row (row offset + g*per + i): the generator streams are those of the ungrouped call.  Default: chosen
 * at dyf_engine_create from the architecture and max_batch (ResNet-UNet on planes <= 128 x 128, not batch_invariant: 3 groups from
 * 432 000 pixels x rows = 120 rows of 60 x 60, 2 from 230 400 = 64 rows; otherwise 1).  Must be called before dyf_load_weights.
 * Calls with fewer than 32 rows, with injected masks / noise, and every other entry point run on the engine itself.
 * Three groups plus the caller's stream fill the 4 hardware queues of a HIP process: with other busy streams or other live engines
 * in the process two groups are the robust choice.
 * dyf_row_groups returns the number of groups in effect (1 = none). */
dyf_status dyf_set_row_groups(dyf_engine* engine, int32_t n_groups);
int32_t dyf_row_groups(const dyf_engine* engine);

/* Sampling precision (ABI 9).  bits = 16 (default): the library's own 16-bit path (bf16, or fp16 in the _f16 build), unchanged.
 * bits = 32: every network forward of the calls that follow -- dyf_net_forward, dyf_sample, dyf_sample_gather -- runs in fp32: fp32
 * NHWC activations, the fp32 parameter copy dyf_load_weights keeps (no training call needed), the convolutions on the fp32 matrix cores.
 * unet_simple and unet.Unet run the layer walk and the kernels of dyf_train_forward without DYF_TRAIN_BATCH_STATS (BatchNorm on running
 * statistics, GroupNorm per sample) -- one walk, recorded on a tape there, bumped through an arena here; SimpleConvNet has an fp32 forward
 * of its own (csrc/simple_conv_net.hip).  The arena is allocated by the FIRST switch to 32 for max_batch rows of the larger network and
 * freed by dyf_engine_destroy: nothing is allocated or synchronised inside a forward, the forward is bitwise repeatable (split-K sums are
 * reduced through a workspace in a fixed order, GroupNorm sums by one workgroup per sample) and a rollout is captured and replayed with
 * use_graph like the 16-bit one.  Both builds of the library implement it alike; it does not depend on dyf_engine_config.dtype.
 * unet.Unet: up to 4096 bottleneck tokens the fp32 Attention core is the training step's (it writes its probabilities into the arena),
 * beyond that a streaming matrix-core kernel that writes nothing of size tokens^2 (the 512^2 configuration: 16 384 tokens); more than
 * 32 767 tokens (4 tokens^2 probabilities per row no longer indexed by 32 bits): DYF_ERR_UNSUPPORTED.  The training step has the same
 * bound (dyf_train_forward).  Any other value of bits: DYF_ERR_INVALID_ARGUMENT.
 *   - the plan walker is the 16-bit one (sampler state, cold-sampling update, noisy condition, forecast stack, log, dyf_get_sampler_state,
 *     dyf_plan_forward_counts are shared); in fp32 there is no paired interpolator forward, no batched refinement and no row groups
 *     (dyf_set_row_groups stays accepted, a call behaves as with one group).  Forward order, and so the order of the generator's forward
 *     counter: forecaster, next-step interpolation, current-step interpolation; then the refinement pass one time after the other.
 *   - dropout mode 1 starts every forward from the generator exactly as the 16-bit path does -- same site numbers (a layer with p = 0
 *     is no site), same per-site salt, same 16-bit keep threshold, same global row keys: for equal seed, row offset and call sequence
 *     an fp32 engine draws the keep bits of a 16-bit engine at every activation site.  The one exception holds in the 16-bit engine's
 *     DEFAULT attention-dropout mode only (DYF_ATTN_DROPOUT_FAST, dyf_set_attention_dropout below): there the attention-probability site
 *     of unet.Unet draws from a head-folded stream of its own with k/256 granularity (rng_keep8, csrc/common.h), while the fp32 path keeps
 *     nn.Dropout's p through the 16-bit threshold on the row's site stream, as the training path does.  With DYF_ATTN_DROPOUT_EXACT a
 *     16-bit engine draws the fp32 engine's keep bits at EVERY site.
 *   - dropout mode 2 applies the caller's uint8 keep masks, layout and site order as in the 16-bit path ((NB, 4, N, N) for the
 *     attention probabilities).
 *   - a graph captured under one precision is never replayed under another.
 * bits = 48 = DYF_SAMPLE_PRECISION_BF16X3, "bf16x3": the fp32 sampling forward of bits = 32 with the convolution operands of
 * dyf_train_set_precision(48).  The convs of unet_simple and unet.Unet that the 16-bit training dispatch takes (its channel rules) stage
 * each fp32 operand value v as hi = bf16(v), lo = bf16(v - hi) and accumulate a_lo b_hi + a_hi b_lo + a_hi b_hi in fp32 on the bf16 matrix
 * cores (4.5e-6 rel-RMS of a conv against float64; a rollout stays inside the 1e-4 per field that bits = 32 is held to).  Everything else
 * is exactly as under 32: fp32 activations and weights, statistics, Linear, attention, stems, readout, every conv outside those rules, the
 * arena and its sizing (the first switch to 32 OR 48 allocates it; its head also holds the 16-bit weight images of a launch), the
 * generator's sites and keep bits, injected masks and noise, the 32 767-token bound, one row group.  SimpleConvNet keeps fp32 conv
 * operands under 48 (its forward is bitwise the one under 32).  Accepted by both builds of the library.
 * dyf_sample_precision returns 16, 32 or 48. */
#define DYF_SAMPLE_PRECISION_BF16X3 48
dyf_status dyf_set_sample_precision(dyf_engine* engine, int32_t bits);
int32_t dyf_sample_precision(const dyf_engine* engine);

/* Dropout on the softmax probabilities of unet.Unet's Attention (attention.py:70) in the 16-bit path, engine generator (dropout mode 1).
 * Added without an ABI bump: two functions and two constants, no struct changes layout.
 *   DYF_ATTN_DROPOUT_FAST (0, default)  the quad form: one keep word per four probabilities on a stream keyed per (row, head), keep
 *       probability floor((1 - p) * 256) / 256 (p = 0.1 drops 10.16 %), survivors scaled by 256 / k so the expectation is exact; up to
 *       65 535 tokens.
 *   DYF_ATTN_DROPOUT_EXACT (1)          nn.Dropout(p) on the stream of the fp32 and training paths, bit for bit: the row's site key,
 *       element (h * N + i) * N + j of the row's (4, N, N) probabilities, 16-bit slice of its pair word against floor((1 - p) * 65536),
 *       survivors scaled by 1 / (1 - p).  For equal seed, row offset and call sequence the engine then draws, at every dropout site, the
 *       keep bits of an fp32 engine -- and of tests/rng_host.py's host restatement.  At most 32 767 tokens (4 N^2 <= 2^32 - 1).
 * The mode applies to every 16-bit forward that follows -- dyf_net_forward, dyf_sample, dyf_sample_gather, the eval-mode loss, the
 * dyf_op_attention_dropout seam -- and to the row groups; injected masks (mode 2), fp32 sampling and the training step do not depend on
 * it.  A graph captured under one mode is never replayed under the other.  Engines without a unet.Unet network accept the call without
 * effect.  DYF_ERR_INVALID_ARGUMENT: any other mode; DYF_ERR_UNSUPPORTED (the mode stays as it was): DYF_ATTN_DROPOUT_EXACT on an
 * engine whose unet.Unet has more than 32 767 bottleneck tokens.  dyf_attention_dropout returns the mode in effect. */
#define DYF_ATTN_DROPOUT_FAST 0
#define DYF_ATTN_DROPOUT_EXACT 1
dyf_status dyf_set_attention_dropout(dyf_engine* engine, int32_t mode);
int32_t dyf_attention_dropout(const dyf_engine* engine);

/* ---- engine-owned exchange of the ensemble-sharded path (one process per GPU; the reference has no inference collective) ------- */
/* Ensemble members / batch items are independent rows for the whole rollout (_base_experiment.py:503-538 tiles them, row = n*B + b),
 * so rank r of `world` samples the contiguous block of global rows [lo_r, hi_r) of a total_rows-row ensemble -- balanced split, the
 * first total_rows % world ranks own one row more -- with NO collective inside the rollout, and ONE RCCL all-gather (xGMI) of the
 * local forecast stack at the end.  The engine owns the communicator: a host binding this ABI needs no torch.distributed.
 *   dyf_comm_unique_id   rank 0 creates the 128-byte RCCL unique id; the caller distributes it (MPI, a file, torch.distributed ...)
 *   dyf_comm_init        every rank, same id: ncclCommInitRank on the engine's device (librccl is dlopen'ed here, on first use)
 *   dyf_sample_gather    dyf_sample of this rank's nb = ceil(total_rows / world) rows (ranks owning fewer repeat a row; call
 *                        dyf_set_row_offset(lo_r) first so the rows draw the masks of the un-sharded batch), then ncclAllGather of the
 *                        contiguous [n_out_slots][nb][C][H][W] stack and one unpack pass, all enqueued on `stream`:
 *                        out_full_dev (n_out_slots, total_rows, C, H, W) holds t{i+1}_preds of ALL rows, global order, on every rank. */
#define DYF_COMM_ID_BYTES 128
dyf_status dyf_comm_unique_id(uint8_t* id_out /* [DYF_COMM_ID_BYTES], host */);
dyf_status dyf_comm_init(dyf_engine* engine, const uint8_t* unique_id, int32_t rank, int32_t world);
dyf_status dyf_comm_destroy(dyf_engine* engine);
/* ranks of the engine's communicator as RCCL itself reports them (ncclCommCount); 0 = the engine owns none (ABI 6) */
dyf_status dyf_comm_count(const dyf_engine* engine, int32_t* ranks_out);
dyf_status dyf_sample_gather(dyf_engine* engine, const float* initial_dev, const float* static_dev, float* out_full_dev, int32_t nb,
                             int32_t total_rows, void* stream);

/* On-device ensemble metrics, replaces evaluate_ensemble_prediction (src/utilities/evaluation.py:10-118) and the
 * .cpu().numpy() round trip in front of it (_base_experiment.py:617-640).  preds_dev: (n_members, n_points) fp32 with
 * n_points = B*C*H*W (the "(N, B, C, H, W)" ensemble stack of one horizon step), targets_dev: (n_points) fp32.
 * out_host[3] receives {mse of the ensemble mean, spread-skill ratio sqrt(mean var)/sqrt(mse), CRPS}, all averaged over
 * every point (mean_over_samples=True).  Synchronises `stream`. */
dyf_status dyf_ensemble_metrics(dyf_engine* engine, const float* preds_dev, const float* targets_dev, int32_t n_members,
                                int64_t n_points, double* out_host, void* stream);   /* n_members <= 15 360: up to 64 members a workgroup stages
                                * [N][256 points] in LDS; beyond that fewer points per workgroup, several threads per point */
/* The same three metrics per SEGMENT, on the device: the curves of evaluate_ensemble_prediction(..., mean_over_samples=False)
 * over a trajectory (N, T, B, C, H, W) with the horizon on the sample axis (forecasting_multi_horizon.py:231-260).  Segment s has
 * n_members x n_points predictions, member n starting at preds_dev[s] + n * member_stride (elements, member_stride >= n_points:
 * n_points for one (N, B, C, H, W) stack per horizon, S * n_points for one (N, S, ...) tensor), and n_points targets at
 * targets_dev[s].  preds_dev / targets_dev are HOST arrays of n_segments device pointers (4-byte alignment suffices); the engine
 * uploads them.  out_dev (device, [3][n_segments]) receives mse, ssr, crps of every segment; accum_dev (device, [3][n_segments],
 * or NULL) += out.  Two launches on `stream`, no atomics: a segment's values do not depend on the other segments of the call, and
 * identical calls give identical bits.  Does NOT synchronise.  n_members in [1, 15360], n_segments in [1, 65535]. */
dyf_status dyf_trajectory_metrics(dyf_engine* engine, int32_t n_segments, const float* const* preds_dev,
                                  const float* const* targets_dev, int32_t n_members, int64_t n_points, int64_t member_stride,
                                  double* out_dev, double* accum_dev, void* stream);
/* The metrics as a function of the ensemble size, in one pass: for every segment and every n = 1..n_members the mse, ssr and crps of
 * the ensemble made of the FIRST n members (evaluate_ensemble_prediction_for_varying_members, evaluation.py:145-156), and every
 * member's own mse (mse_per_mem, evaluation.py:53-60).  Segments, member_stride and the two host arrays of device pointers as in
 * dyf_trajectory_metrics.  out_dev (device, [4][n_segments][n_members]) receives mse, ssr, crps (entry n - 1 = prefix n) and
 * mse_per_mem; accum_dev (device, the same shape, or NULL) += out.  The pair term of prefix n is that of prefix n - 1 plus
 * sum_{m<n} |x_n - x_m|, mean and variance are Welford's (ssr[0] is exactly 0): all prefixes cost the pair work of one score.  Two
 * launches on `stream`, no atomics, partial sums in an engine-owned workspace of at most 64 x n_members x 4 doubles per segment: a
 * segment's values depend neither on the other segments nor on the layout, and identical calls give identical bits.  Does NOT
 * synchronise.  n_members in [1, 256] (DYF_ERR_UNSUPPORTED beyond), n_segments in [1, 65535].  (Additive: no ABI change.) */
dyf_status dyf_ensemble_size_metrics(dyf_engine* engine, int32_t n_segments, const float* const* preds_dev,
                                     const float* const* targets_dev, int32_t n_members, int64_t n_points, int64_t member_stride,
                                     double* out_dev, double* accum_dev, void* stream);
/* Five scores per (segment, GROUP) in one pass: the mean_dims surface of evaluation.py (evaluate_ensemble_mse,
 * evaluate_ensemble_spread_skill_ratio, evaluate_ensemble_crps, evaluate_ensemble_nll, evaluate_ensemble_corr; :83-142).  Segments,
 * member_stride and the two host arrays of device pointers as in dyf_trajectory_metrics.  The n_points points of a segment are viewed
 * as row-major (n_outer, n_groups, n_inner), n_outer * n_groups * n_inner == n_points: point p belongs to group
 * (p / n_inner) % n_groups; (1, 1, n_points) pools the segment, (B, C, H * W) on a (B, C, H, W) target is the per-channel score,
 * (1, B, C * H * W) the per-sample score.  out_dev (device, [5][n_segments][n_groups]) receives per group
 *   mse   mean of (ensemble mean - y)^2            ssr   sqrt(mean population variance) / sqrt(mse)
 *   crps  mean of the ensemble CRPS                nll   mean of 0.5 log(2 pi var) + (mean - y)^2 / (2 var): the Gaussian NLL under the
 *   corr  Pearson correlation of the ensemble mean with y                                                ensemble mean and variance
 * accum_dev (device, the same shape, or NULL) += out.  mean, var and crps per point are the fp32 expressions of
 * dyf_trajectory_metrics, nll is fp32 with the accurate logarithm, sums over points and the correlation's moments (centred per
 * workgroup, joined pairwise) are fp64.  IEEE behaviour as numpy, nothing is clamped: one member has var = 0 and a NaN nll, a group
 * whose ensemble means or targets are constant has a NaN corr.  Two launches on `stream`, no atomics, partial sums in an
 * engine-owned workspace of 9 doubles per workgroup: a group's values depend on its own points, n_members, n_outer and n_inner
 * alone -- not on the other groups or segments, nor on the layout -- and identical calls give identical bits.  Does NOT
 * synchronise.  n_members in [1, 15360], n_segments in [1, 65535]; a segment takes n_outer * n_groups * ceil(n_inner / P)
 * workgroups, P = 256 points up to 64 members (beyond: the largest power of two with n_members * P * 4 <= 60 KB), and at most
 * 2^24 - 1 of them: DYF_ERR_UNSUPPORTED beyond.  A geometry whose product is not n_points is DYF_ERR_INVALID_ARGUMENT.
 * (Additive: no ABI change.) */
dyf_status dyf_ensemble_scores(dyf_engine* engine, int32_t n_segments, const float* const* preds_dev,
                               const float* const* targets_dev, int32_t n_members, int64_t n_points, int64_t member_stride,
                               int64_t n_outer, int32_t n_groups, int64_t n_inner, double* out_dev, double* accum_dev, void* stream);
/* Forecast products per grid point: what an ensemble forecast delivers -- the ensemble mean, the spread, the extremes, quantiles and
 * exceedance probabilities -- reduced over the members on the device, K fields out for N members in (the reference hands back the
 * member stack; numpy's np.mean / np.std / np.min / np.max / np.quantile(method="linear") / (x > t).mean() over the member axis
 * are what the fields are held to).  Segments, member_stride and the host array of device pointers as in dyf_trajectory_metrics
 * (there are no targets).  out_dev (device, [n_segments][K][n_points] fp32) receives the K planes asked for, in the fixed order
 * mean, std, min, max, the quantiles in the order given, the exceedances in the order given.  Per point, members x_0 .. x_{N-1}:
 *   mean, std    the fp32 expressions of dyf_trajectory_metrics: the sum in member order, mean = sum * (1 / N), var = sum (x - mean)^2
 *                * (1 / N) (population), std = sqrtf(var); where several threads share a point their partial sums are joined in a
 *                fixed order
 *   min, max     exact
 *   quantile q   numpy's default ("linear", type 7) on the sorted members: h = (N - 1) q in double on the host, lo = floor(h), hi =
 *                min(lo + 1, N - 1), the fraction h - lo rounded to fp32; value = x_(lo) + frac * (x_(hi) - x_(lo)) in fp32 without
 *                contraction, and x_(lo) itself when frac == 0: q = 0 and q = 1 are the min and max planes, the median of an odd
 *                ensemble is a member.  The order statistics are selected by counting ranks (no sort)
 *   exceedance t (float)#{n : x_n > t} / (float)N, strict
 * A point with a NaN member has NaN in its mean, std, min, max and quantile planes (as numpy); an exceedance counts the comparisons
 * that are true; its neighbours are untouched.  Infinities are specified for min, max and exceedance only; the sign of a zero order
 * statistic is unspecified.  K == 0, a flag that is not 0 / 1, a probability outside [0, 1] or NaN, a NaN threshold, or counts
 * above the two maxima: DYF_ERR_INVALID_ARGUMENT.  One launch on `stream`, no atomics, no workspace: a point's outputs depend on
 * its own members alone -- not on the layout, the segment or the other points -- and identical calls give identical bits.  Does
 * NOT synchronise.  n_members in [1, 15360], n_segments in [1, 65535], at most 2^24 - 1 workgroups per segment (256 points each up
 * to 64 members; beyond: the largest power of two P <= 128 with n_members * P * 4 <= 60 KB): DYF_ERR_UNSUPPORTED beyond.
 * (Additive: no ABI change.) */
#define DYF_MAX_PRODUCT_QUANTILES  16
#define DYF_MAX_PRODUCT_THRESHOLDS 16
typedef struct dyf_products_spec {
    int32_t mean, std, min, max;                 /* 0 / 1 each */
    int32_t n_quantiles;  double quantiles[DYF_MAX_PRODUCT_QUANTILES];    /* probabilities in [0, 1] */
    int32_t n_thresholds; float  thresholds[DYF_MAX_PRODUCT_THRESHOLDS];  /* P(x > threshold) */
} dyf_products_spec;
dyf_status dyf_ensemble_products(dyf_engine* engine, int32_t n_segments, const float* const* preds_dev, int32_t n_members,
                                 int64_t n_points, int64_t member_stride, const dyf_products_spec* spec, float* out_dev, void* stream);
/* The rank histogram (Talagrand diagram) per (segment, GROUP): where the truth falls among the members, the companion of the
 * spread-skill ratio.  Segments, member_stride, the two host arrays of device pointers and the group geometry (n_outer, n_groups,
 * n_inner) exactly as in dyf_ensemble_scores; a geometry whose product is not n_points is DYF_ERR_INVALID_ARGUMENT.  out_dev
 * (device, [n_segments][n_groups][n_members + 1] doubles) receives the bins; accum_dev (device, the same shape, or NULL) += out.
 * For a point with target y, b = #{n : x_n < y} and e = #{n : x_n == y}: each of the bins b .. b + e receives 1 / (e + 1), the
 * uniform split of ties (a boundary-condition pixel, where every member equals the target, spreads over all bins).  A point whose
 * target or any member is NaN contributes nothing: the bins of a group sum to its number of NaN-free points, and without ties every
 * bin is an integer.  Two launches on `stream`, no atomics: a group's points are cut into tiles of 256 consecutive points of one
 * (outer, group) slab, min(tiles of the group, 256) workgroups walk them and each leaves one partial histogram in an engine-owned
 * workspace -- at most n_segments x n_groups x 256 x (n_members + 1) doubles, grown on demand -- which the second launch adds in a
 * fixed order: a group's bins depend on its own points, n_members, n_outer and n_inner alone, and identical calls give identical
 * bits.  Does NOT synchronise.  n_members in [1, 1024] (DYF_ERR_UNSUPPORTED beyond), n_segments in [1, 65535]; n_outer * n_groups *
 * ceil(n_inner / 256) is at most 2^24 - 1 as for dyf_ensemble_scores: DYF_ERR_UNSUPPORTED beyond.  (Additive: no ABI change.) */
dyf_status dyf_rank_histogram(dyf_engine* engine, int32_t n_segments, const float* const* preds_dev, const float* const* targets_dev,
                              int32_t n_members, int64_t n_points, int64_t member_stride, int64_t n_outer, int32_t n_groups,
                              int64_t n_inner, double* out_dev, double* accum_dev, void* stream);
/* The energy score and the member-distance matrix per (segment, GROUP): the multivariate companion of the CRPS, |.| replaced by the
 * Euclidean norm over a whole VECTOR of points, so that an ensemble of coherent fields scores better than one with the same
 * per-point spread and scrambled members.  Segments, member_stride, the two host arrays of device pointers and the group geometry
 * (n_outer, n_groups, n_inner) exactly as in dyf_ensemble_scores; a vector is one (outer o, group g) slab of n_inner contiguous
 * points: (B, 1, C * H * W) scores whole fields, (B, C, H * W) every channel, (points, 1, 1) degenerates to the CRPS of
 * dyf_trajectory_metrics (1 / N and 1 / N^2 weights).  Per vector, members x_0 .. x_{N-1}, target y:
 *   d_i = ||x_i - y||_2        D_ij = ||x_i - x_j||_2
 * out_dev (device, [4][n_segments][n_groups] doubles) receives per (segment, group), every mean over o taken first:
 *   dist_target (plane 2)  mean_o (1 / N) sum_i d_i              dist_pair (plane 3)  mean_o 1 / (N (N - 1)) sum_{i != j} D_ij
 *   es (plane 0)           dist_target - (N - 1) / (2 N) dist_pair    (N = 1: dist_target; the second term is dropped)
 *   es_fair (plane 1)      dist_target - dist_pair / 2
 * member_out_dev (device, [n_segments][n_groups][N], or NULL) receives mean_o d_i, pair_out_dev (device,
 * [n_segments][n_groups][N][N], or NULL) mean_o D_ij: bitwise symmetric, the diagonal exactly 0; accum_dev (device, the shape of
 * out_dev, or NULL) += out.
 *   Stated arithmetic: diff = x_i[p] - x_j[p] (x_i[p] - y[p]) in fp32; the squares accumulate in fp32 (fmaf, in point order) over the
 * points of one tile, DYF_ENERGY_TILE_POINTS consecutive points of the vector; the tile sums are added in float64, in tile order
 * (where a vector is split, over each chunk's consecutive tiles, then over the chunks in chunk order); sqrt in float64, once per
 * vector, after all its tiles; the means over o, then over the members (index order) and the pairs (row i: j = i + 1 .. N - 1 in
 * order, then the rows in order) in float64.  The differences are taken directly: no Gram-matrix form, nothing cancels for close
 * members.  IEEE behaviour as numpy: a NaN in member i of a vector makes d_i and D_i. of its (segment, group) NaN and with them the
 * four planes; other (segment, group) entries are untouched; identical members give exactly 0.0; N = 1 gives es = d_1 and NaN in
 * dist_pair and es_fair.
 *   Three launches on `stream`, no atomics, nothing exchanged between workgroups inside a launch: identical calls give identical
 * bits, and a segment's values depend on its own data, n_members and the geometry alone (not on the other segments or their order).
 * A vector is split over at most C = min(tiles, max(1, 256 / (vectors x block pairs))) workgroups (chunks of equally many consecutive
 * tiles), and only where a segment has fewer than 256 work items (vectors = n_outer x n_groups, tiles = ceil(n_inner / DYF_ENERGY_TILE_POINTS), block pairs = B (B + 1) / 2 with B =
 * ceil(N / 64)).  Engine-owned workspace, grown on demand: at most n_segments x vectors x C x N x (N + 1) doubles of partial sums of squares
 * (never of square roots) and n_segments x n_groups x N x (N + 1) doubles of mean distances; a call that would need more than
 * DYF_ENERGY_MAX_WORKSPACE_DOUBLES is DYF_ERR_UNSUPPORTED, before anything is launched.  Does NOT synchronise.  n_members in
 * [1, DYF_ENERGY_MAX_MEMBERS] (DYF_ERR_UNSUPPORTED beyond), n_segments in [1, 65535]; n_inner >= 1 is arbitrary.  The kernel reads
 * fp32 only: both builds of the library give the same bits.  (Additive: no ABI change.) */
#define DYF_ENERGY_TILE_POINTS 64
#define DYF_ENERGY_MAX_MEMBERS 256
#define DYF_ENERGY_MAX_WORKSPACE_DOUBLES 134217728 /* 2^27: 1 GiB */
dyf_status dyf_energy_score(dyf_engine* engine, int32_t n_segments, const float* const* preds_dev, const float* const* targets_dev,
                            int32_t n_members, int64_t n_points, int64_t member_stride, int64_t n_outer, int32_t n_groups,
                            int64_t n_inner, double* out_dev, double* member_out_dev, double* pair_out_dev, double* accum_dev,
                            void* stream);
/* Radially binned power spectra of an ensemble forecast per (segment, CHANNEL): at which spatial scales the members are as sharp as
 * the truth, where the ensemble mean blurs, and where the spread matches the error of the mean.  Segments, member_stride and the two
 * host arrays of device pointers as in dyf_trajectory_metrics; a segment's members are (batch, channels, height, width) fp32 fields,
 * member m at preds_dev[s] + m * member_stride (member_stride >= batch * channels * height * width), its target alike at
 * targets_dev[s].  Per (b, c), members x_0 .. x_{N-1}, target y:
 *   xbar = (float)((sum_m (double)x_m, member order) / N)      a_m = x_m - xbar      e = xbar - y      (fp32, BEFORE the transform)
 * and Z = F(z) is the 2-D DFT of each of the N + 3 real fields a_0 .. a_{N-1}, xbar, y, e; with window = 1 every field is first
 * multiplied by the separable Hann taper (float)w_H[h] * (float)w_W[w] (one fp32 product), w_n[i] = (1 - cos(2 pi i / n)) / 2.
 * Nothing of the form sum |X_m|^2 - N |Xbar|^2 appears: close members do not cancel.  Four planes, each normalised by 1 / (H W)^2 so
 * that the sum of a plane over all coefficients is mean(z^2) (Parseval), each the mean over b:
 *   spread (plane 0)  (1 / N) sum_m |A_m|^2      mean (plane 1)  |Xbar|^2      target (plane 2)  |Y|^2      error (plane 3)  |E|^2
 * (the host derives members = spread + mean = mean_m |X_m|^2, exact because sum_m a_m = 0, and spread_fair = spread N / (N - 1)).
 *   Shells: L = max(H, W), n_bins = L / 2 + 1; the coefficient with folded indices kx' = min(kx, W - kx), ky' = min(ky, H - ky) has
 * kappa = L sqrt((kx' / W)^2 + (ky' / H)^2) and goes to bin round_half_up(kappa), decided on the host in exact integers: bin = k <=>
 * (2k - 1)^2 H^2 W^2 <= 4 L^2 (kx'^2 H^2 + ky'^2 W^2) < (2k + 1)^2 H^2 W^2.  Bins >= n_bins (the corners) are left out of the shells
 * and kept in `total`, the sum over ALL coefficients.  out_dev (device, [n_segments][channels][4][n_bins + 1] doubles): bins 0 ..
 * n_bins - 1, then total; accum_dev (device, the shape of out_dev, or NULL) += out.
 *   Stated arithmetic: only kx in [0, W / 2] is transformed, a column counted twice unless kx = 0 or 2 kx = W.  Row DFT along w: an
 * fp32 fmaf chain in w order against twiddles (float)cos / (float)sin(2 pi j / W) (float64 on the host, rounded once).  Column DFT
 * along h on v_mfma_f32_16x16x4_f32 (exact fp32): per output four fmaf chains in h order (cos Tr, sin Ti, cos Ti, -sin Tr), joined
 * by one fp32 addition each for the real and the imaginary part.  |Z|^2 = zr^2 + zi^2 and every sum from there on in float64: per
 * coefficient over the members in member order; per workgroup (b, c, tile of 16 kx columns) and shell in (ky, kx) order; per
 * (segment, c) over the workgroups in (b, tile) order; then one division by B (H W)^2 (spread: B (H W)^2 N); total = the sum of
 * the n_bins + 1 joined bins (the corners last) in bin order.
 *   Three launches on `stream`, no atomics, nothing exchanged between workgroups inside a launch: identical calls give identical
 * bits, and a segment's values depend on its own data, n_members and the geometry alone.  Engine-owned workspace, grown on demand:
 * xbar (n_segments B C H W floats), 4 x 16 ceil16(H) x 16 doubles of coefficient planes and 4 (n_bins + 1) doubles of shell sums per
 * workgroup; a call that would need more than DYF_SPECTRUM_MAX_WORKSPACE_DOUBLES is DYF_ERR_UNSUPPORTED, before anything is launched.
 * The twiddle, taper and shell tables are built on the host and copied to the device on the FIRST call of an engine at a geometry
 * (H, W) (a synchronous copy; not inside a stream capture) and kept until dyf_destroy; every later call does NOT synchronise.
 * 2 <= height, width <= DYF_SPECTRUM_MAX_DIM (DYF_ERR_UNSUPPORTED beyond; the transform's LDS, 128 ceil4(H) + 8 (H + W) + 8192 bytes,
 * fits the 160 KB of a compute unit up to there), n_members in [1, DYF_SPECTRUM_MAX_MEMBERS] (DYF_ERR_UNSUPPORTED beyond),
 * n_segments in [1, 65535], window 0 or 1.  The kernels read fp32 only: both builds of the library give the same bits.
 * (Additive: no ABI change.) */
#define DYF_SPECTRUM_MAX_DIM 1024
#define DYF_SPECTRUM_MAX_MEMBERS 256
#define DYF_SPECTRUM_MAX_WORKSPACE_DOUBLES 134217728 /* 2^27: 1 GiB */
dyf_status dyf_power_spectrum(dyf_engine* engine, int32_t n_segments, const float* const* preds_dev, const float* const* targets_dev,
                              int32_t n_members, int64_t member_stride, int32_t batch, int32_t channels, int32_t height, int32_t width,
                              int32_t window, double* out_dev, double* accum_dev, void* stream);
/* Copy one (NB,C,H,W) field of the sampler's state after the most recent dyf_sample call: what sample_loop returns
 * beside the intermediates (dyffusion.py:424-426): (x0_hat, ., x_s), or (x_s, ., x_interpolated_s_next) when the sampling
 * schedule stops before T-1. */
typedef enum dyf_sampler_state { DYF_STATE_X0_HAT = 0, DYF_STATE_X_S = 1, DYF_STATE_X_NEXT = 2 } dyf_sampler_state;
dyf_status dyf_get_sampler_state(dyf_engine* engine, int32_t what, float* out_dev, int32_t nb, void* stream);

/* ---- training step: DYffusion.p_losses in training mode (dyffusion.py:496-567; every arch) -------------------------------- */
/* What the reference gets from torch.autograd over unet_simple.py / unet.py / simple_conv_net.py.  A forward is RECORDED in one of four tape slots (the
 * objective runs up to two interpolator and two forecaster forwards); dyf_train_backward consumes a slot: gradient of a
 * scalar loss w.r.t. the network's parameters (accumulated into the engine's gradient buffers when param_grads != 0) and,
 * when dinputs_dev != NULL, w.r.t. its `inputs` (NB,in_channels,H,W) -- the frozen interpolator is differentiated through.
 * flags: DYF_TRAIN_BATCH_STATS = BatchNorm with batch statistics (+ running-statistics update, momentum 0.1; module.train()),
 * otherwise running statistics (frozen / eval network); DYF_TRAIN_DROPOUT = Dropout layers active (engine generator, same
 * streams as sampling; the backward re-derives the masks).  All arithmetic fp32.
 * unet.Unet: up to 4096 bottleneck tokens the Attention keeps its (tokens x tokens) probabilities for the backward; beyond that the
 * forward keeps the softmax statistics (max, 1 / sum) per (row, head, token) and the backward recomputes the scores tile by tile (nothing of size tokens^2 is
 * written; gradients are bitwise repeatable); more than 32 767 tokens: DYF_ERR_UNSUPPORTED, as in fp32 sampling.
 * SimpleConvNet records with fp32 conv operands only: after dyf_train_set_precision(16) its dyf_train_forward returns DYF_ERR_UNSUPPORTED. */
#define DYF_TRAIN_BATCH_STATS 1
#define DYF_TRAIN_DROPOUT 2
dyf_status dyf_train_forward(dyf_engine* engine, int32_t net, int32_t slot, const float* inputs_dev, const float* time_dev,
                             const float* condition_dev, float* out_dev, int32_t nb, int32_t flags, void* stream);
dyf_status dyf_train_backward(dyf_engine* engine, int32_t slot, const float* dout_dev, float* dinputs_dev, int32_t param_grads,
                              void* stream);
dyf_status dyf_train_zero_grads(dyf_engine* engine, int32_t net);
/* Operand precision of the training convolutions (ABI 8) -- the reference's `trainer.precision` (Lightning; src/configs/trainer/default.yaml:14
 * "precision: 32   # 32 or 16"): 32 = fp32 operands on the fp32 matrix cores (the default; gradients at the 1e-6 level of autograd over the oracle),
 * 16 = "bf16-mixed": activations, gradients, master weights and accumulation stay fp32, the conv operands are rounded to bf16 -- in
 * BOTH builds of the library, whatever dyf_engine_config.dtype is -- while they are staged (csrc/train_halo16.hip,
 * csrc/train_gemm.hip).  Lightning's precision=16 is fp16 + a GradScaler; this engine answers the same request with bf16 operands,
 * which need no loss scale (with mean-reduced losses dL/dout is ~1e-6..1e-7 at real batch sizes, below fp16's normal range).
 * 0 = not set (fp32 operands; the tests' kernel-form switch DYF_TRAIN_OPERANDS of dyffusion_hip_testing.h can select 16-bit operands
 * or bf16x3 operands for such engines).  Applies to the dyf_train_forward / dyf_train_backward calls that follow; a recorded forward and
 * its backward should run under the same setting.
 * 48 = DYF_TRAIN_PRECISION_BF16X3, "bf16x3": fp32-grade convolutions on the 16-bit matrix cores (what
 * torch.set_float32_matmul_precision("high") asks of other back ends).  The convs the 16-bit dispatch takes (the same channel rules as
 * under 16) stage each fp32 operand value v as TWO bf16 values, hi = bf16(v) and lo = bf16(v - hi), and accumulate
 * a_lo b_hi + a_hi b_lo + a_hi b_hi in fp32: a product is good to ~2^-16 (rel-RMS 4.5e-6 of a conv against float64, inside the 1e-5
 * the fp32 kernels are held to; one bf16 term: 2.4e-3).  Nothing else is rounded, and everything else is exactly as under 32: tensors,
 * master weights, accumulation, statistics, every Linear and attention contraction, and every conv outside those channel rules (fp32
 * kernels).  SimpleConvNet keeps recording with fp32 conv operands under 48, as under 0 and 32 (only 16 is refused for it).  The
 * sampling paths do not read the setting (they have their own: dyf_set_sample_precision). */
#define DYF_TRAIN_PRECISION_BF16X3 48
dyf_status dyf_train_set_precision(dyf_engine* engine, int32_t bits);
int32_t dyf_train_precision(const dyf_engine* engine);
/* Deterministic training mode (ABI 9) -- the reference's `trainer.deterministic` (Lightning; src/configs/trainer/default.yaml:18
 * "deterministic: True"): on = 1 makes every floating-point sum of a recorded forward, of its backward and of the criterion independent
 * of the arrival order of workgroups and waves, so two identical steps give bitwise equal losses, gradients and running statistics.  The
 * weight / bias gradients, the BatchNorm / GroupNorm sums of both passes, the LayerNorm gain gradient and the loss value, which the
 * default mode merges with atomics, go as one slab of partial sums per contributor to the step's split-K workspace (64 MB, no further
 * memory) and are added in index order by a second launch; the adjoint of the outer resample becomes a gather (csrc/train.hip,
 * csrc/train_gemm.hip, csrc/train_halo16.hip).  on = 0 (the default) keeps the atomic forms, whose gradients differ from run to run in
 * the last bits.  Applies to the dyf_train_forward / dyf_train_backward / dyf_criterion / dyf_criterion_grad calls that follow (a
 * backward runs under the setting its forward was recorded with); neither sampling path reads it. */
dyf_status dyf_train_set_deterministic(dyf_engine* engine, int32_t on);
int32_t dyf_train_deterministic(const dyf_engine* engine);
/* Copy gradients out by the reference's state_dict names (PyTorch layouts), HOST fp32 buffers; "*.running_mean/var" return the
 * updated BatchNorm statistics. */
/* Refresh only the TRAINING copy of a network's parameters (after optimizer.step()): same arguments as dyf_load_weights, which
 * must have loaded the network once.  The sampling copy (folded / packed 16-bit weights, FiLM tables) is NOT updated: call
 * dyf_load_weights again before sampling the network. */
dyf_status dyf_train_load_weights(dyf_engine* engine, int32_t net, int32_t n_tensors, const char* const* names,
                                  const float* const* data, const int64_t* const* shapes, const int32_t* ndims);
/* dyf_train_load_weights / dyf_train_export with DEVICE pointers (contiguous fp32 tensors on the engine's GPU -- the parameters /
 * gradients of a module that lives on the GPU): device-to-device copies and repack kernels, no host round trip. */
dyf_status dyf_train_load_weights_dev(dyf_engine* engine, int32_t net, int32_t n_tensors, const char* const* names,
                                      const float* const* data_dev, const int64_t* const* shapes, const int32_t* ndims);
dyf_status dyf_train_export_dev(dyf_engine* engine, int32_t net, int32_t n_tensors, const char* const* names, float* const* out_dev);
dyf_status dyf_train_export(dyf_engine* engine, int32_t net, int32_t n_tensors, const char* const* names, float* const* out_host);
/* d(scale * mean criterion)/d pred, kinds as dyf_criterion (the loss terms of p_losses, dyffusion.py:531,557). */
dyf_status dyf_criterion_grad(dyf_engine* engine, const float* pred_dev, const float* target_dev, int64_t count, int32_t kind,
                              float scale, float* dpred_dev, void* stream);

/* ---- engine-resident optimizer: AdamW with global gradient-norm clipping and a weight EMA (additions to ABI 9) --------------- */
/* The last third of a training iteration on the engine's own copies: fp32 master weights, gradients (what dyf_train_backward
 * accumulated), exp_avg / exp_avg_sq and -- optionally -- an EMA shadow of the weights never leave the GPU.  What the reference does with
 * torch.optim.AdamW + `gradient_clip_val` (Lightning: torch.nn.utils.clip_grad_norm_) + LitEma (src/models/modules/ema.py).
 *   create   one optimizer per network slot (0 / 1); any arch with loaded weights (no weights: DYF_ERR_STATE).  State starts at zero, the shadow as a copy of the current weights.
 *            Creating again replaces the optimizer.  It survives dyf_load_weights of the same network and goes with the engine.
 *   step     two launches on `stream`, no host synchronisation: (1) sum of squares of all gradients, one double per workgroup;
 *            (2) every workgroup re-reduces those partial sums in one fixed order (the norm is bitwise the same in every workgroup
 *            and every run), then, chunk by chunk: g *= min(1, max_grad_norm / (norm + 1e-6)); p *= 1 - lr * weight_decay;
 *            m += (1 - beta1)(g - m); v = beta2 v + (1 - beta2) g g; p += (-(lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps);
 *            shadow -= (1 - ema_decay_now)(shadow - p); g = 0 -- each in the roundings of torch's fp32 CPU kernels (no contraction
 *            beyond theirs).  Both layouts of a conv weight are written by the same lane.
 *            BatchNorm running statistics are no parameters and do not move.  A non-finite norm skips the step: only g = 0 is
 *            written, and the step count is not advanced.  bc1 / bc2 = 1 - beta^t come from the host (double), t = applied steps + 1;
 *            the outcome of a step is copied to the host behind it and read when the host next needs it (the next step, dyf_optim_last,
 *            dyf_optim_get_step).  ema_decay_now: the caller evaluates LitEma's warm-up min(decay, (1 + n) / (10 + n)).
 *   last     gradient norm (before clipping) and skipped flag of the most recent step; waits for that step.
 *   export / import   by state_dict name in PyTorch layouts, host or device pointers (on_device), `kind` below; running statistics
 *            ("*.running_mean/var") travel as DYF_OPTIM_WEIGHT only.  Importing gradients REPLACES them.  DYF_OPTIM_WEIGHT_FWD reads a conv
 *            weight from its second ([tap][cin][cout]) copy: the two copies must never disagree, and a test can see that they do not.
 *   swap_ema weights <-> shadow in place, both conv layouts (validation through the EMA weights; calling it twice restores bitwise). */
typedef struct dyf_optim_config {
    double beta1, beta2, eps, weight_decay;   /* doubles, as torch.optim holds them: 1 - beta^t is evaluated in double */
    double max_grad_norm;  /* <= 0: no clipping (the norm is still computed) */
    int32_t ema;           /* keep an EMA shadow */
} dyf_optim_config;
typedef enum dyf_optim_kind { DYF_OPTIM_WEIGHT = 0, DYF_OPTIM_GRAD = 1, DYF_OPTIM_EXP_AVG = 2, DYF_OPTIM_EXP_AVG_SQ = 3, DYF_OPTIM_EMA = 4,
                              DYF_OPTIM_WEIGHT_FWD = 5 /* export only, conv weights only: read from the forward-layout copy */ } dyf_optim_kind;
dyf_status dyf_optim_create(dyf_engine* engine, int32_t net, const dyf_optim_config* config);
dyf_status dyf_optim_destroy(dyf_engine* engine, int32_t net);
dyf_status dyf_optim_step(dyf_engine* engine, int32_t net, double lr, double ema_decay_now, void* stream);
dyf_status dyf_optim_last(dyf_engine* engine, int32_t net, double* grad_norm_out, int32_t* skipped_out);
dyf_status dyf_optim_get_step(dyf_engine* engine, int32_t net, int64_t* step_out);
dyf_status dyf_optim_set_step(dyf_engine* engine, int32_t net, int64_t step);
dyf_status dyf_optim_export(dyf_engine* engine, int32_t net, int32_t kind, int32_t n_tensors, const char* const* names, float* const* out,
                            int32_t on_device);
dyf_status dyf_optim_import(dyf_engine* engine, int32_t net, int32_t kind, int32_t n_tensors, const char* const* names,
                            const float* const* data, int32_t on_device);
dyf_status dyf_optim_swap_ema(dyf_engine* engine, int32_t net, void* stream);

/* ---- boundary conditions of the physical-systems benchmark -------------------------------------------------------------- */
/* Replaces PhysicalSystemsBenchmarkDataModule.boundary_conditions (src/datamodules/physical_systems_benchmark.py:245-297:
 * a Python loop over batch elements with boolean-mask writes), which _evaluation_step applies to every predicted field
 * before it is returned / fed back (src/experiment_types/forecasting_multi_horizon.py:175-182), by ONE masked write over a
 * (n_fields, rows, C, H, W) fp32 stack, in place.  row_meta_dev[row] = batch element whose metadata applies to the row, -1 =
 * untouched (the host resolves the reference's indexing of ensemble stacks).  navier-stokes: preds[fixed_mask] = 0, then
 * channel 0 of grid row 0 = in_velocity*4*y*(0.41-y)/0.41^2*(1-exp(-5t)); spring-mesh: preds = where(fixed_mask, boundary). */
typedef enum dyf_bc_kind { DYF_BC_NAVIER_STOKES = 0, DYF_BC_SPRING_MESH = 1 } dyf_bc_kind;
typedef struct dyf_bc_args {
    int32_t kind;                  /* dyf_bc_kind */
    int32_t n_fields, rows, channels, height, width;
    int32_t n_meta;                /* batch elements the metadata tensors hold */
    const int32_t* row_meta_dev;   /* [rows] */
    const float* time_factor_dev;  /* navier-stokes: 1 - exp(-5 t) of every field (t = its physical time; evaluated by the host
                                    * in double like the reference's math.exp), [n_fields] or [n_fields][n_meta] */
    int32_t times_per_meta;        /* 0 / 1 */
    const uint8_t* fixed_mask_dev; /* [n_meta][C][H][W], non-zero = fixed */
    const float* in_velocity_dev;  /* navier-stokes [n_meta] */
    const float* vertex_y_dev;     /* navier-stokes [n_meta][W]: metadata["vertices"][:, 1, 0, :] */
    const float* boundary_dev;     /* spring-mesh [n_meta][C][H][W]: cat[zeros (p), features[:, 0, 2:] (q)] */
} dyf_bc_args;
dyf_status dyf_apply_boundary_conditions(dyf_engine* engine, const dyf_bc_args* args, float* preds_dev, void* stream);

/* ---- introspection (bench.py FLOP accounting); timing / op-level test seams live in dyffusion_hip_testing.h ---------- */
/* Number of network forwards one dyf_sample call performs under the current plan. */
dyf_status dyf_plan_forward_counts(const dyf_engine* engine, int32_t* n_forecaster, int32_t* n_interpolator);
/* 2*MAC of conv/linear layers of one forward of `net` for one sample (elementwise work excluded). */
dyf_status dyf_net_flops(const dyf_engine* engine, int32_t net, double* flops_per_sample);
/* The same count for the contractions the engine actually EXECUTES after dyf_load_weights: arch unet_simple skips the output
 * columns of the last decoder block that the final resample never reads, contracts init_conv into the first encoder conv, and
 * evaluates the readout only at the 4 neighbours the final bilinear resample reads (<= dyf_net_flops; equal for other archs). */
dyf_status dyf_net_flops_executed(const dyf_engine* engine, int32_t net, double* flops_per_sample);
/* Mean of the training criterion over `count` fp32 elements (src/utilities/utils.py:201-212 `get_loss`, reduction "mean"):
 * kind 0 = L1, 1 = MSE, 2 = smooth-L1 (beta 1).  The reduction the forecaster objective `DYffusion.p_losses`
 * (dyffusion.py:531,557) applies to (prediction, target); out_host[0] receives the scalar. */
dyf_status dyf_criterion(dyf_engine* engine, const float* pred_dev, const float* target_dev, int64_t count, int32_t kind,
                         double* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DYFFUSION_HIP_H */
