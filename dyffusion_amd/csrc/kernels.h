// HBM-bound kernels around the convolutions: launch prototypes.
#pragma once
#include "common.h"

#include <vector>

#define DYF_MAX_IN_CH 32   // max channels entering the network stem (inputs + condition)
#define DYF_MAX_OUT_CH 8   // max output channels of the readout

// K9: sinusoidal features -> Linear -> GELU -> Linear -> SiLU  (misc.py:20-32,54-67; SiLU of every block's time_mlp)
struct TimeMlpArgs {
    const float* time;      // [rows]
    int rows, dim;          // dim = sinusoid width, time_dim = 2*dim
    const float* w1;        // [2dim][dim]
    const float* b1;
    const float* w2;        // [2dim][2dim]
    const float* b2;
    float* silu_out;        // [rows][2dim]
    const float* learned_w = nullptr;  // LearnedSinusoidalPosEmb (misc.py:35-51): `learned_half` frequencies; features
    int learned_half = 0;              // [t, sin(2 pi t w), cos(2 pi t w)], w1 is [2dim][2 learned_half + 1]
};
hipError_t launch_time_mlp(const TimeMlpArgs& a, hipStream_t s);

// K9: per-block FiLM heads fused with the folded norm:  A = a_n*(1+scale), C = c_n*(1+scale)+shift  (all blocks of
// one network in one launch).  With no time embedding scale = shift = 0.
struct FilmArgs {
    const float* silu;      // [rows][tdim] or null
    int rows, tdim, total_c;
    const float* wf;        // [2*total_c][tdim]: per block, scale rows then shift rows (reference Linear layout)
    const float* bf;        // [2*total_c]
    const int* blk_of;      // [total_c] block index of each flattened channel
    const int* blk_off;     // [nblocks] flattened channel offset of each block
    const int* blk_cout;    // [nblocks]
    const float* norm_a;    // [total_c] folded norm scale (1 for the GroupNorm block)
    const float* norm_c;    // [total_c] folded norm shift (0 for the GroupNorm block)
    float* coef_a;          // [rows][total_c]
    float* coef_c;
};
hipError_t launch_film(const FilmArgs& a, hipStream_t s);

// K4+K1: outer bilinear resample of the channel-concatenated NCHW fp32 inputs fused with the 1x1 stem conv
// (unet_simple.py:185-195 upsampler + :166 init_conv) -> NHWC bf16.
struct StemArgs {
    const float* src[4];    // up to 4 NCHW fp32 tensors, concatenated on channels
    int ch[4];
    int nsrc, cin;          // cin = sum(ch)
    int n, h, w;            // native grid
    int src_rows;           // rows held by the source tensors (0: = n); output row r reads source row r % src_rows, so
                            // one launch can run the same inputs under several FiLM rows (paired interpolator calls)
    int out_pitch;          // fused-stem form only: channels per output pixel, 16 (or 0) or 8.  8 (cin <= 8): [rows][uh+2][uw+2][8], channels
                            // cin..7 zero and NO bias slot (conv_enc0_stem_kernel<.., P8> carries init_conv's bias in a k-step of its own)
    int distinct_only;      // fused-stem form only: write just the src_rows distinct rows of the output (rows r >= src_rows would be
                            // copies of row r % src_rows; conv_enc0_stem_kernel then reads each once, ConvArgs::src0_rows).  n stays
                            // the forward's row count.  0: all n rows
    int uh, uw;             // resampled grid (== h, w when there is no outer resampling)
    int resample;           // 0: identity, 1: resample to (uh, uw)
    int nearest;            // outer_sample_mode: 0 bilinear (align_corners=False), 1 nearest
    const float* wgt;       // [dim][cin] fp32
    const float* bias;      // [dim]
    int dim;
    el16_t* out;            // [n][uh][uw][dim]
    DropSpec drop;          // dropout_input on the 1x1 conv's output (stem_kernel only; mode 0 = off)
    // start of a forward that draws masks, folded into the fused-stem kernels (their block 0 does the work of
    // rng_begin_forward_kernel: nothing in the stem reads the row keys, the first consumer is the next launch): null = not folded
    uint32_t* rng_state;
    uint32_t* rng_row_keys;
    int rng_rows, rng_rows_per_fwd;
};
hipError_t launch_stem(const StemArgs& a, hipStream_t s);
// Fused-stem form: only the outer resample, written as a zero-bordered [n][uh+2][uw+2][16] bf16 tensor whose channel
// `cin` is 1 inside the image (carries init_conv's bias through the composed enc0 weights); the 1x1 conv itself is
// folded into the first encoder block's weights (engine.hip: compose_stem_enc0).  StemArgs::out_pitch == 8: 8-channel pixels without
// the bias slot (hipErrorInvalidValue when cin > 8).
hipError_t launch_stem16(const StemArgs& a, hipStream_t s);
// rows of the stem16 tensor a launch writes
inline __host__ __device__ int stem16_out_rows(const StemArgs& a) { return a.distinct_only && a.src_rows > 0 ? a.src_rows : a.n; }

// K2 (materialised form): bilinear x2 upsample of cat[src0, src1] (NHWC bf16) -> NHWC bf16
struct Up2xArgs {
    const el16_t* src0;
    const el16_t* src1;
    int c0, c1;
    int n, h, w;            // low-res dims
    el16_t* out;            // [n][2h][2w][c0+c1]
};
hipError_t launch_up2x(const Up2xArgs& a, hipStream_t s);

// Decoder blocks with a 1 x 1 conv (dec0, dec1 of unet_simple: Upsample(x2, bilinear) -> Conv2d(k = 1) -> BatchNorm -> FiLM -> ReLU ->
// Dropout, unet_simple.py:40-52,72-80): a pointwise conv commutes with the per-channel bilinear upsample (its taps sum to 1), so the
// conv runs on the LOW-res cat[x, skip] -- a quarter of the pixels, no materialised upsample -- into an fp32 tensor, and this pass
// upsamples it and applies the block's epilogue: out[n][2h][2w][c] = drop(act(lerp(lo) * A + C)).
struct Up2xEpiArgs {
    const float* lo;        // [n][h][w][c] fp32: the conv WITHOUT bias (the bias lives in C)
    int n, h, w, c;
    const float* coef_a;    // as ConvArgs: row = sample / coef_div, stride coef_stride
    const float* coef_c;
    int coef_stride, coef_div;
    int act;
    DropSpec drop;
    el16_t* out;            // [n][2h][2w][c]
};
hipError_t launch_up2x_epilogue(const Up2xEpiArgs& a, hipStream_t s);

// K5: GroupNorm(G) + FiLM + LeakyReLU + Dropout on an fp32 NHWC tensor -> NHWC bf16 (unet_simple.py:56 + :72-80)
struct GroupNormArgs {
    const float* x;         // [n][hw][c]
    int n, hw, c, groups;
    const float* gamma;
    const float* beta;
    const float* film_a;    // [rows][...] (1+scale) at film_off + ch ; stride film_stride (0 = broadcast)
    const float* film_c;
    int film_stride;
    int film_div;           // samples per coefficient row (0/1: one row per sample)
    int act;
    DropSpec drop;
    el16_t* out;
};
hipError_t launch_groupnorm(const GroupNormArgs& a, hipStream_t s);

// K3+K4: ConvTranspose2d(k4,s2,p1) readout evaluated only where the final bilinear resample needs it
// (unet_simple.py:141-151 + :195) -> NCHW fp32
struct ReadoutArgs {
    const el16_t* x;        // [n][ih][iw][cin] decoder output
    int n, ih, iw, cin;
    int iw_store;           // columns actually stored per row of x (== iw, or the compact width of the sparse-column decoder block)
    const int16_t* col_map; // [iw]: column -> stored column, -1 = not stored (compact x), or null
    const float* wgt;       // [kh][kw][cin][cout] fp32 (repacked ConvTranspose weight)
    const el16_t* wfrag;    // the same weights as MFMA 16x16x32 A fragments [16 taps][2 k halves][64 lanes][8] bf16 (cin == 64), or null
    const float* bias;      // [cout]
    int cout;
    int oh, ow;             // native grid
    int nearest;            // final resample: 0 bilinear, 1 nearest (outer_sample_mode)
    float* out;             // [n][cout][oh][ow]
    // per-geometry tap tables (launch_readout_tables, built once at weight upload), or null: entry = {int off[4]; float w[4]}.
    // row_tab[oy]: byte offset of input row i(oy, kh) inside a sample (i * iw_store * 128, -1 outside) and its bilinear row weight;
    // col_tab[ox]: byte offset of the stored input column j(ox, kw) (col_map applied, -1 outside) and its column weight
    const uint4* row_tab;
    const uint4* col_tab;
};
hipError_t launch_readout(const ReadoutArgs& a, hipStream_t s);
// once per process, outside any stream capture: the dynamic-LDS cap of the row-staged body of the DMA form (kernels.hip)
hipError_t readout_init();
// fills a.row_tab (oh entries of 32 B) / a.col_tab (ow entries) for the geometry and col_map of `a` (device pointers, writable)
hipError_t launch_readout_tables(const ReadoutArgs& a, hipStream_t s);
// readout.0.weight (cin,cout,4,4) -> ReadoutArgs::wgt's order [tap][cin][cout] (the weight upload and the op seam pack with these two)
inline std::vector<float> pack_readout_weights(const float* w, int cin, int cout) {
    std::vector<float> pk((size_t)16 * cin * cout);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int t = 0; t < 16; ++t) pk[((size_t)t * cin + ci) * cout + co] = w[((size_t)ci * cout + co) * 16 + t];
    return pk;
}
// [tap][64][cout <= 4] fp32 -> ReadoutArgs::wfrag: lane (m = lane & 15, kg = lane >> 4) of (tap, half) holds W[tap][half*32 + kg*8 + e][m]
inline std::vector<el16_t> pack_readout_frag(const std::vector<float>& pk, int cout) {
    std::vector<el16_t> wf((size_t)16 * 2 * 64 * 8, 0);
    for (int t = 0; t < 16; ++t)
        for (int h2 = 0; h2 < 2; ++h2)
            for (int lane = 0; lane < 64; ++lane) {
                const int m = lane & 15, kg = lane >> 4;
                for (int el = 0; el < 8; ++el)
                    if (m < cout)
                        wf[(((size_t)t * 2 + h2) * 64 + lane) * 8 + el] = f32_to_el16(pk[((size_t)t * 64 + h2 * 32 + kg * 8 + el) * cout + m]);
            }
    return wf;
}

// K10: sampler elementwise (dyffusion.py:381-391, :219-227)
hipError_t launch_cold_update(float* x_s, const float* x_cur, const float* x_next, long long count, hipStream_t s, float* copy = nullptr);
// out = tau*cond + (1-tau)*noise ; noise from `noise` if non-null else Box-Muller on the counter RNG
hipError_t launch_noisy_condition(float* out, const float* cond, const float* noise, float tau, long long count,
                                  int row_elems, uint32_t* rng_state, hipStream_t s);
// rng_state (device): {seed_lo, seed_hi, forward counter, global index of the engine's batch row 0, noise-call counter, ...}
#define DYF_RNG_STATE_WORDS 8

// boundary conditions of the physical-systems benchmark on a (fields, rows, C, H, W) fp32 stack, in place (kernels.hip)
struct BcArgs {
    float* preds;
    int kind;                    // 0 navier-stokes, 1 spring-mesh
    int n_fields, rows, c, h, w, n_meta;
    const int* row_meta;         // [rows]
    const float* time_factor;    // [n_fields] or [n_fields][n_meta]: 1 - exp(-5 t)
    int times_per_meta;
    const uint8_t* fixed_mask;   // [n_meta][c][h][w]
    const float* in_velocity;    // [n_meta]
    const float* vertex_y;       // [n_meta][w]
    const float* boundary;       // [n_meta][c][h][w]
};
hipError_t launch_boundary_conditions(const BcArgs& a, hipStream_t s);
hipError_t launch_nhwc_to_nchw_f32(const el16_t* src, int n, int h, int w, int w_store, int c, const int16_t* col_map,
                                   float* out, hipStream_t s);
hipError_t launch_rng_clone(uint32_t* dst, const uint32_t* src, uint32_t row_add, bool counters_only, hipStream_t s);
hipError_t launch_rng_begin_forward(uint32_t* rng_state, uint32_t* row_keys, int rows, int rows_per_fwd, hipStream_t s);
hipError_t launch_fill_f32(float* p, float v, long long count, hipStream_t s);
// sum of the criterion terms |p-t| (kind 0), (p-t)^2 (1), smooth-L1 (2) over `count` fp32 elements -> *sum (device double)
hipError_t launch_criterion_sum(const float* p, const float* t, long long count, int kind, double* sum, hipStream_t s);
// the same sum without atomics (deterministic training mode): one partial per workgroup to partials[CRITERION_MAX_BLOCKS], added in
// workgroup order by a second launch
constexpr int CRITERION_MAX_BLOCKS = 2048;
hipError_t launch_criterion_sum_det(const float* p, const float* t, long long count, int kind, double* partials, double* sum, hipStream_t s);
// points per workgroup of the ensemble kernels that stage a point's members in LDS: 256 up to 64 members (one KB of LDS per member),
// beyond that the largest power of two <= 128 with n_members * P floats <= 60 KB; 0 = none (no member, or more than 15 360)
inline int ensemble_tile_points(int n_members) {
    if (n_members < 1) return 0;
    if (n_members <= 64) return 256;
    int P = 128;
    while (P > 1 && (size_t)n_members * P * sizeof(float) > 60 * 1024) P >>= 1;
    return (size_t)n_members * P * sizeof(float) > 60 * 1024 ? 0 : P;
}
// on-device ensemble metrics (evaluation.py:10-118): sums[3] (fp64, device) = {sum (mean-y)^2, sum var, sum crps} over n_points
// points, member n at preds + n * n_points; up to 15 360 members (ensemble_tile_points).  Without atomics: launch 1 writes every
// wave's three sums to partials[ensemble_metrics_partial_doubles()], launch 2 (one workgroup) adds them in a fixed order into sums
long long ensemble_metrics_partial_doubles(int n_members, long long n_points);
hipError_t launch_ensemble_metrics(const float* preds, const float* targets, int n_members, long long n_points, double* partials,
                                   double* sums, hipStream_t s);
// the same per-point quantities per segment (dyf_trajectory_metrics), without atomics: launch 1 writes one {se, var, crps} partial per
// workgroup to partials[n_segments][trajectory_metrics_blocks()][3], launch 2 (one wave per segment) adds a segment's partials in a
// fixed order and writes out[3][n_segments] = {mse, ssr, crps} (accum[3][n_segments] += out when given).  preds_tab / targets_tab:
// device arrays of n_segments pointers; member n of segment s starts at preds_tab[s] + n * member_stride.
long long trajectory_metrics_blocks(int n_members, long long n_points);  // workgroups per segment; 0 = n_members beyond 15 360
hipError_t launch_trajectory_metrics(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                     long long n_points, long long member_stride, double* partials, double* out, double* accum,
                                     hipStream_t s);
// the metrics of every prefix predictions[:n], n = 1..n_members, of every segment (dyf_ensemble_size_metrics), without atomics:
// launch 1 leaves partials[n_segments][ensemble_size_metrics_groups()][n_members][4] (a workgroup walks several tiles), launch 2
// adds a segment's partials in workgroup order and writes out[4][n_segments][n_members] = {mse, ssr, crps, mse_per_mem}
// (accum += out when given).  Pointer tables and member_stride as launch_trajectory_metrics.
constexpr int ENSEMBLE_SIZE_MAX_MEMBERS = 256;
int ensemble_size_metrics_groups(int n_members, long long n_points);  // workgroups per segment (at most 64); 0 = n_members beyond the limit
hipError_t launch_ensemble_size_metrics(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                        long long n_points, long long member_stride, double* partials, double* out, double* accum,
                                        hipStream_t s);
// five scores per (segment, group) of the points viewed as row-major (n_outer, n_groups, n_inner) (dyf_ensemble_scores), without
// atomics: launch 1 writes ENSEMBLE_SCORES_PARTIAL doubles per workgroup to partials[n_segments][ensemble_scores_blocks()][9] (a
// workgroup's tile lies inside one (outer, group) slab), launch 2 (one wave per (segment, group)) joins a group's partials in a
// fixed order and writes out[5][n_segments][n_groups] = {mse, ssr, crps, nll, corr} (accum += out when given).  Pointer tables and
// member_stride as launch_trajectory_metrics.
constexpr int ENSEMBLE_SCORES_PARTIAL = 9;
constexpr long long ENSEMBLE_SCORES_MAX_BLOCKS = 0xffffffLL;  // workgroups per segment: 256 threads each, below 2^32 threads along x
// n_outer * n_groups * tiles <= ENSEMBLE_SCORES_MAX_BLOCKS (all three positive), without forming a product that could overflow
inline bool ensemble_geometry_fits(long long n_outer, int n_groups, long long tiles) {
    return tiles <= ENSEMBLE_SCORES_MAX_BLOCKS && n_outer <= ENSEMBLE_SCORES_MAX_BLOCKS / tiles &&
           (long long)n_groups <= ENSEMBLE_SCORES_MAX_BLOCKS / (tiles * n_outer);
}
// workgroups per segment = n_outer * n_groups * ceil(n_inner / tile); 0 = n_members beyond 15 360, -1 = beyond ENSEMBLE_SCORES_MAX_BLOCKS
long long ensemble_scores_blocks(int n_members, long long n_outer, int n_groups, long long n_inner);
hipError_t launch_ensemble_scores(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                  long long member_stride, long long n_outer, int n_groups, long long n_inner, double* partials,
                                  double* out, double* accum, hipStream_t s);
// forecast products per point (dyf_ensemble_products; ensemble_products.hip): out[n_segments][planes][n_points] fp32, the planes
// asked for in the order mean, std, min, max, quantiles, exceedances.  A quantile is given by the order statistics lo <= hi it lies
// between and the fp32 fraction (the host computes them from (n_members - 1) q in double).  One launch, no workspace, no atomics.
constexpr int ENSEMBLE_PRODUCTS_MAX_QUANTILES = 16;   // DYF_MAX_PRODUCT_QUANTILES
constexpr int ENSEMBLE_PRODUCTS_MAX_THRESHOLDS = 16;  // DYF_MAX_PRODUCT_THRESHOLDS
constexpr long long ENSEMBLE_PRODUCTS_MAX_BLOCKS = 0xffffffLL;  // workgroups per segment, as ENSEMBLE_SCORES_MAX_BLOCKS
struct EnsembleProductsParams {
    int mean, std, min, max;  // 0 / 1
    int n_quantiles, n_thresholds;
    int lo[ENSEMBLE_PRODUCTS_MAX_QUANTILES], hi[ENSEMBLE_PRODUCTS_MAX_QUANTILES];
    float frac[ENSEMBLE_PRODUCTS_MAX_QUANTILES];
    float thresholds[ENSEMBLE_PRODUCTS_MAX_THRESHOLDS];
};
long long ensemble_products_blocks(int n_members, long long n_points);  // workgroups per segment; 0 = n_members beyond 15 360
hipError_t launch_ensemble_products(const float* const* preds_tab, int n_segments, int n_members, long long n_points,
                                    long long member_stride, const EnsembleProductsParams& pr, float* out, hipStream_t s);
// the rank histogram per (segment, group) of the geometry of launch_ensemble_scores (dyf_rank_histogram; ensemble_products.hip),
// without atomics: launch 1 leaves partials[n_segments][n_groups][rank_histogram_chunks()][n_members + 1], launch 2 adds a group's
// chunks in chunk order and writes out[n_segments][n_groups][n_members + 1] (accum += out when given).
constexpr int RANK_HISTOGRAM_MAX_MEMBERS = 1024;
constexpr int RANK_HISTOGRAM_MAX_CHUNKS = 256;  // partial histograms per (segment, group)
// partial histograms per group = min(n_outer * ceil(n_inner / 256), 256); 0 = bad arguments or n_members beyond the limit, -1 = the
// geometry is beyond the workgroup limit of ensemble_scores_blocks
int rank_histogram_chunks(int n_members, long long n_outer, int n_groups, long long n_inner);
hipError_t launch_rank_histogram(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                 long long member_stride, long long n_outer, int n_groups, long long n_inner, double* partials,
                                 double* out, double* accum, hipStream_t s);
// the energy score and the member-distance matrix per (segment, group) of the geometry of launch_ensemble_scores (dyf_energy_score;
// energy_score.hip), without atomics.  A vector is one (outer, group) slab of n_inner points.  Launch 1 leaves float64 sums of squared
// differences in workspace[n_segments][vectors][chunks][N][N + 1] (entry (i, j), i < j < N: members i and j; entry (i, N): member i and
// the target), launch 2 takes the square roots of the chunk sums and their mean over outer into workspace + partial_doubles
// [n_segments][n_groups][N][N + 1], launch 3 writes out[4][n_segments][n_groups] = {es, es_fair, dist_target, dist_pair} (accum += out
// when given) and, when given, member_out[n_segments][n_groups][N] and pair_out[n_segments][n_groups][N][N].
constexpr int ENERGY_SCORE_MAX_MEMBERS = 256;                 // DYF_ENERGY_MAX_MEMBERS
constexpr int ENERGY_SCORE_TILE_POINTS = 64;                  // DYF_ENERGY_TILE_POINTS
constexpr long long ENERGY_SCORE_MAX_WORKSPACE = 1LL << 27;   // DYF_ENERGY_MAX_WORKSPACE_DOUBLES
struct EnergyScorePlan {
    int blocks;                 // ceil(N / 64) slabs of 64 members
    int block_pairs;            // blocks * (blocks + 1) / 2 pairs (bi <= bj)
    int chunks;                 // workgroups that share a vector's tiles (1 = the vector is not split)
    long long vectors;          // n_outer * n_groups per segment
    long long tiles_per_chunk;  // consecutive tiles of ENERGY_SCORE_TILE_POINTS points per chunk
    long long partial_doubles, mean_doubles;  // the two regions of the workspace
};
// 0 = ok; 1 = bad arguments or n_members beyond the limit; -1 = the workspace would exceed ENERGY_SCORE_MAX_WORKSPACE doubles
int energy_score_plan(int n_segments, int n_members, long long n_outer, int n_groups, long long n_inner, EnergyScorePlan* plan);
hipError_t launch_energy_score(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                               long long member_stride, long long n_outer, int n_groups, long long n_inner, double* workspace,
                               double* out, double* member_out, double* pair_out, double* accum, hipStream_t s);
// the radially binned power spectra of an ensemble per (segment, channel) (dyf_power_spectrum; power_spectrum.hip), without atomics.
// Launch 1 leaves xbar (fp32) in workspace[0 .. mean_doubles), launch 2 every workgroup's four float64 coefficient planes in
// workspace + mean_doubles [workgroups][4][nky * 16][16] and its shell sums behind them [workgroups][4][n_bins + 1] (bin n_bins: the
// corners), launch 3 writes out[n_segments][C][4][n_bins + 1] (last column: the plane's total; accum += out when given).
constexpr int POWER_SPECTRUM_MAX_DIM = 1024;                  // DYF_SPECTRUM_MAX_DIM
constexpr int POWER_SPECTRUM_MAX_MEMBERS = 256;               // DYF_SPECTRUM_MAX_MEMBERS
constexpr long long POWER_SPECTRUM_MAX_WORKSPACE = 1LL << 27; // DYF_SPECTRUM_MAX_WORKSPACE_DOUBLES
struct PowerSpectrumPlan {
    int tiles;   // ceil((W / 2 + 1) / 16) tiles of kx columns
    int nky;     // ceil(H / 16) tiles of ky rows
    int n_bins;  // max(H, W) / 2 + 1
    long long fields, workgroups;  // B * C; n_segments * fields * tiles
    long long mean_doubles, plane_doubles, partial_doubles;  // the three regions of the workspace
};
// 0 = ok; 1 = bad arguments or a limit exceeded; -1 = the workspace would exceed POWER_SPECTRUM_MAX_WORKSPACE doubles
int power_spectrum_plan(int n_segments, int n_members, int batch, int channels, int H, int W, PowerSpectrumPlan* plan);
// the shell of coefficient (ky, kx) of an H x W transform by the exact integer rule (may be >= n_bins: a corner)
int power_spectrum_bin(int H, int W, int ky, int kx);
struct PowerSpectrumTables {  // per geometry, on the device: twiddles and Hann tables (float64 on the host, rounded to fp32), shell lists
    int H = 0, W = 0;
    float* tables = nullptr;             // cosW[W] sinW[W] cosH[H] sinH[H] winH[H] winW[W]
    unsigned short* csr_idx = nullptr;   // [tiles][H * 16]
    int* csr_off = nullptr;              // [tiles][n_bins + 2]
};
hipError_t power_spectrum_tables_create(int H, int W, PowerSpectrumTables* t);  // allocates and copies synchronously
void power_spectrum_tables_destroy(PowerSpectrumTables* t);
hipError_t launch_power_spectrum(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                 long long member_stride, int batch, int channels, int H, int W, int window,
                                 const PowerSpectrumTables& t, double* workspace, double* out, double* accum, hipStream_t s);

// dyf_sample_gather: all-gather receive layout [world][slots][nb][row floats] -> [slots][total_rows][row] in global row order;
// rank r owns the contiguous block of rows shard(r) (the first total_rows % world ranks one extra), its padding rows are dropped
hipError_t launch_gather_unpack(const float* recv, float* out, int world, int slots, int nb, int total_rows, long long row, hipStream_t s);
