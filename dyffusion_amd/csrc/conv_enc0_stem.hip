// enc0 on the fused stem (gfx950): the first encoder block's 4x4 / stride-2 conv over the zero-bordered 16-channel stem16
// tensor (kernels.hip stem16_kernel; init_conv is composed into the weights, engine.hip compose_stem_enc0), K = 16 taps x 16
// channels = 256, cout = 64 or 128.  Reference: unet_simple.py:184-195 (cat -> Upsample -> init_conv) + :121,166 (first UNetBlock).
//
// The layer is HBM-bound: per output pixel 128 B of unique input and 2 * cout B of output against 2 * 256 * cout flop
// (170 flop/byte at cout = 128, under the 312 of the machine).  The general implicit-GEMM kernel (conv_igemm2.hip) spends its time
// in the prologue / epilogue of a K loop of only four 64-wide steps: 447 us for 1.0 GB at NB = 160 (2.25 TB/s).  Here
//   * the pixel operand never touches LDS: with the channel-contiguous 16-channel pixels, the MFMA fragment of k-step s = (kh, kw)
//     is ONE 16-byte global load per lane (lane = output pixel, hi = channel half); the 16 loads of a tile are issued a whole tile
//     ahead of their use, neighbouring taps / rows hit the L1 / L2;
//   * the weights (cout x 256 x 2 B <= 64 KB) stay in LDS as MFMA A fragments for the lifetime of the workgroup, which is
//     persistent: one 8-wave workgroup per CU walks a contiguous range of 32-pixel row segments (a wave keeps its column segment and moves
//     down the rows, so half of its input rows were fetched by its previous tile);
//   * operands are swapped (D^T = W X^T) so the epilogue runs from the accumulators exactly as in conv_igemm2.hip: lane (pixel, hi)
//     holds channels 32 nt + 8 g + 4 hi + {0..3}, exchanged pairwise (v_permlane32_swap) into 16-byte channel rows;
//   * a tile's output (32 pixels x cout channels) is one contiguous run of memory: the 16-byte rows go through a per-wave LDS
//     staging tile and leave as whole 1 KB wave stores: 327 -> 260 us at 160 rows against storing the 32-byte pieces of the
//     128-byte lines straight from the registers, ~100 instructions apart (8 times the store instructions' address work in the
//     texture path; the WRITE_SIZE counter reads 1.42-1.44x the algorithmic bytes for BOTH forms and 1.00x for conv_igemm2, so
//     it is not what separated them).
// Paired launches (ConvArgs::src0_rows = rows held by the stem tensor, n = COPIES x rows): the kernel walks the tiles of the distinct
// rows only -- one load set and one K pass per tile -- and runs the epilogue COPIES times from the same accumulators, copy j with the
// coefficient row, the dropout row key and the output tile of sample r + j * rows.  Per output element the arithmetic is that of a
// pass of its own: the result is bitwise what the un-paired launch gives.
// 8-channel stem (P8, ConvArgs::pix_pitch0 == 8; at most 8 input channels): a pixel is ONE 16-byte load, so k-step s = (kh, kw pair)
// takes pixel (2 oy + kh, 2 ox + 2 kp + hi) -- 8 loads and 8 k-steps per tile instead of 16.  init_conv's bias, which the 16-channel
// stem carries as a 1 in channel slot cin, rides in a ninth k-step: the pixel operand is the 0/1 "tap inside the image" indicator of
// the 16 taps, computed from (oy, ox) without a load, against the composed per-tap bias weights -- the same 16-bit values times the
// same ones, so only the order of the fp32 sums differs from the 16-channel form.
#include "conv.h"
#include "conv_epilogue.h"

#include <type_traits>
typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace {
constexpr int E0_KSTEPS = 16;
constexpr int e0_xsteps(bool p8) { return p8 ? 8 : 16; }  // pixel loads per tile
constexpr int e0_wsteps(bool p8) { return p8 ? 9 : 16; }  // k-steps (weight fragments) per tile
constexpr int E0_WAVES = 8, E0_THREADS = E0_WAVES * 64;  // one workgroup per CU: the weights are fetched once per CU
constexpr int E0_MAX_COPIES = 2;  // (a paired interpolator launch; every copy has its own coefficient row in LDS)
constexpr int e0_lds_bytes(int nt, int copies, bool p8) { return e0_wsteps(p8) * nt * 1024 + copies * E0_WAVES * 2 * nt * 32 * 4 + E0_WAVES * 32 * (nt * 64 + 16); }
}

template <int NT, int COPIES, bool P8>  // cout / 32; output samples per stem row (`tiles` counts the tiles of the distinct rows); 8-channel stem
__global__ __launch_bounds__(512) void conv_enc0_stem_kernel(ConvArgs a, const el16_t* __restrict__ wfrag, int tiles, int tiles_per_wg) {
#if defined(__gfx950__)
    extern __shared__ __attribute__((aligned(16))) unsigned char e0_smem[];
    constexpr int XS = e0_xsteps(P8), WS = e0_wsteps(P8);
    uint4* wl = (uint4*)e0_smem;  // [WS k-steps][NT][64 lanes]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, hi = lane >> 5;
    for (int i = tid; i < WS * NT * 64; i += E0_THREADS) wl[i] = ((const uint4*)wfrag)[i];
    __syncthreads();
    // Epilogue coefficients live in a per-wave LDS row, refreshed when the wave's tile moves to another coefficient row (sample):
    // loaded from global memory inside the epilogue they would make every (nt, g2) step wait for vmcnt(0), i.e. for the
    // acknowledgement of the stores of the step before (gfx9 counts stores in vmcnt) -- 8 exposed store round trips per tile.
    float* coefl_w = (float*)(e0_smem + WS * NT * 1024) + wave * (COPIES * 2 * NT * 32);  // [copy][a | c][cout]
    int coef_row[COPIES];
#pragma unroll
    for (int j = 0; j < COPIES; ++j) coef_row[j] = -1;
    // output staging tile of this wave: [32 pixels][cout * 2 B + 16 B pad] (the pad spreads the pixels' rows over the banks)
    constexpr int OROW = NT * 64 + 16;
    unsigned char* ostage = e0_smem + WS * NT * 1024 + COPIES * E0_WAVES * 2 * NT * 32 * 4 + wave * (32 * OROW);
    const int segs = a.wo >> 5;               // 32-pixel segments per output row
    const int plane = a.ho * a.wo;
    const int t0 = blockIdx.x * tiles_per_wg, t1 = min(t0 + tiles_per_wg, tiles);
    const int cout = NT * 32;

    // the 16 pixel fragments of tile t: k-step s = kh * 4 + kw reads padded input pixel (2 oy + kh, 2 ox + kw), channels 8 hi ..
    // (P8: k-step s = kh * 2 + kp reads the 8 channels of pixel (2 oy + kh, 2 ox + 2 kp + hi))
    auto load = [&](int t, uint4 (&xf)[XS]) {
        const int row = t / segs, seg = t - row * segs;     // row = n * ho + oy
        const int n = row / a.ho, oy = row - n * a.ho;
        if constexpr (P8) {
            const el16_t* p = a.src0 + ((size_t)(n * a.h + 2 * oy) * a.w + 2 * (seg * 32 + l31) + hi) * 8;
#pragma unroll
            for (int kh = 0; kh < 4; ++kh)
#pragma unroll
                for (int kp = 0; kp < 2; ++kp) xf[kh * 2 + kp] = *(const uint4*)(p + ((size_t)kh * a.w + 2 * kp) * 8);
        } else {
            const el16_t* p = a.src0 + ((size_t)(n * a.h + 2 * oy) * a.w + 2 * (seg * 32 + l31)) * 16 + 8 * hi;
#pragma unroll
            for (int kh = 0; kh < 4; ++kh)
#pragma unroll
                for (int kw = 0; kw < 4; ++kw) xf[kh * 4 + kw] = *(const uint4*)(p + ((size_t)kh * a.w + kw) * 16);
        }
        __builtin_amdgcn_sched_barrier(0);  // issue them HERE, a tile ahead: sunk to their uses (the scheduler's choice) every k-step waits for its own load
    };

    auto tile = [&](int td, const uint4 (&xf)[XS], auto act_c, auto mode_c) {
        constexpr int ACT = decltype(act_c)::value, MODE = decltype(mode_c)::value;
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
#pragma unroll
        for (int s = 0; s < WS; ++s) {
            int wlane = lane;
            asm volatile("" : "+v"(wlane));  // keep the (loop-invariant) weight reads inside the tile loop: hoisted they are 256 registers
            uint4 xs;
            if constexpr (P8) {
                if (s < XS) {
                    xs = xf[s];
                } else {
                    // the bias step: lane (l31, hi) holds taps 8 hi + {0..7} = rows kh = 2 hi, 2 hi + 1 x columns kw = 0..3 of the window of
                    // output pixel (oy, ox); a tap is 1 where its padded pixel (2 oy + kh, 2 ox + kw) lies inside the image
                    const int row = td / segs, seg = td - row * segs;
                    const int oy = row % a.ho, ox = seg * 32 + l31;
                    const int py = 2 * oy + 2 * hi, px = 2 * ox;
                    const bool r0 = py >= 1 && py <= a.h - 2, r1 = py + 1 <= a.h - 2;  // (py + 1 >= 1 always)
                    const float c0 = px >= 1 ? 1.0f : 0.0f, c3 = px + 3 <= a.w - 2 ? 1.0f : 0.0f;  // (columns px + 1, px + 2: always inside)
                    const uint32_t w01 = pack_el16x2(c0, 1.0f), w23 = pack_el16x2(1.0f, c3);
                    xs = make_uint4(r0 ? w01 : 0u, r0 ? w23 : 0u, r1 ? w01 : 0u, r1 ? w23 : 0u);
                }
            } else {
                xs = xf[s];
            }
            const el16x8_t xb = __builtin_bit_cast(el16x8_t, xs);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = DYF_MFMA_32x32x16(__builtin_bit_cast(el16x8_t, wl[(s * NT + nt) * 64 + wlane]), xb, acc[nt], 0, 0, 0);
        }
        // ---- epilogue (the scheme of conv_igemm2.hip), once per copy of the tile's stem row
#pragma unroll
        for (int j = 0; j < COPIES; ++j) {
        const int t = td + j * tiles;           // output tile of copy j: sample + j * src0_rows
        float* coefl = coefl_w + j * (2 * NT * 32);
        const int m = t * 32 + l31;             // output pixel: tiles are ordered (n, oy, segment)
        const int n_img = m / plane;
        const uint32_t ob = (uint32_t)m * (uint32_t)cout;
        const RngKey key = drop_row_key(a.drop, n_img);
        const uint32_t row0 = (uint32_t)n_img * (uint32_t)(plane * cout);
        const int crow = __builtin_amdgcn_readfirstlane(a.coef_div > 1 ? n_img / a.coef_div : n_img);  // one sample per tile
        if (crow != coef_row[j]) {
            coef_row[j] = crow;
            const float ps = drop_prescale<ACT, MODE>(a.drop);  // dropout scale folded into the affine, once per row
            if (lane < NT * 8) {
                float4 ca = *(const float4*)(a.coef_a + (size_t)crow * a.coef_stride + lane * 4);
                float4 cc = *(const float4*)(a.coef_c + (size_t)crow * a.coef_stride + lane * 4);
                ca.x *= ps; ca.y *= ps; ca.z *= ps; ca.w *= ps;
                cc.x *= ps; cc.y *= ps; cc.z *= ps; cc.w *= ps;
                *(float4*)(coefl + lane * 4) = ca;
                *(float4*)(coefl + NT * 32 + lane * 4) = cc;
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            uint4 o2[2];
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
                const int cg0 = nt * 32 + 16 * g2;
                float ca[8], cc[8];  // the row's table in LDS is already scaled
                epi_coef(coefl + cg0 + 4 * hi, coefl + NT * 32 + cg0 + 4 * hi, 1.0f, ca, cc);
                const uint32_t e0 = ob + cg0 + 4 * hi;
                o2[g2] = epi_step<ACT, MODE>(acc[nt], 8 * g2, ca, cc, e0, row0, a.drop, key);
            }
            *(uint4*)(ostage + l31 * OROW + (nt * 32 + 8 * hi) * 2) = o2[0];
            *(uint4*)(ostage + l31 * OROW + (nt * 32 + 16 + 8 * hi) * 2) = o2[1];
        }
        // the tile is cout * 64 contiguous bytes of the output: store instruction k writes bytes [1024 k, 1024 k + 1024)
        el16_t* tbase = a.out_el16 + (size_t)t * 32 * cout;
#pragma unroll
        for (int k = 0; k < NT * 2; ++k) {
            const int off = k * 1024 + lane * 16;                 // byte offset inside the tile
            const int px = off / (NT * 64), within = off - px * (NT * 64);
            const uint4 ov = *(const uint4*)(ostage + px * OROW + within);
            *(uint4*)((unsigned char*)tbase + off) = ov;
        }
        }
    };

    auto run = [&](auto act_c, auto mode_c) {
        // Every wave owns an even number of tiles (launcher: tiles per workgroup and the tile count are multiples of 16), and both
        // prefetches are unconditional (the one past the wave's last tile re-reads a valid tile): no branch joins between a
        // load and its use, so the compiler's s_waitcnt vmcnt counts stay exact and the loads really fly a tile ahead.  (With
        // `if (more) load(...)` the join made every k-step wait for the NEWEST 16 loads.)
        uint4 xa[XS], xb[XS];
        int t = t0 + wave;
        if (t >= t1) return;
        load(t, xa);
        for (; t < t1; t += 2 * E0_WAVES) {  // two tiles per turn: the fragment sets swap roles without register moves
            load(t + E0_WAVES, xb);
            tile(t, xa, act_c, mode_c);
            load(t + 2 * E0_WAVES < t1 ? t + 2 * E0_WAVES : t, xa);
            tile(t + E0_WAVES, xb, act_c, mode_c);
        }
    };
    epi_dispatch(a.act, a.drop.mode, run);
#endif
}

// wpk [cout][4 (kh)][64 = kw * 16 + c] (the composed weights of engine.hip, K index k = kh * 64 + kw * 16 + c) -> A fragments
// [k-step s][nt][lane][8]: lane (l31, hi) holds channel 32 nt + l31, k = 16 s + 8 hi + {0..7}
void pack_enc0_stem_frag(const el16_t* wpk, int cout, el16_t* out) {
    const int nt_n = cout / 32;
    for (int s = 0; s < E0_KSTEPS; ++s)
        for (int nt = 0; nt < nt_n; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j)
                    out[(((size_t)s * nt_n + nt) * 64 + lane) * 8 + j] = wpk[(size_t)(32 * nt + (lane & 31)) * 256 + 16 * s + 8 * (lane >> 5) + j];
}

// The same composed weights for the 8-channel stem (cin <= 8 input channels; slot cin of wpk holds the per-tap bias weights) -> A
// fragments [9 k-steps][nt][lane][8]: k-step s = kh * 2 + kp < 8: lane (l31, hi) holds channel 32 nt + l31, tap (kh, 2 kp + hi), input
// channels 0..7 (cin.. are zero); k-step 8: the bias weights of taps 8 hi + {0..7}
void pack_enc0_stem_frag8(const el16_t* wpk, int cout, int cin, el16_t* out) {
    const int nt_n = cout / 32;
    for (int s = 0; s < 9; ++s)
        for (int nt = 0; nt < nt_n; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const size_t co = (size_t)(32 * nt + (lane & 31)), hi = (size_t)(lane >> 5);
                    el16_t v{};
                    if (s == 8) v = wpk[co * 256 + (8 * hi + j) * 16 + cin];
                    else if (j < cin) v = wpk[co * 256 + ((s >> 1) * 4 + 2 * (s & 1) + hi) * 16 + j];
                    out[(((size_t)s * nt_n + nt) * 64 + lane) * 8 + j] = v;
                }
}

// output samples per row of the stem tensor (ConvArgs::src0_rows), 0 = a row count the batch is no multiple of
static int e0_copies(const ConvArgs& a) {
    if (a.src0_rows <= 0 || a.src0_rows == a.n) return 1;
    return a.n % a.src0_rows == 0 ? a.n / a.src0_rows : 0;
}

// the fused-stem view of enc0 (engine.hip fused_enc0_args): 16-channel pixels declared as 64-channel ones, kh = 4, kw = 1
bool conv_enc0_stem_supported(const ConvArgs& a) {
    const bool on = dyf_form_int("DYF_ENC0_STEM", 1) != 0;
    if (!on || (a.pix_pitch0 != 16 && a.pix_pitch0 != 8) || a.c0 != 64 || a.c1 != 0 || a.kh != 4 || a.kw != 1 || a.stride != 2 || a.pad != 0) return false;
    if (a.up2x || a.residual || a.out_f32 || !a.out_el16 || (a.cout != 64 && a.cout != 128)) return false;
    if (a.wo % 32 != 0 || (a.ho * (a.wo / 32)) % 16 != 0 || a.h != 2 * a.ho + 2 || a.w != 2 * a.wo + 2) return false;
    const int copies = e0_copies(a);
    if (copies < 1 || copies > E0_MAX_COPIES) return false;
    const long long nsel = (a.n_sel > 0 ? a.n_sel : a.n) / copies;  // the tiles walked are those of the distinct rows
    if (nsel * a.ho * (a.wo / 32) < 4096) return false;  // persistent form: needs >= 16 tiles for each of 256 workgroups
    return (size_t)a.n * a.ho * a.wo * a.cout < 0xFFFFFFF0ull;
}

namespace {
template <int NT, int COPIES, bool P8>
hipError_t e0_set_lds() {
    return hipFuncSetAttribute((const void*)conv_enc0_stem_kernel<NT, COPIES, P8>, hipFuncAttributeMaxDynamicSharedMemorySize, e0_lds_bytes(NT, COPIES, P8));
}
template <int NT, int COPIES, bool P8>
void e0_launch(const ConvArgs& a, const el16_t* wfrag, int nwg, int tiles, int per, hipStream_t stream) {
    hipLaunchKernelGGL((conv_enc0_stem_kernel<NT, COPIES, P8>), dim3(nwg), dim3(E0_THREADS), e0_lds_bytes(NT, COPIES, P8), stream, a, wfrag, tiles, per);
}
template <int NT>
void e0_launch_nt(const ConvArgs& a, const el16_t* wfrag, int copies, int nwg, int tiles, int per, hipStream_t stream) {
    const bool p8 = a.pix_pitch0 == 8;
    if (copies == 1 && !p8) e0_launch<NT, 1, false>(a, wfrag, nwg, tiles, per, stream);
    else if (copies == 1) e0_launch<NT, 1, true>(a, wfrag, nwg, tiles, per, stream);
    else if (!p8) e0_launch<NT, 2, false>(a, wfrag, nwg, tiles, per, stream);
    else e0_launch<NT, 2, true>(a, wfrag, nwg, tiles, per, stream);
}
}  // namespace

hipError_t conv_enc0_stem_init() {
    for (hipError_t e : {e0_set_lds<4, 1, false>(), e0_set_lds<2, 1, false>(), e0_set_lds<4, 2, false>(), e0_set_lds<2, 2, false>(),
                         e0_set_lds<4, 1, true>(), e0_set_lds<2, 1, true>(), e0_set_lds<4, 2, true>(), e0_set_lds<2, 2, true>()})
        if (e != hipSuccess) return e;
    return hipSuccess;
}

hipError_t launch_conv_enc0_stem(const ConvArgs& a, const el16_t* wfrag, hipStream_t stream) {
    const int copies = e0_copies(a);
    if (copies < 1 || copies > E0_MAX_COPIES) return hipErrorInvalidValue;
    const int tiles = (a.n / copies) * a.ho * (a.wo / 32);  // of the distinct rows
    int nwg = std::min(256, (tiles + 15) / 16);
    int per = (tiles + nwg - 1) / nwg;
    per = (per + 15) / 16 * 16;  // a wave keeps its column segment (wo = 128: 4 segments) and its fragment-set parity
    nwg = (tiles + per - 1) / per;
    dyf_form_note("conv_enc0_stem_kernel", a.n);
    if (a.cout == 128) e0_launch_nt<4>(a, wfrag, copies, nwg, tiles, per, stream);
    else e0_launch_nt<2>(a, wfrag, copies, nwg, tiles, per, stream);
    return hipGetLastError();
}
