// Conv2d on NHWC bf16 for gfx950 (MI355X): implicit-GEMM on MFMA + a shape-agnostic direct kernel.
//
// Replaces the reference's nn.Conv2d -> BatchNorm2d -> FiLM -> (Leaky)ReLU -> Dropout ATen sequence
// (src/models/unet_simple.py:29-82) with one kernel per UNetBlock.
//
// Implicit GEMM:  Y[M = N*Ho*Wo pixels][Cout] = A[M][K = taps*Cin] * Wpk[Cout][K]^T
//   * K is walked one (tap, 64-channel chunk) per step: with NHWC activations every A row of a step is one contiguous
//     128-byte segment of one input pixel, so the A tile is a pure gather of 128-B rows.  Rows are fetched with
//     LDS-DMA (global_load_lds_dwordx4, 16 B/lane, 1 KiB per wave instruction); taps that fall into the zero padding
//     read a 128-B zero page instead.  Weights are pre-packed [Cout][tap][Cin] so a B row is the same kind of segment.
//   * LDS image per stage: A[BM][64] + B[BN][64] bf16, row = 128 B, 16-B chunk index XOR (row & 7): the DMA writes LDS
//     linearly, so the swizzle is applied to the per-lane SOURCE chunk and again on the ds_read_b128 fragment reads.
//   * 4 waves, each owns a 64x64 accumulator (2x2 MFMA 32x32x16 bf16 tiles, 64 fp32 regs); two stages, one barrier per
//     K step, next step's DMA in flight under the current step's 16 MFMAs.
//   * operands swapped (D^T = W X^T): an accumulator lane holds 4 consecutive channels of one pixel, so the epilogue --
//     per-(sample, channel) affine (conv bias + BatchNorm + FiLM folded) -> activation -> dropout (+ residual) -> bf16 --
//     runs straight out of the accumulators (v_permlane32_swap pairs lanes l / l+32 for 16-B stores): no LDS round trip.
//   * dispatch (conv_dispatch.hip conv_choose_form): fused-upsample convs and plain 3x3-s1 / 4x4-s2 convs with 256-channel
//     blocks -> the halo kernel (conv_up_halo.hip); other convs with cout % 128 == 0 and >= 384 tiles -> conv_igemm2_kernel (weights
//     streamed in fragment order); the rest -> this file's conv_igemm_kernel; channels % 64 != 0 -> conv_direct_kernel.
//   * blockIdx -> tile map is XCD-aware (block b runs on XCD b % 8): every XCD walks a contiguous range of tiles so
//     the 3x3 / 4x4 halo re-reads of neighbouring tiles hit that XCD's own L2.
#include "conv.h"
#include "conv_epilogue.h"

#include <algorithm>
#include <type_traits>

typedef __attribute__((ext_vector_type(16))) float f32x16;

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

// ------------------------------------------------------------------------------------------------ epilogue math
struct EpiCtx {
    const float* coef_a;
    const float* coef_c;
    int coef_stride;
    int act;
    int cout;
    int howo;
};

// ------------------------------------------------------------------------------------------------ direct kernel
// One thread per (output pixel, output channel).  Correct for every shape; used for layers the MFMA path does not
// cover (channel counts that are not multiples of 64) and as the on-device cross-check of the MFMA kernel.
__global__ void conv_direct_kernel(ConvArgs a, long long total) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int co = (int)(idx % a.cout);
    const long long m = idx / a.cout;
    const int howo = a.ho * a.wo;
    const int n = (int)(m / howo);
    const int rem = (int)(m % howo);
    const int oy = rem / a.wo, ox = rem % a.wo;
    const int cin = a.c0 + a.c1;
    const el16_t* wrow = a.wpk + (size_t)co * a.kh * a.kw * cin;
    float acc = 0.0f;
    for (int ky = 0; ky < a.kh; ++ky) {
        const int iy = oy * a.stride - a.pad + ky;
        if ((unsigned)iy >= (unsigned)a.h) continue;
        for (int kx = 0; kx < a.kw; ++kx) {
            const int ix = ox * a.stride - a.pad + kx;
            if ((unsigned)ix >= (unsigned)a.w) continue;
            const size_t pix = ((size_t)n * a.h + iy) * a.w + ix;
            const el16_t* wt = wrow + (size_t)(ky * a.kw + kx) * cin;
            const el16_t* p0 = a.src0 + pix * (a.pix_pitch0 ? a.pix_pitch0 : a.c0);
            for (int c = 0; c < a.c0; ++c) acc = fmaf(el16_to_f32(p0[c]), el16_to_f32(wt[c]), acc);
            if (a.c1 > 0) {
                const el16_t* p1 = a.src1 + pix * a.c1;
                for (int c = 0; c < a.c1; ++c) acc = fmaf(el16_to_f32(p1[c]), el16_to_f32(wt[a.c0 + c]), acc);
            }
        }
    }
    const size_t ci = (size_t)(a.coef_div > 1 ? n / a.coef_div : n) * a.coef_stride + co;
    float v = fmaf(acc, a.coef_a[ci], a.coef_c[ci]);
    v = apply_act(v, a.act);
    const uint32_t e = (uint32_t)(m * a.cout + co);
    v = drop_apply(v, e, (uint32_t)n * (uint32_t)(a.ho * a.wo * a.cout), a.drop, drop_row_key(a.drop, n));
    if (a.residual) v += el16_to_f32(a.residual[(size_t)m * a.cout + co]);
    if (a.out_el16) a.out_el16[(size_t)m * a.cout + co] = f32_to_el16(v);
    if (a.out_f32) a.out_f32[(size_t)m * a.cout + co] = v;
}

// ------------------------------------------------------------------------------------------------ MFMA kernel
// Gather addressing: every A row a lane fetches is described by a 32-bit byte offset of its window origin
// (n, oy*stride-pad, ox*stride-pad) in each source plus a bit mask of the taps that fall inside the image.  Per K
// step the lane adds one wave-uniform (tap, chunk) byte offset and selects "out of range" for padded taps: the
// LDS-DMA is a raw buffer load (buffer_load_dwordx4 ... offen lds), whose bounds check returns zeros for offsets
// beyond num_records, so the zero padding costs no memory traffic and ~4 VALU instructions per row.
//
// UP = 1: nn.Upsample(scale_factor=2, bilinear) + Conv2d(3x3, pad 1) of a decoder block (unet_simple.py:40-52) fused
// by PHASE DECOMPOSITION.  Output pixel (2i+py, 2j+px) is a 3x3 stencil over the LOW-res pixels (i+a, j+b) with
// weights that are fixed linear combinations of the 3x3 kernel (host: pack_up2x_weights); replicate-clamping the tap
// coordinates reproduces the edge behaviour of align_corners=False.  What clamping cannot express is the conv's ZERO
// padding of the upsampled image (up[-1] = 0 while the clamped stencil yields in[0]); it is repaired by extra
// "correction taps" that only the first/last output row/column see: -w[ky=0,:] on the border row, -w[:,kx=0] on the
// border column and +w[0,0] on the corner (inclusion/exclusion).  Per phase the packed K axis therefore has 16 taps:
// 0-8 stencil, 9-11 row correction, 12-14 column correction, 15 corner; tiles that touch no border skip 9-15.
// The upsampled tensor (4x the bytes of its input) is never materialised and the FLOP count equals the direct conv's.
struct StepInfo {       // wave-uniform description of the K step being issued
    int dy, dx;         // tap displacement in input pixels
    unsigned need;      // UP: border flags a row must have for this tap to contribute
    unsigned tap_bit;   // !UP: bit of this tap in the row's validity mask
    int wslot;          // index of the tap on the packed-weight K axis
};

template <int BM, int BN, int WM, int WN, int UP>
__global__ __launch_bounds__(256, 2) void conv_igemm_kernel(ConvArgs a, int M, int tiles_m, int tiles_n) {
    static_assert(WM * WN == 4 && BM / WM == 64 && BN / WN == 64, "4 waves, 64x64 accumulator each");
#if defined(__HIP_DEVICE_COMPILE__)  // buffer-resource builtins only exist in the device pass
    constexpr int A_BYTES = BM * 128;
    constexpr int B_BYTES = BN * 128;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int RA = BM / 32;  // A rows gathered per lane per K step
    constexpr int RB = BN / 32;
    constexpr int TH = BM / 16;  // 2-D tile: TH rows of 16 pixels
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware tile id (bijective for any tile count): XCD x = bid % 8 takes a contiguous run of tiles.
    const int total = tiles_m * tiles_n;
    const int bid = blockIdx.x;
    const int xq = total >> 3, xr = total & 7, xcd = bid & 7;
    const int tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    const int tn = tile % tiles_n;
    int tm = tile / tiles_n;
    int phase = 0;
    if (UP) {  // the four phases of one low-res tile are consecutive tiles: they share their input window in L2
        phase = tm & 3;
        tm >>= 2;
    }
    const int py = phase >> 1, px = phase & 1;

    const int cin = a.c0 + a.c1;
    const int cpt = cin >> 6;                 // 64-channel chunks per tap
    const int wtaps = UP ? 16 : a.kh * a.kw;  // taps on the packed-weight K axis
    // the plane the tile walks: output pixels, or (UP) low-res input pixels each owning one output pixel per phase
    const int ph = UP ? a.h : a.ho, pw = UP ? a.w : a.wo;
    const int plane = ph * pw;
    // 2-D tiling when the plane divides into TH x 16 tiles; otherwise BM consecutive raster pixels
    const bool tile2d = UP || ((pw % 16 == 0) && (ph % TH == 0));
    const int tiles_x = pw >> 4, tiles_per_img = tile2d ? tiles_x * (ph / TH) : 1;
    const int sub = lane >> 3;                // row inside an 8-row DMA group
    // LDS swizzle key of a tile row r is (r >> 1) & 7: a ds_read_b128 lane group covers 16 rows whose 128-B rows
    // alternate between the two halves of the 256-B bank row, so the key must change every SECOND row to spread the
    // group over all 16 16-B slots (conflict-free; key r & 7 is 2-way).  DMA rows are (j*4+wave)*8 + sub.
    const int gchunk = (lane & 7) ^ ((((wave & 1) << 2) | (sub >> 1)) & 7);  // swizzled SOURCE chunk of this lane's slot

    const size_t npix = (size_t)a.n * a.h * a.w;
    const int pitch0 = a.pix_pitch0 ? a.pix_pitch0 : a.c0;
    const auto rsrc_a0 = __builtin_amdgcn_make_buffer_rsrc((void*)a.src0, 0, (int)(unsigned)(npix * pitch0 * 2), 0x00020000);
    const auto rsrc_a1 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.c1 ? a.src1 : a.src0), 0,
                                                           (int)(unsigned)(npix * (a.c1 ? a.c1 : a.c0) * 2), 0x00020000);
    const auto rsrc_b = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.wpk, 0, (int)(unsigned)((size_t)(UP ? 4 : 1) * a.cout * wtaps * cpt * 128), 0x00020000);

    // tile position on the plane (2-D tiles)
    int t_img = 0, t_y0 = 0, t_x0 = 0;
    if (tile2d) {
        t_img = tm / tiles_per_img;
        const int t = tm - t_img * tiles_per_img;
        t_y0 = (t / tiles_x) * TH;
        t_x0 = (t % tiles_x) * 16;
    }
    // UP: which correction-tap groups this tile needs (wave-uniform)
    const bool has_row = UP && (py == 0 ? t_y0 == 0 : t_y0 + TH == ph);
    const bool has_col = UP && (px == 0 ? t_x0 == 0 : t_x0 + 16 == pw);
    const int ntaps = UP ? 9 + (has_row ? 3 : 0) + (has_col ? 3 : 0) + (has_row && has_col ? 1 : 0) : a.kh * a.kw;
    const int nk = ntaps * cpt;               // K steps of this tile
    const unsigned need_row = py == 0 ? 1u : 2u, need_col = px == 0 ? 4u : 8u;

    // ---- per-lane gather descriptors for the A rows this lane fetches
    // a_mask: !UP tap validity bits; UP border flags (1 top, 2 bottom, 4 left, 8 right, 16 row exists)
    unsigned a_off0[RA], a_off1[RA], a_mask[RA];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        const int row = (j * 4 + wave) * 8 + sub;
        unsigned mask = 0;
        int pix = 0;
        if (tm * BM + row < M) {
            int n_img, oy, ox;
            if (tile2d) {  // 16-pixel-wide 2-D tile: the taps of one tile re-read a small window from L2
                n_img = t_img;
                oy = t_y0 + (row >> 4);
                ox = t_x0 + (row & 15);
            } else {
                const int m = tm * BM + row;
                n_img = m / plane;
                const int rem = m - n_img * plane;
                oy = rem / pw;
                ox = rem - oy * pw;
            }
            if (UP) {
                pix = (n_img * a.h + oy) * a.w + ox;
                mask = 16u | (oy == 0 ? 1u : 0u) | (oy == a.h - 1 ? 2u : 0u) | (ox == 0 ? 4u : 0u) | (ox == a.w - 1 ? 8u : 0u);
            } else {
                const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
                pix = (n_img * a.h + iy0) * a.w + ix0;  // may be "negative": only ever used together with a valid tap
                // taps inside the image: ky in [ylo, yhi), kx in [xlo, xhi) -> bit (ky*kw + kx)
                const int ylo = max(0, -iy0), yhi = min(a.kh, a.h - iy0);
                const int xlo = max(0, -ix0), xhi = min(a.kw, a.w - ix0);
                const unsigned ym = yhi > ylo ? (1u << yhi) - (1u << ylo) : 0u;
                const unsigned xm = xhi > xlo ? (1u << xhi) - (1u << xlo) : 0u;
                for (int ky = 0; ky < a.kh; ++ky) mask |= (((ym >> ky) & 1u) ? xm : 0u) << (ky * a.kw);
            }
        }
        a_mask[j] = mask;
        a_off0[j] = (unsigned)pix * (unsigned)(pitch0 * 2) + gchunk * 16;
        a_off1[j] = (unsigned)pix * (unsigned)(a.c1 * 2) + gchunk * 16;
    }
    // B rows: row r of the tile is output channel tn*BN + r of this phase's weight set; a K step is one 128-B segment
    unsigned b_off[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int row = (j * 4 + wave) * 8 + sub;
        b_off[j] = (unsigned)(phase * a.cout + tn * BN + row) * (unsigned)(wtaps * cpt * 128) + gchunk * 16;
    }

    // issue-side K-step state (wave-uniform): tap counter (position in this tile's tap list) and chunk
    int is_tap = 0, is_chunk = 0;
    int tap_lo = 0;  // first tap position of the list being walked (9 while a UP tile runs its correction taps)

    auto step_info = [&](int tpos) {
        StepInfo si;
        if (UP) {
            int t = tpos;  // position -> tap id: 0-8 stencil, then the correction groups this tile has
            if (t >= 9) {
                t -= 9;
                if (has_row && t < 3) t += 9;
                else {
                    if (has_row) t -= 3;
                    if (has_col && t < 3) t += 12;
                    else t = 15;
                }
            }
            si.wslot = t;
            si.tap_bit = 0;
            if (t < 9) { si.dy = t / 3 - 1; si.dx = t % 3 - 1; si.need = 16u; }
            else if (t < 12) { si.dy = 0; si.dx = t - 10; si.need = 16u | need_row; }
            else if (t < 15) { si.dy = t - 13; si.dx = 0; si.need = 16u | need_col; }
            else { si.dy = 0; si.dx = 0; si.need = 16u | need_row | need_col; }
        } else {
            si.dy = tpos / a.kw;
            si.dx = tpos - si.dy * a.kw;
            si.wslot = tpos;
            si.tap_bit = 1u << tpos;
            si.need = 0;
        }
        return si;
    };

    // issue the LDS-DMA of K step (is_tap, is_chunk) into `stage`
    auto issue = [&](int stage) {
        char* As = smem + stage * STAGE;
        char* Bs = As + A_BYTES;
        const StepInfo si = step_info(is_tap);
        const int cb = is_chunk << 6;
        const bool second = cb >= a.c0;
        const int csrc = second ? a.c1 : pitch0;
        const int coff = second ? cb - a.c0 : cb;
        const unsigned dyoff = (unsigned)(si.dy * a.w * csrc * 2), dxoff = (unsigned)(si.dx * csrc * 2);
        const unsigned chunk_off = (unsigned)(coff * 2);
        // UP: a tap that would step outside the image is clamped back onto the border pixel (replicate)
        const unsigned kill_y = si.dy < 0 ? 1u : (si.dy > 0 ? 2u : 0u), kill_x = si.dx < 0 ? 4u : (si.dx > 0 ? 8u : 0u);
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const unsigned base = second ? a_off1[j] : a_off0[j];
            unsigned vo;
            if (UP) {
                const unsigned f = a_mask[j];
                const unsigned o = base + chunk_off + ((f & kill_y) ? 0u : dyoff) + ((f & kill_x) ? 0u : dxoff);
                vo = ((f & si.need) == si.need) ? o : 0xFFFFFFFFu;
            } else {
                vo = (a_mask[j] & si.tap_bit) ? base + chunk_off + dyoff + dxoff : 0xFFFFFFFFu;
            }
            if (second)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a1, LDS_PTR(As + (j * 4 + wave) * 1024), 16, vo, 0, 0, 0);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a0, LDS_PTR(As + (j * 4 + wave) * 1024), 16, vo, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, LDS_PTR(Bs + (j * 4 + wave) * 1024), 16, b_off[j],
                                                     (si.wslot * cpt + is_chunk) * 128, 0, 0);
        }
        // K order: taps fastest, then the 64-channel chunk -- all taps of one chunk are consecutive, so a tile's input
        // window for that chunk (a few tens of KB) is fetched from HBM once and re-read from L2 by the other taps
        if (++is_tap == ntaps) {
            is_tap = tap_lo;
            ++is_chunk;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // fragment read offsets: row*128 + ((k16*2 + (lane>>5)) ^ ((row>>1) & 7)) * 16 ; fragment rows are 32-aligned + (lane&31)
    const int l31 = lane & 31, hi = lane >> 5, l7 = (lane >> 1) & 7;
    const int a_row_off = (wm * 64 + l31) * 128;
    const int b_row_off = (wn * 64 + l31) * 128;

    // One K step of MFMAs.  Fragment reads are software-pipelined one k16 sub-step ahead (two register sets), so only
    // the first ds_read latency of a K step is exposed instead of four.
    auto compute = [&](int stage) {
        const char* As = smem + stage * STAGE + a_row_off;
        const char* Bs = smem + stage * STAGE + A_BYTES + b_row_off;
        el16x8_t af[2][2], bfr[2][2];
        {
            const int coff = ((hi ^ l7) << 4);
#pragma unroll
            for (int i = 0; i < 2; ++i) af[0][i] = *(const el16x8_t*)(As + i * 32 * 128 + coff);
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[0][j] = *(const el16x8_t*)(Bs + j * 32 * 128 + coff);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int cs = ks & 1, ns = cs ^ 1;
            if (ks < 3) {
                const int coff = ((((ks + 1) * 2 + hi) ^ l7) << 4);
#pragma unroll
                for (int i = 0; i < 2; ++i) af[ns][i] = *(const el16x8_t*)(As + i * 32 * 128 + coff);
#pragma unroll
                for (int j = 0; j < 2; ++j) bfr[ns][j] = *(const el16x8_t*)(Bs + j * 32 * 128 + coff);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = DYF_MFMA_32x32x16(bfr[cs][j], af[cs][i], acc[i][j], 0, 0, 0);  // D^T = W X^T
        }
    };

    // UP fast path (both sources have the same channel count): the 9 stencil taps are unrolled and each row's gather
    // offset is base + yoff[a] + xoff[b] with per-row, per-direction byte offsets precomputed once per tile (clamped to
    // the border = replicate); one v_add3 per row and K step instead of ~11 VALU.  Rows past M carry an out-of-range
    // base.  The correction taps of border tiles run afterwards through the general `issue` path.
    const bool up_fast = UP && (a.c1 == 0 || a.c1 == a.c0) && npix * (size_t)a.c0 * 2 < 0x7F000000ull;
    if (UP && up_fast) {
        const unsigned rowb = (unsigned)(a.w * a.c0 * 2), pixb = (unsigned)(a.c0 * 2);
        unsigned ybase[RA], y_m[RA], y_p[RA], x_m[RA], x_p[RA];
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const unsigned f = a_mask[j];
            ybase[j] = (f & 16u) ? a_off0[j] : 0x80000000u;
            y_m[j] = (f & 1u) ? 0u : 0u - rowb;
            y_p[j] = (f & 2u) ? 0u : rowb;
            x_m[j] = (f & 4u) ? 0u : 0u - pixb;
            x_p[j] = (f & 8u) ? 0u : pixb;
        }
        const int ncorr = ntaps - 9;
        int chunk = 0;
        unsigned cb_off = 0;  // byte offset of the current chunk inside its source
        bool second = false;

#define ISSUE_STENCIL(T, STAGE_)                                                                                  \
    {                                                                                                             \
        char* As_ = smem + (STAGE_) * STAGE;                                                                      \
        char* Bs_ = As_ + A_BYTES;                                                                                \
        _Pragma("unroll") for (int j = 0; j < RA; ++j) {                                                          \
            const unsigned vo = ybase[j] + cb_off + ((T) / 3 == 0 ? y_m[j] : ((T) / 3 == 2 ? y_p[j] : 0u)) +      \
                                ((T) % 3 == 0 ? x_m[j] : ((T) % 3 == 2 ? x_p[j] : 0u));                           \
            if (second)                                                                                           \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a1, LDS_PTR(As_ + (j * 4 + wave) * 1024), 16, vo, 0, 0, 0); \
            else                                                                                                  \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a0, LDS_PTR(As_ + (j * 4 + wave) * 1024), 16, vo, 0, 0, 0); \
        }                                                                                                         \
        _Pragma("unroll") for (int j = 0; j < RB; ++j)                                                            \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, LDS_PTR(Bs_ + (j * 4 + wave) * 1024), 16, b_off[j],  \
                                                     ((T) * cpt + chunk) * 128, 0, 0);                            \
    }
#define STENCIL_STEP(T)                                                                    \
    {                                                                                      \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                   \
        __syncthreads();                                                                   \
        ISSUE_STENCIL((T) + 1, st ^ 1)                                                     \
        compute(st);                                                                       \
        st ^= 1;                                                                           \
    }
        int st = 0;
        ISSUE_STENCIL(0, 0)
        for (;;) {
            STENCIL_STEP(0) STENCIL_STEP(1) STENCIL_STEP(2) STENCIL_STEP(3)
            STENCIL_STEP(4) STENCIL_STEP(5) STENCIL_STEP(6) STENCIL_STEP(7)
            // tap 8: its successor is tap 0 of the next chunk, the first correction step, or nothing
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const bool last_chunk = chunk + 1 == cpt;
            if (!last_chunk) {
                ++chunk;
                const int cb = chunk << 6;
                second = cb >= a.c0;
                cb_off = (unsigned)((second ? cb - a.c0 : cb) * 2);
                ISSUE_STENCIL(0, st ^ 1)
            } else if (ncorr > 0) {
                tap_lo = 9;
                is_tap = 9;
                is_chunk = 0;
                issue(st ^ 1);
            }
            compute(st);
            st ^= 1;
            if (last_chunk) break;
        }
#undef STENCIL_STEP
#undef ISSUE_STENCIL
        for (int k = 0; k < ncorr * cpt; ++k) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (k + 1 < ncorr * cpt) issue(st ^ 1);
            compute(st);
            st ^= 1;
        }
    } else {
        // split-K (small batches): blockIdx.y walks its share [k0, k1) of the K steps; K order is taps fastest, then chunks
        const int nsplit = a.splitk > 1 ? a.splitk : 1;
        const int k0 = (int)((long long)nk * blockIdx.y / nsplit), k1 = (int)((long long)nk * (blockIdx.y + 1) / nsplit);
        is_chunk = k0 / ntaps;
        is_tap = k0 - is_chunk * ntaps;
        issue(0);
        for (int k = k0; k < k1; ++k) {
            const int cur = (k - k0) & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (k + 1 < k1) issue(cur ^ 1);
            compute(cur);
        }
    }

    if (!UP && a.splitk > 1) {
        // split-K partial: raw fp32 accumulators to splitk_ws[split][m][cout]; conv_splitk_finish_kernel adds the splits in
        // index order (deterministic) and runs the epilogue.  Lane (l31, hi) of accumulator (i, j): pixel l31 of sub-tile i,
        // channels j*32 + 8*g + 4*hi + {0..3}.
        const int l31s = lane & 31, his = lane >> 5;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wm * 64 + i * 32 + l31s;
            if (tm * BM + row >= M) continue;
            int m;
            if (tile2d) m = (t_img * a.ho + t_y0 + (row >> 4)) * a.wo + t_x0 + (row & 15);
            else m = tm * BM + row;
            float* dst = a.splitk_ws + ((size_t)blockIdx.y * M + m) * a.cout + tn * BN + wn * 64 + 4 * his;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *(float4*)(dst + j * 32 + 8 * g) = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        }
        return;
    }

    // ---- epilogue straight from the accumulators.  The operands are swapped (D^T = W X^T), so lane (l31, hi) of
    // accumulator (i, j) holds PIXEL l31 of pixel sub-tile i and CHANNELS j*32 + 8*g + 4*hi + {0..3} (g = register group):
    // the layout of the shared step (conv_epilogue.h) -- affine / activation / dropout / residual in registers, 16-bit pack, exchange
    // between lanes l and l+32 -- after which every lane stores 8 consecutive channels (16 B); fp32 output leaves before the pack.
    auto epilogue = [&](auto act_c, auto mode_c) {
        constexpr int ACT = decltype(act_c)::value, MODE = decltype(mode_c)::value;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wm * 64 + i * 32 + l31;
            const bool valid = tm * BM + row < M;
            int m, n_img;  // m: output pixel index in the NHWC output tensor
            if (tile2d) {
                n_img = t_img;
                const int y = t_y0 + (row >> 4), x = t_x0 + (row & 15);
                m = UP ? (n_img * a.ho + 2 * y + py) * a.wo + 2 * x + px : (n_img * a.ho + y) * a.wo + x;
            } else {
                m = valid ? tm * BM + row : 0;
                n_img = m / plane;
            }
            const uint32_t ob = (uint32_t)m * (uint32_t)a.cout + (uint32_t)(tn * BN + wn * 64);
            const RngKey key = drop_row_key(a.drop, n_img);  // dropout streams are per batch row
            const uint32_t row0 = (uint32_t)n_img * (uint32_t)(a.ho * a.wo * a.cout);
            const uint32_t cb = (uint32_t)((a.coef_div > 1 ? n_img / a.coef_div : n_img) * a.coef_stride + tn * BN + wn * 64 + 4 * hi);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) {
                    const int cg0 = j * 32 + 16 * g2;  // + 4*hi: own channels of group 2*g2; + 8: group 2*g2+1
                    float ca[8], cc[8], v[8];
                    epi_coef(a.coef_a + cb + cg0, a.coef_c + cb + cg0, drop_prescale<ACT, MODE>(a.drop), ca, cc);
                    const uint32_t e0 = ob + cg0 + 4 * hi;
                    epi_values<ACT, MODE>(acc[i][j], 8 * g2, ca, cc, e0, row0, a.drop, key, v);
                    if (a.residual) {
                        const uint2 r0 = valid ? *(const uint2*)(a.residual + (size_t)e0) : make_uint2(0, 0);
                        const uint2 r1 = valid ? *(const uint2*)(a.residual + (size_t)e0 + 8) : make_uint2(0, 0);
                        epi_add_residual(v, r0, r1);
                    }
                    if (a.out_f32 && valid) {
                        *(float4*)(a.out_f32 + (size_t)e0) = make_float4(v[0], v[1], v[2], v[3]);
                        *(float4*)(a.out_f32 + (size_t)e0 + 8) = make_float4(v[4], v[5], v[6], v[7]);
                    }
                    if (a.out_el16) {
                        const uint4 o = epi_pack_swap(v);
                        if (valid) *(uint4*)(a.out_el16 + (size_t)(ob + cg0 + 8 * hi)) = o;
                    }
                }
        }
    };
    epi_dispatch(a.act, a.drop.mode, epilogue);
#endif
}

// ------------------------------------------------------------------------------------------------ split-K finish
// Small batches leave the small-plane / deep-K layers (enc1-enc5, dec1, dec2 of unet_simple) with a handful of workgroups that
// each walk up to 144 K steps: a forward at NB = 1 spent 300 of its 316 us there.  conv_igemm_kernel<128,128> then splits the
// K steps over blockIdx.y; this kernel adds the partials in split order and applies the epilogue of conv_direct_kernel.
__global__ void conv_splitk_finish_kernel(ConvArgs a, long long M) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * a.cout) return;
    const int co = (int)(i % a.cout);
    const long long m = i / a.cout;
    const int n = (int)(m / ((long long)a.ho * a.wo));
    float acc = 0.0f;
    for (int s = 0; s < a.splitk; ++s) acc += a.splitk_ws[((size_t)s * M + m) * a.cout + co];
    const size_t ci = (size_t)(a.coef_div > 1 ? n / a.coef_div : n) * a.coef_stride + co;
    float v = fmaf(acc, a.coef_a[ci], a.coef_c[ci]);
    v = apply_act(v, a.act);
    v = drop_apply(v, (uint32_t)i, (uint32_t)n * (uint32_t)(a.ho * a.wo * a.cout), a.drop, drop_row_key(a.drop, n));
    if (a.residual) v += el16_to_f32(a.residual[i]);
    if (a.out_el16) a.out_el16[i] = f32_to_el16(v);
    if (a.out_f32) a.out_f32[i] = v;
}

// The same finish with 4 consecutive channels per thread (cout % 4 == 0): 16-byte loads of the partials, one keep word per pair,
// 8-byte stores -- the finish of the rows kernels' split-K launches (conv_halo_rows.hip), whose outputs are whole decoder planes.
__global__ __launch_bounds__(256) void conv_splitk_finish4_kernel(ConvArgs a, long long M) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = M * a.cout;
    const long long i = q * 4;
    if (i >= total) return;
    const int co = (int)(i % a.cout);
    const long long m = i / a.cout;
    const int plane = a.ho * a.wo;
    const int n = (int)(m / plane);
    float4 s4 = *(const float4*)(a.splitk_ws + (size_t)i);
    for (int s = 1; s < a.splitk; ++s) {
        const float4 t4 = *(const float4*)(a.splitk_ws + (size_t)s * (size_t)total + (size_t)i);
        s4.x += t4.x; s4.y += t4.y; s4.z += t4.z; s4.w += t4.w;
    }
    const size_t ci = (size_t)(a.coef_div > 1 ? n / a.coef_div : n) * a.coef_stride + co;
    const float4 ca = *(const float4*)(a.coef_a + ci), cc = *(const float4*)(a.coef_c + ci);
    float v[4] = {fmaf(s4.x, ca.x, cc.x), fmaf(s4.y, ca.y, cc.y), fmaf(s4.z, ca.z, cc.z), fmaf(s4.w, ca.w, cc.w)};
    act_drop<4>(v, (uint32_t)i, (uint32_t)n * (uint32_t)(plane * a.cout), a.act, a.drop, drop_row_key(a.drop, n));
    if (a.residual) {
        const uint2 rr = *(const uint2*)(a.residual + (size_t)i);
        v[0] += el16_lo(rr.x); v[1] += el16_hi(rr.x); v[2] += el16_lo(rr.y); v[3] += el16_hi(rr.y);
    }
    if (a.out_f32) *(float4*)(a.out_f32 + (size_t)i) = make_float4(v[0], v[1], v[2], v[3]);
    if (a.out_el16) *(uint2*)(a.out_el16 + (size_t)i) = make_uint2(pack_el16x2(v[0], v[1]), pack_el16x2(v[2], v[3]));
}

hipError_t launch_conv_splitk_finish4(const ConvArgs& a, long long M, hipStream_t stream) {
    if ((a.cout & 3) != 0 || a.splitk_ws == nullptr || a.splitk < 1) return hipErrorInvalidValue;
    const long long quads = M * a.cout / 4;
    hipLaunchKernelGGL(conv_splitk_finish4_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, a, M);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ launchers
bool conv_mfma_supported(const ConvArgs& a) {
    if (a.act == ACT_GELU) return false;  // the MFMA epilogues are instantiated for none / ReLU / LeakyReLU / SiLU
    if (!(a.c0 > 0 && (a.c0 % 64) == 0 && (a.c1 % 64) == 0 && (a.cout % 64) == 0)) return false;
    if (a.kh * a.kw > 32) return false;                       // tap-validity mask is 32 bits
    const size_t npix = (size_t)a.n * a.h * a.w;              // 32-bit buffer offsets
    const size_t lim = 0xFFFFFFF0ull;
    const size_t wtaps = a.up2x ? 64 : (size_t)a.kh * a.kw;
    if (!(npix * a.c0 * 2 < lim && npix * (size_t)a.c1 * 2 < lim && (size_t)a.cout * wtaps * (a.c0 + a.c1) * 2 < lim))
        return false;
    if (a.up2x) {  // fused x2 upsample: 3x3/s1/p1 on a low-res plane that tiles into TH x 16
        const int th = (a.cout % 128 == 0) ? 8 : 16;
        return a.kh == 3 && a.kw == 3 && a.stride == 1 && a.pad == 1 && a.w % 16 == 0 && a.h % th == 0 &&
               a.ho == 2 * a.h && a.wo == 2 * a.w && a.wpk_up != nullptr;
    }
    return true;
}

template <int BM, int BN, int WM, int WN, int UP>
static hipError_t launch_igemm(ConvArgs a, hipStream_t stream) {
    constexpr int lds = 2 * (BM + BN) * 128;
    long long M = (long long)a.n * a.ho * a.wo;
    int tiles_m = (int)((M + BM - 1) / BM);
    if (UP) {  // tiles walk the LOW-res plane once per phase
        M = (long long)a.n * a.h * a.w;
        tiles_m = (int)(M / BM) * 4;
        a.wpk = a.wpk_up;
    }
    const int tiles_n = a.cout / BN;
    a.splitk = 1;
    if (!UP && BM == 128 && a.splitk_ws) {
        // Split factor: the layer's K depth allows nk / 8 (<= 16); the launch takes as much of it as is needed to fill the 512
        // resident workgroups (power of two), and only when its own tiles fill less than a quarter of them -- a layer with many
        // output pixels pays more for writing / re-reading the partials than it gains (enc1 at NB = 7: 224 tiles, 58 MB of
        // partials).  Tiny problems (<= 32 tiles) always get the layer's full factor, so small batches, their row splits and
        // the paired launches sum in the same order and stay bit-identical.
        const bool enabled = dyf_form_int("DYF_SPLITK", 1) != 0;
        const int nk = a.kh * a.kw * ((a.c0 + a.c1) >> 6);
        const long long tiles = (((long long)(a.n_sel > 0 ? a.n_sel : a.n) * a.ho * a.wo + BM - 1) / BM) * tiles_n;
        const long long max_tiles = dyf_form_int("DYF_SPLITK_MAX_TILES", 128);
        const long long fill = dyf_form_int("DYF_SPLITK_FILL", 512);
        int s = std::min(16, nk / 8);
        while (s > 1 && s * tiles > fill) s >>= 1;
        const long long need = (long long)s * M * a.cout;
        if (enabled && s > 1 && tiles <= max_tiles && need <= a.splitk_cap) a.splitk = s;
    }
    dyf_form_note(a.splitk > 1 ? (BM == 128 ? "conv_igemm_kernel<128,128>+splitk" : "conv_igemm_kernel<256,64>+splitk")
                               : (BM == 128 ? (UP ? "conv_igemm_kernel<128,128,UP>" : "conv_igemm_kernel<128,128>")
                                            : (UP ? "conv_igemm_kernel<256,64,UP>" : "conv_igemm_kernel<256,64>")), a.n);
    hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, UP>), dim3(tiles_m * tiles_n, a.splitk), dim3(256), lds, stream, a, (int)M,
                       tiles_m, tiles_n);
    if (a.splitk > 1)
        hipLaunchKernelGGL(conv_splitk_finish_kernel, dim3((unsigned)((M * a.cout + 255) / 256)), dim3(256), 0, stream, a, M);
    return hipGetLastError();
}

// Raise the dynamic-LDS cap of the MFMA kernels once per process (not legal inside a stream capture).
hipError_t conv_init() {
    hipError_t e = hipSuccess;
#define SET_LDS(BM, BN, WM, WN, UP)                                                                     \
    if (e == hipSuccess)                                                                                \
        e = hipFuncSetAttribute((const void*)conv_igemm_kernel<BM, BN, WM, WN, UP>,                     \
                                hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (BM + BN) * 128);
    SET_LDS(128, 128, 2, 2, 0) SET_LDS(128, 128, 2, 2, 1) SET_LDS(256, 64, 4, 1, 0) SET_LDS(256, 64, 4, 1, 1)
#undef SET_LDS
    if (e == hipSuccess) e = conv_up_halo_init();
    if (e == hipSuccess) e = conv_halo_rows_init();
    if (e == hipSuccess) e = conv_igemm2_init();
    if (e == hipSuccess) e = conv_enc0_stem_init();
    return e;
}

// This file's two forms as plain launchers; which form a conv takes is decided in conv_dispatch.hip (conv_choose_form).
hipError_t launch_conv_igemm(const ConvArgs& a, hipStream_t stream) {
    if (a.cout % 128 == 0)
        return a.up2x ? launch_igemm<128, 128, 2, 2, 1>(a, stream) : launch_igemm<128, 128, 2, 2, 0>(a, stream);
    return a.up2x ? launch_igemm<256, 64, 4, 1, 1>(a, stream) : launch_igemm<256, 64, 4, 1, 0>(a, stream);
}

hipError_t launch_conv_direct(const ConvArgs& a, hipStream_t stream) {
    if (a.up2x) return hipErrorInvalidValue;  // the direct kernel has no fused-upsample form: caller materialises
    const long long total = (long long)a.n * a.ho * a.wo * a.cout;
    const int threads = 256;
    dyf_form_note("conv_direct_kernel", a.n);
    hipLaunchKernelGGL(conv_direct_kernel, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0, stream,
                       a, total);
    return hipGetLastError();
}

// Host-side weight transform for the fused x2-upsample conv (see the kernel header): w [cout][cin][3][3] fp32 ->
// [4 phases][cout][16 taps][cin] bf16.
void pack_up2x_weights(const float* w, int cout, int cin, el16_t* out) {
    // coefficient of w[k] (k = 0,1,2) in the stencil tap a = -1,0,+1 and in the border correction, per phase
    static const double E[2][3][3] = {{{0.75, 0.25, 0.0}, {0.25, 0.75, 0.75}, {0.0, 0.0, 0.25}},
                                      {{0.25, 0.0, 0.0}, {0.75, 0.75, 0.25}, {0.0, 0.25, 0.75}}};
    static const double Cc[2][3] = {{-1.0, 0.0, 0.0}, {0.0, 0.0, -1.0}};
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            const int phase = py * 2 + px;
            for (int co = 0; co < cout; ++co)
                for (int ci = 0; ci < cin; ++ci) {
                    const float* k = w + ((size_t)co * cin + ci) * 9;
                    for (int t = 0; t < 16; ++t) {
                        const double* fy;
                        const double* fx;
                        if (t < 9) { fy = E[py][t / 3]; fx = E[px][t % 3]; }
                        else if (t < 12) { fy = Cc[py]; fx = E[px][t - 9]; }
                        else if (t < 15) { fy = E[py][t - 12]; fx = Cc[px]; }
                        else { fy = Cc[py]; fx = Cc[px]; }
                        double v = 0.0;
                        for (int ky = 0; ky < 3; ++ky)
                            for (int kx = 0; kx < 3; ++kx) v += fy[ky] * fx[kx] * (double)k[ky * 3 + kx];
                        out[(((size_t)phase * cout + co) * 16 + t) * cin + ci] = f32_to_el16((float)v);
                    }
                }
        }
}
