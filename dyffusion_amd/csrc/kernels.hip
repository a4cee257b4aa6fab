// HBM-bound kernels of the DYffusion engine (gfx950): stem, x2 bilinear upsample, GroupNorm, readout, time/FiLM heads,
// sampler elementwise.  Every kernel replaces an unfused ATen sequence of the reference (cited per kernel).
#include "kernels.h"

#include <cstdlib>

// ------------------------------------------------------------------------------------------------ block reduce
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float block_sum(float v, float* scratch /* >= 16 floats */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    float t = 0.0f;
    for (int i = 0; i < nw; ++i) t += scratch[i];
    return t;
}

// ------------------------------------------------------------------------------------------------ K9 time MLP
// misc.py:20-32 (SinusoidalPosEmb), :63-66 (Linear -> GELU(erf) -> Linear); the trailing SiLU is the first op of
// every UNetBlock.time_mlp (unet_simple.py:21-23) and is shared by all blocks.
__global__ void time_mlp_kernel(TimeMlpArgs a) {
    extern __shared__ float sh[];  // e[dim] | h[tdim]
    const int row = blockIdx.x, tdim = 2 * a.dim, half = a.dim / 2;
    const int dim = a.learned_w ? 2 * a.learned_half + 1 : a.dim;  // number of time features
    float* e = sh;
    float* h = sh + dim;
    const float t = a.time[row];
    if (a.learned_w) {
        for (int i = threadIdx.x; i < dim; i += blockDim.x) {
            if (i == 0) { e[0] = t; continue; }
            const int j = (i - 1) % a.learned_half;
            const float ang = t * a.learned_w[j] * 6.283185307179586f;
            e[i] = i <= a.learned_half ? sinf(ang) : cosf(ang);
        }
    } else {
        const float step = -logf(10000.0f) / (float)(half - 1);
        for (int i = threadIdx.x; i < dim; i += blockDim.x) {
            const int j = i < half ? i : i - half;
            const float ang = t * expf((float)j * step);
            e[i] = i < half ? sinf(ang) : cosf(ang);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < tdim; j += blockDim.x) {
        float acc = a.b1[j];
        const float* w = a.w1 + (size_t)j * dim;
        for (int i = 0; i < dim; ++i) acc = fmaf(w[i], e[i], acc);
        h[j] = 0.5f * acc * (1.0f + erff(acc * 0.70710678118654752f));
    }
    __syncthreads();
    for (int j = threadIdx.x; j < tdim; j += blockDim.x) {
        float acc = a.b2[j];
        const float* w = a.w2 + (size_t)j * tdim;
        for (int i = 0; i < tdim; ++i) acc = fmaf(w[i], h[i], acc);
        a.silu_out[(size_t)row * tdim + j] = acc / (1.0f + expf(-acc));
    }
}

hipError_t launch_time_mlp(const TimeMlpArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(time_mlp_kernel, dim3(a.rows), dim3(128), (size_t)(3 * a.dim + 2 * a.learned_half + 1) * sizeof(float), s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ K9 FiLM heads
// unet_simple.py:72-78: time_mlp Linear -> chunk(scale, shift) -> x*(scale+1)+shift, folded with the block's
// eval-mode BatchNorm (and conv bias): y = conv*A + C.
__global__ void film_kernel(FilmArgs a) {
    const int fc = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (fc >= a.total_c) return;
    float scale = 0.0f, shift = 0.0f;
    if (a.silu != nullptr) {
        const int b = a.blk_of[fc];
        const int cl = fc - a.blk_off[b];
        const int r_scale = 2 * a.blk_off[b] + cl;
        const int r_shift = r_scale + a.blk_cout[b];
        const float* sv = a.silu + (size_t)row * a.tdim;
        const float* ws = a.wf + (size_t)r_scale * a.tdim;
        const float* wh = a.wf + (size_t)r_shift * a.tdim;
        scale = a.bf[r_scale];
        shift = a.bf[r_shift];
        for (int i = 0; i < a.tdim; ++i) {
            scale = fmaf(ws[i], sv[i], scale);
            shift = fmaf(wh[i], sv[i], shift);
        }
    }
    const float na = a.norm_a[fc], nc = a.norm_c[fc];
    a.coef_a[(size_t)row * a.total_c + fc] = na * (1.0f + scale);
    a.coef_c[(size_t)row * a.total_c + fc] = fmaf(nc, 1.0f + scale, shift);
}

hipError_t launch_film(const FilmArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(film_kernel, dim3((a.total_c + 127) / 128, a.rows), dim3(128), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ K4+K1 stem
// unet_simple.py:184-195: cat[inputs, condition] -> Upsample(size, bilinear) -> init_conv 1x1.  One thread per
// resampled pixel; the sampled channel vector is parked in LDS so the 1x1 can index it dynamically.
__global__ __launch_bounds__(256) void stem_kernel(StemArgs a) {
    extern __shared__ float vals[];  // [cin][256]
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)a.n * a.uh * a.uw;
    const bool live = pix < total;
    const int tid = threadIdx.x;
    if (live) {
        const int n = (int)(pix / ((long long)a.uh * a.uw));
        const int rem = (int)(pix % ((long long)a.uh * a.uw));
        const int y = rem / a.uw, x = rem % a.uw;
        int y0 = y, y1 = y, x0 = x, x1 = x;
        float ly = 0.0f, lx = 0.0f;
        if (a.resample) {
            bilinear_coord(y, (float)a.h / (float)a.uh, a.h, y0, y1, ly, a.nearest != 0);
            bilinear_coord(x, (float)a.w / (float)a.uw, a.w, x0, x1, lx, a.nearest != 0);
        }
        int cbase = 0;
        for (int s = 0; s < a.nsrc; ++s) {
            const float* src = a.src[s] + (size_t)(a.src_rows > 0 ? n % a.src_rows : n) * a.ch[s] * a.h * a.w;
            for (int c = 0; c < a.ch[s]; ++c) {
                const float* p = src + (size_t)c * a.h * a.w;
                const float v00 = p[y0 * a.w + x0], v01 = p[y0 * a.w + x1];
                const float v10 = p[y1 * a.w + x0], v11 = p[y1 * a.w + x1];
                // same association as ATen's CPU kernel: rows first, then columns
                const float top = v00 * (1.0f - lx) + v01 * lx;
                const float bot = v10 * (1.0f - lx) + v11 * lx;
                vals[(cbase + c) * 256 + tid] = top * (1.0f - ly) + bot * ly;
            }
            cbase += a.ch[s];
        }
    }
    __syncthreads();
    if (!live) return;
    el16_t* out = a.out + (size_t)pix * a.dim;
    const int n_row = (int)(pix / ((long long)a.uh * a.uw));
    const RngKey dkey = drop_row_key(a.drop, n_row);
    const uint32_t row0 = (uint32_t)n_row * (uint32_t)(a.uh * a.uw * a.dim);
    for (int d0 = 0; d0 < a.dim; d0 += 8) {
        float acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = (d0 + t < a.dim) ? a.bias[d0 + t] : 0.0f;
        for (int c = 0; c < a.cin; ++c) {
            const float v = vals[c * 256 + tid];
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (d0 + t < a.dim) acc[t] = fmaf(a.wgt[(size_t)(d0 + t) * a.cin + c], v, acc[t]);
        }
        if (a.drop.mode != 0) {  // dropout_input (unet_simple.py:168)
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (d0 + t < a.dim) acc[t] = drop_apply(acc[t], (uint32_t)(pix * a.dim + d0 + t), row0, a.drop, dkey);
        }
        if ((a.dim & 7) == 0) {
            uint4 o;
            o.x = pack_el16x2(acc[0], acc[1]);
            o.y = pack_el16x2(acc[2], acc[3]);
            o.z = pack_el16x2(acc[4], acc[5]);
            o.w = pack_el16x2(acc[6], acc[7]);
            *(uint4*)(out + d0) = o;
        } else {
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (d0 + t < a.dim) out[d0 + t] = f32_to_el16(acc[t]);
        }
    }
}

hipError_t launch_stem(const StemArgs& a, hipStream_t s) {
    const long long total = (long long)a.n * a.uh * a.uw;
    dyf_form_note("stem_kernel", a.n);
    hipLaunchKernelGGL(stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), (size_t)a.cin * 256 * sizeof(float),
                       s, a);
    return hipGetLastError();
}

// rng_begin_forward_kernel's work done by block 0 of a stem launch (StemArgs::rng_state != null): one launch (and one kernel
// boundary) less per forward that draws masks -- 6-7 us of a 250 us one-row forward.  Same arithmetic, same table.
__device__ __forceinline__ void stem_rng_begin(const StemArgs& a) {
    if (a.rng_state == nullptr || blockIdx.x != 0) return;
    const uint32_t lo = a.rng_state[0], hi = a.rng_state[1], fwd0 = a.rng_state[2], row0 = a.rng_state[3];
    for (int r = threadIdx.x; r < a.rng_rows; r += blockDim.x) {
        const RngKey k = rng_row_key(lo, hi, fwd0 + (uint32_t)(r / a.rng_rows_per_fwd), row0 + (uint32_t)(r % a.rng_rows_per_fwd));
        a.rng_row_keys[2 * r] = k.k0;
        a.rng_row_keys[2 * r + 1] = k.k1;
    }
    __syncthreads();  // (every thread of block 0 has read fwd0)
    if (threadIdx.x == 0) a.rng_state[2] = fwd0 + (uint32_t)((a.rng_rows + a.rng_rows_per_fwd - 1) / a.rng_rows_per_fwd);
}

// init_conv is linear and nothing non-linear sits between it and the first encoder conv (dropout_input has p = 0),
// so conv4x4(init_conv(x)) is ONE 4x4 conv on the resampled raw channels.  This kernel only resamples.
__global__ __launch_bounds__(256) void stem16_kernel(StemArgs a) {
    stem_rng_begin(a);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int ph = a.uh + 2, pw = a.uw + 2;
    const long long total = (long long)stem16_out_rows(a) * ph * pw;
    if (idx >= total) return;
    const int n = (int)(idx / ((long long)ph * pw));
    const int rem = (int)(idx % ((long long)ph * pw));
    const int y = rem / pw - 1, x = rem % pw - 1;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((unsigned)y < (unsigned)a.uh && (unsigned)x < (unsigned)a.uw) {
        int y0 = y, y1 = y, x0 = x, x1 = x;
        float ly = 0.0f, lx = 0.0f;
        if (a.resample) {
            bilinear_coord(y, (float)a.h / (float)a.uh, a.h, y0, y1, ly, a.nearest != 0);
            bilinear_coord(x, (float)a.w / (float)a.uw, a.w, x0, x1, lx, a.nearest != 0);
        }
        // channel k of the concatenation lives in source s(k): a static loop over the 16 output slots (the dynamic
        // (source, channel) walk of the first version cost a 16-way select chain per channel)
        const int e0 = a.ch[0], e1 = e0 + (a.nsrc > 1 ? a.ch[1] : 0), e2 = e1 + (a.nsrc > 2 ? a.ch[2] : 0);
        const int nrow = a.src_rows > 0 ? n % a.src_rows : n;
        const int o00 = y0 * a.w + x0, o01 = y0 * a.w + x1, o10 = y1 * a.w + x0, o11 = y1 * a.w + x1;
        const size_t plane = (size_t)a.h * a.w;
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float val = 0.0f;
            if (k < a.cin) {
                const int si = k < e0 ? 0 : (k < e1 ? 1 : (k < e2 ? 2 : 3));
                const int cl = k - (si == 0 ? 0 : (si == 1 ? e0 : (si == 2 ? e1 : e2)));
                const float* p = a.src[si] + ((size_t)nrow * a.ch[si] + cl) * plane;
                const float top = p[o00] * (1.0f - lx) + p[o01] * lx;
                const float bot = p[o10] * (1.0f - lx) + p[o11] * lx;
                val = top * (1.0f - ly) + bot * ly;
            } else if (k == a.cin && a.out_pitch != 8) {
                val = 1.0f;  // carries init_conv's bias through the composed enc0 weights
            }
            v[k] = val;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = pack_el16x2(v[2 * k], v[2 * k + 1]);
    }
    if (a.out_pitch == 8) {  // (cin <= 8: w[4..7] are zero)
        *(uint4*)(a.out + (size_t)idx * 8) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    uint4* o = (uint4*)(a.out + (size_t)idx * 16);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// Row-block form of stem16_kernel: one workgroup per (sample, block of ST_ROWS padded output rows).  The source rows the
// block touches (<= ST_ROWS + 2 when the grid is upsampled: all channels, native width) are staged in LDS as [row][x][channel]
// once, with loads that are contiguous along x; every lane then reads its four taps as 16-byte LDS rows and two lanes share a
// pixel (8 channels = 16 bytes each), so a wave's store instruction writes 1 KB of consecutive bytes.  stem16_kernel issues 4
// scattered 4-byte global loads per channel and pixel (32 per thread for the NS inputs).  The expressions are the same (x
// first, then y); the compiler contracts them into FMAs differently, so the two forms agree to a 16-bit rounding tie, not bit
// for bit.  (One ROW per workgroup was slower than stem16_kernel: 41 280 workgroups each waiting for its own staging round trip.)
constexpr int ST_ROWS = 8;
template <int CP>  // channels padded to a multiple of 4 (LDS row of a source pixel)
__global__ __launch_bounds__(512) void stem16_rows_kernel(StemArgs a, int nblk) {
    extern __shared__ __attribute__((aligned(16))) float st_rows[];  // [ST_ROWS + 2][w][CP]
    stem_rng_begin(a);
    const int ph = a.uh + 2, pw = a.uw + 2;
    const int n = blockIdx.x / nblk, rb = blockIdx.x - n * nblk;
    const int py0 = rb * ST_ROWS, py1 = min(py0 + ST_ROWS, ph);           // padded rows of this block
    const int ya = max(py0 - 1, 0), yb = min(py1 - 2, a.uh - 1);          // image rows among them (ya > yb: border only)
    const float ys = (float)a.h / (float)a.uh, xs = (float)a.w / (float)a.uw;
    int sbase = 0;
    if (ya <= yb) {
        int s0 = ya, s1 = yb, t0, t1;
        float l;
        if (a.resample) {
            bilinear_coord(ya, ys, a.h, s0, t0, l, a.nearest != 0);
            bilinear_coord(yb, ys, a.h, t1, s1, l, a.nearest != 0);
        }
        sbase = s0;
        const int nsrc_rows = s1 - s0 + 1;  // <= ST_ROWS + 2 (host: h <= uh)
        const int nrow = a.src_rows > 0 ? n % a.src_rows : n;
        const size_t plane = (size_t)a.h * a.w;
        const int per_row = a.cin * a.w;
        for (int j = threadIdx.x; j < per_row; j += 512) {  // a thread keeps its (channel, x) and walks the rows: no divisions inside
            const int k = j / a.w, x = j - k * a.w;
            int si = 0, cl = k;
            while (cl >= a.ch[si]) cl -= a.ch[si++];
            const float* sp = a.src[si] + ((size_t)nrow * a.ch[si] + cl) * plane + (size_t)s0 * a.w + x;
            float* dp = st_rows + (size_t)x * CP + k;
            // all row loads in flight together (a rolled loop waited for each load before its LDS store: ~10 serial round trips
            // were the lifetime of a workgroup)
            float tmp[ST_ROWS + 2];
#pragma unroll
            for (int r = 0; r < ST_ROWS + 2; ++r) tmp[r] = r < nsrc_rows ? sp[(size_t)r * a.w] : 0.0f;
#pragma unroll
            for (int r = 0; r < ST_ROWS + 2; ++r)
                if (r < nsrc_rows) dp[(size_t)r * a.w * CP] = tmp[r];
        }
    }
    // per-column (x0, x1, lx) and per-row (y0, y1, ly) stencils, once per workgroup: the item loop below is instruction-bound
    // (the two source-coordinate evaluations and an integer division per 16 bytes were half of it)
    int4* xtab = (int4*)(st_rows + (size_t)(ST_ROWS + 2) * a.w * CP);   // [pw]: x0 * CP, x1 * CP, lx; .w = valid
    int4* ytab = xtab + pw;                                             // [ST_ROWS]: row offsets into st_rows, ly; .w = valid
    for (int px = threadIdx.x; px < pw + ST_ROWS; px += 512) {
        if (px < pw) {
            const int x = px - 1;
            int x0 = x, x1 = x;
            float lx = 0.0f;
            const bool ok = (unsigned)x < (unsigned)a.uw;
            if (ok && a.resample) bilinear_coord(x, xs, a.w, x0, x1, lx, a.nearest != 0);
            xtab[px] = make_int4(ok ? x0 * CP : 0, ok ? x1 * CP : 0, __float_as_int(lx), ok);
        } else {
            const int r = px - pw, y = py0 + r - 1;
            int y0 = y, y1 = y;
            float ly = 0.0f;
            const bool ok = (unsigned)y < (unsigned)a.uh && py0 + r < py1;
            if (ok && a.resample) bilinear_coord(y, ys, a.h, y0, y1, ly, a.nearest != 0);
            ytab[r] = make_int4(ok ? (y0 - sbase) * a.w * CP : 0, ok ? (y1 - sbase) * a.w * CP : 0, __float_as_int(ly), ok);
        }
    }
    __syncthreads();
    const bool p8 = a.out_pitch == 8;  // 8-channel pixels: one 16-byte chunk each, no bias slot
    uint4* oblk = (uint4*)(a.out + (((size_t)n * ph + py0) * pw) * (p8 ? 8 : 16));
    if (a.cin <= 8 && (a.uw & 63) == 0) {
        // At most 8 input channels (the NS nets: 8): channels 8-15 of a pixel are constants (the bias slot, zeros), so only ONE lane per
        // pixel does arithmetic -- the loop is instruction-bound -- and the pixel's two 16-byte halves pass through a per-wave
        // LDS tile so that a wave still stores 2 x 1 KB of consecutive bytes for its 64 consecutive pixels.
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        unsigned char* stg = (unsigned char*)(ytab + ST_ROWS) + wave * 2048;  // [64 pixels][32 B]
        const uint4 zero4 = make_uint4(0, 0, 0, 0);
        const uint4 half1 = a.cin == 8 ? make_uint4(pack_el16x2(1.0f, 0.0f), 0, 0, 0) : zero4;  // slot cin = 1 (init_conv's bias)
        for (int i = threadIdx.x; i < (py1 - py0) * 4; i += 512) {  // the two zero border pixels of every row
            const int rr = i >> 2, q = i & 3;
            if (!p8) oblk[(size_t)rr * 2 * pw + (q < 2 ? q : 2 * pw - 4 + q)] = zero4;
            else if (q < 2) oblk[(size_t)rr * pw + (q ? pw - 1 : 0)] = zero4;
        }
        const int total_in = (py1 - py0) * a.uw;
        int r = 0, j = threadIdx.x;  // interior pixel (row r of the block, column j)
        while (j >= a.uw) { j -= a.uw; ++r; }
        for (int i = threadIdx.x; i < total_in; i += 512) {
            const int4 xt = xtab[j + 1], yt = ytab[r];
            uint4 w = zero4;
            if (yt.w) {
                const int x0 = xt.x, x1 = xt.y;
                const float lx = __int_as_float(xt.z), ly = __int_as_float(yt.z);
                const float* r0 = st_rows + yt.x;
                const float* r1 = st_rows + yt.y;
                float v[8];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float t00[4] = {0, 0, 0, 0}, t01[4] = {0, 0, 0, 0}, t10[4] = {0, 0, 0, 0}, t11[4] = {0, 0, 0, 0};
                    if (4 * q < CP) {
                        const float4 p00 = *(const float4*)(r0 + x0 + 4 * q), p01 = *(const float4*)(r0 + x1 + 4 * q);
                        const float4 p10 = *(const float4*)(r1 + x0 + 4 * q), p11 = *(const float4*)(r1 + x1 + 4 * q);
                        t00[0] = p00.x; t00[1] = p00.y; t00[2] = p00.z; t00[3] = p00.w;
                        t01[0] = p01.x; t01[1] = p01.y; t01[2] = p01.z; t01[3] = p01.w;
                        t10[0] = p10.x; t10[1] = p10.y; t10[2] = p10.z; t10[3] = p10.w;
                        t11[0] = p11.x; t11[1] = p11.y; t11[2] = p11.z; t11[3] = p11.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = 4 * q + e;
                        const float top = t00[e] * (1.0f - lx) + t01[e] * lx;
                        const float bot = t10[e] * (1.0f - lx) + t11[e] * lx;
                        float val = top * (1.0f - ly) + bot * ly;
                        if (k >= a.cin) val = k == a.cin && !p8 ? 1.0f : 0.0f;
                        v[k] = val;
                    }
                }
                w = make_uint4(pack_el16x2(v[0], v[1]), pack_el16x2(v[2], v[3]), pack_el16x2(v[4], v[5]), pack_el16x2(v[6], v[7]));
            }
            if (p8) {  // the pixel IS its first half: a wave stores 1 KB for its 64 consecutive pixels straight from the registers
                oblk[(size_t)r * pw + 1 + j] = w;
                j += 512;
                while (j >= a.uw) { j -= a.uw; ++r; }
                continue;
            }
            *(uint4*)(stg + lane * 32) = w;
            *(uint4*)(stg + lane * 32 + 16) = yt.w ? half1 : zero4;
            uint4* dst = oblk + (size_t)r * 2 * pw + 2 * (1 + j - lane) + lane;  // the wave's 64 pixels: 128 consecutive 16-byte chunks
            dst[0] = *(const uint4*)(stg + lane * 16);
            dst[64] = *(const uint4*)(stg + 1024 + lane * 16);
            j += 512;
            while (j >= a.uw) { j -= a.uw; ++r; }
        }
        return;
    }
    // items: 16-byte chunks, two per pixel (one at pitch 8)
    const int per_row = p8 ? pw : 2 * pw, total = (py1 - py0) * per_row;
    int r = 0, j = threadIdx.x;  // item i = r * per_row + j, advanced without a division (512 <= 2 pw is checked by the launcher)
    while (j >= per_row) { j -= per_row; ++r; }
    for (int i = threadIdx.x; i < total; i += 512) {
        const int px = p8 ? j : j >> 1, half = p8 ? 0 : j & 1;
        const int4 xt = xtab[px], yt = ytab[r];
        uint32_t w[4] = {0, 0, 0, 0};
        if (xt.w && yt.w) {
            const int x0 = xt.x, x1 = xt.y;
            const float lx = __int_as_float(xt.z), ly = __int_as_float(yt.z);
            const float* r0 = st_rows + yt.x;
            const float* r1 = st_rows + yt.y;
            float v[8];
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2) {
                const int q = 2 * half + q2;  // 4-channel group of the concatenation
                float t00[4] = {0, 0, 0, 0}, t01[4] = {0, 0, 0, 0}, t10[4] = {0, 0, 0, 0}, t11[4] = {0, 0, 0, 0};
                if (4 * q < CP) {
                    const float4 p00 = *(const float4*)(r0 + x0 + 4 * q), p01 = *(const float4*)(r0 + x1 + 4 * q);
                    const float4 p10 = *(const float4*)(r1 + x0 + 4 * q), p11 = *(const float4*)(r1 + x1 + 4 * q);
                    t00[0] = p00.x; t00[1] = p00.y; t00[2] = p00.z; t00[3] = p00.w;
                    t01[0] = p01.x; t01[1] = p01.y; t01[2] = p01.z; t01[3] = p01.w;
                    t10[0] = p10.x; t10[1] = p10.y; t10[2] = p10.z; t10[3] = p10.w;
                    t11[0] = p11.x; t11[1] = p11.y; t11[2] = p11.z; t11[3] = p11.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * q + e;
                    const float top = t00[e] * (1.0f - lx) + t01[e] * lx;
                    const float bot = t10[e] * (1.0f - lx) + t11[e] * lx;
                    float val = top * (1.0f - ly) + bot * ly;
                    if (k >= a.cin) val = k == a.cin && !p8 ? 1.0f : 0.0f;  // slot cin carries init_conv's bias through the composed enc0 weights
                    v[4 * q2 + e] = val;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = pack_el16x2(v[2 * k], v[2 * k + 1]);
        }
        oblk[i] = make_uint4(w[0], w[1], w[2], w[3]);
        j += 512;
        while (j >= per_row) { j -= per_row; ++r; }
    }
}

hipError_t launch_stem16(const StemArgs& a, hipStream_t s) {
    const int cp = (a.cin + 3) / 4 * 4;  // cin <= 15 (the fused stem's bias channel is slot cin)
    const size_t lds = (size_t)(ST_ROWS + 2) * a.w * cp * sizeof(float) + (size_t)(a.uw + 2 + ST_ROWS) * 16 + 8 * 2048;  // rows + stencil tables + per-wave output tiles
    const bool rows = dyf_form_int("DYF_STEM16_ROWS", 1) != 0;  // read per launch: the parity test flips it
    const int rows_out = stem16_out_rows(a), pitch = a.out_pitch == 8 ? 8 : 16;
    if ((a.out_pitch != 0 && a.out_pitch != 8 && a.out_pitch != 16) || (pitch == 8 && a.cin > 8)) return hipErrorInvalidValue;
    if (rows && lds <= 48 * 1024 && cp <= 16 && a.h <= a.uh && 2 * (a.uw + 2) >= 512) {
        const int nblk = (a.uh + 2 + ST_ROWS - 1) / ST_ROWS;
        const dim3 grid((unsigned)(rows_out * nblk)), block(512);
        dyf_form_note("stem16_rows_kernel", a.n);  // (the rows of the forward the launch serves, written or not)
        KernelProf kp("stem16_rows_kernel", s, (double)(a.src_rows ? a.src_rows : a.n) * a.h * a.w * a.cin * 4.0 + (double)rows_out * (a.uh + 2) * (a.uw + 2) * pitch * 2.0);
        if (cp == 4) hipLaunchKernelGGL(stem16_rows_kernel<4>, grid, block, lds, s, a, nblk);
        else if (cp == 8) hipLaunchKernelGGL(stem16_rows_kernel<8>, grid, block, lds, s, a, nblk);
        else if (cp == 12) hipLaunchKernelGGL(stem16_rows_kernel<12>, grid, block, lds, s, a, nblk);
        else hipLaunchKernelGGL(stem16_rows_kernel<16>, grid, block, lds, s, a, nblk);
        return hipGetLastError();
    }
    const long long total = (long long)rows_out * (a.uh + 2) * (a.uw + 2);
    dyf_form_note("stem16_kernel", a.n);
    hipLaunchKernelGGL(stem16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ K2 x2 upsample
// unet_simple.py:42 nn.Upsample(scale_factor=2, bilinear) applied to cat[x, skip] (:176-177).
template <int VEC>
__global__ __launch_bounds__(256) void up2x_kernel(Up2xArgs a, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = a.c0 + a.c1;
    const int groups = c / VEC;
    const int g = (int)(idx % groups);
    const long long pix = idx / groups;
    const int ow = 2 * a.w, oh = 2 * a.h;
    const int n = (int)(pix / ((long long)oh * ow));
    const int rem = (int)(pix % ((long long)oh * ow));
    const int y = rem / ow, x = rem % ow;
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_coord(y, 0.5f, a.h, y0, y1, ly);
    bilinear_coord(x, 0.5f, a.w, x0, x1, lx);
    int ch = g * VEC;
    const el16_t* src = a.src0;
    int cs = a.c0;
    if (ch >= a.c0) {
        src = a.src1;
        cs = a.c1;
        ch -= a.c0;
    }
    const size_t base = (size_t)n * a.h * a.w;
    const el16_t* p00 = src + ((base + (size_t)y0 * a.w + x0) * cs + ch);
    const el16_t* p01 = src + ((base + (size_t)y0 * a.w + x1) * cs + ch);
    const el16_t* p10 = src + ((base + (size_t)y1 * a.w + x0) * cs + ch);
    const el16_t* p11 = src + ((base + (size_t)y1 * a.w + x1) * cs + ch);
    el16_t* o = a.out + ((size_t)pix * c + g * VEC);
    if (VEC == 8) {
        const uint4 q00 = *(const uint4*)p00, q01 = *(const uint4*)p01, q10 = *(const uint4*)p10, q11 = *(const uint4*)p11;
        const uint32_t* w00 = (const uint32_t*)&q00;
        const uint32_t* w01 = (const uint32_t*)&q01;
        const uint32_t* w10 = (const uint32_t*)&q10;
        const uint32_t* w11 = (const uint32_t*)&q11;
        uint32_t r[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float lo, hi;
            {
                const float a00 = el16_lo(w00[t]), a01 = el16_lo(w01[t]);
                const float a10 = el16_lo(w10[t]), a11 = el16_lo(w11[t]);
                const float top = a00 * (1.0f - lx) + a01 * lx, bot = a10 * (1.0f - lx) + a11 * lx;
                lo = top * (1.0f - ly) + bot * ly;
            }
            {
                const float a00 = el16_hi(w00[t]), a01 = el16_hi(w01[t]);
                const float a10 = el16_hi(w10[t]), a11 = el16_hi(w11[t]);
                const float top = a00 * (1.0f - lx) + a01 * lx, bot = a10 * (1.0f - lx) + a11 * lx;
                hi = top * (1.0f - ly) + bot * ly;
            }
            r[t] = pack_el16x2(lo, hi);
        }
        *(uint4*)o = make_uint4(r[0], r[1], r[2], r[3]);
    } else {
        const float a00 = el16_to_f32(*p00), a01 = el16_to_f32(*p01), a10 = el16_to_f32(*p10), a11 = el16_to_f32(*p11);
        const float top = a00 * (1.0f - lx) + a01 * lx, bot = a10 * (1.0f - lx) + a11 * lx;
        *o = f32_to_el16(top * (1.0f - ly) + bot * ly);
    }
}

// Quad form: a thread produces the 2 x 2 output pixels of one input pixel (one 16-byte channel chunk) from its 3 x 3 input
// neighbourhood: 9 loads and one index decomposition per FOUR outputs (up2x_kernel<8>: 16 loads and three 64-bit divisions per
// four), same stencils (bilinear_coord) and the same expressions per output.
__global__ __launch_bounds__(256) void up2x_quad_kernel(Up2xArgs a, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = a.c0 + a.c1, groups = c >> 3;
    const int g = (int)(idx % groups);
    const int pix = (int)(idx / groups);           // input pixel (n, i, j)
    const int plane = a.h * a.w;
    const int n = pix / plane, rem = pix - n * plane;
    const int i = rem / a.w, j = rem - i * a.w;
    int ch = g * 8;
    const el16_t* src = a.src0;
    int cs = a.c0;
    if (ch >= a.c0) {
        src = a.src1;
        cs = a.c1;
        ch -= a.c0;
    }
    // rows / columns the four outputs read: output 2i reads (i-1, i), output 2i+1 reads (i, i+1), clamped by bilinear_coord
    int ya[2], yb[2], xa[2], xb[2];
    float ly[2], lx[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        bilinear_coord(2 * i + d, 0.5f, a.h, ya[d], yb[d], ly[d]);
        bilinear_coord(2 * j + d, 0.5f, a.w, xa[d], xb[d], lx[d]);
    }
    const int ys[3] = {ya[0], i, yb[1]}, xs[3] = {xa[0], j, xb[1]};  // (ya[1] == yb[0] == i except at a clamped border, where the weight of the other tap is 0 or the indices coincide)
    uint4 t[3][3];
    const el16_t* base = src + (size_t)n * plane * cs + ch;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) t[r][q] = *(const uint4*)(base + ((size_t)ys[r] * a.w + xs[q]) * cs);
    const int ow = 2 * a.w;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            // taps of output (2i+dy, 2j+dx): rows ys[dy], ys[dy+1], columns xs[dx], xs[dx+1].  At a clamped border (output 0 of
            // input 0) bilinear_coord's second tap is index 1 with weight exactly 0; slot 1 holds index 0 there: finite * 0 either way
            const uint4 q00 = t[dy][dx], q01 = t[dy][dx + 1], q10 = t[dy + 1][dx], q11 = t[dy + 1][dx + 1];
            const uint32_t* w00 = (const uint32_t*)&q00;
            const uint32_t* w01 = (const uint32_t*)&q01;
            const uint32_t* w10 = (const uint32_t*)&q10;
            const uint32_t* w11 = (const uint32_t*)&q11;
            const float fx = lx[dx], fy = ly[dy];
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float lo, hi;
                {
                    const float a00 = el16_lo(w00[k]), a01 = el16_lo(w01[k]), a10 = el16_lo(w10[k]), a11 = el16_lo(w11[k]);
                    const float top = a00 * (1.0f - fx) + a01 * fx, bot = a10 * (1.0f - fx) + a11 * fx;
                    lo = top * (1.0f - fy) + bot * fy;
                }
                {
                    const float a00 = el16_hi(w00[k]), a01 = el16_hi(w01[k]), a10 = el16_hi(w10[k]), a11 = el16_hi(w11[k]);
                    const float top = a00 * (1.0f - fx) + a01 * fx, bot = a10 * (1.0f - fx) + a11 * fx;
                    hi = top * (1.0f - fy) + bot * fy;
                }
                o[k] = pack_el16x2(lo, hi);
            }
            *(uint4*)(a.out + (((size_t)n * 2 * a.h + 2 * i + dy) * ow + 2 * j + dx) * c + g * 8) = make_uint4(o[0], o[1], o[2], o[3]);
        }
}

hipError_t launch_up2x(const Up2xArgs& a, hipStream_t s) {
    const int c = a.c0 + a.c1;
    const bool vec = (a.c0 % 8 == 0) && (a.c1 % 8 == 0);
    const long long total = (long long)a.n * 4 * a.h * a.w * (vec ? c / 8 : c);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    const bool quad = dyf_form_int("DYF_UP2X_QUAD", 1) != 0;  // read per launch (parity test)
    if (vec && quad && a.h >= 2 && a.w >= 2) {
        const long long quads = total / 4;
        dyf_form_note("up2x_quad_kernel", a.n);
        KernelProf kp("up2x_quad_kernel", s, (double)a.n * a.h * a.w * c * 2.0 * 5.0);  // read once, write 4x
        hipLaunchKernelGGL(up2x_quad_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, a, quads);
    } else if (vec)
        hipLaunchKernelGGL(up2x_kernel<8>, dim3(blocks), dim3(256), 0, s, a, total);
    else
        hipLaunchKernelGGL(up2x_kernel<1>, dim3(blocks), dim3(256), 0, s, a, total);
    return hipGetLastError();
}

// Upsample + epilogue of the commuted 1 x 1 decoder blocks (Up2xEpiArgs, kernels.h).  A thread owns one LOW-res pixel and 4 channels:
// 9 float4 loads (its 3 x 3 neighbourhood, stencils of bilinear_coord as in up2x_quad_kernel) make the 2 x 2 outputs.
__global__ __launch_bounds__(256) void up2x_epilogue_kernel(Up2xEpiArgs a, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int groups = a.c >> 2;
    const int g = (int)(idx % groups);
    const int pix = (int)(idx / groups);
    const int plane = a.h * a.w;
    const int n = pix / plane, rem = pix - n * plane;
    const int i = rem / a.w, j = rem - i * a.w;
    int ya[2], yb[2], xa[2], xb[2];
    float ly[2], lx[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        bilinear_coord(2 * i + d, 0.5f, a.h, ya[d], yb[d], ly[d]);
        bilinear_coord(2 * j + d, 0.5f, a.w, xa[d], xb[d], lx[d]);
    }
    const int ys[3] = {ya[0], i, yb[1]}, xs[3] = {xa[0], j, xb[1]};
    float4 t[3][3];
    const float* base = a.lo + (size_t)n * plane * a.c + g * 4;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) t[r][q] = *(const float4*)(base + ((size_t)ys[r] * a.w + xs[q]) * a.c);
    const size_t ci = (size_t)(a.coef_div > 1 ? n / a.coef_div : n) * a.coef_stride + g * 4;
    const float4 ca = *(const float4*)(a.coef_a + ci), cc = *(const float4*)(a.coef_c + ci);
    const RngKey key = drop_row_key(a.drop, n);
    const int ow = 2 * a.w, oh = 2 * a.h;
    const uint32_t row0 = (uint32_t)n * (uint32_t)(oh * ow * a.c);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const float4 q00 = t[dy][dx], q01 = t[dy][dx + 1], q10 = t[dy + 1][dx], q11 = t[dy + 1][dx + 1];
            const float fx = lx[dx], fy = ly[dy];
            auto lerp = [&](float a00, float a01, float a10, float a11) {
                const float top = a00 * (1.0f - fx) + a01 * fx, bot = a10 * (1.0f - fx) + a11 * fx;
                return top * (1.0f - fy) + bot * fy;
            };
            float v[4] = {fmaf(lerp(q00.x, q01.x, q10.x, q11.x), ca.x, cc.x), fmaf(lerp(q00.y, q01.y, q10.y, q11.y), ca.y, cc.y),
                          fmaf(lerp(q00.z, q01.z, q10.z, q11.z), ca.z, cc.z), fmaf(lerp(q00.w, q01.w, q10.w, q11.w), ca.w, cc.w)};
            const uint32_t e0 = (uint32_t)(((n * oh + 2 * i + dy) * ow + 2 * j + dx)) * (uint32_t)a.c + (uint32_t)(g * 4);
            act_drop<4>(v, e0, row0, a.act, a.drop, key);
            *(uint2*)(a.out + (size_t)e0) = make_uint2(pack_el16x2(v[0], v[1]), pack_el16x2(v[2], v[3]));
        }
}

hipError_t launch_up2x_epilogue(const Up2xEpiArgs& a, hipStream_t s) {
    if ((a.c & 3) != 0 || a.h < 1 || a.w < 1 || (size_t)a.n * 4 * a.h * a.w * a.c >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
    const long long total = (long long)a.n * a.h * a.w * (a.c >> 2);
    dyf_form_note("up2x_epilogue_kernel", a.n);
    KernelProf kp("up2x_epilogue_kernel", s, (double)a.n * a.h * a.w * a.c * (4.0 + 4 * 2.0));  // fp32 low-res in, 16-bit x 4 out
    hipLaunchKernelGGL(up2x_epilogue_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, total);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ K5 GroupNorm
// nn.GroupNorm(8, C) of the last encoder block (unet_simple.py:56) + FiLM + LeakyReLU + Dropout (:72-80).
__global__ __launch_bounds__(256) void groupnorm_kernel(GroupNormArgs a) {
    __shared__ float scratch[16];
    const int n = blockIdx.x / a.groups, g = blockIdx.x % a.groups;
    const int cpg = a.c / a.groups;
    const int count = a.hw * cpg;
    const float* x = a.x + (size_t)n * a.hw * a.c + g * cpg;
    float s = 0.0f;
    for (int i = threadIdx.x; i < count; i += blockDim.x) s += x[(size_t)(i / cpg) * a.c + (i % cpg)];
    const float mean = block_sum(s, scratch) / (float)count;
    float v = 0.0f;
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const float d = x[(size_t)(i / cpg) * a.c + (i % cpg)] - mean;
        v = fmaf(d, d, v);
    }
    const float var = block_sum(v, scratch) / (float)count;  // biased, as torch
    const float rstd = rsqrtf(var + 1e-5f);
    const RngKey key = drop_row_key(a.drop, n);
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const int p = i / cpg, ch = g * cpg + (i % cpg);
        float y = (x[(size_t)p * a.c + (i % cpg)] - mean) * rstd * a.gamma[ch] + a.beta[ch];
        const size_t fi = (size_t)(a.film_div > 1 ? n / a.film_div : n) * a.film_stride + ch;
        y = fmaf(y, a.film_a[fi], a.film_c[fi]);
        y = apply_act(y, a.act);
        const size_t e = ((size_t)n * a.hw + p) * a.c + ch;
        y = drop_apply(y, (uint32_t)e, (uint32_t)((size_t)n * a.hw * a.c), a.drop, key);
        a.out[e] = f32_to_el16(y);
    }
}

// Small planes (the GroupNorm block of unet_simple sits at the bottleneck: 4 x 4 pixels x 64 channels per group): ONE WAVE per
// (sample, group) keeps its <= 32 elements per lane in registers -- one pass over memory instead of three, wave reductions instead of
// two block reductions -- mean first, then the variance of the centred values (as groupnorm_kernel and ATen do).
template <int PER>  // float4 pieces per lane
__global__ __launch_bounds__(256) void groupnorm_wave_kernel(GroupNormArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ng = blockIdx.x * 4 + wv;
    if (ng >= a.n * a.groups) return;
    const int n = ng / a.groups, g = ng - n * a.groups;
    const int cpg = a.c / a.groups, q4 = cpg >> 2;   // float4 pieces per pixel of the group
    const int pieces = a.hw * q4;
    const float* x = a.x + (size_t)n * a.hw * a.c + g * cpg;
    float4 v[PER];
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int pc = lane + 64 * k;
        v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (pc < pieces) {
            v[k] = *(const float4*)(x + (size_t)(pc / q4) * a.c + (pc % q4) * 4);
            s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    const float count = (float)(a.hw * cpg);
    const float mean = s / count;
    float var = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (lane + 64 * k < pieces) {
            const float dx = v[k].x - mean, dy = v[k].y - mean, dz = v[k].z - mean, dw = v[k].w - mean;
            var = fmaf(dx, dx, var); var = fmaf(dy, dy, var); var = fmaf(dz, dz, var); var = fmaf(dw, dw, var);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) var += __shfl_xor(var, d, 64);
    const float rstd = rsqrtf(var / count + 1e-5f);
    const RngKey key = drop_row_key(a.drop, n);
    const uint32_t row0 = (uint32_t)((size_t)n * a.hw * a.c);
    const size_t frow = (size_t)(a.film_div > 1 ? n / a.film_div : n) * a.film_stride;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int pc = lane + 64 * k;
        if (pc >= pieces) continue;
        const int p = pc / q4, ch = g * cpg + (pc % q4) * 4;
        const float4 ga = *(const float4*)(a.gamma + ch), be = *(const float4*)(a.beta + ch);
        const float4 fa = *(const float4*)(a.film_a + frow + ch), fc = *(const float4*)(a.film_c + frow + ch);
        float y[4] = {(v[k].x - mean) * rstd * ga.x + be.x, (v[k].y - mean) * rstd * ga.y + be.y, (v[k].z - mean) * rstd * ga.z + be.z,
                      (v[k].w - mean) * rstd * ga.w + be.w};
        y[0] = fmaf(y[0], fa.x, fc.x); y[1] = fmaf(y[1], fa.y, fc.y); y[2] = fmaf(y[2], fa.z, fc.z); y[3] = fmaf(y[3], fa.w, fc.w);
        const uint32_t e0 = row0 + (uint32_t)(p * a.c + ch);
        act_drop<4>(y, e0, row0, a.act, a.drop, key);
        *(uint2*)(a.out + (size_t)e0) = make_uint2(pack_el16x2(y[0], y[1]), pack_el16x2(y[2], y[3]));
    }
}

hipError_t launch_groupnorm(const GroupNormArgs& a, hipStream_t s) {
    const int cpg = a.groups > 0 ? a.c / a.groups : 0;
    const bool wave = dyf_form_int("DYF_GN_WAVE", 1) != 0;  // read per launch (parity test)
    if (wave && cpg > 0 && cpg * a.groups == a.c && (cpg & 3) == 0 && a.act != ACT_GELU &&
        (size_t)a.n * a.hw * a.c < 0xFFFFFFF0ull) {
        const int pieces = a.hw * (cpg >> 2);
        const unsigned blocks = (unsigned)((a.n * a.groups + 3) / 4);
        if (pieces <= 256) {
            dyf_form_note("groupnorm_wave_kernel", a.n);
            hipLaunchKernelGGL(groupnorm_wave_kernel<4>, dim3(blocks), dim3(256), 0, s, a);
            return hipGetLastError();
        }
        if (pieces <= 512) {
            dyf_form_note("groupnorm_wave_kernel", a.n);
            hipLaunchKernelGGL(groupnorm_wave_kernel<8>, dim3(blocks), dim3(256), 0, s, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL(groupnorm_kernel, dim3(a.n * a.groups), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ K3+K4 readout
// ConvTranspose2d(dim -> C, k4, s2, p1) followed by the final bilinear resample to the native grid
// (unet_simple.py:141-151, :195).  The resample (no antialias) reads only 4 neighbours of each native pixel, so the
// transposed conv is evaluated at exactly those positions instead of materialising the 2x-resolution tensor.
// out[u] of a k4/s2/p1 transposed conv gathers input rows i with kh = u + 1 - 2i in [0, 3]: i = (u+1)>>1 and i - 1.
__global__ __launch_bounds__(256) void readout_kernel(ReadoutArgs a) {
    extern __shared__ float wsh[];  // [16][cin][cout]
    const int wcount = 16 * a.cin * a.cout;
    for (int i = threadIdx.x; i < wcount; i += blockDim.x) wsh[i] = a.wgt[i];
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)a.n * a.oh * a.ow;
    if (idx >= total) return;
    const int n = (int)(idx / ((long long)a.oh * a.ow));
    const int rem = (int)(idx % ((long long)a.oh * a.ow));
    const int oy = rem / a.ow, ox = rem % a.ow;
    const int th = 2 * a.ih, tw = 2 * a.iw;  // transposed-conv output grid
    int u0, u1, v0, v1;
    float lu, lv;
    bilinear_coord(oy, (float)th / (float)a.oh, th, u0, u1, lu, a.nearest != 0);
    bilinear_coord(ox, (float)tw / (float)a.ow, tw, v0, v1, lv, a.nearest != 0);
    float acc[DYF_MAX_OUT_CH];
#pragma unroll
    for (int c = 0; c < DYF_MAX_OUT_CH; ++c) acc[c] = 0.0f;
    const int us[2] = {u0, u1}, vs[2] = {v0, v1};
    const float wu[2] = {1.0f - lu, lu}, wv[2] = {1.0f - lv, lv};
#pragma unroll
    for (int a_ = 0; a_ < 2; ++a_) {
#pragma unroll
        for (int b_ = 0; b_ < 2; ++b_) {
            const float bw = wu[a_] * wv[b_];
            const int u = us[a_], v = vs[b_];
            const int i_hi = (u + 1) >> 1, j_hi = (v + 1) >> 1;
#pragma unroll
            for (int di = 0; di < 2; ++di) {
                const int i = i_hi - di, kh = u + 1 - 2 * i;
                if ((unsigned)i >= (unsigned)a.ih) continue;
#pragma unroll
                for (int dj = 0; dj < 2; ++dj) {
                    const int j = j_hi - dj, kw = v + 1 - 2 * j;
                    if ((unsigned)j >= (unsigned)a.iw) continue;
                    const el16_t* px = a.x + (((size_t)n * a.ih + i) * a.iw + j) * a.cin;
                    const float* wt = wsh + (size_t)(kh * 4 + kw) * a.cin * a.cout;
                    for (int ci = 0; ci < a.cin; ++ci) {
                        const float xv = bw * el16_to_f32(px[ci]);
#pragma unroll
                        for (int co = 0; co < DYF_MAX_OUT_CH; ++co)
                            if (co < a.cout) acc[co] = fmaf(xv, wt[ci * a.cout + co], acc[co]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int co = 0; co < DYF_MAX_OUT_CH; ++co)
        if (co < a.cout) a.out[(((size_t)n * a.cout + co) * a.oh + oy) * a.ow + ox] = acc[co] + a.bias[co];
}

// Fast form for cin % 8 == 0 with cin/8 a power of two: LANES = cin/8 lanes share one native pixel, each owns an
// 8-channel slice, so every tap is ONE 16-B load per lane (a full 128-B line per pixel for dim 64) instead of 64
// scattered 2-B loads; partial sums are combined with a butterfly over the LANES lanes.
template <int LANES>
__global__ __launch_bounds__(256) void readout_sliced_kernel(ReadoutArgs a) {
    extern __shared__ float wsh[];  // [16][cin][cout]
    const int wcount = 16 * a.cin * a.cout;
    for (int i = threadIdx.x; i < wcount; i += blockDim.x) wsh[i] = a.wgt[i];
    __syncthreads();
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)a.n * a.oh * a.ow;
    long long idx = gid / LANES;
    const int slice = (int)(gid % LANES);
    const bool live = idx < total;
    if (!live) idx = total - 1;  // keep the whole wave in the shuffles
    const int n = (int)(idx / ((long long)a.oh * a.ow));
    const int rem = (int)(idx % ((long long)a.oh * a.ow));
    const int oy = rem / a.ow, ox = rem % a.ow;
    const int th = 2 * a.ih, tw = 2 * a.iw;
    int u0, u1, v0, v1;
    float lu, lv;
    bilinear_coord(oy, (float)th / (float)a.oh, th, u0, u1, lu, a.nearest != 0);
    bilinear_coord(ox, (float)tw / (float)a.ow, tw, v0, v1, lv, a.nearest != 0);
    float acc[DYF_MAX_OUT_CH];
#pragma unroll
    for (int c = 0; c < DYF_MAX_OUT_CH; ++c) acc[c] = 0.0f;
    const int ci0 = slice * 8;
    // all 16 (neighbour, tap) input vectors are requested up front (one 16-B load each, independent), so the kernel is
    // not a chain of 16 dependent L2 round trips; taps outside the image contribute zero
    uint4 qv[16];
    int wofs[16];
    float bwv[16];
#pragma unroll
    for (int nb4 = 0; nb4 < 4; ++nb4) {
        const int u = (nb4 & 2) ? u1 : u0, v = (nb4 & 1) ? v1 : v0;
        const float bw = ((nb4 & 2) ? lu : 1.0f - lu) * ((nb4 & 1) ? lv : 1.0f - lv);
        const int i_hi = (u + 1) >> 1, j_hi = (v + 1) >> 1;
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            const int i = i_hi - (t4 >> 1), j = j_hi - (t4 & 1);
            const int kh = u + 1 - 2 * i, kw = v + 1 - 2 * j;
            const bool ok = (unsigned)i < (unsigned)a.ih && (unsigned)j < (unsigned)a.iw;
            const int ic = ok ? i : 0, jc = ok ? j : 0;
            const uint4 ld = *(const uint4*)(a.x + (((size_t)n * a.ih + ic) * a.iw + jc) * a.cin + ci0);
            qv[nb4 * 4 + t4] = ok ? ld : make_uint4(0u, 0u, 0u, 0u);
            bwv[nb4 * 4 + t4] = ok ? bw : 0.0f;
            wofs[nb4 * 4 + t4] = ((kh * 4 + kw) * a.cin + ci0) * a.cout;
        }
    }
#pragma unroll
    for (int s16 = 0; s16 < 16; ++s16) {
        const uint32_t qw[4] = {qv[s16].x, qv[s16].y, qv[s16].z, qv[s16].w};
        const float* wt = wsh + wofs[s16];
        const float bw = bwv[s16];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float xv = bw * ((c & 1) ? el16_hi(qw[c >> 1]) : el16_lo(qw[c >> 1]));
#pragma unroll
            for (int co = 0; co < DYF_MAX_OUT_CH; ++co)
                if (co < a.cout) acc[co] = fmaf(xv, wt[c * a.cout + co], acc[co]);
        }
    }
#pragma unroll
    for (int co = 0; co < DYF_MAX_OUT_CH; ++co) {
        if (co < a.cout) {
            float v = acc[co];
#pragma unroll
            for (int off = LANES >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (live && slice == 0) a.out[(((size_t)n * a.cout + co) * a.oh + oy) * a.ow + ox] = v + a.bias[co];
        }
    }
}

// Register-weight form for cin == 64 (the NS backbone): the sliced kernel above is bound by its 384 LDS weight reads per
// thread.  Every native pixel uses each of the 16 (kh, kw) taps of the transposed conv exactly once (u0/u1 and v0/v1 have
// opposite parities), reading a 3x3 window of decoder pixels.  So 32 lanes share a pixel: lane (kh = 0..3, slice = 0..7)
// keeps the weights of its kernel row and 8-channel slice in REGISTERS (4 kw x 8 c x CO), loads the 4 input vectors of
// its row (16 B each; 8 slices = one 128-B line) and the 32 partial sums are combined with a butterfly.  A half-wave
// walks a contiguous run of native pixels (oy fastest: consecutive pixels share two of the three input rows in L1).
template <int CO>
__global__ __launch_bounds__(256) void readout_regw_kernel(ReadoutArgs a, int px_per_half) {
    const int lane = threadIdx.x & 63;
    const int half = (int)((blockIdx.x * 256 + threadIdx.x) >> 5);
    const int kh = (lane >> 3) & 3, slice = lane & 7, ci0 = slice * 8;
    float w[4][8][CO];
#pragma unroll
    for (int kw = 0; kw < 4; ++kw)
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int co = 0; co < CO; ++co) w[kw][c][co] = a.wgt[((size_t)(kh * 4 + kw) * a.cin + ci0 + c) * CO + co];
    float bias[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) bias[co] = a.bias[co];
    const int total = a.n * a.oh * a.ow;
    const int th = 2 * a.ih, tw = 2 * a.iw;
    const float sh = (float)th / (float)a.oh, sw = (float)tw / (float)a.ow;
    const int pu = (kh + 1) & 1;
    // pixel order: (n, ox, oy), oy fastest; the position is advanced incrementally (no per-pixel divisions)
    int idx = half * px_per_half;
    int n, ox, oy;
    {
        const int ic = idx < total ? idx : total - 1;
        n = ic / (a.oh * a.ow);
        const int rem = ic - n * (a.oh * a.ow);
        ox = rem / a.oh;
        oy = rem - ox * a.oh;
    }
    // one pixel's inputs: 4 vectors of this lane's kernel row + their bilinear weights
    struct Px {
        uint4 q[4];
        float bw[4];
        int out_off;  // element offset of channel 0 in `out`, or -1
    };
    auto fetch = [&](Px& p) {
        const bool live = idx < total;
        int u0, u1, v0, v1;
        float lu, lv;
        bilinear_coord(oy, sh, th, u0, u1, lu, a.nearest != 0);
        bilinear_coord(ox, sw, tw, v0, v1, lv, a.nearest != 0);
        // kernel row kh pairs with the neighbour u of parity (kh + 1) & 1: kh = u + 1 - 2 i, i = ((u + 1) >> 1) - (kh >> 1)
        const float wu = ((u0 & 1) == pu ? 1.0f - lu : 0.0f) + ((u1 & 1) == pu ? lu : 0.0f);
        const int u = (u1 & 1) == pu ? u1 : u0;
        const int i = ((u + 1) >> 1) - (kh >> 1);
        const bool row_ok = (unsigned)i < (unsigned)a.ih;
        const el16_t* row = a.x + ((size_t)n * a.ih + (row_ok ? i : 0)) * a.iw * a.cin + ci0;
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) {
            const int pv = (kw + 1) & 1;
            const float wv = ((v0 & 1) == pv ? 1.0f - lv : 0.0f) + ((v1 & 1) == pv ? lv : 0.0f);
            const int v = (v1 & 1) == pv ? v1 : v0;
            const int j = ((v + 1) >> 1) - (kw >> 1);
            const bool ok = row_ok && (unsigned)j < (unsigned)a.iw;
            const uint4 qv = *(const uint4*)(row + (size_t)(ok ? j : 0) * a.cin);
            // taps outside the image contribute exactly zero whatever the (possibly never written) fallback pixel holds
            p.q[kw] = ok ? qv : make_uint4(0u, 0u, 0u, 0u);
            p.bw[kw] = ok ? wu * wv : 0.0f;
        }
        p.out_off = live ? ((n * CO) * a.oh + oy) * a.ow + ox : -1;
        // advance (clamped at the last pixel so that the whole wave stays in the shuffles)
        ++idx;
        if (idx < total) {
            if (++oy == a.oh) {
                oy = 0;
                if (++ox == a.ow) { ox = 0; ++n; }
            }
        }
    };
    auto reduce_store = [&](const Px& p) {
        float acc[CO];
#pragma unroll
        for (int co = 0; co < CO; ++co) acc[co] = 0.0f;
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) {
            const uint32_t qw[4] = {p.q[kw].x, p.q[kw].y, p.q[kw].z, p.q[kw].w};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float xv = p.bw[kw] * ((c & 1) ? el16_hi(qw[c >> 1]) : el16_lo(qw[c >> 1]));
#pragma unroll
                for (int co = 0; co < CO; ++co) acc[co] = fmaf(xv, w[kw][c][co], acc[co]);
            }
        }
#pragma unroll
        for (int co = 0; co < CO; ++co) {
            float v = acc[co];
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (p.out_off >= 0 && (lane & 31) == 0) a.out[(size_t)p.out_off + (size_t)co * a.oh * a.ow] = v + bias[co];
        }
    };
    // two pixels in flight: the loads of pixel it+1 are issued before the FMAs of pixel it
    Px p0, p1;
    fetch(p0);
    for (int it = 0; it < px_per_half; it += 2) {
        fetch(p1);
        reduce_store(p0);
        fetch(p0);
        reduce_store(p1);
    }
}

// MFMA form for cin == 64, cout <= 4 (the NS backbone): the register-weight form above is VALU-bound (~230 VALU per lane and
// pixel).  Here a wave takes 16 native pixels at a time; for each of the 16 (kh, kw) taps the 64-channel contraction of all 16
// pixels is two v_mfma_f32_16x16x32_bf16 (A = the tap's weights as a [16 (cout, zero-padded)][32 k] fragment held in
// registers for the whole kernel, B = the pixels' input vectors: lane (pixel p, k-group g) loads 16 B of pixel p's tap
// vector, exactly its MFMA operand), and the bilinear weight of the tap scales the 3 result rows with 3 FMAs.  Coordinates
// are computed once per pixel by 4 lanes instead of 32.  Weights are bf16 here (fp32 in the other forms).
typedef __attribute__((ext_vector_type(4))) float ro_f32x4;

__global__ __launch_bounds__(256, 4) void readout_mfma_kernel(ReadoutArgs a, int groups_per_wave) {
#if defined(__HIP_DEVICE_COMPILE__)
    // weight fragments [tap][k half][lane] x 16 B in LDS (32 KB): lane (m = lane & 15, k-group) holds
    // W[tap][half*32 + kg*8 + e][co = m] (0 for m >= cout); fragment reads are lane-linear, i.e. conflict-free
    extern __shared__ __attribute__((aligned(16))) char ro_smem[];
    for (int i = threadIdx.x; i < 16 * 2 * 64; i += 256) ((uint4*)ro_smem)[i] = ((const uint4*)a.wfrag)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave_id = (int)((blockIdx.x * 256 + threadIdx.x) >> 6);
    const int p = lane & 15, kg = lane >> 4;
    const el16x8_t* wl = (const el16x8_t*)ro_smem + lane;
    const int total = a.n * a.oh * a.ow;
    const int th = 2 * a.ih, tw = 2 * a.iw;
    const float sh = (float)th / (float)a.oh, sw = (float)tw / (float)a.ow;
    const int plane = a.oh * a.ow;
    for (int g = 0; g < groups_per_wave; ++g) {
        const int idx0 = (wave_id * groups_per_wave + g) * 16;
        if (idx0 >= total) break;  // wave-uniform
        int idx = idx0 + p;
        const bool live = idx < total;
        if (!live) idx = total - 1;
        // pixel order (n, oy, ox), ox fastest: the 16 pixels of a group read the same three input rows.  (Tried: vertical strips,
        // oy fastest, whose 4-row windows overlap -- 90 instead of 256 distinct input pixels per group, but every load then
        // touches 16 different rows: 312 vs 253 us per paired launch.)
        const int n = idx / plane;
        const int rem = idx - n * plane;
        const int oy = rem / a.ow, ox = rem - oy * a.ow;
        int u0, u1, v0, v1;
        float lu, lv;
        bilinear_coord(oy, sh, th, u0, u1, lu, a.nearest != 0);
        bilinear_coord(ox, sw, tw, v0, v1, lv, a.nearest != 0);
        // per kernel row / column: byte offset of the input row / column (or -1) and bilinear weight (see readout_regw_kernel)
        int ro[4], co_[4];
        float rw[4], cw[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int par = (k + 1) & 1;
            rw[k] = ((u0 & 1) == par ? 1.0f - lu : 0.0f) + ((u1 & 1) == par ? lu : 0.0f);
            const int u = (u1 & 1) == par ? u1 : u0;
            const int i = ((u + 1) >> 1) - (k >> 1);
            ro[k] = (unsigned)i < (unsigned)a.ih ? i * a.iw_store * 64 : -1;
            cw[k] = ((v0 & 1) == par ? 1.0f - lv : 0.0f) + ((v1 & 1) == par ? lv : 0.0f);
            const int v = (v1 & 1) == par ? v1 : v0;
            const int j = ((v + 1) >> 1) - (k >> 1);
            int js = (unsigned)j < (unsigned)a.iw ? j : -1;
            if (js >= 0 && a.col_map) js = a.col_map[js];  // compact input: stored column of j (always stored when read)
            co_[k] = js >= 0 ? js * 64 : -1;
        }
        // LOADS are issued with a coalesced lane map -- lane s fetches 16-B chunk (s & 3) of pixel (s >> 2), so a quad of
        // lanes reads 64 contiguous bytes (with the MFMA's own lane map, pixel = lane & 15, every quad touches four cache
        // lines and the texture path needs 4x the cycles) -- and moved to their MFMA lane with ds_bpermute:
        // MFMA lane t = (pixel t & 15, k-group t >> 4) takes the registers of load lane (t & 15) * 4 + (t >> 4).
        const int lp = lane >> 2, lc = lane & 3;  // pixel / chunk this lane LOADS
        const int src4 = (lp)*4;                  // byte address (lane * 4) of a lane that holds pixel lp's coordinates: lane lp
        int l_ro[4], l_co[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            l_ro[k] = __builtin_amdgcn_ds_bpermute(src4, ro[k]);
            l_co[k] = __builtin_amdgcn_ds_bpermute(src4, co_[k]);
        }
        const int l_n = __builtin_amdgcn_ds_bpermute(src4, n);
        const el16_t* img = a.x + (size_t)l_n * a.ih * a.iw_store * 64 + lc * 8;
        const int take4 = ((lane & 15) * 4 + (lane >> 4)) * 4;
        float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        // two batches of 8 taps (2 kernel rows): all 16 vector loads of a batch are in flight before its MFMAs
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            uint4 q0[8], q1[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int kh = b * 2 + (t >> 2), kw = t & 3;
                const bool ok = l_ro[kh] >= 0 && l_co[kw] >= 0;
                const el16_t* px = img + (ok ? l_ro[kh] + l_co[kw] : 0);
                q0[t] = *(const uint4*)px;
                q1[t] = *(const uint4*)(px + 32);
                if (!ok) { q0[t] = make_uint4(0u, 0u, 0u, 0u); q1[t] = q0[t]; }  // taps outside the image: data 0
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int kh = b * 2 + (t >> 2), kw = t & 3, tap = kh * 4 + kw;
                uint4 m0, m1;
                m0.x = __builtin_amdgcn_ds_bpermute(take4, q0[t].x); m0.y = __builtin_amdgcn_ds_bpermute(take4, q0[t].y);
                m0.z = __builtin_amdgcn_ds_bpermute(take4, q0[t].z); m0.w = __builtin_amdgcn_ds_bpermute(take4, q0[t].w);
                m1.x = __builtin_amdgcn_ds_bpermute(take4, q1[t].x); m1.y = __builtin_amdgcn_ds_bpermute(take4, q1[t].y);
                m1.z = __builtin_amdgcn_ds_bpermute(take4, q1[t].z); m1.w = __builtin_amdgcn_ds_bpermute(take4, q1[t].w);
                ro_f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
                d = DYF_MFMA_16x16x32(wl[(tap * 2 + 0) * 64], __builtin_bit_cast(el16x8_t, m0), d, 0, 0, 0);
                d = DYF_MFMA_16x16x32(wl[(tap * 2 + 1) * 64], __builtin_bit_cast(el16x8_t, m1), d, 0, 0, 0);
                const float bw = (ro[kh] >= 0 && co_[kw] >= 0) ? rw[kh] * cw[kw] : 0.0f;  // this lane's own pixel
#pragma unroll
                for (int r = 0; r < 4; ++r) out[r] = fmaf(bw, d[r], out[r]);
            }
        }
        // rows 0..3 of the 16x16 result (= output channels) live in lanes 0-15 (k-group 0), column = pixel
        if (live && kg == 0) {
            float* o = a.out + ((size_t)n * a.cout * a.oh + oy) * a.ow + ox;
            const size_t cs = (size_t)a.oh * a.ow;
            o[0] = out[0] + a.bias[0];
            if (a.cout > 1) o[cs] = out[1] + a.bias[1];
            if (a.cout > 2) o[2 * cs] = out[2] + a.bias[2];
            if (a.cout > 3) o[3 * cs] = out[3] + a.bias[3];
        }
    }
#endif
}

// Tap tables of the readout for one geometry: the coordinate arithmetic of readout_mfma_kernel, evaluated once per output row /
// column instead of once per pixel and forward (the MFMA forms spend most of their issue slots on it: 16 pixels per wave).
__global__ void readout_tables_kernel(ReadoutArgs a, uint4* row_tab, uint4* col_tab) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int th = 2 * a.ih, tw = 2 * a.iw;
    if (t < a.oh) {
        int u0, u1;
        float lu;
        bilinear_coord(t, (float)th / (float)a.oh, th, u0, u1, lu, a.nearest != 0);
        int off[4];
        float w[4];
        for (int k = 0; k < 4; ++k) {
            const int par = (k + 1) & 1;
            w[k] = ((u0 & 1) == par ? 1.0f - lu : 0.0f) + ((u1 & 1) == par ? lu : 0.0f);
            const int u = (u1 & 1) == par ? u1 : u0;
            const int i = ((u + 1) >> 1) - (k >> 1);
            off[k] = (unsigned)i < (unsigned)a.ih ? i * a.iw_store * 128 : -1;
        }
        row_tab[2 * t] = make_uint4((unsigned)off[0], (unsigned)off[1], (unsigned)off[2], (unsigned)off[3]);
        row_tab[2 * t + 1] = make_uint4(__float_as_uint(w[0]), __float_as_uint(w[1]), __float_as_uint(w[2]), __float_as_uint(w[3]));
    }
    if (t < a.ow) {
        int v0, v1;
        float lv;
        bilinear_coord(t, (float)tw / (float)a.ow, tw, v0, v1, lv, a.nearest != 0);
        int off[4];
        float w[4];
        for (int k = 0; k < 4; ++k) {
            const int par = (k + 1) & 1;
            w[k] = ((v0 & 1) == par ? 1.0f - lv : 0.0f) + ((v1 & 1) == par ? lv : 0.0f);
            const int v = (v1 & 1) == par ? v1 : v0;
            const int j = ((v + 1) >> 1) - (k >> 1);
            int js = (unsigned)j < (unsigned)a.iw ? j : -1;
            if (js >= 0 && a.col_map) js = a.col_map[js];
            off[k] = js >= 0 ? js * 128 : -1;
        }
        col_tab[2 * t] = make_uint4((unsigned)off[0], (unsigned)off[1], (unsigned)off[2], (unsigned)off[3]);
        col_tab[2 * t + 1] = make_uint4(__float_as_uint(w[0]), __float_as_uint(w[1]), __float_as_uint(w[2]), __float_as_uint(w[3]));
    }
}

hipError_t launch_readout_tables(const ReadoutArgs& a, hipStream_t s) {
    const int n = a.oh > a.ow ? a.oh : a.ow;
    hipLaunchKernelGGL(readout_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, (uint4*)a.row_tab, (uint4*)a.col_tab);
    return hipGetLastError();
}

// The DMA form: the same arithmetic as readout_mfma_kernel with the tap coordinates from tables and the decoder tensor brought
// into LDS by `buffer_load ... lds`.  It has two bodies that compute the same words (tests/test_gpu_readout_rows.py); launch_readout
// notes the form readout_dma_kernel for both, and `+rows` / `+gather` beside it.
//   GATHER BODY (this kernel; DYF_READOUT_ROWS=0, and stored rows wider than the rows body's LDS plan): per output pixel, 16 taps x
//   128 B gathered into a per-wave staging area (lane i fetches piece (i & 3) ^ (pixel & 3) of pixel i >> 2 into slot i: the swizzle
//   keeps the fragment reads conflict-free; the MFMA lane (pixel p, k-group g) reads its operand back with ONE ds_read_b128 from slot
//   4p + (g ^ (p & 3))), one MFMA pair per tap whose 16 result rows hold <= 4 output channels.  Taps outside the image get the
//   out-of-range offset (DMA writes zeros).  8 KB of weight rows + 4 x 8 KB staging per workgroup, four workgroups per CU.  At the NS
//   geometry it gathers 19 MB per image from a 3.4 MB tensor and is bound by the LDS pipe serving 64 fragment reads per 16 pixels:
//   240 us per paired 160-row launch, 124 us per 80 rows.  A vertical-strip variant that gathered every input row segment once PER
//   OUTPUT PIXEL STRIP (284 us) still contracted per output pixel and tap.
//   ROWS BODY (readout_dma_rows_kernel below, the default): the contraction depends on the decoder pixel and the tap only, so every
//   decoder row is staged once per band of output rows and contracted once per pixel and kernel row (4 MFMA pairs per 16 decoder
//   pixels instead of 16 per 16 output pixels), and the 16 products of an output pixel are blended from LDS in the gather body's
//   order.  One coalesced pass over the tensor (plus the rows neighbouring bands share): 178 / 88 us for the same launches.
__global__ __launch_bounds__(256, 4) void readout_dma_kernel(ReadoutArgs a, int groups_per_wave) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char rd_smem[];
    // weights: [tap][half][k-group][row m < 4] x 16 B  (row m of the 16-row A fragment; rows >= cout are zero in wfrag)
    for (int i = threadIdx.x; i < 16 * 2 * 4 * 4; i += 256) {
        const int m = i & 3, kg = (i >> 2) & 3, th = i >> 4;
        ((uint4*)rd_smem)[i] = ((const uint4*)a.wfrag)[th * 64 + kg * 16 + m];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_id = (int)((blockIdx.x * 256 + threadIdx.x) >> 6);
    const int p = lane & 15, kg = lane >> 4;
    char* stage = rd_smem + 8192 + wave * 8192;  // [4 taps][2 halves][64 slots] x 16 B
    const uint4* wl = (const uint4*)rd_smem + kg * 4 + (p & 3);
    const bool wrow = p < 4;
    const int total = a.n * a.oh * a.ow;
    const int th = 2 * a.ih, tw = 2 * a.iw;
    const float sh = (float)th / (float)a.oh, sw = (float)tw / (float)a.ow;
    const int plane = a.oh * a.ow;
    const size_t xbytes = (size_t)a.n * a.ih * a.iw_store * 64 * sizeof(el16_t);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)(unsigned)xbytes, 0x00020000);
    const int lp = lane >> 2, lc = lane & 3;             // pixel / slot piece this lane FETCHES
    const unsigned piece_off = (unsigned)((lc ^ (lp & 3)) * 16);
    const int src4 = lp * 4;                             // ds_bpermute byte address of lane lp (holds pixel lp's coordinates)
    const unsigned rd_off = (unsigned)((p * 4 + (kg ^ (p & 3))) * 16);
    for (int g = 0; g < groups_per_wave; ++g) {
        const int idx0 = (wave_id * groups_per_wave + g) * 16;
        if (idx0 >= total) break;  // wave-uniform
        int idx = idx0 + p;
        const bool live = idx < total;
        if (!live) idx = total - 1;
        const int n = idx / plane;
        const int rem = idx - n * plane;
        const int oy = rem / a.ow, ox = rem - oy * a.ow;
        // tap tables (readout_tables_kernel): row offsets / weights of this output row, column offsets / weights of this column
        const uint4 rto = a.row_tab[2 * oy], rtw = a.row_tab[2 * oy + 1], cto = a.col_tab[2 * ox], ctw = a.col_tab[2 * ox + 1];
        const int nbase = n * a.ih * a.iw_store * 128;
        const int rto_[4] = {(int)rto.x, (int)rto.y, (int)rto.z, (int)rto.w};
        const int ro[4] = {rto_[0] >= 0 ? nbase + rto_[0] : -1, rto_[1] >= 0 ? nbase + rto_[1] : -1, rto_[2] >= 0 ? nbase + rto_[2] : -1,
                           rto_[3] >= 0 ? nbase + rto_[3] : -1};
        const int co_[4] = {(int)cto.x, (int)cto.y, (int)cto.z, (int)cto.w};
        const float rw[4] = {__uint_as_float(rtw.x), __uint_as_float(rtw.y), __uint_as_float(rtw.z), __uint_as_float(rtw.w)};
        const float cw[4] = {__uint_as_float(ctw.x), __uint_as_float(ctw.y), __uint_as_float(ctw.z), __uint_as_float(ctw.w)};
        int l_ro[4], l_co[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            l_ro[k] = __builtin_amdgcn_ds_bpermute(src4, ro[k]);
            l_co[k] = __builtin_amdgcn_ds_bpermute(src4, co_[k]);
        }
        float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        // 8 batches of 2 taps, two staging halves: the DMA of batch b + 1 is in flight while batch b is consumed (with one batch
        // of 4 taps at a time every group paid four exposed memory round trips -- the kernel's time was that latency chain)
        auto issue = [&](int bt) {
            const int kh = bt >> 1;
            char* st = stage + (bt & 1) * 4096;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kw = (bt & 1) * 2 + t;
                const bool ok = l_ro[kh] >= 0 && l_co[kw] >= 0;
                const unsigned vo = ok ? (unsigned)(l_ro[kh] + l_co[kw]) + piece_off : 0xFFFFFFFFu;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(st + (t * 2 + 0) * 1024), 16, vo, 0, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(st + (t * 2 + 1) * 1024), 16,
                                                         ok ? vo + 64u : 0xFFFFFFFFu, 0, 0, 0);
            }
        };
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the previous group's fragment reads are complete
        issue(0);
#pragma unroll
        for (int bt = 0; bt < 8; ++bt) {
            if (bt + 1 < 8) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // batch bt - 1 has been read out of the half that is refilled
                issue(bt + 1);
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");    // batch bt has landed
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            const int kh = bt >> 1;
            const char* st = stage + (bt & 1) * 4096;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kw = (bt & 1) * 2 + t, tap = kh * 4 + kw;
                const uint4 b0 = *(const uint4*)(st + (t * 2 + 0) * 1024 + rd_off);
                const uint4 b1 = *(const uint4*)(st + (t * 2 + 1) * 1024 + rd_off);
                uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
                if (wrow) {
                    w0 = wl[(tap * 2 + 0) * 16];
                    w1 = wl[(tap * 2 + 1) * 16];
                }
                ro_f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
                d = DYF_MFMA_16x16x32(__builtin_bit_cast(el16x8_t, w0), __builtin_bit_cast(el16x8_t, b0), d, 0, 0, 0);
                d = DYF_MFMA_16x16x32(__builtin_bit_cast(el16x8_t, w1), __builtin_bit_cast(el16x8_t, b1), d, 0, 0, 0);
                const float bw = (ro[kh] >= 0 && co_[kw] >= 0) ? rw[kh] * cw[kw] : 0.0f;  // this lane's own pixel
#pragma unroll
                for (int r = 0; r < 4; ++r) out[r] = fmaf(bw, d[r], out[r]);
            }
        }
        if (live && kg == 0) {
            float* o = a.out + ((size_t)n * a.cout * a.oh + oy) * a.ow + ox;
            const size_t cs = (size_t)a.oh * a.ow;
            o[0] = out[0] + a.bias[0];
            if (a.cout > 1) o[cs] = out[1] + a.bias[1];
            if (a.cout > 2) o[2 * cs] = out[2] + a.bias[2];
            if (a.cout > 3) o[3 * cs] = out[3] + a.bias[3];
        }
    }
#endif
}

// ROWS BODY of the readout_dma_kernel form: the same numbers, word for word, without the per-output-pixel gather.  The per-tap
// contraction d = MFMA(w_tap, x_pixel) of the gather body depends on the decoder pixel and the tap only, so here every decoder row
// is staged ONCE per band (whole rows by `buffer_load ... lds`, 1 KB tiles of 8 pixels, swizzled) and contracted ONCE per pixel: for
// kernel row kh the four kw taps are stacked into the 16 rows of one A fragment (row 4 kw + c), so one MFMA pair per 16 pixels
// leaves z[pixel p][kh][kw = kg][c = 0..3] in lane (p, kg) -- the same dot products by the same instruction over the same K order.
// Wave w contracts the 16-pixel groups w and w + 4 for all four kh (8 A fragments in registers): every fragment is read once.
// A workgroup owns one image x one band of `band` output rows (<= RR_MAXQ * 256 pixels, partial sums in registers) and streams the
// band's decoder rows in DESCENDING order: the input rows of kh = 0..3 of an output row never increase (tests/
// test_readout_rows_premise.py), so blending row by row, kh ascending inside a row, IS the gather body's tap order
// kh = 0..3, kw = 0..3.  A tap with valid offsets is blended whatever its weight; a tap at an invalid column is fmaf(0, 0, out) as in
// the gather body; invalid rows below the image (a suffix of kh) are one fmaf(0, 0, out) after the stream (it can only turn -0
// into +0, and repeating it changes nothing); invalid rows above it come first, when out is still +0.
// LDS: z [4 kh][4 kw][16 G columns] float4 = 4 G KB (G = 16-pixel groups of a stored row) + 3 staging buffers of 2 G tiles of
// 1 KB (one tile = one wave's DMA instruction; wave w issues tiles w, w + 4, ..): 28 + 42 = 70 KB at the NS compact width 104
// (G = 7), two workgroups per CU; rows k + 1 and k + 2 are in flight while row k is contracted and blended.  80 KB at most:
// stored rows of up to 128 columns (launch_readout sends wider ones to the gather body); readout_init raises the kernel's
// dynamic-LDS cap once per process.  The workgroups of a launch all do the same work and two are resident per CU, so the launch
// takes whole rounds of 512: launch_readout picks the band that minimises rounds x decoder rows per band (readout_rows_band).
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): 236 VGPRs + 12 AGPRs, no scratch, 70 KB of LDS at the NS width: two
// workgroups (8 waves) per CU.
#define RR_MAXQ 4
#define RR_NOCOL 0xFFFFFFFFu
#define RR_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// Every LDS access behind the first DMA is an asm statement that waits for itself: the compiler puts a vmcnt(0) in front of an LDS
// read it can see while an LDS-DMA is pending (it cannot tell the buffers apart), which would drain the row in flight.
typedef __attribute__((ext_vector_type(4))) unsigned ro_u32x4;
// both K halves of the fragments of two 16-pixel groups
__device__ __forceinline__ void rr_read_frags(unsigned a0, unsigned a1, unsigned b0, unsigned b1, ro_u32x4& x0, ro_u32x4& x1, ro_u32x4& y0, ro_u32x4& y1) {
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(x0), "=&v"(x1), "=&v"(y0), "=&v"(y1) : "v"(a0), "v"(a1), "v"(b0), "v"(b1) : "memory");
}
__device__ __forceinline__ void rr_read_z4(unsigned a0, unsigned a1, unsigned a2, unsigned a3, ro_f32x4& z0, ro_f32x4& z1, ro_f32x4& z2, ro_f32x4& z3) {
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(z0), "=&v"(z1), "=&v"(z2), "=&v"(z3) : "v"(a0), "v"(a1), "v"(a2), "v"(a3) : "memory");
}
__device__ __forceinline__ void rr_write_z(unsigned addr, ro_f32x4 d) { asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(d) : "memory"); }

__global__ __launch_bounds__(256) void readout_dma_rows_kernel(ReadoutArgs a, int band, int nbands, int G) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char rr_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 15, kg = lane >> 4;
    const int n = (int)blockIdx.x / nbands, oy0 = ((int)blockIdx.x - n * nbands) * band;
    const int rows_here = (a.oh - oy0 < band ? a.oh - oy0 : band);
    const int rowbytes = a.iw_store * 128, WC = G * 16;
    const unsigned z0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)rr_smem;  // LDS byte addresses
    const unsigned stage0 = z0 + (unsigned)(G * 4096);
    char* stage = rr_smem + G * 4096;
    const int stage_sz = G * 2048;
    const int tiles = (a.iw_store + 7) / 8;                            // 1 KB tiles of a stored row (<= 2 G)
    const int ntile = wave < tiles ? (tiles - wave + 3) / 4 : 0;     // DMA instructions of this wave per row (<= 4)
    // A fragments of kernel row kh: lane (m = 4 kw + c, kg) takes lane (c, kg) of tap (kh, kw)
    uint4 A[4][2];
#pragma unroll
    for (int kh = 0; kh < 4; ++kh)
#pragma unroll
        for (int h = 0; h < 2; ++h) A[kh][h] = ((const uint4*)a.wfrag)[((kh * 4 + (p >> 2)) * 2 + h) * 64 + kg * 16 + (p & 3)];
    // decoder rows of the band (byte offsets inside a sample, multiples of rowbytes): lane l looks at output row l (band <= 64)
    int rhi = -1, rlo = 0x7FFFFFFF;
    if (lane < rows_here) {
        const uint4 o = a.row_tab[2 * (oy0 + lane)];
        const int ov[4] = {(int)o.x, (int)o.y, (int)o.z, (int)o.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ov[k] >= 0) {
                rhi = ov[k] > rhi ? ov[k] : rhi;
                rlo = ov[k] < rlo ? ov[k] : rlo;
            }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int h2 = __shfl_xor(rhi, off, 64), l2 = __shfl_xor(rlo, off, 64);
        rhi = h2 > rhi ? h2 : rhi;
        rlo = l2 < rlo ? l2 : rlo;
    }
    rhi = __builtin_amdgcn_readfirstlane(rhi);
    rlo = __builtin_amdgcn_readfirstlane(rlo);
    // this thread's output pixels: pixel tid + 256 q of the band, row-major
    int ro[RR_MAXQ][4];
    unsigned zc[RR_MAXQ][4];  // byte offset of the stored column inside a z line, or RR_NOCOL
    float rw[RR_MAXQ][4], cw[RR_MAXQ][4], out[RR_MAXQ][4];
    const int npix = rows_here * a.ow;
#pragma unroll
    for (int q = 0; q < RR_MAXQ; ++q) {
        const int pix = tid + 256 * q;
        const bool ok = pix < npix;
        const int oyl = ok ? pix / a.ow : 0, ox = ok ? pix - oyl * a.ow : 0;
        const uint4 rto = a.row_tab[2 * (oy0 + oyl)], rtw = a.row_tab[2 * (oy0 + oyl) + 1];
        const uint4 cto = a.col_tab[2 * ox], ctw = a.col_tab[2 * ox + 1];
        ro[q][0] = ok ? (int)rto.x : -2; ro[q][1] = ok ? (int)rto.y : -2; ro[q][2] = ok ? (int)rto.z : -2; ro[q][3] = ok ? (int)rto.w : -2;
        zc[q][0] = (int)cto.x >= 0 ? cto.x >> 3 : RR_NOCOL; zc[q][1] = (int)cto.y >= 0 ? cto.y >> 3 : RR_NOCOL;  // (js * 128 -> js * 16)
        zc[q][2] = (int)cto.z >= 0 ? cto.z >> 3 : RR_NOCOL; zc[q][3] = (int)cto.w >= 0 ? cto.w >> 3 : RR_NOCOL;
        rw[q][0] = __uint_as_float(rtw.x); rw[q][1] = __uint_as_float(rtw.y); rw[q][2] = __uint_as_float(rtw.z); rw[q][3] = __uint_as_float(rtw.w);
        cw[q][0] = __uint_as_float(ctw.x); cw[q][1] = __uint_as_float(ctw.y); cw[q][2] = __uint_as_float(ctw.z); cw[q][3] = __uint_as_float(ctw.w);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[q][c] = 0.0f;
    }
    const size_t xbytes = (size_t)a.n * a.ih * a.iw_store * 64 * sizeof(el16_t);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)(unsigned)xbytes, 0x00020000);
    const unsigned nbase = (unsigned)n * (unsigned)a.ih * (unsigned)rowbytes;
    // staging image: a tile is 8 whole pixels (1 KB, contiguous in x: one DMA instruction reads full 128-B lines), pixel pl's piece c
    // (16 B, c = 4 half + kg) in slot 8 pl + (c ^ pl) -- the 16 lanes a ds_read_b128 serves together then fall on 16 different slots
    const int lp = lane >> 3;                 // pixel of its tile this lane FETCHES
    const unsigned piece_off = (unsigned)(((lane & 7) ^ lp) * 16);
    const unsigned rd_base = (unsigned)((p >> 3) * 1024 + (p & 7) * 128);
    const unsigned rd_off0 = rd_base + (unsigned)((kg ^ (p & 7)) * 16), rd_off1 = rd_base + (unsigned)(((4 + kg) ^ (p & 7)) * 16);
    const unsigned zw = z0 + (unsigned)((kg * WC + p) * 16);  // this lane's D of group 0, kh = 0: z[0][kw = kg][p]
    // row at byte offset rb (rb < rlo: none, every lane out of range: the waits below count ntile instructions per row) -> buffer b:
    // tile wave + 4 t; pad pixels of a ragged last tile get the out-of-range offset (DMA writes zeros); the pad tiles of a ragged
    // last group are never written -- the z columns contracted from them are never blended
    auto issue = [&](int rb, int b) {
        for (int t = 0; t < ntile; ++t) {
            const int tile = wave + 4 * t, px = tile * 8 + lp;
            const bool ok = rb >= rlo && px < a.iw_store;
            const unsigned vo = ok ? nbase + (unsigned)rb + (unsigned)(px * 128) + piece_off : 0xFFFFFFFFu;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(stage + b * stage_sz + tile * 1024), 16, vo, 0, 0, 0);
        }
    };
    if (rhi >= 0) {
        issue(rhi, 0);
        issue(rhi - rowbytes, 1);
        int b = 0;
        for (int rb = rhi; rb >= rlo; rb -= rowbytes) {
            // row rb has landed (this wave's pieces; the barrier makes that every wave's): only the instructions of the next row may be out
            switch (ntile) {
                case 0: break;
                case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
                case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
                case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
                default: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            }
            RR_BARRIER();  // ... and every wave is done with z (blend of the previous row) and with the buffer refilled next
            issue(rb - 2 * rowbytes, b == 0 ? 2 : b - 1);
            if (wave < G) {
                const bool two = wave + 4 < G;  // (no second group: its reads repeat the first)
                const unsigned st = stage0 + (unsigned)(b * stage_sz + wave * 2048), st2 = st + (two ? 4 * 2048u : 0u);
                ro_u32x4 x0, x1, y0, y1;
                rr_read_frags(st + rd_off0, st + rd_off1, st2 + rd_off0, st2 + rd_off1, x0, x1, y0, y1);
#pragma unroll
                for (int kh = 0; kh < 4; ++kh) {
                    ro_f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
                    d = DYF_MFMA_16x16x32(__builtin_bit_cast(el16x8_t, A[kh][0]), __builtin_bit_cast(el16x8_t, x0), d, 0, 0, 0);
                    d = DYF_MFMA_16x16x32(__builtin_bit_cast(el16x8_t, A[kh][1]), __builtin_bit_cast(el16x8_t, x1), d, 0, 0, 0);
                    rr_write_z(zw + (unsigned)(kh * 4 * WC * 16 + wave * 256), d);
                }
                if (two) {
#pragma unroll
                    for (int kh = 0; kh < 4; ++kh) {
                        ro_f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
                        d = DYF_MFMA_16x16x32(__builtin_bit_cast(el16x8_t, A[kh][0]), __builtin_bit_cast(el16x8_t, y0), d, 0, 0, 0);
                        d = DYF_MFMA_16x16x32(__builtin_bit_cast(el16x8_t, A[kh][1]), __builtin_bit_cast(el16x8_t, y1), d, 0, 0, 0);
                        rr_write_z(zw + (unsigned)(kh * 4 * WC * 16 + (wave + 4) * 256), d);
                    }
                }
            }
            RR_BARRIER();
#pragma unroll
            for (int q = 0; q < RR_MAXQ; ++q)
#pragma unroll
                for (int kh = 0; kh < 4; ++kh)
                    if (ro[q][kh] == rb) {
                        ro_f32x4 zv[4];
                        const unsigned zr = z0 + (unsigned)(kh * 4 * WC * 16);
                        rr_read_z4(zr + (zc[q][0] != RR_NOCOL ? zc[q][0] : 0u), zr + (unsigned)(WC * 16) + (zc[q][1] != RR_NOCOL ? zc[q][1] : 0u),
                                   zr + (unsigned)(2 * WC * 16) + (zc[q][2] != RR_NOCOL ? zc[q][2] : 0u),
                                   zr + (unsigned)(3 * WC * 16) + (zc[q][3] != RR_NOCOL ? zc[q][3] : 0u), zv[0], zv[1], zv[2], zv[3]);
#pragma unroll
                        for (int kw = 0; kw < 4; ++kw) {
                            const bool ok = zc[q][kw] != RR_NOCOL;  // an invalid column: fmaf(0, 0, out), as in the gather body
                            const float bw = ok ? rw[q][kh] * cw[q][kw] : 0.0f;
#pragma unroll
                            for (int c = 0; c < 4; ++c) out[q][c] = fmaf(bw, ok ? zv[kw][c] : 0.0f, out[q][c]);
                        }
                    }
            b = b == 2 ? 0 : b + 1;
        }
    }
    const size_t cs = (size_t)a.oh * a.ow;
#pragma unroll
    for (int q = 0; q < RR_MAXQ; ++q) {
        const int pix = tid + 256 * q;
        if (pix < npix) {
            if (ro[q][3] == -1) {  // kernel rows below the image: the gather body's fmaf(0, 0, out)
#pragma unroll
                for (int c = 0; c < 4; ++c) out[q][c] = fmaf(0.0f, 0.0f, out[q][c]);
            }
            float* o = a.out + ((size_t)n * a.cout * a.oh + oy0) * a.ow + pix;
            o[0] = out[q][0] + a.bias[0];
            if (a.cout > 1) o[cs] = out[q][1] + a.bias[1];
            if (a.cout > 2) o[2 * cs] = out[q][2] + a.bias[2];
            if (a.cout > 3) o[3 * cs] = out[q][3] + a.bias[3];
        }
    }
#endif
}

// LDS plan of the rows body for stored rows of iw_store columns: bytes and G (16-pixel groups)
static size_t readout_rows_lds(int iw_store, int* G) {
    *G = (iw_store + 15) / 16;
    return (size_t)*G * 4096 + (size_t)3 * *G * 2048;
}
// Output rows per workgroup: at most RR_MAXQ * 256 pixels and 64 rows, at least 8 (or oh); among those the band with the least
// rounds (of 2 workgroups on each of 256 CUs) x decoder rows streamed per band (band * ih / oh and the rows its ends share with
// the neighbours) -- 19 rows (12 bands) for the 80-image NS launch, 14 (16 bands) for the paired one
static int readout_rows_band(const ReadoutArgs& a) {
    int cap = RR_MAXQ * 256 / a.ow;
    cap = cap > 64 ? 64 : cap;
    cap = cap > a.oh ? a.oh : cap;
    int best = cap;
    double best_cost = 0.0;
    for (int band = cap; band >= (cap < 8 ? cap : 8); --band) {
        const long long wgs = (long long)a.n * ((a.oh + band - 1) / band);
        const double cost = (double)((wgs + 511) / 512) * ((double)band * a.ih / a.oh + 3.0);
        if (band == cap || cost < best_cost) {
            best = band;
            best_cost = cost;
        }
    }
    return best;
}
#define RR_LDS_MAX (80 * 1024)

// Raise the dynamic-LDS cap of the rows body once per process (not legal inside a stream capture).
hipError_t readout_init() {
    return hipFuncSetAttribute((const void*)readout_dma_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RR_LDS_MAX);
}

hipError_t launch_readout(const ReadoutArgs& a, hipStream_t s) {
    const long long total = (long long)a.n * a.oh * a.ow;
    const bool regw = dyf_form_int("DYF_READOUT_REGW", 1) != 0;
    const bool use_mfma = dyf_form_int("DYF_READOUT_MFMA", 1) != 0;
    if (a.col_map && !(a.wfrag && a.cin == 64 && a.cout >= 1 && a.cout <= 4)) return hipErrorInvalidValue;
    if ((use_mfma || a.col_map) && a.wfrag && a.cin == 64 && a.cout >= 1 && a.cout <= 4 && total < (1ll << 30)) {
        const long long groups = (total + 15) / 16;
        long long waves = 256ll * 16;  // 4 waves per SIMD
        int per = (int)((groups + waves - 1) / waves);
        if (per < 1) per = 1;
        waves = (groups + per - 1) / per;
        // DMA-staged gather (DYF_READOUT_DMA=0: the register-shuffle form); the DMA's buffer descriptor addresses < 4 GB
        const bool use_dma = dyf_form_int("DYF_READOUT_DMA", 1) != 0;
        const bool dma = use_dma && a.row_tab && a.col_tab && (size_t)a.n * a.ih * a.iw_store * 128 < 0x7F000000ull;
        dyf_form_note(dma ? "readout_dma_kernel" : "readout_mfma_kernel", a.n);
        KernelProf kp(dma ? "readout_dma_kernel" : "readout_mfma_kernel", s,
                      (double)a.n * a.ih * a.iw_store * a.cin * 2.0 + (double)a.n * a.cout * a.oh * a.ow * 4.0);
        // rows body (DYF_READOUT_ROWS=0: the gather body) wherever its LDS plan fits; decided from `a` alone
        int G = 0;
        const size_t rows_lds = readout_rows_lds(a.iw_store, &G);
        const bool rows = dma && dyf_form_int("DYF_READOUT_ROWS", 1) != 0 && rows_lds <= RR_LDS_MAX && a.ow <= RR_MAXQ * 256;
        if (dma) dyf_form_note(rows ? "readout_dma_kernel+rows" : "readout_dma_kernel+gather", a.n);
        if (rows) {
            const int band = readout_rows_band(a), nbands = (a.oh + band - 1) / band;
            hipLaunchKernelGGL(readout_dma_rows_kernel, dim3((unsigned)(a.n * nbands)), dim3(256), rows_lds, s, a, band, nbands, G);
        } else if (dma)
            hipLaunchKernelGGL(readout_dma_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 8192 + 4 * 8192, s, a, per);
        else
            hipLaunchKernelGGL(readout_mfma_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 32768, s, a, per);
        return hipGetLastError();
    }
    if (regw && a.cin == 64 && a.cout >= 1 && a.cout <= 4 && total < (1ll << 30)) {
        // ~16 waves per CU; a half-wave owns a contiguous run of pixels
        int halves = 256 * 16 * 2;
        int per = (int)((total + halves - 1) / halves);
        if (per < 8) per = 8;
        per += per & 1;  // the kernel walks two pixels per iteration
        halves = (int)((total + per - 1) / per);
        const unsigned blocks = (unsigned)((halves + 7) / 8);
#define RW_CASE(C)                                                                                      \
        if (a.cout == C) {                                                                              \
            dyf_form_note("readout_regw_kernel<" #C ">", a.n);                                          \
            hipLaunchKernelGGL(readout_regw_kernel<C>, dim3(blocks), dim3(256), 0, s, a, per);          \
            return hipGetLastError();                                                                   \
        }
        RW_CASE(1) RW_CASE(2) RW_CASE(3) RW_CASE(4)
#undef RW_CASE
    }
    const size_t lds = (size_t)16 * a.cin * a.cout * sizeof(float);
    const int lanes = (a.cin % 8 == 0) ? a.cin / 8 : 0;
#define RO_CASE(L)                                                                                                   \
    if (lanes == L) {                                                                                                \
        dyf_form_note("readout_sliced_kernel<" #L ">", a.n);                                                         \
        hipLaunchKernelGGL(readout_sliced_kernel<L>, dim3((unsigned)((total * L + 255) / 256)), dim3(256), lds, s, a); \
        return hipGetLastError();                                                                                    \
    }
    RO_CASE(1) RO_CASE(2) RO_CASE(4) RO_CASE(8) RO_CASE(16)
#undef RO_CASE
    dyf_form_note("readout_kernel", a.n);
    hipLaunchKernelGGL(readout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), lds, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ K10 sampler
// dyffusion.py:388  x_s = x_s - I(s) + I(s_next), kept in fp32 (SURVEY hard-part (f))
// copy: second destination of the new x_s (the forecast-stack slot of a step that emits a prediction; saves the copy node), or null
__global__ void cold_update_kernel(float* x_s, const float* x_cur, const float* x_next, long long count, float* copy) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const float v = x_s[i] - x_cur[i] + x_next[i];
        x_s[i] = v;
        if (copy) copy[i] = v;
    }
}

hipError_t launch_cold_update(float* x_s, const float* x_cur, const float* x_next, long long count, hipStream_t s, float* copy) {
    hipLaunchKernelGGL(cold_update_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, x_s, x_cur, x_next,
                       count, copy);
    return hipGetLastError();
}

// dyffusion.py:219-227  forward_cond = tfactor*condition + (1-tfactor)*randn_like(condition)
// Engine draws (noise == nullptr): Box-Muller on two hashed words per element; the stream is keyed by (seed, noise-call
// counter rng_state[4], GLOBAL batch row rng_state[3] + n) and the element index inside the row, like the dropout masks.
__global__ void noisy_condition_kernel(float* out, const float* cond, const float* noise, float tau, long long count,
                                       int row_elems, const uint32_t* rng_state) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float z;
    if (noise != nullptr) {
        z = noise[i];
    } else {
        const uint32_t n = (uint32_t)(i / row_elems), e = (uint32_t)(i - (long long)n * row_elems);
        const RngKey rk = rng_row_key(rng_state[0], rng_state[1] ^ 0x4E6F6973u, rng_state[4], rng_state[3] + n);
        const uint32_t w0 = fmix32(e * 0x9E3779B1u + rk.k0), w1 = fmix32(w0 ^ rk.k1);
        const float u1 = ((float)(w0 >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u2 = ((float)(w1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
        z = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
    }
    out[i] = tau * cond[i] + (1.0f - tau) * z;
}

__global__ void rng_bump_kernel(uint32_t* state, int slot, uint32_t by) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[slot] += by;
}

// row groups (engine.hip): a child engine's stream position = the parent's, its batch row 0 = the parent's row 0 + row_add;
// counters_only: the parent adopts the counters a child advanced (words 2 and 4)
__global__ void rng_clone_kernel(uint32_t* dst, const uint32_t* src, uint32_t row_add, int counters_only) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (counters_only) {
        dst[2] = src[2];
        dst[4] = src[4];
        return;
    }
    for (int i = 0; i < DYF_RNG_STATE_WORDS; ++i) dst[i] = src[i];
    dst[3] = src[3] + row_add;
}

hipError_t launch_rng_clone(uint32_t* dst, const uint32_t* src, uint32_t row_add, bool counters_only, hipStream_t s) {
    hipLaunchKernelGGL(rng_clone_kernel, dim3(1), dim3(64), 0, s, dst, src, row_add, counters_only ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_noisy_condition(float* out, const float* cond, const float* noise, float tau, long long count,
                                  int row_elems, uint32_t* rng_state, hipStream_t s) {
    hipLaunchKernelGGL(noisy_condition_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, out, cond, noise,
                       tau, count, row_elems, rng_state);
    if (noise == nullptr)  // every call draws a fresh field (dyffusion.py:227 randn_like), also on graph replay
        hipLaunchKernelGGL(rng_bump_kernel, dim3(1), dim3(64), 0, s, rng_state, 4, 1u);
    return hipGetLastError();
}

// Start of a forward that draws dropout masks: fill the row-key table of the launch and advance the forward counter.
// Launch row r belongs to forward (counter + r / rows_per_fwd) and global batch row (row offset + r % rows_per_fwd): a
// paired interpolator launch (2 nb rows = two forwards of nb rows) draws exactly the masks of two separate forwards.
__global__ __launch_bounds__(256) void rng_begin_forward_kernel(uint32_t* state, uint32_t* row_keys, int rows, int rows_per_fwd) {
    const uint32_t lo = state[0], hi = state[1], fwd0 = state[2], row0 = state[3];
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const RngKey k = rng_row_key(lo, hi, fwd0 + (uint32_t)(r / rows_per_fwd), row0 + (uint32_t)(r % rows_per_fwd));
        row_keys[2 * r] = k.k0;
        row_keys[2 * r + 1] = k.k1;
    }
    __syncthreads();
    if (threadIdx.x == 0) state[2] = fwd0 + (uint32_t)((rows + rows_per_fwd - 1) / rows_per_fwd);
}

hipError_t launch_rng_begin_forward(uint32_t* rng_state, uint32_t* row_keys, int rows, int rows_per_fwd, hipStream_t s) {
    hipLaunchKernelGGL(rng_begin_forward_kernel, dim3(1), dim3(256), 0, s, rng_state, row_keys, rows, rows_per_fwd);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ boundary conditions
// PhysicalSystemsBenchmarkDataModule.boundary_conditions (src/datamodules/physical_systems_benchmark.py:245-297), applied by
// _evaluation_step to every predicted field (forecasting_multi_horizon.py:175-182): ONE masked write over the whole
// (fields, rows, C, H, W) stack instead of a Python loop over batch elements with boolean-mask index_put_ calls.
//   navier-stokes: preds[fixed_mask] = 0, then channel 0 / first grid row = parabolic inflow
//                  in_velocity * 4 * y * (0.41 - y) / 0.41^2 * (1 - exp(-5 t)), evaluated in fp32 in the reference's order
//   spring-mesh:   preds = where(fixed_mask, boundary, preds), boundary = cat[0 (p), q of the first time step]
// row_meta[row] is the batch element whose metadata applies to the row, -1 = row untouched (the reference's indexing of
// ensemble stacks is resolved on the host, dyffusion_amd/boundary.py).
__global__ void boundary_conditions_kernel(BcArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int chw = a.c * a.h * a.w;
    const long long total = (long long)a.n_fields * a.rows * chw;
    if (i >= total) return;
    const int e = (int)(i % chw);
    const int row = (int)((i / chw) % a.rows), f = (int)(i / ((long long)chw * a.rows));
    const int b = a.row_meta[row];
    if (b < 0) return;
    const bool fixed = a.fixed_mask[(size_t)b * chw + e] != 0;
    if (a.kind == 0) {
        if (e < a.w) {  // channel 0, grid row 0: left_boundary_indexing[0, 0, :]
            const float growth = a.time_factor[a.times_per_meta ? f * a.n_meta + b : f];  // (float)(1 - exp(-5 t)), host double math
            const float vy = a.vertex_y[(size_t)b * a.w + e];
            const float s0 = (float)((double)a.in_velocity[b] * 4.0);           // python float product, cast by the tensor op
            float v = s0 * vy;
            v = v * (0.41f - vy);
            v = v / (float)(0.41 * 0.41);
            a.preds[i] = v * growth;
        } else if (fixed) {
            a.preds[i] = 0.0f;
        }
    } else if (fixed) {
        a.preds[i] = a.boundary[(size_t)b * chw + e];
    }
}

hipError_t launch_boundary_conditions(const BcArgs& a, hipStream_t s) {
    const long long total = (long long)a.n_fields * a.rows * a.c * a.h * a.w;
    hipLaunchKernelGGL(boundary_conditions_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// test seam (dyf_debug_read_block_output): NHWC bf16 activation -> NCHW fp32; col_map (or null) maps a dense column to its
// column in a compact tensor of width w_store, -1 = not stored (NaN)
__global__ void nhwc_to_nchw_f32_kernel(const el16_t* src, int n, int h, int w, int w_store, int c, const int16_t* col_map,
                                        float* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)n * c * h * w;
    if (i >= total) return;
    const int x = (int)(i % w), y = (int)((i / w) % h), ch = (int)((i / ((long long)w * h)) % c), b = (int)(i / ((long long)w * h * c));
    const int xs = col_map ? col_map[x] : x;
    out[i] = xs < 0 ? __uint_as_float(0x7fc00000u) : el16_to_f32(src[(((size_t)b * h + y) * w_store + xs) * c + ch]);
}

hipError_t launch_nhwc_to_nchw_f32(const el16_t* src, int n, int h, int w, int w_store, int c, const int16_t* col_map,
                                   float* out, hipStream_t s) {
    const long long total = (long long)n * c * h * w;
    hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, n, h, w, w_store, c,
                       col_map, out);
    return hipGetLastError();
}

__global__ void fill_f32_kernel(float* p, float v, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = v;
}

hipError_t launch_fill_f32(float* p, float v, long long count, hipStream_t s) {
    hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, p, v, count);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ ensemble metrics
// On-device form of src/utilities/evaluation.py:10-118 (evaluate_ensemble_prediction).  Three entries reduce the N members x_n of a
// grid point with target y to the same four fp32 values, through the two helpers below:
//   mean = (sum_n x_n) / N
//   se   = (mean - y)^2                                 -> "mse" of the ensemble mean           (evaluation.py:43-45)
//   var  = (sum_n (x_n - mean)^2) / N  (population)     -> spread^2 of the spread-skill ratio   (evaluation.py:107-116)
//   crps = mean_n |x_n - y| - 1/(2 N^2) sum_{n,m} |x_n - x_m|  -> CRPS of the empirical ensemble CDF (xskillscore/properscoring
//          crps_ensemble, evaluation.py:83-95); `pair` below is the sum over n < m, half the sum over ordered pairs
// and differ in what they do with them: dyf_ensemble_metrics (this section) sums over all points with fp64 atomics,
// dyf_trajectory_metrics per segment and dyf_ensemble_scores per (segment, group) in a fixed order.  HBM-bound: every prediction is
// read exactly once (members staged in LDS); the O(N^2) pair term runs out of LDS.
//   Contraction is written out, not left to the compiler, so that the three entries hold the same bits for the same point whatever
// surrounds the helper (tests/test_gpu_ensemble_scores.py::test_pooled compares two of them bitwise): with 1 / N = inv,
//   both forms    m2 = fmaf(x - mean, x - mean, m2);  mean = sum * inv;  se = (mean - y) * (mean - y);  var = m2 * inv
//   one thread    crps = fmaf(sabs, inv, -(pair * inv * inv))
//   tiled         crps = sabs * inv - pair * inv * inv   (two rounded products, one subtraction)
// and nothing else is fused.
struct ensemble_point {
    float mean, y, se, var, crps;
};

// Up to 64 members, one thread per point: `preds` is the point's first member, member n lies n * member_stride behind it.  The
// members are staged as xs[n * 256 + tid]; a thread reads only what it wrote, so there is no barrier.
__device__ __forceinline__ ensemble_point ensemble_point_reduce(const float* preds, long long member_stride, float y, int n_members,
                                                                float* xs /* LDS, [n_members][256] */) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    float sum = 0.0f, sabs = 0.0f;
    for (int n = 0; n < n_members; ++n) {
        const float x = preds[(long long)n * member_stride];
        xs[n * 256 + tid] = x;
        sum += x;
        sabs += fabsf(x - y);
    }
    const float inv = 1.0f / (float)n_members;
    const float mean = sum * inv;
    float m2 = 0.0f, pair = 0.0f;
    for (int n = 0; n < n_members; ++n) {
        const float x = xs[n * 256 + tid];
        m2 = fmaf(x - mean, x - mean, m2);
        for (int m = n + 1; m < n_members; ++m) pair += fabsf(x - xs[m * 256 + tid]);
    }
    return {mean, y, (mean - y) * (mean - y), m2 * inv, fmaf(sabs, inv, -(pair * inv * inv))};
}

// More than 64 members (the reference has no cap, evaluation.py:10-80): the [N][256] staging tile no longer fits the 64 KB of LDS,
// so a workgroup takes P = ensemble_tile_points() < 256 points (N * P floats staged) and T = 256 / P threads share a point: thread
// (point pi = tid % P, share sh = tid / P) owns the members n = sh, sh + T, ...; the shares' partial sums meet in LDS and are added
// in share order.  The O(N^2) pair term is then spread over all 256 threads.  `preds` / `targets` are the tile's first point, of which
// the first n_live (1..P) exist.  EVERY thread of the workgroup calls this (it holds barriers); `holds` is set for share 0 of a live
// point, whose se / var / crps are the point's -- every other thread gets zeros there (mean and y are the point's in all its shares).
__device__ __forceinline__ ensemble_point ensemble_point_reduce_tiled(const float* preds, long long member_stride, int n_live,
                                                                      const float* targets, int n_members, int P,
                                                                      float* xs /* LDS, [n_members][P] */,
                                                                      float* red /* LDS, [2][256] */, bool& holds) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, T = 256 / P;
    const int pi = tid % P, sh = tid / P;
    const bool live = pi < n_live;
    for (int i = tid; i < n_members * P; i += 256) {  // staging: consecutive threads -> consecutive points of one member
        const int n = i / P, q = i - n * P;
        xs[i] = q < n_live ? preds[(long long)n * member_stride + q] : 0.0f;
    }
    __syncthreads();
    const float y = live ? targets[pi] : 0.0f;
    float sum = 0.0f, sabs = 0.0f;
    for (int n = sh; n < n_members; n += T) {
        const float x = xs[n * P + pi];
        sum += x;
        sabs += fabsf(x - y);
    }
    red[tid] = sum;
    red[256 + tid] = sabs;
    __syncthreads();
    float tsum = 0.0f, tabs = 0.0f;
    for (int k = 0; k < T; ++k) {  // every share adds the T partials in the same order: all hold the same mean
        tsum += red[k * P + pi];
        tabs += red[256 + k * P + pi];
    }
    const float inv = 1.0f / (float)n_members;
    const float mean = tsum * inv;
    __syncthreads();
    float m2 = 0.0f;
    double pair = 0.0;  // up to N^2 / 2 terms per point: rows in fp32, the sum of rows in fp64
    for (int n = sh; n < n_members; n += T) {
        const float x = xs[n * P + pi];
        m2 = fmaf(x - mean, x - mean, m2);
        float row = 0.0f;
        for (int m = n + 1; m < n_members; ++m) row += fabsf(x - xs[m * P + pi]);
        pair += (double)row;
    }
    red[tid] = m2;
    red[256 + tid] = (float)pair;
    __syncthreads();
    ensemble_point pt = {mean, y, 0.0f, 0.0f, 0.0f};
    holds = live && sh == 0;
    if (holds) {
        float tm2 = 0.0f, tpair = 0.0f;
        for (int k = 0; k < T; ++k) {
            tm2 += red[k * P + pi];
            tpair += red[256 + k * P + pi];
        }
        pt.se = (mean - y) * (mean - y);
        pt.var = tm2 * inv;
        pt.crps = tabs * inv - tpair * inv * inv;
    }
    return pt;
}

// The workgroup's sums of K values per thread, in fp64 and a fixed order: a wave butterfly, then the four wave sums meet in LDS
// (ensemble_wave_sums) and ensemble_block_total adds those of value k in wave order.
template <int K>
__device__ __forceinline__ void ensemble_wave_sums(double (&v)[K], double* wsum /* LDS, [4][K] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], off, 64);
    }
    const int tid = threadIdx.x;
    __syncthreads();  // wsum lies over the staged members (and over the sums of the round before): every wave is done reading them
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) wsum[(tid >> 6) * K + k] = v[k];
    }
    __syncthreads();
}
template <int K>
__device__ __forceinline__ double ensemble_block_total(const double* wsum, int k) {
    return ((wsum[k] + wsum[K + k]) + wsum[2 * K + k]) + wsum[3 * K + k];
}

// dyf_ensemble_metrics: one segment, flat points, member stride n_points; {se, var, crps} summed over all points in fp64: a wave
// butterfly, the wave's three sums to partials[blockIdx.x * 4 + wave][3], and ensemble_metrics_finish_kernel adds the waves' sums in a
// fixed order.  No atomics: two evaluations of the same fields give the same bits (the epochs' tests compare them bit for bit; with
// one unordered atomic per wave that held only while the waves happened to arrive in the same order).
__device__ __forceinline__ void ensemble_wave_partial(const ensemble_point& pt, double* partials) {
    double d0 = pt.se, d1 = pt.var, d2 = pt.crps;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        d0 += __shfl_xor(d0, off, 64);
        d1 += __shfl_xor(d1, off, 64);
        d2 += __shfl_xor(d2, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        double* w = partials + ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 3;
        w[0] = d0, w[1] = d1, w[2] = d2;
    }
}

// One workgroup: thread t adds the wave sums t, t + 256, ... in order, then thread k < 3 adds the 256 thread sums of quantity k in
// thread order.
__global__ __launch_bounds__(256) void ensemble_metrics_finish_kernel(const double* partials, long long n_waves, double* sums) {
    __shared__ double part[3][256];
    double a[3] = {0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < n_waves; i += 256) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] += partials[i * 3 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) part[k][threadIdx.x] = a[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int t = 0; t < 256; ++t) s += part[threadIdx.x][t];
        sums[threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void ensemble_metrics_kernel(const float* preds, const float* targets, int n_members,
                                                               long long n_points, double* partials) {
    extern __shared__ float xs[];  // [n_members][256]
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    ensemble_point pt = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (p < n_points) pt = ensemble_point_reduce(preds + p, n_points, targets[p], n_members, xs);
    ensemble_wave_partial(pt, partials);
}

__global__ __launch_bounds__(256) void ensemble_metrics_tiled_kernel(const float* preds, const float* targets, int n_members,
                                                                     long long n_points, double* partials, int P) {
    extern __shared__ float xs[];  // [n_members][P] members, then [2][256] partials
    const long long p0 = (long long)blockIdx.x * P;
    const int n_live = n_points - p0 < P ? (int)(n_points - p0) : P;
    bool holds;
    ensemble_wave_partial(ensemble_point_reduce_tiled(preds + p0, n_points, n_live, targets + p0, n_members, P, xs,
                                                      xs + (size_t)n_members * P, holds), partials);
}

// Reduction of the training criterion (src/utilities/utils.py:201-212, reduction = "mean"): sum over all elements of
// |p - t| (kind 0), (p - t)^2 (kind 1) or smooth-L1 with beta = 1 (kind 2); fp32 per lane, wave butterfly, one fp64 atomic
// per wave.  HBM-bound: both tensors are read once with 16-byte loads.
__global__ __launch_bounds__(256) void criterion_sum_kernel(const float* p, const float* t, long long count, int kind, double* sum) {
    const long long n4 = count >> 2;
    float acc = 0.0f;
    auto term = [&](float d) {
        const float ad = fabsf(d);
        return kind == 0 ? ad : kind == 1 ? d * d : (ad < 1.0f ? 0.5f * d * d : ad - 0.5f);
    };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 a = ((const float4*)p)[i], b = ((const float4*)t)[i];
        acc += term(a.x - b.x) + term(a.y - b.y) + term(a.z - b.z) + term(a.w - b.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) acc += term(p[n4 * 4 + threadIdx.x] - t[n4 * 4 + threadIdx.x]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(sum, (double)acc);
}

hipError_t launch_criterion_sum(const float* p, const float* t, long long count, int kind, double* sum, hipStream_t s) {
    hipError_t e = hipMemsetAsync(sum, 0, sizeof(double), s);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((count / 4 + 1023) / 1024, 2048));
    dyf_form_note("criterion_sum_kernel:atomic", 0);
    hipLaunchKernelGGL(criterion_sum_kernel, dim3(grid), dim3(256), 0, s, p, t, count, kind, sum);
    return hipGetLastError();
}

// The same terms without atomics: the four wave sums of a workgroup meet in LDS and leave, added in wave order, as partials[blockIdx.x];
// criterion_finish_kernel (one wave) adds the partials: lane l takes l, l + 64, ... in order, then the lanes' sums in lane order.
__global__ __launch_bounds__(256) void criterion_partial_kernel(const float* p, const float* t, long long count, int kind, double* partials) {
    __shared__ float wsum[4];
    const long long n4 = count >> 2;
    float acc = 0.0f;
    auto term = [&](float d) {
        const float ad = fabsf(d);
        return kind == 0 ? ad : kind == 1 ? d * d : (ad < 1.0f ? 0.5f * d * d : ad - 0.5f);
    };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 a = ((const float4*)p)[i], b = ((const float4*)t)[i];
        acc += term(a.x - b.x) + term(a.y - b.y) + term(a.z - b.z) + term(a.w - b.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) acc += term(p[n4 * 4 + threadIdx.x] - t[n4 * 4 + threadIdx.x]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (double)wsum[0] + (double)wsum[1] + (double)wsum[2] + (double)wsum[3];
}
__global__ __launch_bounds__(64) void criterion_finish_kernel(const double* partials, int n, double* sum) {
    __shared__ double lane_sum[64];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) a += partials[i];
    lane_sum[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int l = 0; l < 64; ++l) s += lane_sum[l];
        *sum = s;
    }
}

hipError_t launch_criterion_sum_det(const float* p, const float* t, long long count, int kind, double* partials, double* sum, hipStream_t s) {
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((count / 4 + 1023) / 1024, CRITERION_MAX_BLOCKS));
    dyf_form_note("criterion_sum_kernel:det", 0);
    hipLaunchKernelGGL(criterion_partial_kernel, dim3(grid), dim3(256), 0, s, p, t, count, kind, partials);
    hipLaunchKernelGGL(criterion_finish_kernel, dim3(1), dim3(64), 0, s, partials, (int)grid, sum);
    return hipGetLastError();
}

long long ensemble_metrics_partial_doubles(int n_members, long long n_points) {
    const int P = ensemble_tile_points(n_members);
    return P == 0 ? 0 : (n_points + P - 1) / P * 12;  // four waves x three sums per workgroup
}

hipError_t launch_ensemble_metrics(const float* preds, const float* targets, int n_members, long long n_points, double* partials,
                                   double* sums, hipStream_t s) {
    const int P = ensemble_tile_points(n_members);
    if (P == 0) return hipErrorInvalidValue;  // > 15 360 members
    const dim3 grid((unsigned)((n_points + P - 1) / P));
    if (n_members > 64)
        hipLaunchKernelGGL(ensemble_metrics_tiled_kernel, grid, dim3(256), ((size_t)n_members * P + 2 * 256) * sizeof(float), s, preds,
                           targets, n_members, n_points, partials, P);
    else
        hipLaunchKernelGGL(ensemble_metrics_kernel, grid, dim3(256), (size_t)n_members * 256 * sizeof(float), s, preds, targets,
                           n_members, n_points, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ensemble_metrics_finish_kernel, dim3(1), dim3(256), 0, s, partials, (long long)grid.x * 4, sums);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ trajectory metrics
// The per-point values of ensemble_point_reduce summed per SEGMENT (dyf_trajectory_metrics: one segment = one horizon step of a test
// trajectory, evaluate_ensemble_prediction(..., mean_over_samples=False), evaluation.py:44-45,92-96,112), with no atomics: blockIdx.y
// is the segment, the workgroup's sums (ensemble_wave_sums, ensemble_block_total) leave as partials[segment][blockIdx.x][3] and
// trajectory_metrics_finish_kernel adds a segment's partials.  A segment's sums depend on its own points alone (the split into
// workgroups is a function of n_members and n_points), so they are the same bits whichever segments share the call.  Member n of a
// segment starts n * member_stride elements behind the segment's pointer; the pointers are only 4-byte aligned (an (N, S, ...) tensor
// with an odd n_points), so every load is a dword, consecutive lanes on consecutive addresses.
__device__ __forceinline__ void trajectory_block_partial(const ensemble_point& pt, double* wsum, double* partials) {
    double v[3] = {pt.se, pt.var, pt.crps};
    ensemble_wave_sums<3>(v, wsum);
    const int tid = threadIdx.x;
    if (tid < 3) partials[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 3 + tid] = ensemble_block_total<3>(wsum, tid);
}

__global__ __launch_bounds__(256) void trajectory_metrics_kernel(const float* const* preds_tab, const float* const* targets_tab,
                                                                 int n_members, long long n_points, long long member_stride,
                                                                 double* partials) {
    extern __shared__ double traj_lds[];  // [n_members][256] floats; the first 96 bytes again for the four wave sums (64 members fill 64 KB)
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    ensemble_point pt = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (p < n_points)
        pt = ensemble_point_reduce(preds_tab[blockIdx.y] + p, member_stride, targets_tab[blockIdx.y][p], n_members, (float*)traj_lds);
    trajectory_block_partial(pt, traj_lds, partials);
}

__global__ __launch_bounds__(256) void trajectory_metrics_tiled_kernel(const float* const* preds_tab, const float* const* targets_tab,
                                                                       int n_members, long long n_points, long long member_stride,
                                                                       double* partials, int P) {
    extern __shared__ double traj_lds[];  // floats: [n_members][P] members (the first 96 bytes again for the wave sums), then [2][256] partials
    float* xs = (float*)traj_lds;
    const long long p0 = (long long)blockIdx.x * P;
    const int n_live = n_points - p0 < P ? (int)(n_points - p0) : P;
    bool holds;
    const ensemble_point pt = ensemble_point_reduce_tiled(preds_tab[blockIdx.y] + p0, member_stride, n_live, targets_tab[blockIdx.y] + p0,
                                                          n_members, P, xs, xs + (size_t)n_members * P, holds);
    trajectory_block_partial(pt, traj_lds, partials);
}

// One wave per segment: lane l adds the partials l, l + 64, ... in order, then lane 0 the lanes' sums in lane order; division as
// dyf_ensemble_metrics does it on the host.  accum is read and written by this wave alone (ordered by the stream).
__global__ __launch_bounds__(64) void trajectory_metrics_finish_kernel(const double* partials, long long n_blocks, long long n_points,
                                                                       int n_segments, double* out, double* accum) {
    __shared__ double lane_sum[3][64];
    const int seg = blockIdx.x, lane = threadIdx.x;
    const double* part = partials + (long long)seg * n_blocks * 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (long long i = lane; i < n_blocks; i += 64) {
        a0 += part[i * 3 + 0];
        a1 += part[i * 3 + 1];
        a2 += part[i * 3 + 2];
    }
    lane_sum[0][lane] = a0;
    lane_sum[1][lane] = a1;
    lane_sum[2][lane] = a2;
    __syncthreads();
    if (lane == 0) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int l = 0; l < 64; ++l) {
            s0 += lane_sum[0][l];
            s1 += lane_sum[1][l];
            s2 += lane_sum[2][l];
        }
        const double mse = s0 / (double)n_points;
        const double ssr = sqrt(s1 / (double)n_points) / sqrt(mse);
        const double crps = s2 / (double)n_points;
        out[seg] = mse;
        out[(long long)n_segments + seg] = ssr;
        out[2LL * n_segments + seg] = crps;
        if (accum) {
            accum[seg] += mse;
            accum[(long long)n_segments + seg] += ssr;
            accum[2LL * n_segments + seg] += crps;
        }
    }
}

long long trajectory_metrics_blocks(int n_members, long long n_points) {
    const int P = ensemble_tile_points(n_members);
    return P ? (n_points + P - 1) / P : 0;
}

hipError_t launch_trajectory_metrics(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                     long long n_points, long long member_stride, double* partials, double* out, double* accum,
                                     hipStream_t s) {
    const int P = ensemble_tile_points(n_members);
    const long long blocks = trajectory_metrics_blocks(n_members, n_points);
    // 256 * blocks threads along x stay below 2^32
    if (P == 0 || blocks < 1 || blocks > 0xffffffLL || n_segments < 1 || n_segments > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)n_segments);
    if (n_members > 64) {
        const size_t lds = ((size_t)n_members * P + 2 * 256) * sizeof(float);
        hipLaunchKernelGGL(trajectory_metrics_tiled_kernel, grid, dim3(256), lds, s, preds_tab, targets_tab, n_members, n_points,
                           member_stride, partials, P);
    } else {
        hipLaunchKernelGGL(trajectory_metrics_kernel, grid, dim3(256), (size_t)n_members * 256 * sizeof(float), s, preds_tab,
                           targets_tab, n_members, n_points, member_stride, partials);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(trajectory_metrics_finish_kernel, dim3((unsigned)n_segments), dim3(64), 0, s, partials, blocks, n_points,
                       n_segments, out, accum);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ ensemble-size metrics
// The metrics of EVERY prefix predictions[:n], n = 1..N, of every segment in one pass (dyf_ensemble_size_metrics:
// evaluate_ensemble_prediction_for_varying_members, evaluation.py:145-156, and its mse_per_mem).  A thread owns one point and walks
// the members in storage order with running recurrences in fp32: Welford's mean / M2 (M2 is exactly 0 after one member), the sum of
// |x - y|, and the pair term, which grows by row_n = sum_{m<n} |x_n - x_m| -- all N prefix scores for the pair work of one.  After
// member n the point contributes {(mean - y)^2, M2 / n, sabs / n - pair / n^2, (x_n - y)^2} to prefix n.
//   Staging: members in fours, xs[quad][thread] as float4, so the pair loop reads four members per ds_read_b128 on consecutive
// 16-byte slots (conflict-free) and is bound by its two VALU operations per pair, not by LDS reads.  A thread reads only what it
// wrote: the staging needs no barrier.
//   Reduction: an LDS transpose per quad, not fp64 shuffles per n.  The 16 fp32 values of a quad (4 members x 4 quantities) go to
// the wave's own [16][68]-float scratch (rows padded by 16 bytes: the ds_read_b128 lane groups meet no bank twice); lane l then
// adds columns 16 (l & 3) .. + 15 of row l >> 2 in fp64, in column order, two xor-shuffles join the four quarters, and lanes with
// l & 3 == 0 add the sum to the wave's fp64 accumulator in LDS.  Per quad and lane that is 16 conversions and 18 fp64 additions,
// against 16 x 6 shuffle steps for the butterfly form.
//   Tiles: workgroup b of a segment takes the tiles b, b + G, ... with G = ensemble_size_metrics_groups(n_members, n_points), so the
// partials are [n_segments][G][n_members][4] doubles whatever n_points is; the waves' accumulators are added in wave order, and
// ensemble_size_metrics_finish_kernel adds a segment's G partials in workgroup order.  Nothing depends on the other segments of the
// call or on the layout, and there are no atomics.  blockDim.x = 256 up to 64 members, 64 (one wave) beyond.
constexpr int ENS_SIZE_MAX_GROUPS = 64;     // workgroups per segment
constexpr int ENS_SIZE_SCRATCH_ROW = 68;    // floats per row of the transpose scratch
typedef const __attribute__((address_space(1))) float* ens_size_gptr;  // the table's pointers are global memory: global, not flat, loads

__global__ __launch_bounds__(256) void ensemble_size_metrics_kernel(const float* const* preds_tab, const float* const* targets_tab,
                                                                    int n_members, long long n_points, long long member_stride,
                                                                    long long n_tiles, double* partials) {
    extern __shared__ double ens_size_lds[];  // [waves][quads * 16] fp64 accumulators, [quads][P] float4 members, [waves][16][68] + [quads * 4] floats
    const int P = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = P >> 6;
    const int n_quads = (n_members + 3) >> 2;
    double* acc = ens_size_lds + (size_t)wave * n_quads * 16;
    float4* xs = (float4*)(ens_size_lds + (size_t)n_waves * n_quads * 16);
    float* scratch = (float*)(xs + (size_t)n_quads * P) + (size_t)wave * 16 * ENS_SIZE_SCRATCH_ROW;
    float* invs = (float*)(xs + (size_t)n_quads * P) + (size_t)n_waves * 16 * ENS_SIZE_SCRATCH_ROW;  // 1 / (n + 1), n < 4 * quads
    const ens_size_gptr preds = (ens_size_gptr)preds_tab[blockIdx.y], targets = (ens_size_gptr)targets_tab[blockIdx.y];
    for (int i = tid; i < n_quads * 4; i += P) invs[i] = 1.0f / (float)(i + 1);
    for (int i = lane; i < n_quads * 16; i += 64) acc[i] = 0.0;
    __syncthreads();
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long p = tile * P + tid;
        const bool live = p < n_points;
        const long long pc = live ? p : n_points - 1;  // every lane loads a valid address and takes part in the transpose
        const float y = live ? targets[pc] : 0.0f;
        const ens_size_gptr column = preds + pc;
        for (int q0 = 0; q0 < n_quads; q0 += 4) {  // 16 dword loads in flight per lane, then their four LDS writes
            float v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = column[(long long)min(4 * q0 + i, n_members - 1) * member_stride];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (!live || 4 * q0 + i >= n_members) v[i] = 0.0f;  // a dead lane's values are all zeros, and so are its contributions
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (q0 + u < n_quads) xs[(size_t)(q0 + u) * P + tid] = make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
        }
        float mean = 0.0f, m2 = 0.0f, sabs = 0.0f, pair = 0.0f;
        for (int q = 0; q < n_quads; ++q) {
            const float4 xq = xs[(size_t)q * P + tid];
            const float x[4] = {xq.x, xq.y, xq.z, xq.w};
            float row[4] = {0.0f, fabsf(x[1] - x[0]), fabsf(x[2] - x[0]) + fabsf(x[2] - x[1]),
                            (fabsf(x[3] - x[0]) + fabsf(x[3] - x[1])) + fabsf(x[3] - x[2])};
#pragma unroll 2
            for (int m = 0; m < q; ++m) {
                const float4 o = xs[(size_t)m * P + tid];
#pragma unroll
                for (int j = 0; j < 4; ++j) row[j] += (fabsf(x[j] - o.x) + fabsf(x[j] - o.y)) + (fabsf(x[j] - o.z) + fabsf(x[j] - o.w));
            }
            const float4 iq = ((const float4*)invs)[q];
            const float invq[4] = {iq.x, iq.y, iq.z, iq.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // members past n_members (zeros) run the recurrences too: nothing reads their prefixes
                const float inv = invq[j];
                const float d = x[j] - mean;
                mean += d * inv;
                m2 += d * (x[j] - mean);
                sabs += fabsf(x[j] - y);
                pair += row[j];
                float* col = scratch + (j * 4) * ENS_SIZE_SCRATCH_ROW + lane;
                col[0] = (mean - y) * (mean - y);
                col[ENS_SIZE_SCRATCH_ROW] = m2 * inv;
                col[2 * ENS_SIZE_SCRATCH_ROW] = sabs * inv - pair * inv * inv;
                col[3 * ENS_SIZE_SCRATCH_ROW] = (x[j] - y) * (x[j] - y);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the wave's LDS operations complete in order: only the compiler is held
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const float4* part = (const float4*)(scratch + (lane >> 2) * ENS_SIZE_SCRATCH_ROW + (lane & 3) * 16);
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 f = part[i];
                s += (double)f.x;
                s += (double)f.y;
                s += (double)f.z;
                s += (double)f.w;
            }
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if ((lane & 3) == 0) acc[q * 16 + (lane >> 2)] += s;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next quad rewrites the scratch behind these reads
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    __syncthreads();
    double* out = partials + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * n_members * 4;
    for (int i = tid; i < n_members * 4; i += P) {  // i = member * 4 + quantity = quad * 16 + scratch row
        double s = ens_size_lds[i];
        for (int w = 1; w < n_waves; ++w) s += ens_size_lds[(size_t)w * n_quads * 16 + i];
        out[i] = s;
    }
}

// One workgroup per segment, thread n = prefix n + 1: adds the G partials in workgroup order, divides, writes out[4][n_segments][N] =
// {mse, ssr, crps, mse_per_mem}.  accum is read and written by this thread alone (ordered by the stream).
__global__ __launch_bounds__(256) void ensemble_size_metrics_finish_kernel(const double* partials, int n_groups, int n_members,
                                                                           long long n_points, int n_segments, double* out,
                                                                           double* accum) {
    const int seg = blockIdx.x, n = threadIdx.x;
    if (n >= n_members) return;
    const double* part = partials + ((long long)seg * n_groups * n_members + n) * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int g = 0; g < n_groups; ++g, part += (long long)n_members * 4) {
        s0 += part[0];
        s1 += part[1];
        s2 += part[2];
        s3 += part[3];
    }
    const double mse = s0 / (double)n_points;
    const double v[4] = {mse, sqrt(s1 / (double)n_points) / sqrt(mse), s2 / (double)n_points, s3 / (double)n_points};
    const long long plane = (long long)n_segments * n_members, at = (long long)seg * n_members + n;
    for (int k = 0; k < 4; ++k) {
        out[k * plane + at] = v[k];
        if (accum) accum[k * plane + at] += v[k];
    }
}

static int ensemble_size_metrics_threads(int n_members) { return n_members <= 64 ? 256 : 64; }

int ensemble_size_metrics_groups(int n_members, long long n_points) {
    if (n_members < 1 || n_members > ENSEMBLE_SIZE_MAX_MEMBERS || n_points < 1) return 0;
    const int P = ensemble_size_metrics_threads(n_members);
    return (int)std::min<long long>((n_points + P - 1) / P, ENS_SIZE_MAX_GROUPS);
}

hipError_t launch_ensemble_size_metrics(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                        long long n_points, long long member_stride, double* partials, double* out, double* accum,
                                        hipStream_t s) {
    const int groups = ensemble_size_metrics_groups(n_members, n_points);
    if (groups < 1 || n_segments < 1 || n_segments > 65535) return hipErrorInvalidValue;
    const int P = ensemble_size_metrics_threads(n_members), waves = P / 64, quads = (n_members + 3) / 4;
    const size_t lds = (size_t)waves * quads * 16 * sizeof(double) + (size_t)quads * P * 4 * sizeof(float) +
                       (size_t)waves * 16 * ENS_SIZE_SCRATCH_ROW * sizeof(float) + (size_t)quads * 4 * sizeof(float);  // at most 89.25 KB (64 members)
    hipError_t e = hipFuncSetAttribute((const void*)ensemble_size_metrics_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (e != hipSuccess) return e;
    dyf_form_note(P == 256 ? "ensemble_size_metrics_kernel:lds_transpose" : "ensemble_size_metrics_kernel:lds_transpose+wave", 0);
    hipLaunchKernelGGL(ensemble_size_metrics_kernel, dim3((unsigned)groups, (unsigned)n_segments), dim3(P), lds, s, preds_tab, targets_tab,
                       n_members, n_points, member_stride, (n_points + P - 1) / P, partials);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ensemble_size_metrics_finish_kernel, dim3((unsigned)n_segments), dim3(256), 0, s, partials, groups, n_members,
                       n_points, n_segments, out, accum);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ ensemble scores
// Five scores per (segment, GROUP) in one pass (dyf_ensemble_scores: evaluate_ensemble_mse / _spread_skill_ratio / _crps / _nll with
// mean_dims and evaluate_ensemble_corr, evaluation.py:83-142).  A segment's points are row-major (n_outer, n_groups, n_inner) and
// point p belongs to group (p / n_inner) % n_groups.  Work mapping: blockIdx.x = slab * tiles_per_slab + tile with slab = outer *
// n_groups + group, so a workgroup's tile lies inside one (outer, group) slab and its partial belongs to one group; blockIdx.y is the
// segment.  To the per-point values of ensemble_point_reduce (pooled, (1, 1, n_points), the tiles, the block sums and the finish
// order are those of dyf_trajectory_metrics, and mse / ssr / crps its bits) this adds nll = 0.5 log(2 pi var) + se / (2 var) in fp32
// with the accurate logf; no clamp: one member has var = 0 and a NaN nll, as numpy.
//   Correlation: a workgroup leaves the mean of its points' ensemble means and targets and their CENTRED second moments about
// those (fp64, from the fp32 mean and y; a second round over values the threads still hold), and the finish kernel joins the
// workgroups' moments pairwise (Chan et al.).  The raw moments sum(m), sum(m^2), ... would give the same correlation on ordinary
// data, but for a group whose means or targets are constant their difference is rounding noise, not the exact zero that makes
// numpy's corrcoef NaN; here a constant c gives workgroup means of exactly c (up to 256 copies of a 24-bit value add exactly in
// fp64), deviations, M2 and co-moment of exactly 0 at every join, and corr = 0 / 0.
//   partials[n_segments][blocks][9] = {sum se, sum var, sum crps, sum nll, mean of m, mean of y, M2 m, M2 y, co-moment}; the live
// points of a tile follow from the geometry.  ensemble_scores_finish_kernel (one wave per (segment, group)) walks the group's
// partials in (outer, tile) order: lane l takes entries l, l + 64, ..., lane 0 joins the lanes in lane order.  No atomics; a group's
// result depends on its own points, n_members and (n_outer, n_inner) alone.

// `holds`: this thread carries a live point's values (the others add zeros); n_live: the live points of the tile (>= 1).
__device__ __forceinline__ void scores_block_partial(bool holds, const ensemble_point& pt, int n_live, double* wsum, double* partials) {
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (holds) {
        const float nll = 0.5f * logf(6.2831853071795865f * pt.var) + pt.se / (2.0f * pt.var);
        v[0] = pt.se;
        v[1] = pt.var;
        v[2] = pt.crps;
        v[3] = nll;
        v[4] = pt.mean;
        v[5] = pt.y;
    }
    ensemble_wave_sums<6>(v, wsum);
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = ensemble_block_total<6>(wsum, k);  // every thread: the workgroup's sums
    const double mm = v[4] / (double)n_live, my = v[5] / (double)n_live;
    double c[3] = {0.0, 0.0, 0.0};
    if (holds) {
        const double dm = (double)pt.mean - mm, dy = (double)pt.y - my;
        c[0] = dm * dm;
        c[1] = dy * dy;
        c[2] = dm * dy;
    }
    ensemble_wave_sums<3>(c, wsum);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ensemble_block_total<3>(wsum, k);
    if (threadIdx.x == 0) {
        double* partial = partials + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * ENSEMBLE_SCORES_PARTIAL;
        partial[0] = v[0];
        partial[1] = v[1];
        partial[2] = v[2];
        partial[3] = v[3];
        partial[4] = mm;
        partial[5] = my;
        partial[6] = c[0];
        partial[7] = c[1];
        partial[8] = c[2];
    }
}

__global__ __launch_bounds__(256) void ensemble_scores_kernel(const float* const* preds_tab, const float* const* targets_tab,
                                                              int n_members, long long member_stride, long long n_inner,
                                                              unsigned tiles_per_slab, double* partials) {
    extern __shared__ double scores_lds[];  // [n_members][256] floats; the first 192 bytes again for the wave sums
    const unsigned slab = blockIdx.x / tiles_per_slab, tile = blockIdx.x - slab * tiles_per_slab;
    const long long q = (long long)tile * 256 + threadIdx.x;  // within the slab
    const long long p = (long long)slab * n_inner + q;
    const bool live = q < n_inner;
    ensemble_point pt = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (live)
        pt = ensemble_point_reduce(preds_tab[blockIdx.y] + p, member_stride, targets_tab[blockIdx.y][p], n_members, (float*)scores_lds);
    const int n_live = n_inner - (long long)tile * 256 < 256 ? (int)(n_inner - (long long)tile * 256) : 256;
    scores_block_partial(live, pt, n_live, scores_lds, partials);
}

__global__ __launch_bounds__(256) void ensemble_scores_tiled_kernel(const float* const* preds_tab, const float* const* targets_tab,
                                                                    int n_members, long long member_stride, long long n_inner,
                                                                    unsigned tiles_per_slab, double* partials, int P) {
    extern __shared__ double scores_lds[];  // floats: [n_members][P] members (the first 192 bytes again for the wave sums), then [2][256] partials
    float* xs = (float*)scores_lds;
    const unsigned slab = blockIdx.x / tiles_per_slab, tile = blockIdx.x - slab * tiles_per_slab;
    const long long q0 = (long long)tile * P;            // within the slab
    const long long p0 = (long long)slab * n_inner + q0;
    const int n_live = n_inner - q0 < P ? (int)(n_inner - q0) : P;
    bool holds;
    const ensemble_point pt = ensemble_point_reduce_tiled(preds_tab[blockIdx.y] + p0, member_stride, n_live, targets_tab[blockIdx.y] + p0,
                                                          n_members, P, xs, xs + (size_t)n_members * P, holds);
    scores_block_partial(holds, pt, n_live, scores_lds, partials);
}

struct scores_moments {
    double n, mm, my, m2m, m2y, c;  // points, the two means, the centred second moments and the co-moment about them
};
__device__ __forceinline__ void scores_join(scores_moments& a, const scores_moments& b) {
    if (b.n == 0.0) return;
    if (a.n == 0.0) {
        a = b;
        return;
    }
    const double n = a.n + b.n, dm = b.mm - a.mm, dy = b.my - a.my, f = a.n * b.n / n, w = b.n / n;
    a.m2m += b.m2m + dm * dm * f;
    a.m2y += b.m2y + dy * dy * f;
    a.c += b.c + dm * dy * f;
    a.mm += dm * w;
    a.my += dy * w;
    a.n = n;
}

// One wave per (segment, group): blockIdx.x the group, blockIdx.y the segment.  accum is read and written by this wave alone
// (ordered by the stream).
__global__ __launch_bounds__(64) void ensemble_scores_finish_kernel(const double* partials, long long n_blocks, long long n_outer,
                                                                    int n_groups, long long n_inner, long long tiles_per_slab,
                                                                    int tile_points, int n_segments, double* out, double* accum) {
    __shared__ double lane_state[10][64];
    const int g = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x;
    const double* part = partials + (long long)seg * n_blocks * ENSEMBLE_SCORES_PARTIAL;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    scores_moments mo = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const long long count = n_outer * tiles_per_slab;
    for (long long j = lane; j < count; j += 64) {
        const long long o = j / tiles_per_slab, t = j - o * tiles_per_slab;
        const double* b = part + ((o * n_groups + g) * tiles_per_slab + t) * ENSEMBLE_SCORES_PARTIAL;
        a0 += b[0];
        a1 += b[1];
        a2 += b[2];
        a3 += b[3];
        const long long left = n_inner - t * tile_points;
        const scores_moments bm = {(double)(left < tile_points ? left : (long long)tile_points), b[4], b[5], b[6], b[7], b[8]};
        scores_join(mo, bm);
    }
    lane_state[0][lane] = a0;
    lane_state[1][lane] = a1;
    lane_state[2][lane] = a2;
    lane_state[3][lane] = a3;
    lane_state[4][lane] = mo.n;
    lane_state[5][lane] = mo.mm;
    lane_state[6][lane] = mo.my;
    lane_state[7][lane] = mo.m2m;
    lane_state[8][lane] = mo.m2y;
    lane_state[9][lane] = mo.c;
    __syncthreads();
    if (lane == 0) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        scores_moments all = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int l = 0; l < 64; ++l) {
            s0 += lane_state[0][l];
            s1 += lane_state[1][l];
            s2 += lane_state[2][l];
            s3 += lane_state[3][l];
            const scores_moments lm = {lane_state[4][l], lane_state[5][l], lane_state[6][l], lane_state[7][l], lane_state[8][l],
                                       lane_state[9][l]};
            scores_join(all, lm);
        }
        const double n = (double)n_outer * (double)n_inner;
        const double mse = s0 / n;
        const double v[5] = {mse, sqrt(s1 / n) / sqrt(mse), s2 / n, s3 / n, (all.c / n) / sqrt((all.m2m / n) * (all.m2y / n))};
        const long long plane = (long long)n_segments * n_groups, at = (long long)seg * n_groups + g;
        for (int k = 0; k < 5; ++k) {
            out[k * plane + at] = v[k];
            if (accum) accum[k * plane + at] += v[k];
        }
    }
}

long long ensemble_scores_blocks(int n_members, long long n_outer, int n_groups, long long n_inner) {
    const int P = ensemble_tile_points(n_members);
    if (P == 0 || n_outer < 1 || n_groups < 1 || n_inner < 1) return 0;
    const long long tiles = (n_inner + P - 1) / P;
    if (!ensemble_geometry_fits(n_outer, n_groups, tiles)) return -1;
    return tiles * n_outer * n_groups;
}

hipError_t launch_ensemble_scores(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                  long long member_stride, long long n_outer, int n_groups, long long n_inner, double* partials,
                                  double* out, double* accum, hipStream_t s) {
    const long long blocks = ensemble_scores_blocks(n_members, n_outer, n_groups, n_inner);
    if (blocks < 1 || n_segments < 1 || n_segments > 65535) return hipErrorInvalidValue;
    const int P = ensemble_tile_points(n_members);
    const long long tiles = (n_inner + P - 1) / P;
    const dim3 grid((unsigned)blocks, (unsigned)n_segments);
    if (n_members > 64) {
        const size_t lds = ((size_t)n_members * P + 2 * 256) * sizeof(float);
        dyf_form_note("ensemble_scores_kernel:slab+tiled", 0);
        hipLaunchKernelGGL(ensemble_scores_tiled_kernel, grid, dim3(256), lds, s, preds_tab, targets_tab, n_members, member_stride,
                           n_inner, (unsigned)tiles, partials, P);
    } else {
        dyf_form_note("ensemble_scores_kernel:slab", 0);
        hipLaunchKernelGGL(ensemble_scores_kernel, grid, dim3(256), (size_t)n_members * 256 * sizeof(float), s, preds_tab, targets_tab,
                           n_members, member_stride, n_inner, (unsigned)tiles, partials);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ensemble_scores_finish_kernel, dim3((unsigned)n_groups, (unsigned)n_segments), dim3(64), 0, s, partials, blocks,
                       n_outer, n_groups, n_inner, tiles, P, n_segments, out, accum);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ exchange unpack
__global__ __launch_bounds__(256) void gather_unpack_kernel(const float4* recv, float4* out, int world, int slots, int nb, int total_rows,
                                                            long long row4) {
    const int g = blockIdx.y;                 // global row
    const int slot = blockIdx.z;
    const int base = total_rows / world, extra = total_rows % world;
    // owner of global row g under the balanced contiguous split: ranks < extra own base + 1 rows
    const int cut = extra * (base + 1);
    const int r = g < cut ? g / (base + 1) : extra + (g - cut) / max(base, 1);
    const int j = g < cut ? g - r * (base + 1) : (g - cut) - (r - extra) * base;
    const float4* src = recv + (((size_t)r * slots + slot) * nb + j) * row4;
    float4* dst = out + ((size_t)slot * total_rows + g) * row4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < row4; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void gather_unpack_scalar_kernel(const float* recv, float* out, int world, int slots, int nb,
                                                                   int total_rows, long long row) {
    const int g = blockIdx.y, slot = blockIdx.z;
    const int base = total_rows / world, extra = total_rows % world, cut = extra * (base + 1);
    const int r = g < cut ? g / (base + 1) : extra + (g - cut) / max(base, 1);
    const int j = g < cut ? g - r * (base + 1) : (g - cut) - (r - extra) * base;
    const float* src = recv + (((size_t)r * slots + slot) * nb + j) * row;
    float* dst = out + ((size_t)slot * total_rows + g) * row;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < row; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

hipError_t launch_gather_unpack(const float* recv, float* out, int world, int slots, int nb, int total_rows, long long row, hipStream_t s) {
    const bool vec = row % 4 == 0 && ((uintptr_t)recv & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const long long units = vec ? row / 4 : row;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((units + 1023) / 1024, 64)), (unsigned)total_rows, (unsigned)slots);
    if (vec)
        hipLaunchKernelGGL(gather_unpack_kernel, grid, dim3(256), 0, s, (const float4*)recv, (float4*)out, world, slots, nb, total_rows, units);
    else
        hipLaunchKernelGGL(gather_unpack_scalar_kernel, grid, dim3(256), 0, s, recv, out, world, slots, nb, total_rows, row);
    return hipGetLastError();
}
