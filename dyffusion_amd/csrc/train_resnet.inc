// Training step of the ResNet-UNet (arch DYF_ARCH_UNET_RESNET; SURVEY 8f-2): recorded forward + backward of
// src/models/unet.py:26-109, 266-315 and src/models/modules/attention.py:7-73 -- what the reference gets from torch.autograd
// when `DYffusion.p_losses` (src/diffusion/dyffusion.py:496-567) trains the OISST forecaster: weight-standardised 3x3 convs
// (gradient THROUGH the standardisation), GroupNorm + FiLM + SiLU + Dropout, residual 1x1 convs, channel LayerNorm (gain),
// LinearAttention (softmax over d of q, softmax over pixels of k, two 32 x 32 contractions per head), Attention (softmax over
// keys, dropout on the probabilities), nearest x2 upsampling, 4x4 / stride-2 down convs, the 7x7 stem, the 1x1 head, skip
// concatenations, the time MLP and the per-block FiLM heads.
//
// The same mechanism records arch unet_simple (src/models/unet_simple.py:13-82, 164-197; us_walk): BatchNorm2d on batch or running
// statistics, the x2 bilinear upsample of a concatenation that is never written, the outer resample, the ConvTranspose2d readout.
//
// This file is #included by train.hip (it uses that file's kernels and helpers: convolutions on the fp32 matrix cores, the
// normalisation / FiLM / dropout kernels, the dense layers, the caching allocator).  Everything is fp32, NHWC.  Structure: a small
// tape -- every op of the forward pushes a closure that, given the gradient of its output, ACCUMULATES into the gradients of its
// inputs and of its parameters; dyf_train_backward runs the closures in reverse.  A layer walk is written once, as a template over
// its context: RCtx launches (and records, or -- fp32 sampling -- bumps through the engine's arena), RCount sizes that arena.  The new kernels below are written for
// correctness (one thread per output, plain loops): the convolutions, 97 % of the FLOPs, run on train_gemm.hip.
#include <deque>
#include <functional>
#include <memory>

namespace dyf {

// RParam / TrainNet (one parameter in its training layout; the parameters and gradients of one network): train_internal.h

struct RT {                  // an activation of the recorded forward and (during the backward) its gradient
    float* p = nullptr;
    float* g = nullptr;
    size_t n = 0;
    uint8_t need = 0;        // who wants its gradient: 0 whoever produced it, 1 only a caller that asked for the network input's, 2 nobody
};

struct RTape {
    int net = -1, nb = 0, flags = 0;
    int det = 0;                 // the deterministic mode the forward was recorded under: its backward runs under the same
    std::vector<void*> owned;
    std::deque<RT> ts;                                         // stable addresses
    std::vector<std::function<dyf_status()>> back;             // run in reverse
    RT *out = nullptr, *x_in = nullptr;
    int in_lo = 0;               // first channel of the caller's `inputs` inside x_in (unet.Unet concatenates the condition first)
    uint32_t* row_keys = nullptr;
    std::shared_ptr<void> ctx;   // the recording context the closures point into (RCtx), alive until the slot is re-recorded
};

}  // namespace dyf

namespace {

// ------------------------------------------------------------------------------------------------ kernels
// WeightStandardizedConv2d (unet.py:26-40): w_hat = (w - mean) * rsqrt(var + 1e-5) per output channel over its K = taps * cin
// weights (biased variance), written in both conv layouts
__global__ __launch_bounds__(256) void t_ws_fwd(const float* w, int K, int cin, int cout, float* wh, float* wht, float* rstd) {
    __shared__ double red[2][256];
    const int co = blockIdx.x;
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < K; i += 256) {
        const double v = w[(size_t)co * K + i];
        s += v;
        q += v * v;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = q;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            red[0][threadIdx.x] += red[0][threadIdx.x + d];
            red[1][threadIdx.x] += red[1][threadIdx.x + d];
        }
        __syncthreads();
    }
    const double mean = red[0][0] / K, var = red[1][0] / K - mean * mean;
    const float rs = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + 1e-5)), mu = (float)mean;
    for (int i = threadIdx.x; i < K; i += 256) {
        const float v = (w[(size_t)co * K + i] - mu) * rs;
        wh[(size_t)co * K + i] = v;
        wht[(size_t)i * cout + co] = v;   // i = tap * cin + ci
    }
    if (threadIdx.x == 0) rstd[co] = rs;
}
// dw += rstd * (dwh - mean(dwh) - wh * mean(dwh * wh))
__global__ __launch_bounds__(256) void t_ws_bwd(const float* dwh, const float* wh, const float* rstd, int K, float* gw) {
    __shared__ double red[2][256];
    const int co = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < K; i += 256) {
        const double d = dwh[(size_t)co * K + i];
        a += d;
        b += d * wh[(size_t)co * K + i];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            red[0][threadIdx.x] += red[0][threadIdx.x + d];
            red[1][threadIdx.x] += red[1][threadIdx.x + d];
        }
        __syncthreads();
    }
    const float m1 = (float)(red[0][0] / K), m2 = (float)(red[1][0] / K), rs = rstd[co];
    for (int i = threadIdx.x; i < K; i += 256) {
        const size_t e = (size_t)co * K + i;
        gw[e] += rs * (dwh[e] - m1 - wh[e] * m2);
    }
}

// LearnedSinusoidalPosEmb (misc.py:35-51): f[r] = [t, sin(2 pi t w_j) (j < half), cos(2 pi t w_j)]; dw_j = sum_r 2 pi t (cos * g_sin - sin * g_cos)
__global__ void t_learned_sinu_fwd(const float* time, const float* w, int rows, int half, float* f) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int F = 2 * half + 1;
    if (i >= (long long)rows * F) return;
    const int r = (int)(i / F), k = (int)(i % F);
    const float t = time[r];
    if (k == 0) { f[i] = t; return; }
    const float ang = t * w[(k - 1) % half] * 6.283185307179586f;
    f[i] = k <= half ? sinf(ang) : cosf(ang);
}
__global__ void t_learned_sinu_bwd(const float* time, const float* w, const float* df, int rows, int half, float* gw) {
    const int F = 2 * half + 1;
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
        double acc = 0.0;
        for (int r = 0; r < rows; ++r) {
            const float t = time[r], ang = t * w[j] * 6.283185307179586f;
            acc += (double)(6.283185307179586f * t) * ((double)cosf(ang) * df[(size_t)r * F + 1 + j] - (double)sinf(ang) * df[(size_t)r * F + 1 + half + j]);
        }
        gw[j] += (float)acc;
    }
}

struct RDrop {               // dropout of one site: engine generator, stream keyed by (forward, global row, site)
    int on;
    float scale;
    uint32_t thresh16;
    RngKey salt;
    const uint32_t* row_keys;
    const uint8_t* mask;     // sampling, dropout mode 2: the caller's keep mask of the site ([rows][per], the tensor's own layout)
    uint32_t per;            // elements of one batch row at this site
};
__device__ __forceinline__ float r_keep(const RDrop& d, int b, uint32_t e_in_row) {
    if (d.mask) return d.mask[(size_t)b * d.per + e_in_row] ? d.scale : 0.0f;
    if (!d.on) return 1.0f;
    const RngKey rk = rng_stream_key(RngKey{d.row_keys[2 * b], d.row_keys[2 * b + 1]}, d.salt);
    return rng_keep(e_in_row, rk, d.thresh16) ? d.scale : 0.0f;
}

// channel LayerNorm with gain (unet.py:43-52: biased variance over the channels of a pixel, eps 1e-5) + Dropout
// (LinearAttention.to_qkv = Sequential(Dropout, Conv), attention.py:12).  One thread per pixel; stats[pixel] = (mean, rstd).
// 16 lanes per pixel (lane l holds channels l, l + 16, ...: a pixel's row is read as coalesced 64-byte pieces), butterflies over the
// 16 lanes.  (First form: one thread per pixel walking its C channels -- every load a different cache line: 79 / 132 us per call.)
__device__ __forceinline__ float ln_sum16(float v) {
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}
__global__ void t_ln_fwd(const float* x, const float* g, int n, int hw, int C, RDrop dr, float* y, float2* stats) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = t >> 4;
    const int l = (int)(t & 15);
    const bool live = i < (long long)n * hw;
    const long long ic = live ? i : (long long)n * hw - 1;
    const float* xp = x + (size_t)ic * C;
    float s = 0.0f;
    for (int c = l; c < C; c += 16) s += xp[c];
    const float mu = ln_sum16(s) / C;
    float v = 0.0f;
    for (int c = l; c < C; c += 16) v = fmaf(xp[c] - mu, xp[c] - mu, v);
    const float rs = rsqrtf(ln_sum16(v) / C + 1e-5f);
    if (!live) return;
    if (l == 0) stats[i] = make_float2(mu, rs);
    const int b = (int)(i / hw);
    const uint32_t e0 = (uint32_t)((i - (long long)b * hw) * C);
    for (int c = l; c < C; c += 16) y[(size_t)i * C + c] = (xp[c] - mu) * rs * g[c] * r_keep(dr, b, e0 + c);
}
__global__ void t_ln_bwd_x(const float* x, const float* g, const float* dy, const float2* stats, int n, int hw, int C, RDrop dr, float* gx) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = t >> 4;
    const int l = (int)(t & 15);
    const bool live = i < (long long)n * hw;
    const long long ic = live ? i : (long long)n * hw - 1;
    const float mu = stats[ic].x, rs = stats[ic].y;
    const int b = (int)(ic / hw);
    const uint32_t e0 = (uint32_t)((ic - (long long)b * hw) * C);
    float m1 = 0.0f, m2 = 0.0f;
    for (int c = l; c < C; c += 16) {
        const float d = dy[(size_t)ic * C + c] * r_keep(dr, b, e0 + c) * g[c], xh = (x[(size_t)ic * C + c] - mu) * rs;
        m1 += d;
        m2 = fmaf(d, xh, m2);
    }
    m1 = ln_sum16(m1) / C;
    m2 = ln_sum16(m2) / C;
    if (!live) return;
    for (int c = l; c < C; c += 16) {
        const float d = dy[(size_t)i * C + c] * r_keep(dr, b, e0 + c) * g[c], xh = (x[(size_t)i * C + c] - mu) * rs;
        gx[(size_t)i * C + c] += rs * (d - m1 - xh * m2);
    }
}
// dg[c] += sum over pixels of dy * keep * xhat.  A workgroup takes LN_GCHUNK pixels, thread = (pixel group, channel): coalesced rows,
// fp64 sums, the pixel groups meet in LDS, one fp32 atomic per (workgroup, channel).  (First form, kept for channel counts that do
// not divide 256: one workgroup per channel striding over all pixels, 4 bytes used of every line -- 347 us per call.)
constexpr int LN_GCHUNK = 64;
__global__ __launch_bounds__(256) void t_ln_bwd_g_rows(const float* x, const float* dy, const float2* stats, int n, int hw, int C, RDrop dr, float* gg) {
    __shared__ double red[256];
    const int c = threadIdx.x % C, sub = threadIdx.x / C, nsub = 256 / C;
    const long long total = (long long)n * hw, i0 = (long long)blockIdx.x * LN_GCHUNK, i1 = i0 + LN_GCHUNK < total ? i0 + LN_GCHUNK : total;
    double a = 0.0;
    for (long long i = i0 + sub; i < i1; i += nsub) {
        const int b = (int)(i / hw);
        const uint32_t e = (uint32_t)((i - (long long)b * hw) * C + c);
        const float2 st = stats[i];
        a += (double)(dy[(size_t)i * C + c] * r_keep(dr, b, e) * (x[(size_t)i * C + c] - st.x) * st.y);
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (sub == 0) {
        for (int j = 1; j < nsub; ++j) a += red[j * C + c];
        atomicAdd(gg + c, (float)a);
    }
}
// deterministic mode: the same sums per workgroup (any chunk of pixels), stored to slab blockIdx.x of the workspace (C floats per slab)
__global__ __launch_bounds__(256) void t_ln_bwd_g_slab(const float* x, const float* dy, const float2* stats, int n, int hw, int C, RDrop dr, int chunk, float* ws) {
    __shared__ double red[256];
    const int c = threadIdx.x % C, sub = threadIdx.x / C, nsub = 256 / C;
    const long long total = (long long)n * hw, i0 = (long long)blockIdx.x * chunk, i1 = i0 + chunk < total ? i0 + chunk : total;
    double a = 0.0;
    for (long long i = i0 + sub; i < i1; i += nsub) {
        const int b = (int)(i / hw);
        const uint32_t e = (uint32_t)((i - (long long)b * hw) * C + c);
        const float2 st = stats[i];
        a += (double)(dy[(size_t)i * C + c] * r_keep(dr, b, e) * (x[(size_t)i * C + c] - st.x) * st.y);
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (sub == 0) {
        for (int j = 1; j < nsub; ++j) a += red[j * C + c];
        ws[(size_t)blockIdx.x * C + c] = (float)a;
    }
}
__global__ __launch_bounds__(256) void t_ln_bwd_g(const float* x, const float* dy, const float2* stats, int n, int hw, int C, RDrop dr, float* gg) {
    __shared__ double red[256];
    const int c = blockIdx.x;
    double a = 0.0;
    for (long long i = threadIdx.x; i < (long long)n * hw; i += 256) {
        const int b = (int)(i / hw);
        const uint32_t e = (uint32_t)((i - (long long)b * hw) * C + c);
        a += (double)(dy[(size_t)i * C + c] * r_keep(dr, b, e) * (x[(size_t)i * C + c] - stats[i].x) * stats[i].y);
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) gg[c] += (float)red[0];
}

// ---- LinearAttention core (attention.py:22-49, rescale "qkv"), 4 heads x 32; qkv (n, hw, 384) = [q | k | v] x (head, 32)
constexpr int RH = 4, RD = 32, RHID = 128;
// sq = softmax over the 32 channels of a head, per pixel (unscaled)
__global__ void t_la_qsoft(const float* qkv, long long npix, float* sq) {
    // one thread per element, a head's 32 channels on 32 neighbouring lanes: coalesced rows, max / sum by butterflies
    // (first form: one thread per (pixel, head) walking its 128 bytes alone -- 330 us per call at 64 x 3 600 pixels)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix * RHID) return;  // RHID is a multiple of the wave: whole waves leave
    const long long p = i / RHID;
    const int c = (int)(i % RHID);
    const float v = qkv[(size_t)p * 3 * RHID + c];
    float m = v;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 32));
    const float ex = expf(v - m);
    float t = ex;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 32);
    sq[i] = ex / t;
}
// per (sample, channel of k): max and sum of exp over the pixels
// two steps: (1) a workgroup walks LA_PCHUNK pixels of one sample, thread = (pixel parity, channel): rows of 128 consecutive floats,
// running (max, sum of exp) per thread; (2) the chunks of a (sample, channel) are merged in chunk order.  (First form: one workgroup
// per (sample, channel) striding over the pixels, 4 bytes used of every line it touched: 230 us per call.)
constexpr int LA_PCHUNK = 32;
__global__ __launch_bounds__(256) void t_la_kstat_part(const float* qkv, int hw, float2* part) {
    __shared__ float2 red[RHID];
    const int n = blockIdx.y, ck = blockIdx.x, ch = threadIdx.x & (RHID - 1), half = threadIdx.x >> 7;
    const int p0 = ck * LA_PCHUNK, p1 = min(hw, p0 + LA_PCHUNK);
    const float* k = qkv + (size_t)n * hw * 3 * RHID + RHID + ch;
    float m = -INFINITY, t = 0.0f;
    for (int p = p0 + half; p < p1; p += 2) {
        const float v = k[(size_t)p * 3 * RHID];
        const float mn = fmaxf(m, v);
        t = t * expf(m - mn) + expf(v - mn);
        m = mn;
    }
    if (half) red[ch] = make_float2(m, t);
    __syncthreads();
    if (!half) {
        const float2 o = red[ch];
        const float mn = fmaxf(m, o.x);
        if (mn > -INFINITY) t = t * expf(m - mn) + o.y * expf(o.x - mn);
        part[((size_t)n * gridDim.x + ck) * RHID + ch] = make_float2(mn, t);
    }
}
__global__ void t_la_kstat_finish(const float2* part, int nchunk, int count, float* kmax, float* ksum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (sample, channel)
    if (i >= count) return;
    const int n = i / RHID, ch = i % RHID;
    float m = -INFINITY, t = 0.0f;
    for (int ck = 0; ck < nchunk; ++ck) {
        const float2 o = part[((size_t)n * nchunk + ck) * RHID + ch];
        const float mn = fmaxf(m, o.x);
        t = t * expf(m - mn) + o.y * expf(o.x - mn);
        m = mn;
    }
    kmax[i] = m;
    ksum[i] = t;
}
__global__ void t_la_ksoft(const float* qkv, int hw, long long total, const float* kmax, const float* ksum, float* sk) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % RHID);
    const long long p = i / RHID;
    const int n = (int)(p / hw);
    sk[i] = expf(qkv[(size_t)p * 3 * RHID + RHID + ch] - kmax[n * RHID + ch]) / ksum[n * RHID + ch];
}
// M[n][h][d][e] = alpha * sum_p A[p][h*32 + d] * B[p][h*32 + e]; A / B rows `sa` / `sb` floats apart.  The pixel sum is split over
// workgroups (LA_CHUNK pixels each, 32-pixel stages of both operands in LDS, fp64 partial sums) and merged in split order by
// t_la_outer_finish: deterministic.  (First form: one workgroup per (n, h), every thread walking all pixels with strided loads --
// 1.13 ms per call at 8 x 3 600 pixels, 44 % of the OISST training step.)
constexpr int LA_CHUNK = 256;
__global__ __launch_bounds__(256) void t_la_outer_part(const float* A, int sa, const float* B, int sb, int hw, double* part) {
    __shared__ float sA[32][RD + 1], sB[32][RD];
    const int n = blockIdx.y, h = blockIdx.x, sp = blockIdx.z;
    const float* a = A + (size_t)n * hw * sa + h * RD;
    const float* b = B + (size_t)n * hw * sb + h * RD;
    const int p0 = sp * LA_CHUNK, p1 = min(hw, p0 + LA_CHUNK);
    const int e2 = threadIdx.x % RD, d0 = threadIdx.x / RD;  // outputs (d0 + 8 k, e2), k = 0..3
    const int lp = threadIdx.x / RD, lc = threadIdx.x % RD;   // staging role: pixel lp (+8 j), channel lc
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int pb = p0; pb < p1; pb += 32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = pb + lp + 8 * j;
            sA[lp + 8 * j][lc] = p < p1 ? a[(size_t)p * sa + lc] : 0.0f;
            sB[lp + 8 * j][lc] = p < p1 ? b[(size_t)p * sb + lc] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < 32; ++q) {
            const double bv = (double)sB[q][e2];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += (double)sA[q][d0 + 8 * k] * bv;
        }
        __syncthreads();
    }
    double* o = part + ((size_t)(sp * gridDim.y + n) * RH + h) * RD * RD;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[(d0 + 8 * k) * RD + e2] = acc[k];
}
__global__ void t_la_outer_finish(const double* part, int nsplit, long long count, float alpha, float* M) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double t = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) t += part[(size_t)sp * count + i];
    M[i] = (float)(alpha * t);
}
// The three per-pixel products with a head's 32 x 32 matrix share one shape: grid (pixel chunks, samples), thread = (pixel parity,
// channel (h, j)); the thread's row / column of the matrix sits in 32 registers for the whole chunk, a pixel's 32 partner values are
// read as eight 16-byte loads that every lane of the head shares (one line per head and instruction), results leave as coalesced
// rows.  (First forms: one thread per (pixel, head) or per element re-reading the matrix from L1 for every pixel -- 100-420 us per
// call at 64 x 3 600 pixels.)
// out[p][h*32 + e] = scale * sum_d ctx[h][d][e] * sq[p][h*32 + d]
__global__ __launch_bounds__(256) void t_la_out(const float* ctx, const float* sq, int hw, float scale, float* out) {
    const int n = blockIdx.y, ch = threadIdx.x & (RHID - 1), half = threadIdx.x >> 7, h = ch / RD, j = ch % RD;
    const int p0 = blockIdx.x * LA_PCHUNK, p1 = min(hw, p0 + LA_PCHUNK);
    const float* c = ctx + (size_t)(n * RH + h) * RD * RD;
    float col[RD];
#pragma unroll
    for (int d = 0; d < RD; ++d) col[d] = scale * c[d * RD + j];
    for (int p = p0 + half; p < p1; p += 2) {
        const float4* s4 = (const float4*)(sq + ((size_t)n * hw + p) * RHID + h * RD);
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < RD / 4; ++q) {
            const float4 v = s4[q];
            acc = fmaf(col[4 * q], v.x, fmaf(col[4 * q + 1], v.y, fmaf(col[4 * q + 2], v.z, fmaf(col[4 * q + 3], v.w, acc))));
        }
        out[((size_t)n * hw + p) * RHID + ch] = acc;
    }
}
// dq (into dqkv's q third): dqs[d] = scale * sum_e ctx[d][e] dout[p][e]; dq = sq * (dqs - sum_d sq dqs)
__global__ __launch_bounds__(256) void t_la_dq(const float* ctx, const float* sq, const float* dout, int hw, float scale, float* dqkv) {
    const int n = blockIdx.y, ch = threadIdx.x & (RHID - 1), half = threadIdx.x >> 7, h = ch / RD, j = ch % RD;
    const int p0 = blockIdx.x * LA_PCHUNK, p1 = min(hw, p0 + LA_PCHUNK);
    const float* c = ctx + (size_t)(n * RH + h) * RD * RD;
    float row[RD];
#pragma unroll
    for (int e2 = 0; e2 < RD; ++e2) row[e2] = scale * c[j * RD + e2];
    for (int p = p0 + half; p < p1; p += 2) {
        const size_t pix = (size_t)n * hw + p;
        const float4* g4 = (const float4*)(dout + pix * RHID + h * RD);
        float dqs = 0.0f;
#pragma unroll
        for (int q = 0; q < RD / 4; ++q) {
            const float4 v = g4[q];
            dqs = fmaf(row[4 * q], v.x, fmaf(row[4 * q + 1], v.y, fmaf(row[4 * q + 2], v.z, fmaf(row[4 * q + 3], v.w, dqs))));
        }
        const float sv = sq[pix * RHID + ch];
        float inner = sv * dqs;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) inner += __shfl_xor(inner, o, 32);
        dqkv[pix * 3 * RHID + ch] = sv * (dqs - inner);
    }
}
// v third: dv[p][e] = (1/hw) sum_d dctx[d][e] sk[p][d];  k third (raw): dks[p][d] = (1/hw) sum_e dctx[d][e] v[p][e]
__global__ __launch_bounds__(256) void t_la_dkv(const float* dctx, const float* sk, const float* qkv, int hw, float* dqkv) {
    const int n = blockIdx.y, ch = threadIdx.x & (RHID - 1), half = threadIdx.x >> 7, h = ch / RD, j = ch % RD;
    const int p0 = blockIdx.x * LA_PCHUNK, p1 = min(hw, p0 + LA_PCHUNK);
    const float* dc = dctx + (size_t)(n * RH + h) * RD * RD;
    const float inv = 1.0f / (float)hw;
    float col[RD], row[RD];
#pragma unroll
    for (int t = 0; t < RD; ++t) {
        col[t] = inv * dc[t * RD + j];  // e = j, d = t
        row[t] = inv * dc[j * RD + t];  // d = j, e = t
    }
    for (int p = p0 + half; p < p1; p += 2) {
        const size_t pix = (size_t)n * hw + p;
        const float4* s4 = (const float4*)(sk + pix * RHID + h * RD);
        const float4* v4 = (const float4*)(qkv + pix * 3 * RHID + 2 * RHID + h * RD);
        float av = 0.0f, ak = 0.0f;
#pragma unroll
        for (int q = 0; q < RD / 4; ++q) {
            const float4 a = s4[q], b = v4[q];
            av = fmaf(col[4 * q], a.x, fmaf(col[4 * q + 1], a.y, fmaf(col[4 * q + 2], a.z, fmaf(col[4 * q + 3], a.w, av))));
            ak = fmaf(row[4 * q], b.x, fmaf(row[4 * q + 1], b.y, fmaf(row[4 * q + 2], b.z, fmaf(row[4 * q + 3], b.w, ak))));
        }
        dqkv[pix * 3 * RHID + 2 * RHID + ch] = av;
        dqkv[pix * 3 * RHID + RHID + ch] = ak;
    }
}
// R[n][ch] = sum_p sk[p][ch] * dks[p][ch]: chunk sums over coalesced rows (fp64), merged in chunk order
__global__ __launch_bounds__(256) void t_la_kred_part(const float* sk, const float* dqkv, int hw, double* part) {
    __shared__ double red[RHID];
    const int n = blockIdx.y, ck = blockIdx.x, ch = threadIdx.x & (RHID - 1), half = threadIdx.x >> 7;
    const int p0 = ck * LA_PCHUNK, p1 = min(hw, p0 + LA_PCHUNK);
    double a = 0.0;
    for (int p = p0 + half; p < p1; p += 2)
        a += (double)sk[((size_t)n * hw + p) * RHID + ch] * dqkv[((size_t)n * hw + p) * 3 * RHID + RHID + ch];
    if (half) red[ch] = a;
    __syncthreads();
    if (!half) part[((size_t)n * gridDim.x + ck) * RHID + ch] = a + red[ch];
}
__global__ void t_la_kred_finish(const double* part, int nchunk, int count, float* R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (sample, channel)
    if (i >= count) return;
    const int n = i / RHID, ch = i % RHID;
    double a = 0.0;
    for (int ck = 0; ck < nchunk; ++ck) a += part[((size_t)n * nchunk + ck) * RHID + ch];
    R[i] = (float)a;
}
__global__ void t_la_dk(const float* sk, const float* R, int hw, long long total, float* dqkv) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % RHID);
    const long long p = i / RHID;
    const int n = (int)(p / hw);
    float* d = dqkv + (size_t)p * 3 * RHID + RHID + ch;
    *d = sk[i] * (*d - R[n * RHID + ch]);
}

// ---- Attention core (attention.py:62-72): P = softmax_j(scale q_i . k_j), dropout on P, out_i = sum_j P_ij v_j.
// One thread per (sample, head, query); P (n, h, N, N) is kept for the backward.  Dropout element index inside the row's stream:
// (h * N + i) * N + j (the sampling path's, AttnArgs::drop).
__global__ void t_at_fwd(const float* qkv, int N, long long rows, float scale, RDrop dr, float* P, float* out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int i = (int)(r % N), h = (int)((r / N) % RH), n = (int)(r / ((long long)N * RH));
    const float* base = qkv + (size_t)n * N * 3 * RHID + h * RD;
    float q[RD];
    for (int d = 0; d < RD; ++d) q[d] = base[(size_t)i * 3 * RHID + d] * scale;
    float* Pr = P + (size_t)r * N;
    float m = -INFINITY;
    for (int j = 0; j < N; ++j) {
        const float* k = base + (size_t)j * 3 * RHID + RHID;
        float s = 0.0f;
        for (int d = 0; d < RD; ++d) s = fmaf(q[d], k[d], s);
        Pr[j] = s;
        m = fmaxf(m, s);
    }
    float sum = 0.0f;
    for (int j = 0; j < N; ++j) {
        const float ex = expf(Pr[j] - m);
        Pr[j] = ex;
        sum += ex;
    }
    float o[RD];
    for (int d = 0; d < RD; ++d) o[d] = 0.0f;
    const float inv = 1.0f / sum;
    for (int j = 0; j < N; ++j) {
        const float pj = Pr[j] * inv;
        Pr[j] = pj;
        const float pd = pj * r_keep(dr, n, (uint32_t)(((size_t)h * N + i) * N + j));
        const float* v = base + (size_t)j * 3 * RHID + 2 * RHID;
        for (int d = 0; d < RD; ++d) o[d] = fmaf(pd, v[d], o[d]);
    }
    for (int d = 0; d < RD; ++d) out[((size_t)n * N + i) * RHID + h * RD + d] = o[d];
}

// ---- the same core, streaming (a sampling forward of more than 4096 tokens: nothing of size N^2 is written).  Online softmax on the
// fp32 matrix cores (mfma_f32_32x32x2f32: an exact k-ordered fp32 fma chain).  One wave per 32 queries, AS_NW waves per workgroup share
// every 32-key K / V tile through LDS (double-buffered; the next tile's global loads fly under the current tile's MFMAs).
//   S^T = K Q^T   16 MFMAs: A = K[key = l&31][d], B = Q[query = l&31][d] (16 registers, loaded once, pre-scaled as t_at_fwd does);
//                 k-step s of lane half hi = l>>5 is channel d = 16 hi + s, so a lane's K fragment is 64 contiguous bytes of its key's
//                 row (4 ds_read_b128; rows padded to 36 floats: the 16-lane groups of a b128 read then cover the 16 slots once).
//   A lane owns query column l&31; accumulator r is key kr(r) = (r&3) + 8 (r>>2) + 4 hi.  Row max: in-lane + one exchange with the lane
//   32 away.  The row sum stays a per-lane partial (both halves share the max) and is joined once after the last tile.
//   O^T = V^T P^T 16 MFMAs: B = the S^T accumulators as they are (k-step r carries keys kr(r) of both halves), A = V[kr(r)][d = l&31]
//                 (ds_read_b32 along a row: 32 banks).  O^T accumulator r is channel kr(r) of the lane's query.
// Dropout is on the normalised probability: keep * scale multiplies p in P V only, never the running sum.  Element index and generator
// are t_at_fwd's (r_keep, one keep word per element: a pair of an odd N straddles two queries, so nothing is shared across elements).
// Keys >= N score -inf (p = 0 exactly) and their V rows are staged as zeros; tile 0 always holds key 0, so the running max is finite
// from the first tile on and (-inf) - (-inf) never occurs.
typedef __attribute__((ext_vector_type(16))) float as_f32x16;
constexpr int AT_KEEP_P_MAX = 4096;    // most tokens t_at_fwd keeps its (tokens x tokens) probabilities for (the training step's limit)
constexpr int AT_STREAM_MAX = 32767;   // most tokens of the streaming core: 4 N^2 <= 2^32 - 1, the dropout element index is uint32_t
constexpr int AS_NW = 4;    // waves per workgroup: 128 queries
constexpr int AS_KS = 36;   // floats per K row in LDS
static_assert(AS_NW * 64 == 32 * (RD / 4), "one float4 of K and one of V per thread stage a 32-key tile");
__device__ __forceinline__ int as_key(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
// LSE (a recorded forward past the kept-probabilities limit): also writes the query's softmax statistics (m, 1 / l) to lse (n, h, N, 2), all
// the streaming backward keeps besides out.  (The pair, not the log-sum-exp m + log l: at scores of 50 one ulp of that sum is 4e-6, a common
// factor on the whole row of P = exp(s - L) that dq = sum_j dS_ij k_j amplifies by |k| / spread(k) -- 1e-5 on the "rising" draw of the
// tests; exp(s - m) / l is the forward's own normalisation.)  The sampling instantiation (LSE = false) computes what it always did.
template <bool DROP, bool LSE>
__global__ __launch_bounds__(64 * AS_NW) void t_at_stream_fwd(const float* __restrict__ qkv, int N, float scale, RDrop dr, float* __restrict__ out,
                                                              float* __restrict__ lse) {
    __shared__ __attribute__((aligned(16))) float Ks[2][32 * AS_KS];
    __shared__ __attribute__((aligned(16))) float Vs[2][32 * RD];
    const int tid = threadIdx.x, l = tid & 63, lq = l & 31, hi = l >> 5;
    const int h = blockIdx.y, n = blockIdx.z;
    const int q0 = ((int)blockIdx.x * AS_NW + (tid >> 6)) * 32;
    const bool active = q0 < N;  // wave-uniform: a wave past the last query only helps staging
    const int qi = q0 + lq, qc = qi < N ? qi : N - 1;
    const float* base = qkv + (size_t)n * N * 3 * RHID + h * RD;
    float qf[16];
    {
        const float4* qp = (const float4*)(base + (size_t)qc * 3 * RHID + 16 * hi);
        for (int c = 0; c < 4; ++c) {
            const float4 v = qp[c];
            qf[4 * c] = v.x * scale; qf[4 * c + 1] = v.y * scale; qf[4 * c + 2] = v.z * scale; qf[4 * c + 3] = v.w * scale;
        }
    }
    // staging: thread -> (key tid>>3, channels 4 (tid&7) ..+3) of the tile
    const int sk = tid >> 3, sc = (tid & 7) * 4;
    float4 kreg, vreg;
    auto fetch = [&](int kt) {
        const int j = kt + sk;
        kreg = vreg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < N) {
            const float* p = base + (size_t)j * 3 * RHID + sc;
            kreg = *(const float4*)(p + RHID);
            vreg = *(const float4*)(p + 2 * RHID);
        }
    };
    auto stage = [&](int b) {
        *(float4*)(&Ks[b][sk * AS_KS + sc]) = kreg;
        *(float4*)(&Vs[b][sk * RD + sc]) = vreg;
    };
    as_f32x16 o;
    for (int r = 0; r < 16; ++r) o[r] = 0.0f;
    float m = -INFINITY, lsum = 0.0f;
    const uint32_t ebase = ((uint32_t)h * (uint32_t)N + (uint32_t)qc) * (uint32_t)N;
    const int tiles = (N + 31) / 32;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int t = 0; t < tiles; ++t) {
        const int b = t & 1, kt = t * 32;
        if (t + 1 < tiles) fetch(kt + 32);
        if (active) {
            as_f32x16 s;
            for (int r = 0; r < 16; ++r) s[r] = 0.0f;
            const float4* kp = (const float4*)(&Ks[b][lq * AS_KS + 16 * hi]);
            for (int c = 0; c < 4; ++c) {
                const float4 kv = kp[c];
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, qf[4 * c], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, qf[4 * c + 1], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, qf[4 * c + 2], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, qf[4 * c + 3], s, 0, 0, 0);
            }
            if (kt + 32 > N)  // the ragged last tile
                for (int r = 0; r < 16; ++r)
                    if (kt + as_key(r, hi) >= N) s[r] = -INFINITY;
            float mx = s[0];
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            float mn = fmaxf(m, mx);
            if (mn == -INFINITY) mn = 0.0f;
            const float alpha = __expf(m - mn);
            m = mn;
            float ps = 0.0f;
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(s[r] - mn);
                s[r] = p;
                ps += p;
            }
            lsum = lsum * alpha + ps;
            for (int r = 0; r < 16; ++r) o[r] *= alpha;
            if (DROP)
                for (int r = 0; r < 16; ++r) {
                    const int j = kt + as_key(r, hi);
                    s[r] = j < N ? s[r] * r_keep(dr, n, ebase + (uint32_t)j) : 0.0f;
                }
            const float* vp = &Vs[b][lq];
            for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[as_key(r, hi) * RD], s[r], o, 0, 0, 0);
        }
        if (t + 1 < tiles) stage(b ^ 1);
        __syncthreads();
    }
    if (!active || qi >= N) return;
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / lsum;
    if constexpr (LSE) {
        if (hi == 0) ((float2*)lse)[((size_t)n * RH + h) * N + qi] = make_float2(m, inv);
    }
    float* op = out + ((size_t)n * N + qi) * RHID + h * RD + 4 * hi;
    for (int g = 0; g < 4; ++g) *(float4*)(op + 8 * g) = make_float4(o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv);
}
// the launch of the streaming core; d.on / d.mask select the dropout instantiation
// (lse: where a recorded forward keeps its softmax statistics; null = sampling)
static inline void launch_t_at_stream_fwd(const float* qkv, int nb, int N, float scale, const RDrop& d, float* out, hipStream_t st, float* lse = nullptr) {
    dyf_form_note("t_at_stream_fwd", nb);
    const dim3 grid((unsigned)((N + 32 * AS_NW - 1) / (32 * AS_NW)), RH, (unsigned)nb);
    const bool dropping = d.on || d.mask;
    if (lse) {
        if (dropping) hipLaunchKernelGGL((t_at_stream_fwd<true, true>), grid, dim3(64 * AS_NW), 0, st, qkv, N, scale, d, out, lse);
        else hipLaunchKernelGGL((t_at_stream_fwd<false, true>), grid, dim3(64 * AS_NW), 0, st, qkv, N, scale, d, out, lse);
    } else if (dropping) hipLaunchKernelGGL((t_at_stream_fwd<true, false>), grid, dim3(64 * AS_NW), 0, st, qkv, N, scale, d, out, lse);
    else hipLaunchKernelGGL((t_at_stream_fwd<false, false>), grid, dim3(64 * AS_NW), 0, st, qkv, N, scale, d, out, lse);
}

// ---- the streaming backward (a recorded forward that took t_at_stream_fwd<.., LSE>): the scores are recomputed per 32 x 32 tile on the
// same fma chain as the forward, P = exp(s - m) / l with the saved statistics, and
//   dP_ij = keep_ij (dout_i . v_j)        D_i = sum_j P_ij dP_ij                dS_ij = P_ij (dP_ij - D_i)
//   dq_i = scale sum_j dS_ij k_j          dk_j = scale sum_i dS_ij q_i          dv_j = sum_i P_ij keep_ij dout_i
// D is summed from the recomputed P and dP in a first sweep over the keys, not taken as dout_i . out_i: equal in exact arithmetic, but in
// fp32 the rounding of out leaves noise of 1e-7 |dout| |out| in dS where it is exactly 0 (one key: P = 1, dS = 0, as t_at_bwd_row gives
// it).  keep enters as a select and the dropout scale 1 / (1 - p) multiplies the finished sums, so dP - D is one subtraction of two values
// the kernels compute alike (D counts without the scale).
// Nothing of size N^2 is written and there are no atomics: a wave owns its 32 output rows, so the gradients are bitwise repeatable.
// Two kernels with the forward's lane maps (accumulator r of a lane is row as_key(r, hi), the lane's column is l & 31) and staging:
//   t_at_stream_bwd_dq   one wave per 32 queries: Q (pre-scaled), dout, (m, 1 / l) in registers; K / V tiles through double-buffered LDS, twice.
//                        S^T = K Q^T and dP^T = V dout^T leave a lane with its query's column: the first sweep sums D (a per-lane partial,
//                        joined with the lane 32 away as the forward joins its row sum) and writes it (n, h, N); in the second the dS^T
//                        accumulators are the B operand of dq^T = K^T dS^T (A = K[as_key(r, hi)][d = l & 31], a column read of the tile).
//   t_at_stream_bwd_dkv  the mirror image, one wave per 32 keys: K, V in registers; Q (pre-scaled at staging as the forward pre-scales it:
//                        dk then needs no final scale), dout, (m, 1 / l), D tiles through LDS.  S = Q K^T and dP = dout V^T leave a lane with its
//                        key's column; P keep and dS are the B operands of dv^T = dout^T (P keep) and dk^T = Q^T dS.
// Rows of a staged tile past N are zeros and their P / dS are set to exactly 0; waves past the last query / key only help staging.
// Dropout: r_keep on element (h N + i) N + j of the row's stream, as the forward (never evaluated past N: an injected mask ends there).
template <bool DROP>
__global__ __launch_bounds__(64 * AS_NW) void t_at_stream_bwd_dq(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse, int N,
                                                                 float scale, RDrop dr, float* __restrict__ Dm, float* __restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) float Ks[2][32 * AS_KS];
    __shared__ __attribute__((aligned(16))) float Vs[2][32 * AS_KS];
    const int tid = threadIdx.x, l = tid & 63, lq = l & 31, hi = l >> 5;
    const int h = blockIdx.y, n = blockIdx.z;
    const int q0 = ((int)blockIdx.x * AS_NW + (tid >> 6)) * 32;
    const bool active = q0 < N;
    const int qi = q0 + lq, qc = qi < N ? qi : N - 1;
    const float* base = qkv + (size_t)n * N * 3 * RHID + h * RD;
    float qf[16], gf[16];
    {
        const float4* qp = (const float4*)(base + (size_t)qc * 3 * RHID + 16 * hi);
        const float4* gp = (const float4*)(dout + ((size_t)n * N + qc) * RHID + h * RD + 16 * hi);
        for (int c = 0; c < 4; ++c) {
            const float4 v = qp[c], g = gp[c];
            qf[4 * c] = v.x * scale; qf[4 * c + 1] = v.y * scale; qf[4 * c + 2] = v.z * scale; qf[4 * c + 3] = v.w * scale;
            gf[4 * c] = g.x; gf[4 * c + 1] = g.y; gf[4 * c + 2] = g.z; gf[4 * c + 3] = g.w;
        }
    }
    const size_t stat = ((size_t)n * RH + h) * N + qc;
    const float2 mil = ((const float2*)lse)[stat];  // (m, 1 / l) of the lane's query
    float Dq = 0.0f;
    const int sk = tid >> 3, sc = (tid & 7) * 4;
    float4 kreg, vreg;
    auto fetch = [&](int kt) {
        const int j = kt + sk;
        kreg = vreg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < N) {
            const float* p = base + (size_t)j * 3 * RHID + sc;
            kreg = *(const float4*)(p + RHID);
            vreg = *(const float4*)(p + 2 * RHID);
        }
    };
    auto stage = [&](int b) {
        *(float4*)(&Ks[b][sk * AS_KS + sc]) = kreg;
        *(float4*)(&Vs[b][sk * AS_KS + sc]) = vreg;
    };
    as_f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const uint32_t ebase = ((uint32_t)h * (uint32_t)N + (uint32_t)qc) * (uint32_t)N;
    const int tiles = (N + 31) / 32;
    for (int sweep = 0; sweep < 2; ++sweep) {  // 0: D, 1: dq (the last barrier of sweep 0 frees buffer 0 for the first stage of sweep 1)
        float dpart = 0.0f;
        fetch(0);
        stage(0);
        __syncthreads();
        for (int t = 0; t < tiles; ++t) {
            const int b = t & 1, kt = t * 32;
            if (t + 1 < tiles) fetch(kt + 32);
            if (active) {
                as_f32x16 s, dp;
                for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.0f;
                const float4* kp = (const float4*)(&Ks[b][lq * AS_KS + 16 * hi]);
                const float4* vp = (const float4*)(&Vs[b][lq * AS_KS + 16 * hi]);
                for (int c = 0; c < 4; ++c) {
                    const float4 kv = kp[c];
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, qf[4 * c], s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, qf[4 * c + 1], s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, qf[4 * c + 2], s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, qf[4 * c + 3], s, 0, 0, 0);
                    const float4 vv = vp[c];
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.x, gf[4 * c], dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.y, gf[4 * c + 1], dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.z, gf[4 * c + 2], dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.w, gf[4 * c + 3], dp, 0, 0, 0);
                }
                for (int r = 0; r < 16; ++r) {
                    const int j = kt + as_key(r, hi);
                    const bool valid = j < N;  // a key past N: P = 0 exactly
                    bool keep = valid;
                    if (DROP) keep = valid && r_keep(dr, n, ebase + (uint32_t)j) != 0.0f;
                    const float p = valid ? __expf(s[r] - mil.x) * mil.y : 0.0f, g = keep ? dp[r] : 0.0f;
                    if (sweep == 0) dpart = fmaf(p, g, dpart);
                    else s[r] = p * (g - Dq);
                }
                if (sweep == 1) {
                    const float* kc = &Ks[b][lq];
                    for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[as_key(r, hi) * AS_KS], s[r], acc, 0, 0, 0);
                }
            }
            if (t + 1 < tiles) stage(b ^ 1);
            __syncthreads();
        }
        if (sweep == 0) {
            Dq = dpart + __shfl_xor(dpart, 32, 64);  // (a + b = b + a: both halves hold the same bits)
            if (active && hi == 0 && qi < N) Dm[stat] = Dq;
        }
    }
    if (!active || qi >= N) return;
    const float so = DROP ? scale * dr.scale : scale;
    float* op = dqkv + ((size_t)n * N + qi) * 3 * RHID + h * RD + 4 * hi;
    for (int g = 0; g < 4; ++g) *(float4*)(op + 8 * g) = make_float4(acc[4 * g] * so, acc[4 * g + 1] * so, acc[4 * g + 2] * so, acc[4 * g + 3] * so);
}
template <bool DROP>
__global__ __launch_bounds__(64 * AS_NW) void t_at_stream_bwd_dkv(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                                  const float* __restrict__ Dm, int N, float scale, RDrop dr, float* __restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) float Qs[2][32 * AS_KS];
    __shared__ __attribute__((aligned(16))) float Gs[2][32 * AS_KS];
    __shared__ float Ss[2][3][32];  // per query of the tile: m, 1 / l, D
    const int tid = threadIdx.x, l = tid & 63, lq = l & 31, hi = l >> 5;
    const int h = blockIdx.y, n = blockIdx.z;
    const int k0 = ((int)blockIdx.x * AS_NW + (tid >> 6)) * 32;
    const bool active = k0 < N;
    const int kj = k0 + lq, kc = kj < N ? kj : N - 1;
    const float* base = qkv + (size_t)n * N * 3 * RHID + h * RD;
    const float* gbase = dout + (size_t)n * N * RHID + h * RD;
    const size_t srow = ((size_t)n * RH + h) * N;
    float kf[16], vf[16];
    {
        const float4* kp = (const float4*)(base + (size_t)kc * 3 * RHID + RHID + 16 * hi);
        const float4* vp = (const float4*)(base + (size_t)kc * 3 * RHID + 2 * RHID + 16 * hi);
        for (int c = 0; c < 4; ++c) {
            const float4 k = kp[c], v = vp[c];
            kf[4 * c] = k.x; kf[4 * c + 1] = k.y; kf[4 * c + 2] = k.z; kf[4 * c + 3] = k.w;
            vf[4 * c] = v.x; vf[4 * c + 1] = v.y; vf[4 * c + 2] = v.z; vf[4 * c + 3] = v.w;
        }
    }
    // staging: thread -> (query tid>>3, channels 4 (tid&7) ..+3) of the tile; threads 0..31 its m, 32..63 its 1 / l, 64..95 its D
    const int sq = tid >> 3, sc = (tid & 7) * 4;
    float4 qreg, greg;
    float sreg = 0.0f;
    auto fetch = [&](int qt) {
        const int i = qt + sq;
        qreg = greg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < N) {
            const float4 v = *(const float4*)(base + (size_t)i * 3 * RHID + sc);
            qreg = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
            greg = *(const float4*)(gbase + (size_t)i * RHID + sc);
        }
        if (tid < 96) {
            const int ii = qt + (tid & 31);
            sreg = ii >= N ? 0.0f : tid < 64 ? lse[2 * (srow + ii) + (tid >> 5)] : Dm[srow + ii];
        }
    };
    auto stage = [&](int b) {
        *(float4*)(&Qs[b][sq * AS_KS + sc]) = qreg;
        *(float4*)(&Gs[b][sq * AS_KS + sc]) = greg;
        if (tid < 96) Ss[b][tid >> 5][tid & 31] = sreg;
    };
    as_f32x16 dk, dv;
    for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.0f;
    const int tiles = (N + 31) / 32;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int t = 0; t < tiles; ++t) {
        const int b = t & 1, qt = t * 32;
        if (t + 1 < tiles) fetch(qt + 32);
        if (active) {
            as_f32x16 s, dp;
            for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.0f;
            const float4* qp = (const float4*)(&Qs[b][lq * AS_KS + 16 * hi]);
            const float4* gp = (const float4*)(&Gs[b][lq * AS_KS + 16 * hi]);
            for (int c = 0; c < 4; ++c) {
                const float4 qv = qp[c];
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.x, kf[4 * c], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.y, kf[4 * c + 1], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.z, kf[4 * c + 2], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.w, kf[4 * c + 3], s, 0, 0, 0);
                const float4 gv = gp[c];
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(gv.x, vf[4 * c], dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(gv.y, vf[4 * c + 1], dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(gv.z, vf[4 * c + 2], dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(gv.w, vf[4 * c + 3], dp, 0, 0, 0);
            }
            for (int r = 0; r < 16; ++r) {
                const int ir = as_key(r, hi), i = qt + ir;
                const bool valid = i < N;  // a query past N: P = 0 exactly
                bool keep = valid;
                if (DROP) keep = valid && r_keep(dr, n, ((uint32_t)h * (uint32_t)N + (uint32_t)i) * (uint32_t)N + (uint32_t)kc) != 0.0f;
                const float p = valid ? __expf(s[r] - Ss[b][0][ir]) * Ss[b][1][ir] : 0.0f, g = keep ? dp[r] : 0.0f;
                s[r] = keep ? p : 0.0f;
                dp[r] = p * (g - Ss[b][2][ir]);
            }
            const float *gc = &Gs[b][lq], *qc = &Qs[b][lq];
            for (int r = 0; r < 16; ++r) {
                dv = __builtin_amdgcn_mfma_f32_32x32x2f32(gc[as_key(r, hi) * AS_KS], s[r], dv, 0, 0, 0);
                dk = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[as_key(r, hi) * AS_KS], dp[r], dk, 0, 0, 0);
            }
        }
        if (t + 1 < tiles) stage(b ^ 1);
        __syncthreads();
    }
    if (!active || kj >= N) return;
    const float so = DROP ? dr.scale : 1.0f;
    float* op = dqkv + ((size_t)n * N + kj) * 3 * RHID + RHID + h * RD + 4 * hi;
    for (int g = 0; g < 4; ++g) {
        *(float4*)(op + 8 * g) = make_float4(dk[4 * g] * so, dk[4 * g + 1] * so, dk[4 * g + 2] * so, dk[4 * g + 3] * so);
        *(float4*)(op + RHID + 8 * g) = make_float4(dv[4 * g] * so, dv[4 * g + 1] * so, dv[4 * g + 2] * so, dv[4 * g + 3] * so);
    }
}
// the two launches of the streaming backward: D (n, h, N) is written by the first and read by the second (one stream orders them)
static inline void launch_t_at_stream_bwd(const float* qkv, const float* dout, const float* lse, int nb, int N, float scale,
                                          const RDrop& d, float* Dm, float* dqkv, hipStream_t st) {
    dyf_form_note("t_at_stream_bwd_dq", nb);
    dyf_form_note("t_at_stream_bwd_dkv", nb);
    const dim3 grid((unsigned)((N + 32 * AS_NW - 1) / (32 * AS_NW)), RH, (unsigned)nb);
    if (d.on || d.mask) {
        hipLaunchKernelGGL(t_at_stream_bwd_dq<true>, grid, dim3(64 * AS_NW), 0, st, qkv, dout, lse, N, scale, d, Dm, dqkv);
        hipLaunchKernelGGL(t_at_stream_bwd_dkv<true>, grid, dim3(64 * AS_NW), 0, st, qkv, dout, lse, Dm, N, scale, d, dqkv);
    } else {
        hipLaunchKernelGGL(t_at_stream_bwd_dq<false>, grid, dim3(64 * AS_NW), 0, st, qkv, dout, lse, N, scale, d, Dm, dqkv);
        hipLaunchKernelGGL(t_at_stream_bwd_dkv<false>, grid, dim3(64 * AS_NW), 0, st, qkv, dout, lse, Dm, N, scale, d, dqkv);
    }
}
// row pass of the backward: dS (n, h, N, N) = P * (dP - sum_j P dP), dP_ij = keep_ij * (dout_i . v_j); dq_i = scale * sum_j dS_ij k_j
__global__ void t_at_bwd_row(const float* qkv, const float* P, const float* dout, int N, long long rows, float scale, RDrop dr, float* dS,
                             float* dqkv) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int i = (int)(r % N), h = (int)((r / N) % RH), n = (int)(r / ((long long)N * RH));
    const float* base = qkv + (size_t)n * N * 3 * RHID + h * RD;
    const float* Pr = P + (size_t)r * N;
    float* Sr = dS + (size_t)r * N;
    float go[RD];
    for (int d = 0; d < RD; ++d) go[d] = dout[((size_t)n * N + i) * RHID + h * RD + d];
    float inner = 0.0f;
    for (int j = 0; j < N; ++j) {
        const float* v = base + (size_t)j * 3 * RHID + 2 * RHID;
        float a = 0.0f;
        for (int d = 0; d < RD; ++d) a = fmaf(go[d], v[d], a);
        a *= r_keep(dr, n, (uint32_t)(((size_t)h * N + i) * N + j));
        Sr[j] = a;
        inner = fmaf(Pr[j], a, inner);
    }
    float dq[RD];
    for (int d = 0; d < RD; ++d) dq[d] = 0.0f;
    for (int j = 0; j < N; ++j) {
        const float ds = Pr[j] * (Sr[j] - inner);
        Sr[j] = ds;
        const float* k = base + (size_t)j * 3 * RHID + RHID;
        for (int d = 0; d < RD; ++d) dq[d] = fmaf(ds, k[d], dq[d]);
    }
    for (int d = 0; d < RD; ++d) dqkv[((size_t)n * N + i) * 3 * RHID + h * RD + d] = scale * dq[d];
}
// column pass: dk_j = scale * sum_i dS_ij q_i;  dv_j = sum_i P_ij keep_ij dout_i
__global__ void t_at_bwd_col(const float* qkv, const float* P, const float* dS, const float* dout, int N, long long rows, float scale, RDrop dr,
                             float* dqkv) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int j = (int)(r % N), h = (int)((r / N) % RH), n = (int)(r / ((long long)N * RH));
    const float* base = qkv + (size_t)n * N * 3 * RHID + h * RD;
    float dk[RD], dv[RD];
    for (int d = 0; d < RD; ++d) dk[d] = dv[d] = 0.0f;
    for (int i = 0; i < N; ++i) {
        const size_t e = ((size_t)(n * RH + h) * N + i) * N + j;
        const float ds = dS[e], pd = P[e] * r_keep(dr, n, (uint32_t)(((size_t)h * N + i) * N + j));
        const float* q = base + (size_t)i * 3 * RHID;
        const float* go = dout + ((size_t)n * N + i) * RHID + h * RD;
        for (int d = 0; d < RD; ++d) {
            dk[d] = fmaf(ds, q[d], dk[d]);
            dv[d] = fmaf(pd, go[d], dv[d]);
        }
    }
    for (int d = 0; d < RD; ++d) {
        dqkv[((size_t)n * N + j) * 3 * RHID + RHID + h * RD + d] = scale * dk[d];
        dqkv[((size_t)n * N + j) * 3 * RHID + 2 * RHID + h * RD + d] = dv[d];
    }
}

// nn.Upsample(scale_factor=2, mode="nearest") (unet.py:16-19) and its adjoint (accumulating)
__global__ void t_up2n_fwd(const float* in, int n, int h, int w, int C, float* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * 4 * h * w * C) return;
    const int c = (int)(i % C);
    const long long px = i / C;
    const int x = (int)(px % (2 * w)), y = (int)((px / (2 * w)) % (2 * h)), b = (int)(px / ((long long)4 * h * w));
    out[i] = in[(((size_t)b * h + y / 2) * w + x / 2) * C + c];
}
__global__ void t_up2n_bwd(const float* dout, int n, int h, int w, int C, float* din) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * h * w * C) return;
    const int c = (int)(i % C);
    const long long px = i / C;
    const int x = (int)(px % w), y = (int)((px / w) % h), b = (int)(px / ((long long)h * w));
    const float* d = dout + (((size_t)b * 2 * h + 2 * y) * 2 * w + 2 * x) * C + c;
    din[i] += d[0] + d[C] + d[(size_t)2 * w * C] + d[(size_t)2 * w * C + C];
}
template <int V>
__global__ __launch_bounds__(256) void t_sum2(const float* a, const float* b, long long n, float* out) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (V == 4 && i + 3 < n) {
        const float4 x = *(const float4*)(a + i), y = *(const float4*)(b + i);
        *(float4*)(out + i) = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
        return;
    }
    for (int k = 0; k < V; ++k)
        if (i + k < n) out[i + k] = a[i + k] + b[i + k];
}
inline void launch_t_sum2(const float* a, const float* b, long long n, float* out, hipStream_t st) {
    if (t_vec4_ok(0, a, b, out)) hipLaunchKernelGGL(t_sum2<4>, dim3(nblk((n + 3) / 4)), dim3(256), 0, st, a, b, n, out);
    else hipLaunchKernelGGL(t_sum2<1>, dim3(nblk(n)), dim3(256), 0, st, a, b, n, out);
}
// da += d[..., :ca], db += d[..., ca:]
__global__ void t_split2_acc(const float* d, int ca, int cb, long long pixels, float* da, float* db) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int C = ca + cb;
    if (i >= pixels * C) return;
    const int c = (int)(i % C);
    const long long p = i / C;
    if (c < ca) da[p * ca + c] += d[i];
    else db[p * cb + (c - ca)] += d[i];
}
// [co][tap][ci] -> (co, ci, tap): PyTorch's conv-weight layout (gradient export)
__global__ void t_unpack_conv(const float* g, int cout, int cin, int taps, float* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)cout * cin * taps) return;
    const int tp = (int)(i % taps), ci = (int)((i / taps) % cin), co = (int)(i / ((long long)taps * cin));
    out[i] = g[((size_t)co * taps + tp) * cin + ci];
}
// [co][taps][ci] -> [taps][ci][co]
__global__ void t_w_transpose(const float* w, int cout, int K, float* wt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)cout * K) return;
    const int co = (int)(i / K), k = (int)(i % K);
    wt[(size_t)k * cout + co] = w[i];
}

// ------------------------------------------------------------------------------------------------ the recording context
struct RCtx {
    dyf_engine* e;
    dyf::TrainNet& W;
    dyf::RTape& T;
    const dyf_net_config& c;
    hipStream_t st;
    int nb;
    bool drop_on, param_grads = true;
    bool want_dinputs = false;           // the backward's caller asked for the gradient of the network input
    int site = 0;
    double* sums = nullptr;              // the (S | Q) sums of the norm whose statistics are being taken (stat_sums), reused op after op
    size_t sums_cap = 0, sums_hint = 0;  // (sums_hint: the largest request the walk expects, so that the block is taken once)
    double* norm_bwd = nullptr;          // the sums of the norm adjoint that is running (A | B | Cc | Dd | S1 | S2): one block per backward,
    size_t norm_bwd_doubles = 0;         // sized for the largest norm the forward recorded
    std::vector<void*>* tmp = nullptr;   // backward temporaries (gradients of activations), freed when the backward is done
    dyf_status err = DYF_OK;
    FwdMem mem{};                        // where the forward's tensors come from: the tape's blocks, or the sampling arena
    const uint8_t* const* masks = nullptr;  // sampling, dropout mode 2: one keep mask per site with p > 0, in execution order
    // an op's adjoint: kept only by a recorded forward
    template <typename F>
    void back(F&& f) { if (mem.recording()) T.back.push_back(std::forward<F>(f)); }

    // DYF_TRAIN_DEBUG=1: synchronise after every recorded op and report the first failing one (debugging aid)
    dyf::RT* dbg(dyf::RT* y, const char* what) {
        const bool on = dyf_form_int("DYF_TRAIN_DEBUG", 0) != 0;
        if (on) {
            const hipError_t se = hipDeviceSynchronize();
            fprintf(stderr, "train op %-10s -> %zu floats: %s\n", what, y ? y->n : (size_t)0, hipGetErrorString(se));
        }
        return y;
    }
    dyf::RT* make(size_t n) {
        T.ts.emplace_back();
        dyf::RT* t = &T.ts.back();
        t->n = n;
        if (mem.get(&t->p, n) != DYF_OK) err = DYF_ERR_HIP;
        return t;
    }
    float* fbuf(size_t n, bool zero = false) {  // forward-lifetime scratch kept for the backward
        float* p = nullptr;
        if (mem.get(&p, n, zero) != DYF_OK) err = DYF_ERR_HIP;
        return p;
    }
    float* grad(dyf::RT* t) {  // gradient buffer of an activation (zero on first use)
        if (!t->g && talloc(e, *tmp, &t->g, t->n, true) != DYF_OK) err = DYF_ERR_HIP;
        return t->g;
    }
    // gradient contribution dx (a fresh scratch buffer of t->n floats that nobody else keeps) to activation t: the FIRST contribution
    // becomes the gradient buffer itself (no memset, no add), later ones are added
    void accum(dyf::RT* t, float* dx) {
        if (!t->g) { t->g = dx; return; }
        launch_t_add(t->g, dx, (long long)t->n, st);
    }
    float* tbuf(size_t n, bool zero = false) {
        float* p = nullptr;
        if (talloc(e, *tmp, &p, n, zero) != DYF_OK) err = DYF_ERR_HIP;
        return p;
    }
    // does anything upstream of t take a gradient?  (the network input and what is resampled from it: only when the caller asked)
    bool wants(const dyf::RT* t) const { return t->need == 0 || (t->need == 1 && want_dinputs); }
    // deterministic mode: pixels per workgroup of a norm's sum kernels -- the caller's rule, more where the slabs (slab_doubles each)
    // of all pixel ranges would not fit the workspace
    static int det_norm_ppb(int hw, int ppb, size_t slab_doubles) {
        const long long max_slabs = std::max<long long>(1, (long long)(TRAIN_SPLITK_FLOATS / 2 / slab_doubles));
        return (int)std::max<long long>(ppb, (hw + max_slabs - 1) / max_slabs);
    }
    // the adjoint of a resample: the scatter with atomics, or (deterministic mode) the gather
    void resize_bwd(const float* dout, int h, int w, int C, int oh, int ow, int nearest, float* din) {
        if (train_det()) {
            dyf_form_note("t_resize_bwd:det", nb);
            hipLaunchKernelGGL(t_resize_bwd_gather, dim3(nblk((long long)nb * h * w * C)), dim3(256), 0, st, dout, nb, h, w, C, oh, ow, nearest, din);
        } else {
            dyf_form_note("t_resize_bwd:atomic", nb);
            hipLaunchKernelGGL(t_resize_bwd, dim3(nblk((long long)nb * oh * ow * C)), dim3(256), 0, st, dout, nb, h, w, C, oh, ow, nearest, din);
        }
    }
    double* stat_sums(size_t n) {  // n zeroed doubles; one stream orders the reuse (the statistics are final before the next norm's memset)
        if (n > sums_cap) {
            sums_cap = std::max(n, sums_hint);
            if (mem.get(&sums, sums_cap) != DYF_OK) err = DYF_ERR_HIP;
        }
        if (sums && hipMemsetAsync(sums, 0, n * sizeof(double), st) != hipSuccess) err = DYF_ERR_HIP;
        return sums;
    }
    dyf::RParam& P(const std::string& k) { return W.P.at(k); }
    // salt_site: the generator's site number when it is not the execution order (unet_simple: block i is site i, dropout_input site 12)
    RDrop drop(float p, size_t per, int salt_site = -1) {
        RDrop d{};
        if (p <= 0.0f) return d;            // p = 0 layers draw nothing and consume no site (as the sampling path's DropCtx)
        const int s = site++;
        if (masks) {                        // injected: the caller's mask of this site
            d.scale = 1.0f / (1.0f - p);
            d.mask = masks[s];
            d.per = (uint32_t)per;
            return d;
        }
        if (!drop_on) return d;
        d.on = 1;
        d.scale = 1.0f / (1.0f - p);
        d.thresh16 = keep_threshold16(p);
        d.salt = rng_layer_salt((uint32_t)(salt_site >= 0 ? salt_site : s));
        d.row_keys = T.row_keys;
        return d;
    }

    // ---- conv (+ bias), optionally weight-standardised: x (nb, h, w, cin) -> (nb, ho, wo, cout)
    dyf::RT* conv(dyf::RT* x, int h, int w, int cin, int cout, int k, int s, int p, const std::string& name, bool has_bias, bool ws) {
        const int ho = (h + 2 * p - k) / s + 1, wo = (w + 2 * p - k) / s + 1;
        const TConv g{nb, h, w, cin, ho, wo, cout, k, s, p};
        dyf::RParam& pw = P(name + ".weight");
        dyf::RParam* pb = has_bias ? &P(name + ".bias") : nullptr;
        const int K = k * k * cin;
        float *wh = pw.w, *wht = pw.wt, *rstd = nullptr;
        if (ws) {
            wh = fbuf((size_t)cout * K);
            wht = fbuf((size_t)cout * K);
            rstd = fbuf(cout);
            hipLaunchKernelGGL(t_ws_fwd, dim3(cout), dim3(256), 0, st, pw.w, K, cin, cout, wh, wht, rstd);
        }
        dyf::RT* y = make((size_t)nb * ho * wo * cout);
        if (conv_fwd(e, g, x->p, wht, pb ? pb->w : nullptr, y->p, st) != DYF_OK) err = DYF_ERR_HIP;
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;  // nothing downstream needed this output
            dyf::RParam& qw = P(name + ".weight");
            if (param_grads) {
                float* gb = has_bias ? P(name + ".bias").g : nullptr;
                if (ws) {
                    float* dwh = tbuf((size_t)cout * K, true);
                    dyf_status r = conv_wgrad(e, g, y->g, x->p, dwh, gb, st);
                    if (r != DYF_OK) return r;
                    hipLaunchKernelGGL(t_ws_bwd, dim3(cout), dim3(256), 0, st, dwh, wh, rstd, K, qw.g);
                } else {
                    dyf_status r = conv_wgrad(e, g, y->g, x->p, qw.g, gb, st);
                    if (r != DYF_OK) return r;
                }
            }
            if (wants(x)) {
                float* dx = tbuf(x->n);
                dyf_status r = conv_dgrad(e, g, y->g, wh, nullptr, dx, st);
                if (r != DYF_OK) return r;
                accum(x, dx);
            }
            return DYF_OK;
        });
        return dbg(y, "conv");
    }

    // ---- normalisation + FiLM + activation + Dropout: GroupNorm + SiLU of unet.Block (unet.py:58-76), BatchNorm2d / GroupNorm(8) +
    // (Leaky)ReLU of UNetBlock (unet_simple.py:13-82).  kind 0: BatchNorm on batch statistics (updates name.running_mean / .running_var,
    // momentum 0.1), 1: BatchNorm on the running statistics (no sums are taken), 2: GroupNorm(G).  ss (nb, 2C) = (scale | shift) or null.
    // ppb_rec: pixels per workgroup of the sum kernels of a RECORDED forward, the caller's rule (norm_ppb_*); a sampling forward takes ONE
    // workgroup per sample -- every sum meets its zero-filled slot once, no order of atomics to depend on.
    // res: SimpleConvNet's residual (simple_conv_net.py:52-54), y = keep * act(..) + res in the same launch; the adjoint hands y's gradient on to it
    dyf::RT* norm_act(dyf::RT* z, int hw, int C, const std::string& name, dyf::RT* ss, float p_drop, int kind, int G, int act, int ppb_rec,
                      int salt_site = -1, dyf::RT* res = nullptr) {
        const int gn = kind == 2 ? 1 : 0, nidx = gn ? nb * G : C;
        float *mean = fbuf(nidx), *rstd = fbuf(nidx);
        const int ppb = mem.recording() ? ppb_rec : hw;
        double *S = nullptr, *Q = nullptr;
        if (kind != 1) {
            S = stat_sums((size_t)nb * C * 2);
            Q = S + (size_t)nb * C;
            if (train_det()) {  // slabs of (S | Q) per pixel range, added in range order
                double* ws = (double*)splitk_ws(e);
                const int dppb = det_norm_ppb(hw, ppb, (size_t)nb * C * 2);
                const int slabs = (hw + dppb - 1) / dppb;
                if (!ws) err = DYF_ERR_STATE;
                dyf_form_note("t_nc_sums:det", nb);
                if (ws && slabs > 1) {
                    hipLaunchKernelGGL(t_nc_sums<true>, dim3(slabs, nb), dim3(256), 0, st, z->p, hw, C, dppb, ws, ws + (size_t)nb * C);
                    det_reduce(ws, slabs, (long long)nb * C * 2, (long long)nb * C * 2, S, st);
                } else if (ws) {
                    hipLaunchKernelGGL(t_nc_sums<true>, dim3(1, nb), dim3(256), 0, st, z->p, hw, C, dppb, S, Q);
                }
            } else {
                dyf_form_note("t_nc_sums:atomic", nb);
                hipLaunchKernelGGL(t_nc_sums<false>, dim3((hw + ppb - 1) / ppb, nb), dim3(256), 0, st, z->p, hw, C, ppb, S, Q);
            }
        }
        hipLaunchKernelGGL(t_stats_finalize, dim3(nblk(std::max(nidx, C))), dim3(256), 0, st, kind, S, Q, nb, hw, C, G,
                           gn ? (float*)nullptr : P(name + ".running_mean").w, gn ? (float*)nullptr : P(name + ".running_var").w, mean, rstd);
        const RDrop d = drop(p_drop, (size_t)hw * C, salt_site);
        const TNorm a{nb, hw, C, G, gn, act, mean, rstd, P(name + ".weight").w, P(name + ".bias").w, ss ? ss->p : nullptr, d.on, d.scale,
                      d.thresh16, d.salt, d.row_keys, d.mask};
        dyf::RT* y = make(z->n);
        launch_t_norm_fwd(a, z->p, y->p, st, res ? res->p : nullptr);
        const size_t nS = ((size_t)std::max(nidx, C) + 3) / 4 * 4;  // floats of S1 and of S2 (16-byte aligned behind the doubles)
        norm_bwd_doubles = std::max(norm_bwd_doubles, (size_t)nb * C * 4 + nS);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            if (!norm_bwd && talloc(e, *tmp, &norm_bwd, norm_bwd_doubles, false) != DYF_OK) return DYF_ERR_HIP;
            double *A = norm_bwd, *B = A + (size_t)nb * C, *Cc = A + (size_t)2 * nb * C, *Dd = A + (size_t)3 * nb * C;
            if (hipMemsetAsync(A, 0, (size_t)nb * C * 4 * sizeof(double), st) != hipSuccess) return DYF_ERR_HIP;
            float *S1 = (float*)(A + (size_t)nb * C * 4), *S2 = S1 + nS;
            float* dss = ss ? tbuf((size_t)nb * 2 * C) : nullptr;
            const bool gelu = a.act == ACT_GELU;  // the instantiations with its derivative
            if (train_det()) {  // (as the forward's sums)
                double* ws = (double*)splitk_ws(e);
                const size_t nC = (size_t)nb * C;
                const int dppb = det_norm_ppb(hw, ppb, nC * 4);
                const int slabs = (hw + dppb - 1) / dppb;
                if (!ws) return DYF_ERR_STATE;
                dyf_form_note("t_norm_bwd_sums:det", nb);
                auto* kern = gelu ? t_norm_bwd_sums<true, true> : t_norm_bwd_sums<true, false>;
                if (slabs > 1) {
                    hipLaunchKernelGGL(kern, dim3(slabs, nb), dim3(256), 0, st, a, z->p, y->g, dppb, ws, ws + nC, ws + 2 * nC, ws + 3 * nC);
                    det_reduce(ws, slabs, (long long)nC * 4, (long long)nC * 4, A, st);
                } else {
                    hipLaunchKernelGGL(kern, dim3(1, nb), dim3(256), 0, st, a, z->p, y->g, dppb, A, B, Cc, Dd);
                }
            } else {
                dyf_form_note("t_norm_bwd_sums:atomic", nb);
                auto* kern = gelu ? t_norm_bwd_sums<false, true> : t_norm_bwd_sums<false, false>;
                hipLaunchKernelGGL(kern, dim3((hw + ppb - 1) / ppb, nb), dim3(256), 0, st, a, z->p, y->g, ppb, A, B, Cc, Dd);
            }
            // (running statistics: the norm is a fixed affine map, S1 = S2 = 0)
            hipLaunchKernelGGL(t_norm_bwd_combine, dim3(nblk(std::max(nb * C, nb * G))), dim3(256), 0, st, a, A, B, Cc, Dd,
                               param_grads ? P(name + ".weight").g : (float*)nullptr, param_grads ? P(name + ".bias").g : (float*)nullptr, dss, S1, S2,
                               kind != 1 ? 1 : 0);
            float* dz = tbuf(z->n);
            launch_t_norm_bwd_apply(a, z->p, y->g, S1, S2, gn ? 1.0f / ((float)hw * (C / G)) : 1.0f / ((float)nb * hw), dz, st);
            accum(z, dz);
            if (ss) accum(ss, dss);
            // y's gradient reaches the residual unchanged, and y is done with it: the buffer itself becomes (the first contribution to) res's gradient
            if (res && wants(res)) accum(res, y->g);
            return DYF_OK;
        });
        return dbg(y, "norm_act");
    }

    // ---- y (rows, O) = Linear(f(x (rows, K))), f = SiLU when pre (FiLM heads: mlp = Sequential(SiLU, Linear), unet.py:93).
    // shared_silu: x is the alias silu_shared made; the adjoint adds its d silu(x) into x's gradient (zero on first use) and leaves silu' to it
    dyf::RT* linear(dyf::RT* x, int rows, int K, int O, const std::string& name, int pre, bool shared_silu = false) {
        dyf::RT* y = make((size_t)rows * O);
        hipLaunchKernelGGL(t_linear_fwd, dim3((unsigned)((O + 3) / 4), (unsigned)((rows + 15) / 16)), dim3(256), 0, st, x->p, P(name + ".weight").w, P(name + ".bias").w, rows, K, O, pre, y->p);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            if (param_grads)
                hipLaunchKernelGGL(t_linear_bwd_w, dim3(nblk((long long)O * K)), dim3(256), 0, st, x->p, y->g, rows, K, O, pre, P(name + ".weight").g,
                                   P(name + ".bias").g);
            if (!wants(x)) return DYF_OK;
            float* dx = shared_silu ? grad(x) : tbuf(x->n);
            hipLaunchKernelGGL(t_linear_bwd_x, dim3((unsigned)(rows * ((K + 15) / 16))), dim3(256), 0, st, x->p, P(name + ".weight").w, y->g, rows, K, O,
                               shared_silu ? 0 : pre, shared_silu ? 1 : 0, dx);
            if (!shared_silu) accum(x, dx);
            return DYF_OK;
        });
        return dbg(y, "linear");
    }
    // ---- SiLU(x) feeding several `linear(.., pre = 1, shared_silu)` heads (the 12 FiLM heads of unet_simple, unet_simple.py:29,66): an alias
    // of x -- the heads apply the SiLU themselves -- whose gradient collects d silu(x) head by head; silu' is applied once, here.  x leads
    // to parameters only (the time MLP), so without parameter gradients nothing is launched.
    dyf::RT* silu_shared(dyf::RT* x) {
        T.ts.emplace_back();
        dyf::RT* y = &T.ts.back();
        y->p = x->p;
        y->n = x->n;
        back([=]() -> dyf_status {
            if (!y->g || !param_grads) return DYF_OK;
            float* dx = tbuf(x->n);
            hipLaunchKernelGGL(t_silu_bwd, dim3(nblk((long long)x->n)), dim3(256), 0, st, x->p, y->g, (long long)x->n, dx);
            accum(x, dx);
            return DYF_OK;
        });
        return y;
    }
    // ---- LearnedSinusoidalPosEmb features (rows, 2 half + 1) of the time values; the frequencies are a parameter
    dyf::RT* learned_sinu(const float* time_dev, int half) {
        dyf::RT* y = make((size_t)nb * (2 * half + 1));
        const std::string name = "time_emb_mlp.0.weights";
        hipLaunchKernelGGL(t_learned_sinu_fwd, dim3(nblk((long long)nb * (2 * half + 1))), dim3(256), 0, st, time_dev, P(name).w, nb, half, y->p);
        back([=]() -> dyf_status {
            if (!y->g || !param_grads) return DYF_OK;
            hipLaunchKernelGGL(t_learned_sinu_bwd, dim3(1), dim3(256), 0, st, time_dev, P(name).w, y->g, nb, half, P(name).g);
            return DYF_OK;
        });
        return dbg(y, "learned_sinu");
    }
    // ---- Dropout over a whole tensor (dropout_input / dropout_input_for_residual, unet.py:276-277); per = elements of one sample
    // in_place (unet_simple's dropout_input on the stem's output, unet_simple.py:116,168): x is overwritten and returned -- its producer must
    // not need its own output for its adjoint (a conv does not) -- and the adjoint maps x's gradient where it lies
    dyf::RT* dropout(dyf::RT* x, long long per, float p, bool in_place = false, int salt_site = -1) {
        const RDrop d = drop(p, (size_t)per, salt_site);
        if (!d.on && !d.mask) return x;
        dyf::RT* y = in_place ? x : make(x->n);
        if (d.mask) hipLaunchKernelGGL(t_mask_map, dim3(nblk((long long)x->n)), dim3(256), 0, st, x->p, y->p, (long long)x->n, d.scale, d.mask);
        else hipLaunchKernelGGL(t_dropout_map, dim3(nblk((long long)x->n)), dim3(256), 0, st, x->p, y->p, nb, per, d.scale, d.thresh16, d.salt, d.row_keys);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            float* dx = in_place ? y->g : tbuf(x->n);  // the adjoint is the same keep map on the gradient
            hipLaunchKernelGGL(t_dropout_map, dim3(nblk((long long)x->n)), dim3(256), 0, st, y->g, dx, nb, per, d.scale, d.thresh16, d.salt, d.row_keys);
            if (!in_place) accum(x, dx);
            return DYF_OK;
        });
        return dbg(y, "dropout");
    }
    // ---- torch.cat of up to three NCHW sources on the channel axis -> NHWC
    dyf::RT* inputs(const Source* src, int hw, int cin) {
        dyf::RT* y = make((size_t)nb * hw * cin);
        hipLaunchKernelGGL(t_nchw_cat_to_nhwc, dim3(nblk((long long)nb * hw * cin)), dim3(256), 0, st, src[0].p, src[0].ch, src[1].p, src[1].ch, src[2].p,
                           src[2].ch, nb, hw, y->p);
        y->need = 1;
        return dbg(y, "inputs");
    }
    // ---- per-row time values: the caller's, or one value for the whole batch (a sampling plan's step)
    const float* times(const float* time_dev, float value) {
        if (time_dev) return time_dev;
        float* tv = fbuf(nb);
        hipLaunchKernelGGL(t_fill, dim3(nblk(nb)), dim3(256), 0, st, value, nb, tv);
        return tv;
    }
    dyf::RT* sinusoid(const float* time_dev, int dim) {
        dyf::RT* y = make((size_t)nb * dim);
        hipLaunchKernelGGL(t_sinusoid, dim3(nblk(nb * dim)), dim3(256), 0, st, time_dev, nb, dim, y->p);
        y->need = 2;  // a function of the time values alone
        return dbg(y, "sinusoid");
    }
    dyf::RT* gelu(dyf::RT* x) {
        dyf::RT* y = make(x->n);
        hipLaunchKernelGGL(t_gelu_fwd, dim3(nblk((long long)x->n)), dim3(256), 0, st, x->p, (long long)x->n, y->p);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            hipLaunchKernelGGL(t_gelu_bwd, dim3(nblk((long long)x->n)), dim3(256), 0, st, x->p, (long long)x->n, y->g);  // in place: y is done with it
            accum(x, y->g);
            return DYF_OK;
        });
        return dbg(y, "gelu");
    }
    dyf::RT* add(dyf::RT* a, dyf::RT* b) {
        dyf::RT* y = make(a->n);
        launch_t_sum2(a->p, b->p, (long long)a->n, y->p, st);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            // y's gradient goes to both inputs: b gets a copy / an add first, then a may take the buffer over (y is done with it)
            if (b->g) {
                launch_t_add(b->g, y->g, (long long)b->n, st);
            } else {
                float* db = tbuf(b->n);
                if (hipMemcpyAsync(db, y->g, b->n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return DYF_ERR_HIP;
                b->g = db;
            }
            if (a != b) accum(a, y->g);
            else launch_t_add(a->g, y->g, (long long)a->n, st);
            return DYF_OK;
        });
        return dbg(y, "add");
    }
    dyf::RT* cat(dyf::RT* a, int ca, dyf::RT* b, int cb, long long pixels) {
        if ((long long)a->n != pixels * ca || (long long)b->n != pixels * cb) {
            fprintf(stderr, "dyffusion train: cat size mismatch: a %zu vs %lld x %d, b %zu vs %lld x %d\n", a->n, pixels, ca, b->n, pixels, cb);
            err = DYF_ERR_INVALID_ARGUMENT;
            return make((size_t)pixels * (ca + cb));
        }
        dyf::RT* y = make((size_t)pixels * (ca + cb));
        launch_t_concat2(a->p, ca, b->p, cb, pixels, y->p, st);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            hipLaunchKernelGGL(t_split2_acc, dim3(nblk(pixels * (ca + cb))), dim3(256), 0, st, y->g, ca, cb, pixels, grad(a), grad(b));
            return DYF_OK;
        });
        return dbg(y, "cat");
    }
    dyf::RT* up2_nearest(dyf::RT* x, int h, int w, int C) {
        dyf::RT* y = make(x->n * 4);
        hipLaunchKernelGGL(t_up2n_fwd, dim3(nblk((long long)y->n)), dim3(256), 0, st, x->p, nb, h, w, C, y->p);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            hipLaunchKernelGGL(t_up2n_bwd, dim3(nblk((long long)x->n)), dim3(256), 0, st, y->g, nb, h, w, C, grad(x));
            return DYF_OK;
        });
        return dbg(y, "up2_nearest");
    }
    // ---- x2 bilinear upsample (align_corners=False) in front of a decoder conv (unet_simple.py:50-52) of x (nb, h, w, ca) or, with x2
    // (nb, h, w, cb), of a torch.cat([x, x2]) (:176-177) that is never written: the gather reads both parts and its adjoint writes the two
    // gradients, no concat tensor and no split pass.  Channel counts that are no multiples of 4 and target sizes other than (2h, 2w) take the
    // general resample, on the concatenation made by `cat`.
    dyf::RT* up2_bilinear(dyf::RT* x, int ca, dyf::RT* x2, int cb, int h, int w, int oh, int ow) {
        const int C = ca + (x2 ? cb : 0);
        const bool up2 = C % 4 == 0 && oh == 2 * h && ow == 2 * w;
        if (x->n != (size_t)nb * h * w * ca || (x2 && x2->n != (size_t)nb * h * w * cb)) {  // (a skip of another plane: never read past it)
            err = DYF_ERR_INVALID_ARGUMENT;
            return make((size_t)nb * oh * ow * C);
        }
        if (x2 && !(up2 && ca % 4 == 0 && cb % 4 == 0)) {
            x = cat(x, ca, x2, cb, (long long)nb * h * w);
            x2 = nullptr;
        }
        const int Ca4 = x2 ? ca / 4 : C / 4;
        dyf::RT* y = make((size_t)nb * oh * ow * C);
        if (up2) hipLaunchKernelGGL(t_up2x_fwd, dim3(nblk((long long)nb * oh * ow * (C / 4))), dim3(256), 0, st, x->p, nb, h, w, C / 4, y->p, Ca4, x2 ? x2->p : (const float*)nullptr);
        else hipLaunchKernelGGL(t_resize_fwd, dim3(nblk((long long)y->n)), dim3(256), 0, st, x->p, nb, h, w, C, oh, ow, 0, y->p);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            if (!up2) {
                resize_bwd(y->g, h, w, C, oh, ow, 0, grad(x));
                return DYF_OK;
            }
            float *dx = tbuf(x->n), *dx2 = x2 ? tbuf(x2->n) : nullptr;  // the kernel writes every element of both
            hipLaunchKernelGGL(t_up2x_bwd, dim3(nblk((long long)nb * h * w * (C / 4))), dim3(256), 0, st, y->g, nb, h, w, C / 4, dx, Ca4, dx2);
            accum(x, dx);
            if (x2) accum(x2, dx2);
            return DYF_OK;
        });
        return dbg(y, "up2_bilinear");
    }
    // ---- F.interpolate(size=(oh, ow)), bilinear (align_corners=False) or nearest: unet_simple's outer resample; the identity when the sizes match
    dyf::RT* resize(dyf::RT* x, int h, int w, int C, int oh, int ow, int nearest) {
        if (h == oh && w == ow) return x;
        dyf::RT* y = make((size_t)nb * oh * ow * C);
        y->need = x->need;
        hipLaunchKernelGGL(t_resize_fwd, dim3(nblk((long long)y->n)), dim3(256), 0, st, x->p, nb, h, w, C, oh, ow, nearest, y->p);
        back([=]() -> dyf_status {
            if (!y->g || !wants(x)) return DYF_OK;
            resize_bwd(y->g, h, w, C, oh, ow, nearest, grad(x));
            return DYF_OK;
        });
        return dbg(y, "resize");
    }
    // ---- ConvTranspose2d(cin -> C, 4, stride 2, pad 1), unet_simple's readout (unet_simple.py:136), as the DATA GRADIENT of the conv C -> cin
    // (4 x 4 / 2 / 1) whose [cin][tap][C] weight the packed (cin, C, 4, 4) tensor is; the adjoint is that conv's weight gradient with x in the
    // place of dz, and its forward (the transposed pack) for the gradient of x
    dyf::RT* conv_transpose4s2(dyf::RT* x, int h, int w, int cin, int C, const std::string& name) {
        const TConv g{nb, 2 * h, 2 * w, C, h, w, cin, 4, 2, 1};
        dyf::RT* y = make((size_t)nb * 4 * h * w * C);
        if (conv_dgrad(e, g, x->p, P(name + ".weight").w, P(name + ".bias").w, y->p, st) != DYF_OK) err = DYF_ERR_HIP;
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            dyf::RParam& qw = P(name + ".weight");
            if (param_grads) {
                dyf_status r = conv_wgrad(e, g, x->p, y->g, qw.g, nullptr, st);
                if (r != DYF_OK) return r;
                r = launch_bias_grad(e, y->g, (long long)nb * 4 * h * w, C, P(name + ".bias").g, st);
                if (r != DYF_OK) return r;
            }
            if (!wants(x)) return DYF_OK;
            float* dx = tbuf(x->n);
            dyf_status r = conv_fwd(e, g, y->g, qw.wt, nullptr, dx, st);
            if (r != DYF_OK) return r;
            accum(x, dx);
            return DYF_OK;
        });
        return dbg(y, "conv_transpose4s2");
    }
    dyf::RT* layernorm(dyf::RT* x, int hw, int C, const std::string& gname, float p_drop) {
        float2* stats = nullptr;
        if (mem.get(&stats, (size_t)nb * hw) != DYF_OK) err = DYF_ERR_HIP;
        const RDrop d = drop(p_drop, (size_t)hw * C);
        dyf::RT* y = make(x->n);
        hipLaunchKernelGGL(t_ln_fwd, dim3(nblk((long long)nb * hw * 16)), dim3(256), 0, st, x->p, P(gname).w, nb, hw, C, d, y->p, stats);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            if (param_grads) {
                if (C <= 256 && 256 % C == 0 && train_det()) {  // slabs of C sums per pixel chunk, added in chunk order
                    float* ws = splitk_ws(e);
                    if (!ws) return DYF_ERR_STATE;
                    const long long total = (long long)nb * hw;
                    const long long slabs0 = std::min<long long>(1024, (total + LN_GCHUNK - 1) / LN_GCHUNK);
                    const int chunk = (int)((total + slabs0 - 1) / slabs0), slabs = (int)((total + chunk - 1) / chunk);
                    dyf_form_note("t_ln_bwd_g_rows:det", nb);
                    hipLaunchKernelGGL(t_ln_bwd_g_slab, dim3((unsigned)slabs), dim3(256), 0, st, x->p, y->g, stats, nb, hw, C, d, chunk, ws);
                    det_reduce(ws, slabs, C, C, P(gname).g, st);
                } else if (C <= 256 && 256 % C == 0) {
                    dyf_form_note("t_ln_bwd_g_rows:atomic", nb);
                    hipLaunchKernelGGL(t_ln_bwd_g_rows, dim3((unsigned)(((long long)nb * hw + LN_GCHUNK - 1) / LN_GCHUNK)), dim3(256), 0, st, x->p, y->g, stats,
                                       nb, hw, C, d, P(gname).g);
                } else {
                    hipLaunchKernelGGL(t_ln_bwd_g, dim3(C), dim3(256), 0, st, x->p, y->g, stats, nb, hw, C, d, P(gname).g);
                }
            }
            hipLaunchKernelGGL(t_ln_bwd_x, dim3(nblk((long long)nb * hw * 16)), dim3(256), 0, st, x->p, P(gname).w, y->g, stats, nb, hw, C, d, grad(x));
            return DYF_OK;
        });
        return dbg(y, "layernorm");
    }
    // LinearAttention core on qkv (nb, hw, 384) -> (nb, hw, 128)
    dyf::RT* linattn(dyf::RT* qkv, int hw) {
        const long long npix = (long long)nb * hw, tot = npix * RHID;
        const float scale = 1.0f / sqrtf((float)RD);
        float *sq = fbuf(tot), *sk = fbuf(tot), *kmax = fbuf((size_t)nb * RHID), *ksum = fbuf((size_t)nb * RHID);
        float* ctx = fbuf((size_t)nb * RH * RD * RD);
        const int pchunks = (hw + LA_PCHUNK - 1) / LA_PCHUNK;
        float2* kpart = (float2*)fbuf((size_t)2 * nb * pchunks * RHID);
        hipLaunchKernelGGL(t_la_qsoft, dim3(nblk(tot)), dim3(256), 0, st, qkv->p, npix, sq);
        hipLaunchKernelGGL(t_la_kstat_part, dim3(pchunks, nb), dim3(256), 0, st, qkv->p, hw, kpart);
        hipLaunchKernelGGL(t_la_kstat_finish, dim3(nblk((long long)nb * RHID)), dim3(256), 0, st, kpart, pchunks, nb * RHID, kmax, ksum);
        hipLaunchKernelGGL(t_la_ksoft, dim3(nblk(tot)), dim3(256), 0, st, qkv->p, hw, tot, kmax, ksum, sk);
        // ctx[d][e] = sum_p sk[p][d] * v[p][e] / hw   (v = v / (h w), attention.py:48)
        const int nsplit = (hw + LA_CHUNK - 1) / LA_CHUNK;
        const long long mcount = (long long)nb * RH * RD * RD;
        double* part = (double*)fbuf((size_t)2 * nsplit * mcount);  // split partials of both outer products (forward, then backward)
        hipLaunchKernelGGL(t_la_outer_part, dim3(RH, nb, nsplit), dim3(256), 0, st, sk, RHID, qkv->p + 2 * RHID, 3 * RHID, hw, part);
        hipLaunchKernelGGL(t_la_outer_finish, dim3(nblk(mcount)), dim3(256), 0, st, part, nsplit, mcount, 1.0f / (float)hw, ctx);
        dyf::RT* y = make(tot);
        hipLaunchKernelGGL(t_la_out, dim3(pchunks, nb), dim3(256), 0, st, ctx, sq, hw, scale, y->p);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            float* dctx = tbuf((size_t)nb * RH * RD * RD);
            float* dq = tbuf(qkv->n);
            float* R = tbuf((size_t)nb * RHID);
            // dctx[d][e] = scale * sum_p sq[p][d] * dout[p][e]
            hipLaunchKernelGGL(t_la_outer_part, dim3(RH, nb, nsplit), dim3(256), 0, st, sq, RHID, y->g, RHID, hw, part);
            hipLaunchKernelGGL(t_la_outer_finish, dim3(nblk(mcount)), dim3(256), 0, st, part, nsplit, mcount, scale, dctx);
            double* rpart = (double*)tbuf((size_t)2 * nb * pchunks * RHID);
            hipLaunchKernelGGL(t_la_dq, dim3(pchunks, nb), dim3(256), 0, st, ctx, sq, y->g, hw, scale, dq);
            hipLaunchKernelGGL(t_la_dkv, dim3(pchunks, nb), dim3(256), 0, st, dctx, sk, qkv->p, hw, dq);
            hipLaunchKernelGGL(t_la_kred_part, dim3(pchunks, nb), dim3(256), 0, st, sk, dq, hw, rpart);
            hipLaunchKernelGGL(t_la_kred_finish, dim3(nblk((long long)nb * RHID)), dim3(256), 0, st, rpart, pchunks, nb * RHID, R);
            hipLaunchKernelGGL(t_la_dk, dim3(nblk(tot)), dim3(256), 0, st, sk, R, hw, tot, dq);
            accum(qkv, dq);
            return DYF_OK;
        });
        return dbg(y, "linattn");
    }
    // Attention core on qkv (nb, N, 384) -> (nb, N, 128), dropout on the probabilities
    // A recorded forward of N >= DYF_TRAIN_ATTN_STREAM_MIN tokens (kernel-form switch, default AT_KEEP_P_MAX + 1; `streaming`: the op seam's
    // ATTENTION_STREAM) keeps the softmax statistics (m, 1 / l) per (row, head, token) instead of the probabilities and records the streaming adjoint.
    dyf::RT* attention(dyf::RT* qkv, int N, float p_drop, bool streaming = false) {
        const long long rows = (long long)nb * RH * N;
        const float scale = 1.0f / sqrtf((float)RD);
        if (!mem.recording() && N > AT_KEEP_P_MAX) {  // sampling past the kept-probabilities limit: the streaming core, no P, no adjoint
            const RDrop d = drop(p_drop, (size_t)RH * N * N);
            dyf::RT* y = make((size_t)nb * N * RHID);
            launch_t_at_stream_fwd(qkv->p, nb, N, scale, d, y->p, st);
            return dbg(y, "attention");
        }
        const long long stream_min = dyf_form_int("DYF_TRAIN_ATTN_STREAM_MIN", AT_KEEP_P_MAX + 1);
        if (mem.recording() && (streaming || N > AT_KEEP_P_MAX || N >= stream_min)) {
            float* L = fbuf((size_t)2 * rows);
            const RDrop d = drop(p_drop, (size_t)RH * N * N);
            dyf::RT* y = make((size_t)nb * N * RHID);
            launch_t_at_stream_fwd(qkv->p, nb, N, scale, d, y->p, st, L);
            back([=]() -> dyf_status {
                if (!y->g) return DYF_OK;
                float* D = tbuf((size_t)rows);
                float* dq = tbuf(qkv->n);  // both kernels together write every element
                if (err != DYF_OK) return err;
                launch_t_at_stream_bwd(qkv->p, y->g, L, nb, N, scale, d, D, dq, st);
                accum(qkv, dq);
                return DYF_OK;
            });
            return dbg(y, "attention");
        }
        dyf_form_note("t_at_fwd", nb);
        float* Pm = fbuf((size_t)rows * N);
        const RDrop d = drop(p_drop, (size_t)RH * N * N);
        dyf::RT* y = make((size_t)nb * N * RHID);
        hipLaunchKernelGGL(t_at_fwd, dim3(nblk(rows, 64)), dim3(64), 0, st, qkv->p, N, rows, scale, d, Pm, y->p);
        back([=]() -> dyf_status {
            if (!y->g) return DYF_OK;
            float* dS = tbuf((size_t)rows * N);
            float* dq = tbuf(qkv->n);
            hipLaunchKernelGGL(t_at_bwd_row, dim3(nblk(rows, 64)), dim3(64), 0, st, qkv->p, Pm, y->g, N, rows, scale, d, dS, dq);
            hipLaunchKernelGGL(t_at_bwd_col, dim3(nblk(rows, 64)), dim3(64), 0, st, qkv->p, Pm, dS, y->g, N, rows, scale, d, dq);
            accum(qkv, dq);
            return DYF_OK;
        });
        return dbg(y, "attention");
    }
};

// the layer names of unet.Unet's state_dict in execution order (as unet_resnet.hip's rn_load_weights)
struct RNames {
    std::vector<std::string> blocks, attns;
    std::vector<int> dims, lev_h, lev_w;
    int nlev;
};
RNames rn_names(const dyf_engine* e, const dyf_net_config& c) {
    RNames r;
    r.nlev = c.n_mults;
    r.dims.push_back(c.dim);
    for (int i = 0; i < c.n_mults; ++i) r.dims.push_back(c.dim * c.dim_mults[i]);
    int h = e->cfg.height, w = e->cfg.width;
    for (int l = 0; l < r.nlev; ++l) {
        r.lev_h.push_back(h);
        r.lev_w.push_back(w);
        if (l < r.nlev - 1 && !c.keep_spatial_dims) { h /= 2; w /= 2; }
    }
    return r;
}


// The allocations of RCtx's ops without their launches: what one forward of `nb` rows takes from the sampling arena.  Op by op the
// same make / fbuf / mem.get calls as above, so rn_walk<RCount> sizes the arena that rn_walk<RCtx> then bumps through.
struct RCount {
    const dyf_net_config& c;
    int nb;
    size_t bytes = 0;
    std::deque<dyf::RT> ts;
    void take(size_t n, size_t el = sizeof(float)) { bytes += f32_arena_block(n * el); }
    dyf::RT* make(size_t n) { ts.emplace_back(); ts.back().n = n; take(n); return &ts.back(); }
    dyf::RT* conv(dyf::RT*, int h, int w, int cin, int cout, int k, int s, int p, const std::string&, bool, bool ws) {
        const int ho = (h + 2 * p - k) / s + 1, wo = (w + 2 * p - k) / s + 1;
        if (ws) { take((size_t)cout * k * k * cin); take((size_t)cout * k * k * cin); take(cout); }
        return make((size_t)nb * ho * wo * cout);
    }
    size_t sums_cap = 0, sums_hint = 0;
    dyf::RT* norm_act(dyf::RT* z, int, int C, const std::string&, dyf::RT*, float, int kind, int G, int, int, int = -1, dyf::RT* = nullptr) {
        const size_t nidx = kind == 2 ? (size_t)nb * G : (size_t)C;
        take(nidx); take(nidx);
        if (kind != 1 && (size_t)nb * C * 2 > sums_cap) { sums_cap = std::max((size_t)nb * C * 2, sums_hint); take(sums_cap, sizeof(double)); }
        return make(z->n);
    }
    dyf::RT* linear(dyf::RT*, int rows, int, int O, const std::string&, int, bool = false) { return make((size_t)rows * O); }
    dyf::RT* silu_shared(dyf::RT* x) { return x; }
    dyf::RT* learned_sinu(const float*, int half) { return make((size_t)nb * (2 * half + 1)); }
    dyf::RT* dropout(dyf::RT* x, long long, float p, bool in_place = false, int = -1) { return p > 0.0f && !in_place ? make(x->n) : x; }
    dyf::RT* inputs(const Source*, int hw, int cin) { return make((size_t)nb * hw * cin); }
    const float* times(const float*, float) { take(nb); return nullptr; }
    dyf::RT* sinusoid(const float*, int dim) { return make((size_t)nb * dim); }
    dyf::RT* gelu(dyf::RT* x) { return make(x->n); }
    dyf::RT* add(dyf::RT* a, dyf::RT*) { return make(a->n); }
    dyf::RT* cat(dyf::RT*, int ca, dyf::RT*, int cb, long long pixels) { return make((size_t)pixels * (ca + cb)); }
    dyf::RT* up2_nearest(dyf::RT* x, int, int, int) { return make(x->n * 4); }
    dyf::RT* up2_bilinear(dyf::RT* x, int ca, dyf::RT* x2, int cb, int h, int w, int oh, int ow) {
        const int C = ca + (x2 ? cb : 0);
        if (x2 && !(C % 4 == 0 && oh == 2 * h && ow == 2 * w && ca % 4 == 0 && cb % 4 == 0)) cat(x, ca, x2, cb, (long long)nb * h * w);
        return make((size_t)nb * oh * ow * C);
    }
    dyf::RT* resize(dyf::RT* x, int h, int w, int C, int oh, int ow, int) { return h == oh && w == ow ? x : make((size_t)nb * oh * ow * C); }
    dyf::RT* conv_transpose4s2(dyf::RT*, int h, int w, int, int C, const std::string&) { return make((size_t)nb * 4 * h * w * C); }
    dyf::RT* layernorm(dyf::RT* x, int hw, int, const std::string&, float) { take((size_t)nb * hw, sizeof(float2)); return make(x->n); }
    dyf::RT* linattn(dyf::RT*, int hw) {
        const size_t tot = (size_t)nb * hw * RHID;
        take(tot); take(tot); take((size_t)nb * RHID); take((size_t)nb * RHID); take((size_t)nb * RH * RD * RD);
        take((size_t)2 * nb * ((hw + LA_PCHUNK - 1) / LA_PCHUNK) * RHID);
        take((size_t)2 * ((hw + LA_CHUNK - 1) / LA_CHUNK) * nb * RH * RD * RD * 2);
        return make(tot);
    }
    // (counts a sampling forward: past AT_KEEP_P_MAX the streaming core keeps no P.  A recorded forward takes its blocks from the caching
    // allocator instead: P and dS, or -- the streaming pair -- the softmax statistics (2 nb * 4 * N floats) and the row sums D (nb * 4 * N))
    dyf::RT* attention(dyf::RT*, int N, float) {
        if (N <= AT_KEEP_P_MAX) take((size_t)nb * RH * N * N);
        return make((size_t)nb * N * RHID);
    }
};

// Pixels per workgroup of the norm sums of a RECORDED forward (norm_act's ppb_rec), one rule per backbone.  unet.Unet: about 2 048
// workgroups per launch on its planes (16 pixels each left 14 400 workgroups of 60 x 60 x 64 rows with four fp64 atomics per thread: 104 us
// per backward-sums launch, 10x its traffic time).  unet_simple: at most 256 workgroups per sample.
inline int rn_norm_ppb(int hw, int nb) { return std::max(std::max(16, (hw + 255) / 256), (int)std::min<long long>(128, ((long long)hw * nb + 2047) / 2048)); }
inline int us_norm_ppb(int hw) { return std::max(16, (hw + 255) / 256); }

// The layer walk of unet.Unet.forward (unet.py:262-315), shared by the recorded forward, the sampling forward (both RCtx: they differ
// in where RCtx::mem takes the tensors from) and the sizing of the sampling arena (RCount).  src: up to three NCHW sources in channel
// order (condition first, unet.py:269).  Returns the NHWC output.
template <typename Ctx>
RT* rn_walk(Ctx& X, const dyf_net_config& c, const RNames& R, int nb, int H, int W, int cin_total, const Source* src, const float* time_dev_in,
            float time_value, RT** x_in) {
    const int hw = H * W;
    const int cin = cin_total, dim = c.dim, tdim = 2 * c.dim;
    // ---- inputs: torch.cat((condition, x), 1) (unet.py:269), NCHW -> NHWC
    RT* xin = X.inputs(src, hw, cin);
    *x_in = xin;
    // ---- time embedding: sinusoid -> Linear -> GELU -> Linear (misc.py:54-67)
    RT* temb = nullptr;
    if (c.with_time_emb) {
        const float* time_dev = X.times(time_dev_in, time_value);
        RT* e0 = nullptr;
        int tfeat = dim;
        if (c.learned_sinusoidal_dim > 0) {  // LearnedSinusoidalPosEmb (misc.py:35-51): [t, sin(2 pi t w), cos(2 pi t w)], w learnable
            tfeat = c.learned_sinusoidal_dim + 1;
            e0 = X.learned_sinu(time_dev, c.learned_sinusoidal_dim / 2);
        } else {
            e0 = X.sinusoid(time_dev, dim);
        }
        temb = X.linear(X.gelu(X.linear(e0, nb, tfeat, tdim, "time_emb_mlp.1", 0)), nb, tdim, tdim, "time_emb_mlp.3", 0);
    }
    auto resblock = [&](const std::string& pre, RT* x, int cx, int cout, int hh, int ww) -> RT* {
        RT* ss = temb ? X.linear(temb, nb, tdim, 2 * cout, pre + ".mlp.1", 1) : nullptr;
        const int ppb = rn_norm_ppb(hh * ww, nb);
        RT* h1 = X.norm_act(X.conv(x, hh, ww, cx, cout, 3, 1, 1, pre + ".block1.proj", true, true), hh * ww, cout, pre + ".block1.norm", ss,
                            c.block_dropout1, 2, c.groups, ACT_SILU, ppb);
        RT* h2 = c.single_conv_layer ? h1  // double_conv_layer=False: block2 = Identity
                                     : X.norm_act(X.conv(h1, hh, ww, cout, cout, 3, 1, 1, pre + ".block2.proj", true, true), hh * ww, cout,
                                                  pre + ".block2.norm", nullptr, c.dropout, 2, c.groups, ACT_SILU, ppb);
        RT* res = cx != cout ? X.conv(x, hh, ww, cx, cout, 1, 1, 0, pre + ".residual_conv", true, false) : x;
        return X.add(h2, res);
    };
    auto attn = [&](const std::string& pre, RT* x, int C, int hh, int ww, bool linear) -> RT* {
        RT* ln = X.layernorm(x, hh * ww, C, pre + ".fn.norm.g", linear ? c.attn_dropout : 0.0f);
        RT* qkv = X.conv(ln, hh, ww, C, 3 * RHID, 1, 1, 0, pre + (linear ? ".fn.fn.to_qkv.1" : ".fn.fn.to_qkv"), false, false);
        RT* core = linear ? X.linattn(qkv, hh * ww) : X.attention(qkv, hh * ww, c.attn_dropout);
        return X.add(X.conv(core, hh, ww, RHID, C, 1, 1, 0, pre + ".fn.fn.to_out", true, false), x);
    };
    const int ks = c.init_kernel_size;
    RT* x = X.conv(xin, H, W, cin, dim, ks, 1, c.init_padding, "init_conv", true, false);
    RT* r0 = X.dropout(x, (long long)hw * dim, c.input_dropout);  // dropout_input_for_residual first, then dropout_input
    x = X.dropout(x, (long long)hw * dim, c.input_dropout);
    std::vector<std::pair<RT*, int>> skips;
    for (int l = 0; l < R.nlev; ++l) {
        const int hh = R.lev_h[l], ww = R.lev_w[l], dl = R.dims[l];
        const std::string pre = "downs." + std::to_string(l);
        x = resblock(pre + ".0", x, dl, dl, hh, ww);
        skips.emplace_back(x, dl);
        x = resblock(pre + ".1", x, dl, dl, hh, ww);
        x = attn(pre + ".2", x, dl, hh, ww, true);
        skips.emplace_back(x, dl);
        if (l < R.nlev - 1 && !c.keep_spatial_dims) x = X.conv(x, hh, ww, dl, R.dims[l + 1], 4, 2, 1, pre + ".3", true, false);
        else x = X.conv(x, hh, ww, dl, R.dims[l + 1], 3, 1, 1, pre + ".3", true, false);
    }
    {
        const int hh = R.lev_h.back(), ww = R.lev_w.back(), dm = R.dims[R.nlev];
        x = resblock("mid_block1", x, dm, dm, hh, ww);
        x = attn("mid_attn", x, dm, hh, ww, false);
        x = resblock("mid_block2", x, dm, dm, hh, ww);
    }
    for (int l = R.nlev - 1, u = 0; l >= 0; --l, ++u) {
        const int hh = R.lev_h[l], ww = R.lev_w[l], dout = R.dims[l + 1], din = R.dims[l];
        const std::string pre = "ups." + std::to_string(u);
        auto s1 = skips.back(); skips.pop_back();
        x = resblock(pre + ".0", X.cat(x, dout, s1.first, s1.second, (long long)nb * hh * ww), dout + din, dout, hh, ww);
        auto s2 = skips.back(); skips.pop_back();
        x = resblock(pre + ".1", X.cat(x, dout, s2.first, s2.second, (long long)nb * hh * ww), dout + din, dout, hh, ww);
        x = attn(pre + ".2", x, dout, hh, ww, true);
        if (l > 0 && !c.keep_spatial_dims) x = X.conv(X.up2_nearest(x, hh, ww, dout), 2 * hh, 2 * ww, dout, din, 3, 1, 1, pre + ".3.1", true, false);
        else x = X.conv(x, hh, ww, dout, din, 3, 1, 1, pre + ".3", true, false);
    }
    x = resblock("final_res_block", X.cat(x, dim, r0, dim, (long long)nb * hw), 2 * dim, dim, H, W);
    RT* y = X.conv(x, H, W, dim, c.out_channels, 1, 1, 0, "final_conv", true, false);
    return y;
}

// The layer walk of unet_simple's UNet.forward (unet_simple.py:164-197), used as rn_walk is: cat -> outer resample -> 1x1 stem ->
// dropout_input -> 6 encoder and 6 decoder UNetBlocks (conv -> norm -> FiLM -> activation -> dropout; a decoder block upsamples x2 first, and
// the skip a decoder block's output is concatenated with is left to the next block's upsample) -> ConvTranspose2d readout -> outer resample.
// src: the NCHW sources in channel order.  bn_batch: BatchNorm on batch statistics (module.train()).
template <typename Ctx>
RT* us_walk(Ctx& X, const Net& n, int nb, int H, int W, const Source* src, const float* time_dev_in, float time_value, bool bn_batch, RT** x_in) {
    const dyf_net_config& c = n.cfg;
    RT* film = nullptr;  // SiLU(time embedding), what every block's FiLM head starts from
    if (c.with_time_emb) {
        const float* time_dev = X.times(time_dev_in, time_value);
        RT* e0 = X.sinusoid(time_dev, n.dim);
        film = X.silu_shared(X.linear(X.gelu(X.linear(e0, nb, n.dim, n.tdim, "time_emb_mlp.1", 0)), nb, n.tdim, n.tdim, "time_emb_mlp.3", 0));
    }
    RT* xin = X.inputs(src, H * W, n.cin_total);
    *x_in = xin;
    RT* x = X.conv(X.resize(xin, H, W, n.cin_total, n.uh, n.uw, c.outer_nearest), n.uh, n.uw, n.cin_total, n.dim, 1, 1, 0, "init_conv", true, false);
    x = X.dropout(x, (long long)n.uh * n.uw * n.dim, c.input_dropout, true, (int)DYF_INPUT_DROP_SITE);
    RT *y[12], *skip = nullptr;
    int lh = n.uh, lw = n.uw;
    for (int i = 0; i < 12; ++i) X.sums_hint = std::max(X.sums_hint, (size_t)nb * 2 * n.blk[i].cout);
    for (int i = 0; i < 12; ++i) {
        const UBlock& b = n.blk[i];
        const std::string pre = i < 6 ? "input_ops." + std::to_string(i) : "output_ops." + std::to_string(i - 6);
        const std::string conv = pre + ".ops." + (b.transposed ? "1" : "0"), norm = pre + ".ops." + (b.transposed ? "2" : "1");
        if (b.transposed) x = X.up2_bilinear(x, skip ? n.blk[i - 1].cout : b.cin, skip, skip ? n.blk[11 - i].cout : 0, lh, lw, b.in_h, b.in_w);
        RT* z = X.conv(x, b.in_h, b.in_w, b.cin, b.cout, b.k, b.stride, b.pad, conv, true, false);
        RT* ss = film ? X.linear(film, nb, n.tdim, 2 * b.cout, pre + ".time_mlp.1", 1, true) : nullptr;
        const int ohw = b.out_h * b.out_w;
        x = y[i] = X.norm_act(z, ohw, b.cout, norm, ss, c.dropout, b.gn ? 2 : bn_batch ? 0 : 1, 8, b.act, us_norm_ppb(ohw), i);
        lh = b.out_h; lw = b.out_w;
        skip = i >= 6 && i < 11 ? y[10 - i] : nullptr;  // torch.cat([x, skip]) (:176-177)
    }
    return X.resize(X.conv_transpose4s2(x, lh, lw, n.dim, c.out_channels, "readout.0"), 2 * lh, 2 * lw, c.out_channels, H, W, c.outer_nearest);
}

// The layer walk of SimpleConvNet.forward (simple_conv_net.py:112-131), used as the two above are: cat (inputs, condition) -> per kernel size
// [Conv2d(k, 'same') -> BatchNorm2d -> FiLM -> GELU -> Dropout -> + block input where cin == dim] (:38-55) -> 1 x 1 head.  A block is a conv
// and ONE norm_act (GELU, the residual in the same launch).  Dropout site i = block i with salt rng_layer_salt(i), as sc_forward /
// sc_f32_forward draw them: MC dropout and training share their streams.  Kernel sizes travel in cfg.n_mults / dim_mults.
template <typename Ctx>
RT* sc_walk(Ctx& X, const Net& n, int nb, int H, int W, const Source* src, const float* time_dev_in, float time_value, bool bn_batch, RT** x_in) {
    const dyf_net_config& c = n.cfg;
    const int hw = H * W;
    RT* film = nullptr;  // SiLU(time embedding), what every block's FiLM head starts from
    if (c.with_time_emb) {
        const float* time_dev = X.times(time_dev_in, time_value);
        RT* e0 = X.sinusoid(time_dev, n.dim);
        film = X.silu_shared(X.linear(X.gelu(X.linear(e0, nb, n.dim, n.tdim, "time_emb_mlp.1", 0)), nb, n.tdim, n.tdim, "time_emb_mlp.3", 0));
    }
    RT* x = X.inputs(src, hw, n.cin_total);
    *x_in = x;
    X.sums_hint = std::max(X.sums_hint, (size_t)nb * 2 * n.dim);
    int cin = n.cin_total;
    for (int i = 0; i < c.n_mults; ++i) {
        const int k = c.dim_mults[i];
        const std::string pre = "convs." + std::to_string(i);
        RT* z = X.conv(x, H, W, cin, n.dim, k, 1, (k - 1) / 2, pre + ".conv", true, false);
        RT* ss = film ? X.linear(film, nb, n.tdim, 2 * n.dim, pre + ".time_mlp.1", 1, true) : nullptr;
        x = X.norm_act(z, hw, n.dim, pre + ".norm", ss, c.dropout, bn_batch ? 0 : 1, 8, ACT_GELU, us_norm_ppb(hw), i, cin == n.dim ? x : nullptr);
        cin = n.dim;
    }
    return X.conv(x, H, W, n.dim, c.out_channels, 1, 1, 0, "head", true, false);
}

// ---- the one place that tells the backbones apart: which walk, the order of its sources, what a recorded forward cannot serve
// the training step's sources in the order the backbone concatenates them (unet.Unet: (condition, x), unet.py:269; unet_simple: (x,
// condition), and SimpleConvNet as unet_simple, simple_conv_net.py:121); returns the first channel of `inputs` inside the concatenation
inline int net_sources(const Net& n, const float* inputs_dev, const float* cond_dev, Source src[3]) {
    src[0] = {inputs_dev, n.cfg.in_channels};
    src[1] = {cond_dev, cond_dev ? n.cfg.cond_channels : 0};
    src[2] = {nullptr, 0};
    if (n.rn) std::swap(src[0], src[1]);
    return n.rn ? src[0].ch : 0;
}
// null, or why the net's forward cannot be recorded: past AT_KEEP_P_MAX tokens unet.Unet's bottleneck Attention records the streaming
// pair, whose dropout element index (h N + i) N + j is uint32_t as in sampling (rn_f32_supported)
inline const char* net_record_refusal(const dyf_engine* e, const Net& n) {
    if (!n.rn) return nullptr;
    const RNames R = rn_names(e, n.cfg);
    return (long long)R.lev_h.back() * R.lev_w.back() <= AT_STREAM_MAX
               ? nullptr
               : "training step: the bottleneck Attention indexes its (4 x tokens x tokens) probabilities with 32 bits -- at most 32767 tokens";
}
template <typename Ctx>
RT* net_walk(Ctx& X, const dyf_engine* e, const Net& n, int nb, const Source* src, const float* time_dev, float time_value, bool bn_batch, RT** x_in) {
    const int H = e->cfg.height, W = e->cfg.width;
    if (n.rn) return rn_walk(X, n.cfg, rn_names(e, n.cfg), nb, H, W, n.cin_total, src, time_dev, time_value, x_in);
    if (n.sc) return sc_walk(X, n, nb, H, W, src, time_dev, time_value, bn_batch, x_in);
    return us_walk(X, n, nb, H, W, src, time_dev, time_value, bn_batch, x_in);
}

}  // namespace

namespace dyf {

// (co, ci, taps) -> [co][tap][ci] (a) and, when asked for, [tap][ci][co] (at): the training layouts of a conv weight and of its gradient
static void rn_pack_conv(const float* host, int cout, int cin, int taps, std::vector<float>& a, std::vector<float>* at) {
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tp = 0; tp < taps; ++tp) {
                const float x = host[((size_t)co * cin + ci) * taps + tp];
                a[((size_t)co * taps + tp) * cin + ci] = x;
                if (at) (*at)[((size_t)tp * cin + ci) * cout + co] = x;
            }
}

// every tensor of `sd` into `t` in its training layout, and one zeroed gradient arena behind them (the loader's and the op seam's)
static dyf_status rn_fill_params(dyf_engine* e, TrainNet& t, std::map<std::string, TensorView>& sd) {
    auto ends_with = [](const std::string& s, const char* tail) { const size_t k = strlen(tail); return s.size() > k && s.compare(s.size() - k, k, tail) == 0; };
    for (auto& kv : sd) {
        const TensorView& v = kv.second;
        RParam p;
        p.n = (size_t)v.numel();
        p.stat = ends_with(kv.first, ".running_mean") || ends_with(kv.first, ".running_var");
        std::vector<float> host(v.data, v.data + v.numel());
        const bool is_conv = v.shape.size() == 4 && !ends_with(kv.first, ".norm.g");
        if (is_conv) {  // (co, ci, kh, kw) -> [co][tap][ci]; unet_simple's readout ConvTranspose2d (dim, C, 4, 4) -> [dim][tap][C] (RCtx::conv_transpose4s2)
            p.conv = 1; p.cout = (int)v.shape[0]; p.cin = (int)v.shape[1]; p.taps = (int)(v.shape[2] * v.shape[3]);
            std::vector<float> a(host.size()), at(host.size());
            rn_pack_conv(host.data(), p.cout, p.cin, p.taps, a, &at);
            dyf_status s = tupload(e, t.owned, &p.w, a);
            if (s == DYF_OK) s = tupload(e, t.owned, &p.wt, at);
            if (s != DYF_OK) return s;
        } else {
            dyf_status s = tupload(e, t.owned, &p.w, host);
            if (s != DYF_OK) return s;
        }
        t.P[kv.first] = p;
    }
    size_t total = 0;
    for (auto& kv : t.P) total += kv.second.stat ? 0 : (kv.second.n + 63) / 64 * 64;
    t.g_arena = nullptr;
    t.g_arena_floats = total;
    dyf_status gs = talloc(e, t.owned, &t.g_arena, total, true);
    if (gs != DYF_OK) return gs;
    size_t off = 0;
    for (auto& kv : t.P) {
        if (kv.second.stat) continue;
        kv.second.g = t.g_arena + off;
        off += (kv.second.n + 63) / 64 * 64;
    }
    return DYF_OK;
}

// fp32 training copy of a network's parameters (called by dyf_load_weights for every arch)
dyf_status train_store_params(dyf_engine* e, int which, std::map<std::string, TensorView>& sd) {
    if (!e->train) e->train = new TrainState();
    if (!e->train->net[which]) e->train->net[which] = new TrainNet();
    TrainNet& t = *e->train->net[which];
    TK(hipDeviceSynchronize());
    // an engine-resident optimizer keeps its state across a reload of the same network (the sampling copy is refreshed through here after
    // optimizer steps): the gradients accumulated so far move to the new arena, the chunk table is rebuilt over the new pointers
    float* keep_g = nullptr;
    const size_t keep_n = t.optim && t.ready ? t.g_arena_floats : 0;
    if (keep_n) {
        TK(hipMalloc(&keep_g, keep_n * sizeof(float)));
        TK(hipMemcpy(keep_g, t.g_arena, keep_n * sizeof(float), hipMemcpyDeviceToDevice));
    }
    tfree(e, t.owned);
    t.P.clear();
    t.ready = false;
    dyf_status s = rn_fill_params(e, t, sd);
    if (s == DYF_OK) s = optim_rebind(e, t);
    if (s == DYF_OK && keep_g && t.optim && hipMemcpy(t.g_arena, keep_g, keep_n * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess)
        s = fail(e, DYF_ERR_HIP, "dyf_load_weights: moving the accumulated gradients failed");
    if (keep_g) (void)hipFree(keep_g);
    if (s != DYF_OK) return s;
    TK(hipDeviceSynchronize());
    t.ready = true;
    return DYF_OK;
}

// the recorded forward of either backbone into tape `slot` (dyf_train_forward)
dyf_status train_forward(dyf_engine* e, int which, int slot, const float* inputs_dev, const float* time_dev, const float* cond_dev, float* out_dev,
                         int nb, int flags, hipStream_t st) {
    TrainNet* wp = e->train ? e->train->net[which] : nullptr;
    if (!wp || !wp->ready) return fail(e, DYF_ERR_STATE, "training needs loaded weights (dyf_load_weights)");
    Net& n = e->net[which];
    const dyf_net_config& c = n.cfg;
    if ((c.cond_channels > 0) != (cond_dev != nullptr)) return fail(e, DYF_ERR_INVALID_ARGUMENT, "condition must be given iff num_conditional_channels > 0");
    if (c.with_time_emb && !time_dev) return fail(e, DYF_ERR_INVALID_ARGUMENT, "time must be given when with_time_emb");
    if (const char* why = net_record_refusal(e, n)) return fail(e, DYF_ERR_UNSUPPORTED, why);
    if (n.sc && e->train_precision == 16)
        return fail(e, DYF_ERR_UNSUPPORTED, "training step: SimpleConvNet records in fp32 -- 16-bit conv operands (dyf_train_set_precision(16)) are not supported for it");
    const int hw = e->cfg.height * e->cfg.width;
    e->train->stream = st;
    if (!e->train->tape[slot]) e->train->tape[slot] = new RTape();
    RTape& T = *e->train->tape[slot];
    TK(hipStreamSynchronize(st));
    tfree(e, T.owned);
    T.back.clear();
    T.ctx.reset();
    T.ts.clear();
    T.net = which; T.nb = nb; T.flags = flags; T.row_keys = nullptr; T.out = nullptr;
    T.det = train_det() ? 1 : 0;
    const bool any_p = c.dropout > 0.0f || c.block_dropout1 > 0.0f || c.attn_dropout > 0.0f || c.input_dropout > 0.0f;
    const bool drop_on = (flags & DYF_TRAIN_DROPOUT) && any_p;
    if (drop_on) {  // this forward's dropout streams (engine generator, keyed per global row); a copy of the keys stays for the backward
        if (nb > 2 * e->cfg.max_batch) return fail(e, DYF_ERR_INVALID_ARGUMENT, "batch larger than the engine's row-key table");
        TK(launch_rng_begin_forward(e->rng_state, e->row_keys, nb, nb, st));
        dyf_status s = talloc(e, T.owned, &T.row_keys, (size_t)2 * nb, false);
        if (s != DYF_OK) return s;
        TK(hipMemcpyAsync(T.row_keys, e->row_keys, (size_t)2 * nb * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    }
    RCtx* Xp = new RCtx{e, *wp, T, c, st, nb, drop_on};
    T.ctx = std::shared_ptr<void>(Xp, [](void* p) { delete (RCtx*)p; });
    RCtx& X = *Xp;
    Source src[3];
    T.in_lo = net_sources(n, inputs_dev, cond_dev, src);
    X.mem = FwdMem{e, &T.owned, st};
    RT* y = net_walk(X, e, n, nb, src, time_dev, 0.0f, (flags & DYF_TRAIN_BATCH_STATS) != 0, &T.x_in);
    T.out = y;
    if (X.err != DYF_OK) return fail(e, X.err, "training forward: allocation / launch failed");
    hipLaunchKernelGGL(t_nhwc_to_nchw, dim3(nblk((long long)nb * hw * c.out_channels)), dim3(256), 0, st, y->p, nb, hw, c.out_channels, 0, c.out_channels, out_dev);
    TK(hipGetLastError());
    return DYF_OK;
}

// ---- fp32 sampling (dyf_set_sample_precision(32)): the same walk on the engine's bump arena, nothing recorded
// bytes one forward of `nb` rows takes from the arena: the walk itself, counting
size_t f32_walk_bytes(const dyf_engine* e, const Net& n, int nb) {
    RCount K{n.cfg, nb};
    Source none[3] = {{nullptr, 0}, {nullptr, 0}, {nullptr, 0}};
    RT* xi = nullptr;
    (void)net_walk(K, e, n, nb, none, nullptr, 0.0f, false, &xi);
    return K.bytes;
}

// past 4096 tokens the sampling forward takes the streaming Attention core, whose dropout element index (h N + i) N + j is uint32_t:
// 4 N^2 <= 2^32 - 1, N <= 32 767
bool rn_f32_supported(const dyf_engine* e, const Net& n) {
    const RNames R = rn_names(e, n.cfg);
    return (long long)R.lev_h.back() * R.lev_w.back() <= AT_STREAM_MAX;
}

// test seam (dyf_op_attention_f32): the fp32 Attention core alone.  form 0: t_at_fwd with scratch probabilities; form 1: the streaming
// core at any supported N.  p > 0: the caller's keep mask (nb, 4, N, N), or the engine's generator armed as dyf_op_attention_dropout does.
dyf_status f32_op_attention(dyf_engine* e, const float* qkv, int nb, int N, float p, const uint8_t* mask, int form, float* out, hipStream_t st) {
    if (form == 0 && N > AT_KEEP_P_MAX)
        return fail(e, DYF_ERR_UNSUPPORTED, "dyf_op_attention_f32: form 0 keeps its (tokens x tokens) probabilities -- at most 4096 tokens");
    if (N > AT_STREAM_MAX)
        return fail(e, DYF_ERR_UNSUPPORTED, "dyf_op_attention_f32: the dropout element index is 32 bits -- at most 32767 tokens");
    RDrop d{};
    if (p > 0.0f) {
        d.scale = 1.0f / (1.0f - p);
        if (mask) {
            d.mask = mask;
            d.per = (uint32_t)((size_t)RH * N * N);
        } else {
            if (nb > 2 * e->cfg.max_batch) return fail(e, DYF_ERR_INVALID_ARGUMENT, "more rows than the engine's row-key table (2 max_batch)");
            TK(launch_rng_begin_forward(e->rng_state, e->row_keys, nb, nb, st));
            d.on = 1;
            d.thresh16 = keep_threshold16(p);
            d.salt = rng_layer_salt(0u);
            d.row_keys = e->row_keys;
        }
    }
    const float scale = 1.0f / sqrtf((float)RD);
    float* P = nullptr;
    if (form == 0) {
        const long long rows = (long long)nb * RH * N;
        TK(hipMalloc(&P, (size_t)rows * N * sizeof(float)));
        hipLaunchKernelGGL(t_at_fwd, dim3(nblk(rows, 64)), dim3(64), 0, st, qkv, N, rows, scale, d, P, out);
    } else {
        launch_t_at_stream_fwd(qkv, nb, N, scale, d, out, st);
    }
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (P) (void)hipFree(P);
    if (err != hipSuccess) return fail(e, DYF_ERR_HIP, std::string("dyf_op_attention_f32: ") + hipGetErrorString(err));
    return DYF_OK;
}

// the backward of a recorded forward: its closures in reverse (the training step's and the op seam's)
static dyf_status rn_run_adjoints(RTape& T, RCtx& X) {
    dyf_status r = DYF_OK;
    for (auto it = T.back.rbegin(); it != T.back.rend() && r == DYF_OK; ++it) r = (*it)();
    if (r == DYF_OK && X.err != DYF_OK) r = X.err;
    return r;
}

dyf_status train_backward(dyf_engine* e, int slot, const float* dout_dev, float* dinputs_dev, int param_grads, hipStream_t st) {
    RTape* tp = e->train ? e->train->tape[slot] : nullptr;
    if (!tp || tp->net < 0 || !tp->out) return fail(e, DYF_ERR_STATE, "no forward recorded in this tape slot");
    RTape& T = *tp;
    const TrainDetScope det(T.det);  // the mode its forward was recorded under
    Net& n = e->net[T.net];
    const dyf_net_config& c = n.cfg;
    e->train->stream = st;
    std::vector<void*> tmp;
    RCtx& X = *(RCtx*)T.ctx.get();   // the closures hold a pointer to this object
    X.st = st;
    X.tmp = &tmp;
    X.param_grads = param_grads != 0;
    X.want_dinputs = dinputs_dev != nullptr;
    X.norm_bwd = nullptr;
    X.err = DYF_OK;
    const int hw = e->cfg.height * e->cfg.width;
    for (auto& t : T.ts) t.g = nullptr;
    T.out->g = X.tbuf(T.out->n);
    if (X.err != DYF_OK) { tfree(e, tmp); return fail(e, X.err, "training backward: allocation failed"); }
    hipLaunchKernelGGL(t_nchw_to_nhwc, dim3(nblk((long long)T.nb * hw * c.out_channels)), dim3(256), 0, st, dout_dev, T.nb, hw, c.out_channels, T.out->g);
    dyf_status r = rn_run_adjoints(T, X);
    if (r == DYF_OK && dinputs_dev && !T.x_in->g) r = DYF_ERR_STATE;  // every walk's first conv reaches the network input
    if (r == DYF_OK && dinputs_dev)
        hipLaunchKernelGGL(t_nhwc_to_nchw, dim3(nblk((long long)T.nb * hw * c.in_channels)), dim3(256), 0, st, T.x_in->g, T.nb, hw, n.cin_total, T.in_lo,
                           c.in_channels, dinputs_dev);
    hipError_t se = hipStreamSynchronize(st);
    for (auto& t : T.ts) t.g = nullptr;
    tfree(e, tmp);
    if (r != DYF_OK) return fail(e, r, "training backward failed");
    if (se != hipSuccess) return fail(e, DYF_ERR_HIP, std::string("training backward: ") + hipGetErrorString(se));
    return DYF_OK;
}

// what leaves by one parameter's name, in its PyTorch layout (conv: (co, ci, kh, kw)), to `out` on the device or the host: its gradient, or
// -- a BatchNorm running statistic -- the statistic as the recorded forwards updated it
// (stage: p.n floats of device scratch for the unpacked copy of a conv weight on its way to the host; the copy below is synchronous, so one
// block serves a whole export)
// (from: another buffer in the parameter's training layout -- its weights, or its slice of an optimizer arena; dyf_optim_export)
static dyf_status rn_export_param(dyf_engine* e, float* stage, const RParam& p, float* out, bool dev, const float* from = nullptr) {
    const float* src = from ? from : p.stat ? p.w : p.g;
    if (p.conv) {
        hipLaunchKernelGGL(t_unpack_conv, dim3(nblk((long long)p.n)), dim3(256), 0, 0, src, p.cout, p.cin, p.taps, dev ? out : stage);
        src = stage;
        if (dev) return DYF_OK;
    }
    if (dev) TK(hipMemcpy(out, src, p.n * sizeof(float), hipMemcpyDeviceToDevice));
    else { TK(hipDeviceSynchronize()); TK(hipMemcpy(out, src, p.n * sizeof(float), hipMemcpyDeviceToHost)); }
    return DYF_OK;
}

// gradients (and running statistics) by state_dict name in PyTorch layouts (dyf_train_export, dyf_train_export_dev)
dyf_status train_export(dyf_engine* e, int which, int n_tensors, const char* const* names, float* const* out, bool dev) {
    TrainNet* t = e->train ? e->train->net[which] : nullptr;
    if (!t || !t->ready) return fail(e, DYF_ERR_STATE, "training needs loaded weights (dyf_load_weights)");
    TK(hipDeviceSynchronize());
    std::vector<void*> tmp;
    size_t stage_n = 0;
    for (int i = 0; i < n_tensors; ++i) {
        auto it = t->P.find(names[i]);
        if (it == t->P.end()) return fail(e, DYF_ERR_INVALID_ARGUMENT, std::string("dyf_train_export: unknown tensor '") + names[i] + "'");
        if (it->second.conv && !dev) stage_n = std::max(stage_n, it->second.n);
    }
    float* stage = nullptr;
    if (stage_n) {  // (after a backward the pool holds that backward's temporaries: one of them serves, no block is added)
        dyf_status s = talloc(e, tmp, &stage, stage_n, false, true);
        if (s != DYF_OK) return s;
    }
    for (int i = 0; i < n_tensors; ++i) {
        dyf_status s = rn_export_param(e, stage, t->P.at(names[i]), out[i], dev);
        if (s != DYF_OK) { tfree(e, tmp); return s; }
    }
    TK(hipDeviceSynchronize());
    tfree(e, tmp);
    return DYF_OK;
}

// test seam (dyf_op_train_f32): ONE op of the recorded forward and its adjoint.  The op is the RCtx member function itself, recording on
// a scratch tape over a scratch parameter set; the backward is rn_run_adjoints, the loop train_backward runs -- no launch is restated
// here.  Parameters arrive in PyTorch layouts on the host and go through rn_fill_params; the gradient buffers start from the caller's
// contents (conv weights packed as the weights are) and leave through rn_export_param.
dyf_status f32_op_train(dyf_engine* e, const dyf_train_op* dp, const float* const* inputs, const float* const* params, const float* dout,
                        float* y_out, float* const* dinputs, float* const* dparams, hipStream_t st) {
    const dyf_train_op& d = *dp;
    auto refuse = [&](dyf_status s, const char* what) { return fail(e, s, std::string("dyf_op_train_f32: ") + what); };
    if (d.nb < 1 || d.h < 1 || d.w < 1 || d.c < 1) return refuse(DYF_ERR_INVALID_ARGUMENT, "nb, h, w and c must be positive");
    if (!(d.p >= 0.0f && d.p < 1.0f)) return refuse(DYF_ERR_INVALID_ARGUMENT, "p must be in [0, 1)");
    const bool has_p = d.op == DYF_TOP_GN_ACT || d.op == DYF_TOP_NORM_ACT || d.op == DYF_TOP_LAYERNORM || d.op == DYF_TOP_ATTENTION || d.op == DYF_TOP_DROPOUT ||
                       d.op == DYF_TOP_ATTENTION_STREAM;
    const bool has_c2 = d.op == DYF_TOP_CONV || d.op == DYF_TOP_LINEAR || d.op == DYF_TOP_CAT || d.op == DYF_TOP_CONVT;
    if ((d.flags & DYF_TOP_SAMPLE) && d.op != DYF_TOP_CONV) return refuse(DYF_ERR_UNSUPPORTED, "DYF_TOP_SAMPLE: conv only");
    const bool sample = (d.flags & DYF_TOP_SAMPLE) != 0;  // the forward alone, launched the way a sampling forward launches it
    const int flags_ok = d.op == DYF_TOP_CONV ? (DYF_TOP_WS | DYF_TOP_BIAS | DYF_TOP_SAMPLE) : d.op == DYF_TOP_GN_ACT ? DYF_TOP_FILM : d.op == DYF_TOP_LINEAR ? DYF_TOP_PRE
                         : d.op == DYF_TOP_ADD ? DYF_TOP_SAME
                         : d.op == DYF_TOP_NORM_ACT ? (DYF_TOP_FILM | DYF_TOP_RUNNING | DYF_TOP_MASK | DYF_TOP_LEAKY | DYF_TOP_RELU | DYF_TOP_ACT_GELU | DYF_TOP_RESIDUAL)
                         : d.op == DYF_TOP_UP2_BILINEAR ? DYF_TOP_GRAD_IN : d.op == DYF_TOP_RESIZE ? DYF_TOP_NEAREST : 0;
    if (d.op < DYF_TOP_CONV || d.op > DYF_TOP_ATTENTION_STREAM) return refuse(DYF_ERR_INVALID_ARGUMENT, "unknown op");
    if (d.flags & ~flags_ok) return refuse(DYF_ERR_INVALID_ARGUMENT, "a flag this op does not take");
    if (d.p > 0.0f && !has_p) return refuse(DYF_ERR_INVALID_ARGUMENT, "this op has no dropout");
    if (d.op == DYF_TOP_UP2_BILINEAR ? d.c2 < 0 : has_c2 ? d.c2 < 1 : d.c2 != 0)
        return refuse(DYF_ERR_INVALID_ARGUMENT, "c2 must be positive for conv / linear / cat / convt, 0 or the second source's channels for up2_bilinear, 0 otherwise");
    if (d.op == DYF_TOP_CONV ? (d.k < 1 || d.stride < 1 || d.pad < 0 || d.h + 2 * d.pad < d.k || d.w + 2 * d.pad < d.k)
        : d.op == DYF_TOP_RESIZE ? (d.k < 1 || d.stride < 1 || d.pad != 0) : (d.k != 0 || d.stride != 0 || d.pad != 0))
        return refuse(DYF_ERR_INVALID_ARGUMENT, "k / stride / pad: a conv geometry with at least one output pixel, the output size of a resize, 0 for every other op");
    if (d.op == DYF_TOP_GN_ACT ? (d.groups < 1 || d.c % d.groups != 0) : d.op == DYF_TOP_NORM_ACT ? (d.groups < 0 || (d.groups > 0 && d.c % d.groups != 0)) : d.groups != 0)
        return refuse(DYF_ERR_INVALID_ARGUMENT, "groups must divide c for gn_act / norm_act (norm_act: 0 = BatchNorm) and be 0 otherwise");
    if (d.op == DYF_TOP_NORM_ACT && (((d.flags & DYF_TOP_RUNNING) && d.groups > 0) || (!!(d.flags & DYF_TOP_LEAKY) + !!(d.flags & DYF_TOP_RELU) + !!(d.flags & DYF_TOP_ACT_GELU) > 1) || ((d.flags & DYF_TOP_MASK) && !(d.p > 0.0f))))
        return refuse(DYF_ERR_INVALID_ARGUMENT, "norm_act: running statistics are BatchNorm's, one activation, a mask needs p > 0");
    if ((d.flags & DYF_TOP_GRAD_IN) && (d.c2 < 1 || !dinputs || !dinputs[1])) return refuse(DYF_ERR_INVALID_ARGUMENT, "up2_bilinear: a gradient to start from needs the second source and its gradient buffer");
    if ((d.op == DYF_TOP_LINEAR || d.op == DYF_TOP_LEARNED_SINU) && (d.h != 1 || d.w != 1)) return refuse(DYF_ERR_INVALID_ARGUMENT, "linear / learned_sinu take rows: h = w = 1");
    const long long hw = (long long)d.h * d.w, px = hw * d.nb;
    const bool attn_core = d.op == DYF_TOP_LINATTN || d.op == DYF_TOP_ATTENTION || d.op == DYF_TOP_ATTENTION_STREAM;
    const long long cmax = std::max<long long>(d.c + d.c2, attn_core ? 3 * RHID : 0);
    const long long ohw = d.op == DYF_TOP_RESIZE ? (long long)d.k * d.stride : hw;  // the larger plane of the op (x2 upsamples: the 4 below)
    if (std::max(hw, ohw) * cmax * 4 >= (1ll << 32) || std::max(hw, ohw) * d.nb * cmax * 4 >= (1ll << 31)) return refuse(DYF_ERR_UNSUPPORTED, "tensor too large for the op seam (2^31 elements)");
    if (attn_core && d.c != 3 * RHID) return refuse(DYF_ERR_INVALID_ARGUMENT, "the attention cores take qkv of 384 channels");
    if (d.op == DYF_TOP_ATTENTION && hw > AT_KEEP_P_MAX) return refuse(DYF_ERR_UNSUPPORTED, "the Attention core keeps its (tokens x tokens) probabilities -- at most 4096 tokens");
    if (d.op == DYF_TOP_ATTENTION_STREAM && hw > AT_STREAM_MAX) return refuse(DYF_ERR_UNSUPPORTED, "the streaming Attention core indexes its (4 x tokens x tokens) probabilities with 32 bits -- at most 32767 tokens");
    if (d.p > 0.0f && d.nb > 2 * e->cfg.max_batch) return refuse(DYF_ERR_INVALID_ARGUMENT, "more rows than the engine's row-key table (2 max_batch)");

    // inputs (floats each) and parameters (name, PyTorch shape) of the op
    struct PS { std::string name; std::vector<int64_t> shape; };
    std::vector<PS> ps;
    std::vector<size_t> in_n;
    const size_t xn = (size_t)px * d.c;
    switch (d.op) {
    case DYF_TOP_CONV:
        in_n = {xn};
        ps.push_back({"op.weight", {d.c2, d.c, d.k, d.k}});
        if (d.flags & DYF_TOP_BIAS) ps.push_back({"op.bias", {d.c2}});
        break;
    case DYF_TOP_GN_ACT:
        in_n = {xn};
        if (d.flags & DYF_TOP_FILM) in_n.push_back((size_t)d.nb * 2 * d.c);
        ps = {{"op.weight", {d.c}}, {"op.bias", {d.c}}};
        break;
    case DYF_TOP_LAYERNORM: in_n = {xn}; ps = {{"op.norm.g", {1, d.c, 1, 1}}}; break;
    case DYF_TOP_LINEAR: in_n = {xn}; ps = {{"op.weight", {d.c2, d.c}}, {"op.bias", {d.c2}}}; break;
    case DYF_TOP_LEARNED_SINU: in_n = {(size_t)d.nb}; ps = {{"time_emb_mlp.0.weights", {d.c}}}; break;
    case DYF_TOP_ADD: in_n = {xn}; if (!(d.flags & DYF_TOP_SAME)) in_n.push_back(xn); break;
    case DYF_TOP_CAT: in_n = {xn, (size_t)px * d.c2}; break;
    case DYF_TOP_NORM_ACT:
        in_n = {xn};
        if (d.flags & DYF_TOP_FILM) in_n.push_back((size_t)d.nb * 2 * d.c);
        if (d.flags & DYF_TOP_RESIDUAL) in_n.push_back(xn);
        ps = {{"op.weight", {d.c}}, {"op.bias", {d.c}}};
        if (d.groups == 0) { ps.push_back({"op.running_mean", {d.c}}); ps.push_back({"op.running_var", {d.c}}); }
        break;
    case DYF_TOP_UP2_BILINEAR: in_n = {xn}; if (d.c2) in_n.push_back((size_t)px * d.c2); break;
    case DYF_TOP_CONVT: in_n = {xn}; ps = {{"op.weight", {d.c, d.c2, 4, 4}}, {"op.bias", {d.c2}}}; break;
    default: in_n = {xn}; break;
    }
    for (size_t i = 0; i < in_n.size(); ++i)
        if (!inputs[i]) return refuse(DYF_ERR_INVALID_ARGUMENT, "an input pointer is null");
    // norm_act with DYF_TOP_MASK: the caller's keep mask follows the inputs; the forward alone runs (the adjoints draw from the generator)
    const uint8_t* mask = (d.flags & DYF_TOP_MASK) ? (const uint8_t*)inputs[in_n.size()] : nullptr;
    if ((d.flags & DYF_TOP_MASK) && !mask) return refuse(DYF_ERR_INVALID_ARGUMENT, "the mask pointer is null");
    for (size_t i = 0; i < ps.size(); ++i)
        if (!params || !dparams || !params[i] || !dparams[i]) return refuse(DYF_ERR_INVALID_ARGUMENT, "a parameter or parameter-gradient pointer is null");

    if (!e->train) e->train = new TrainState();
    e->train->stream = st;
    // DYF_TOP_SAMPLE: the operands of dyf_set_sample_precision (16 has no fp32 walk: fp32 operands), the default kernel forms and the
    // sampling-forward scope, as f32_net_forward sets them
    const TrainPrecisionScope precision(!sample ? e->train_precision : e->sample_precision == DYF_SAMPLE_PRECISION_BF16X3 ? DYF_TRAIN_PRECISION_BF16X3 : 32);
    const TrainDetScope det(sample ? 0 : e->train_deterministic);
    const SampleForwardScope sampling(sample ? 1 : 0);
    dyf_net_config c = e->net[0].cfg;
    c.groups = d.groups;
    TrainNet W;
    RTape T;
    std::vector<void*> tmp;
    auto done = [&](dyf_status s) {  // everything back to the engine's pool, whatever happened
        const hipError_t se = hipDeviceSynchronize();
        for (auto& t : T.ts) t.g = nullptr;
        T.back.clear();
        tfree(e, tmp);
        tfree(e, T.owned);
        tfree(e, W.owned);
        if (s == DYF_OK && se != hipSuccess) return fail(e, DYF_ERR_HIP, std::string("dyf_op_train_f32: ") + hipGetErrorString(se));
        return s;
    };
#define OPK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return done(fail(e, DYF_ERR_HIP, std::string("dyf_op_train_f32: " #expr ": ") + hipGetErrorString(_e))); } while (0)
    {
        std::map<std::string, TensorView> sd;
        for (size_t i = 0; i < ps.size(); ++i) sd[ps[i].name] = TensorView{params[i], ps[i].shape};
        dyf_status s = rn_fill_params(e, W, sd);
        if (s != DYF_OK) return done(s);
        std::vector<std::vector<float>> g0(ps.size());  // the caller's gradient contents, in the gradient buffers' layout
        for (size_t i = 0; i < ps.size(); ++i) {
            const RParam& p = W.P.at(ps[i].name);
            if (p.stat) continue;  // no gradient: the updated statistic leaves in its place
            g0[i].assign(dparams[i], dparams[i] + p.n);
            if (p.conv) {
                std::vector<float> a(p.n);
                rn_pack_conv(g0[i].data(), p.cout, p.cin, p.taps, a, nullptr);
                g0[i].swap(a);
            }
            OPK(hipMemcpyAsync(p.g, g0[i].data(), p.n * sizeof(float), hipMemcpyHostToDevice, st));
        }
        OPK(hipStreamSynchronize(st));
    }
    bool drop_on = false;
    if (d.p > 0.0f && !mask) {  // a new forward of the generator, site 0 (as f32_op_attention)
        OPK(launch_rng_begin_forward(e->rng_state, e->row_keys, d.nb, d.nb, st));
        T.row_keys = e->row_keys;
        drop_on = true;
    }
    RCtx X{e, W, T, c, st, d.nb, drop_on};
    X.mem = FwdMem{e, &T.owned, st};
    X.tmp = &tmp;
    X.masks = mask ? &mask : nullptr;
    RT* in[3] = {nullptr, nullptr, nullptr};
    if (d.op != DYF_TOP_LEARNED_SINU)
        for (size_t i = 0; i < in_n.size(); ++i) {
            in[i] = X.make(in_n[i]);
            if (X.err != DYF_OK) return done(refuse(X.err, "allocation failed"));
            OPK(hipMemcpyAsync(in[i]->p, inputs[i], in_n[i] * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    RT* y = nullptr;
    switch (d.op) {
    case DYF_TOP_CONV: y = X.conv(in[0], d.h, d.w, d.c, d.c2, d.k, d.stride, d.pad, "op", (d.flags & DYF_TOP_BIAS) != 0, (d.flags & DYF_TOP_WS) != 0); break;
    case DYF_TOP_GN_ACT: y = X.norm_act(in[0], (int)hw, d.c, "op", in[1], d.p, 2, d.groups, ACT_SILU, rn_norm_ppb((int)hw, d.nb)); break;
    case DYF_TOP_NORM_ACT: {
        const bool film = (d.flags & DYF_TOP_FILM) != 0;
        y = X.norm_act(in[0], (int)hw, d.c, "op", film ? in[1] : nullptr, d.p, d.groups > 0 ? 2 : (d.flags & DYF_TOP_RUNNING) ? 1 : 0, d.groups,
                       (d.flags & DYF_TOP_LEAKY) ? ACT_LEAKY : (d.flags & DYF_TOP_RELU) ? ACT_RELU : (d.flags & DYF_TOP_ACT_GELU) ? ACT_GELU : ACT_SILU,
                       us_norm_ppb((int)hw), -1, (d.flags & DYF_TOP_RESIDUAL) ? in[film ? 2 : 1] : nullptr);
        break;
    }
    case DYF_TOP_UP2_BILINEAR: y = X.up2_bilinear(in[0], d.c, in[1], d.c2, d.h, d.w, 2 * d.h, 2 * d.w); break;
    case DYF_TOP_RESIZE: y = X.resize(in[0], d.h, d.w, d.c, d.k, d.stride, (d.flags & DYF_TOP_NEAREST) ? 1 : 0); break;
    case DYF_TOP_CONVT: y = X.conv_transpose4s2(in[0], d.h, d.w, d.c, d.c2, "op"); break;
    case DYF_TOP_LAYERNORM: y = X.layernorm(in[0], (int)hw, d.c, "op.norm.g", d.p); break;
    case DYF_TOP_LINATTN: y = X.linattn(in[0], (int)hw); break;
    case DYF_TOP_ATTENTION: y = X.attention(in[0], (int)hw, d.p); break;
    case DYF_TOP_ATTENTION_STREAM: y = X.attention(in[0], (int)hw, d.p, true); break;
    case DYF_TOP_LINEAR: y = X.linear(in[0], d.nb, d.c, d.c2, "op", (d.flags & DYF_TOP_PRE) ? 1 : 0); break;
    case DYF_TOP_LEARNED_SINU: y = X.learned_sinu(inputs[0], d.c); break;
    case DYF_TOP_DROPOUT: y = X.dropout(in[0], hw * d.c, d.p); break;
    case DYF_TOP_GELU: y = X.gelu(in[0]); break;
    case DYF_TOP_ADD: y = X.add(in[0], (d.flags & DYF_TOP_SAME) ? in[0] : in[1]); break;
    case DYF_TOP_CAT: y = X.cat(in[0], d.c, in[1], d.c2, px); break;
    default: y = X.up2_nearest(in[0], d.h, d.w, d.c); break;
    }
    if (X.err != DYF_OK || !y) return done(refuse(X.err != DYF_OK ? X.err : DYF_ERR_HIP, "forward: allocation / launch failed"));
    OPK(hipGetLastError());
    OPK(hipMemcpyAsync(y_out, y->p, y->n * sizeof(float), hipMemcpyDeviceToDevice, st));
    // the backward, as train_backward starts it: the output's gradient, then the closures in reverse
    for (auto& t : T.ts) t.g = nullptr;
    if (y == in[0]) {  // a resize to the same size is the identity: so is its adjoint
        X.grad(y);
        OPK(hipMemcpyAsync(y->g, dout, y->n * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (!mask && !sample) {
        float* gy = X.grad(y);
        if (d.flags & DYF_TOP_GRAD_IN) {  // the second source's gradient starts from the caller's
            float* g1 = X.grad(in[1]);
            if (X.err == DYF_OK) OPK(hipMemcpyAsync(g1, dinputs[1], in_n[1] * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        if (X.err != DYF_OK) return done(refuse(X.err, "allocation failed"));
        OPK(hipMemcpyAsync(gy, dout, y->n * sizeof(float), hipMemcpyDeviceToDevice, st));
        dyf_status r = rn_run_adjoints(T, X);
        if (r != DYF_OK) return done(refuse(r, "backward failed"));
        OPK(hipGetLastError());
    }
    for (size_t i = 0; i < in_n.size() && dinputs && !mask && !sample; ++i) {
        if (!dinputs[i] || !in[i]) continue;
        if (in[i]->g) OPK(hipMemcpyAsync(dinputs[i], in[i]->g, in_n[i] * sizeof(float), hipMemcpyDeviceToDevice, st));
        else OPK(hipMemsetAsync(dinputs[i], 0, in_n[i] * sizeof(float), st));
    }
    OPK(hipStreamSynchronize(st));
    if (sample) return done(DYF_OK);  // no adjoint ran: no gradient is written
    float* stage = X.tbuf(ps.empty() ? 1 : W.P.at(ps[0].name).n);  // (a conv weight is its op's first parameter)
    if (X.err != DYF_OK) return done(refuse(X.err, "allocation failed"));
    for (size_t i = 0; i < ps.size(); ++i) {
        dyf_status s = rn_export_param(e, stage, W.P.at(ps[i].name), dparams[i], false);
        if (s != DYF_OK) return done(s);
    }
#undef OPK
    return done(DYF_OK);
}

}  // namespace dyf
