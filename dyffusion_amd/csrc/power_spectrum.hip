// Radially binned power spectra of an ensemble forecast (gfx950; dyf_power_spectrum): per (segment, channel) the shell sums of
// |F(z)|^2 / (H W)^2 of the N member anomalies a_m = x_m - xbar (plane 0, spread: their mean over m), the ensemble mean xbar (plane
// 1), the target y (plane 2) and the error e = xbar - y (plane 3), averaged over the batch.  The reference has no counterpart; float64
// numpy (np.fft.fft2 on the full spectrum) is what the results are held to (tests/power_spectrum_refs.py).
//   Every shipped transform size is small and awkward (221 = 13 x 17, 42, 60), so the 2-D DFT is taken directly, as two small GEMMs:
// the row DFT along W on the VALU, the column DFT along H on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32, an fmaf
// chain).  Anomalies and the error are taken in fp32 BEFORE the transform; nothing of the form sum |X_m|^2 - N |Xbar|^2 appears.
//   Launch 1 (power_spectrum_mean_kernel): xbar = (float)(float64 member sum in member order / N) per point into the workspace.  It
// is a launch of its own because a field of up to 1024 x 1024 does not fit LDS beside the transform's buffers and every workgroup of
// launch 2 needs the whole row of it.
//   Launch 2 (power_spectrum_kernel): one workgroup of 4 waves per (segment; b, c, tile of 16 kx columns of the half spectrum kx in
// [0, W / 2]); it walks the N + 3 fields a_0 .. a_{N-1}, xbar, y, e in that order.  Per field:
//   stage 1  T[h][kx] = sum_w z[h][w] e^{-2 pi i kx w / W}.  16 rows x 128 columns of z (anomaly and Hann taper applied while they are
//            loaded, coalesced) are staged in LDS; thread (kx, row) runs the fmaf chain over w, the twiddle index (kx w) mod W advanced
//            by addition and conditional subtraction into an LDS table.  T (re, im) is H' x 16 floats each in LDS, H' = H rounded up
//            to 4; rows past H and columns past W / 2 are zero.
//   stage 2  Z = Omega T: a wave owns the ky tiles wave, wave + 4, ..; per K step of 4 rows h four MFMAs on four independent
//            accumulators (cos Tr, sin Ti | cos Ti, -sin Tr), the Omega fragment gathered from an H-entry LDS table by the index
//            (ky h) mod H, advanced the same way.  Ragged K, ragged ky tiles and ragged kx tiles meet zeros in LDS (rows of T) or are
//            never binned (rows ky >= H, columns kx > W / 2); no divergent MFMA.
//   power    p = w_kx (zr^2 + zi^2) in float64, w_kx = 1 for kx = 0 and kx = W / 2 (W even), else 2.  The lane that owns coefficient
//            (ky, kx) of the tile adds p to its own float64 slot of the workgroup's plane buffer in the workspace (the spread plane
//            sums over the members in member order; the other planes are written once).  No LDS is left for H' x 16 doubles beside
//            T at H = 1024, and the slot is private to one lane, so this needs no atomics.
// After the last field the workgroup bins its four planes: thread `bin` walks the tile's list of that shell's coefficients (built on
// the host from the exact integer rule, (ky, kx) order) and writes one float64 per (plane, bin); the corners (bin >= n_bins) are the
// extra bin n_bins.  This differs from the issue's sketch (bins accumulated per field in LDS): 4 x (n_bins + 1) doubles beside T do not
// fit 160 KB at 1024 x 1024, and binning once per workgroup instead of once per field takes it off the hot path.
//   Launch 3 (power_spectrum_join_kernel): per (segment, c) the workgroups' bins are added in (b, tile) order, divided by B (H W)^2
// (and N for the spread); `total` is the sum of a plane's n_bins + 1 bins in bin order.  No atomics, nothing exchanged between
// workgroups inside a launch: identical calls give identical bits, and the kernels read fp32 only, so both builds give the same bits.
#include "kernels.h"

#include <cmath>
#include <vector>

namespace {

constexpr int PS_ZROWS = 16, PS_ZCOLS = 128;  // the staged block of z
typedef float ps_f32x4 __attribute__((ext_vector_type(4)));

struct PsArgs {
    const float* const* preds_tab;
    const float* const* targets_tab;
    const float* xbar;     // [n_segments][B][C][H][W]
    const float* tables;   // cosW[W] sinW[W] cosH[H] sinH[H] winH[H] winW[W]
    const unsigned short* csr_idx;  // [tiles][H * 16]: ky * 16 + kx_local, sorted by bin, (ky, kx) order inside a bin
    const int* csr_off;             // [tiles][n_bins + 2]
    double* planes;    // [workgroup][4][nky * 16][16]
    double* partials;  // [workgroup][4][n_bins + 1]
    long long member_stride;
    int n_members, channels, H, W, Wh, tiles, Hp, nky, n_bins1, window;
};

__global__ __launch_bounds__(256) void power_spectrum_mean_kernel(const float* const* preds_tab, int n_members, long long member_stride,
                                                                  long long points, float* xbar) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= points) return;
    const float* src = preds_tab[blockIdx.y] + p;
    double s = 0.0;
    for (int m = 0; m < n_members; ++m) s += (double)src[(long long)m * member_stride];
    xbar[(long long)blockIdx.y * points + p] = (float)(s / (double)n_members);
}

__global__ __launch_bounds__(256) void power_spectrum_kernel(PsArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ float ps_lds[];
    const int H = a.H, W = a.W, Hp = a.Hp;
    float* Tr = ps_lds;
    float* Ti = Tr + Hp * 16;
    float* cW = Ti + Hp * 16;
    float* sW = cW + W;
    float* cH = sW + W;
    float* sH = cH + H;
    float* zbuf = sH + H;  // [PS_ZROWS][PS_ZCOLS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x % a.tiles;
    const long long bc = blockIdx.x / a.tiles;  // b * C + c
    const long long wg = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const long long field_off = bc * H * W;  // of (b, c) inside a segment's (B, C, H, W)
    const float* preds = a.preds_tab[blockIdx.y] + field_off;
    const float* target = a.targets_tab[blockIdx.y] + field_off;
    const float* xbar = a.xbar + ((long long)blockIdx.y * gridDim.x / a.tiles) * H * W + field_off;
    const float* winH = a.tables + 2 * W + 2 * H;
    const float* winW = winH + H;
    double* planes = a.planes + wg * 4 * a.nky * 256;

    for (int i = tid; i < 2 * W + 2 * H; i += 256) cW[i] = a.tables[i];  // the four tables are contiguous in both places
    for (int i = tid; i < (Hp - H) * 16; i += 256) Tr[H * 16 + i] = 0.0f, Ti[H * 16 + i] = 0.0f;

    const int kxl = tid & 15, hr = tid >> 4;
    const int kx = tile * 16 + kxl;
    const bool kx_valid = kx < a.Wh;
    const int kstep = kx % W;
    const int N = a.n_members;
    for (int f = 0; f < N + 3; ++f) {
        // ---- stage 1: the row DFT of 16 rows at a time
        const float* member = preds + (long long)(f < N ? f : 0) * a.member_stride;
        for (int hb = 0; hb < H; hb += PS_ZROWS) {
            float tr = 0.0f, ti = 0.0f;
            int idx = 0;
            for (int wc = 0; wc < W; wc += PS_ZCOLS) {
                __syncthreads();  // zbuf (and, for the first block of a field, T) has been read
#pragma unroll
                for (int i = 0; i < PS_ZROWS * PS_ZCOLS / 256; ++i) {
                    const int e = tid + 256 * i, r = e / PS_ZCOLS, col = e % PS_ZCOLS;
                    const int h = hb + r, w = wc + col;
                    float z = 0.0f;
                    if (h < H && w < W) {
                        const long long o = (long long)h * W + w;
                        z = f < N ? member[o] - xbar[o] : f == N ? xbar[o] : f == N + 1 ? target[o] : xbar[o] - target[o];
                        if (a.window) z *= winH[h] * winW[w];
                    }
                    zbuf[e] = z;
                }
                __syncthreads();
                const int wn = min(PS_ZCOLS, W - wc);
                const float* zr = zbuf + hr * PS_ZCOLS;
                for (int j = 0; j < wn; ++j) {
                    const float z = zr[j];
                    tr = fmaf(z, cW[idx], tr);
                    ti = fmaf(-z, sW[idx], ti);
                    idx += kstep;
                    if (idx >= W) idx -= W;
                }
            }
            if (hb + hr < H) {
                Tr[(hb + hr) * 16 + kxl] = kx_valid ? tr : 0.0f;
                Ti[(hb + hr) * 16 + kxl] = kx_valid ? ti : 0.0f;
            }
        }
        __syncthreads();
        // ---- stage 2: the column DFT on the matrix cores, 16 ky x 16 kx per wave and tile
        const int q = lane >> 4, col = lane & 15;
        const int pl = f < N ? 0 : f - N + 1;
        const int colx = tile * 16 + col;
        const double wk = (colx == 0 || 2 * colx == W) ? 1.0 : 2.0;
        for (int kt = wave; kt < a.nky; kt += 4) {
            const int kym = (kt * 16 + col) % H;  // the A fragment's row: lane & 15
            int idx = (kym * q) % H;
            const int step = (4 * kym) % H;
            ps_f32x4 r1 = {0.0f, 0.0f, 0.0f, 0.0f}, r2 = r1, i1 = r1, i2 = r1;
            for (int h0 = 0; h0 < Hp; h0 += 4) {
                const float c = cH[idx], s = sH[idx];
                const float tr = Tr[(h0 + q) * 16 + col], ti = Ti[(h0 + q) * 16 + col];
                r1 = __builtin_amdgcn_mfma_f32_16x16x4f32(c, tr, r1, 0, 0, 0);
                r2 = __builtin_amdgcn_mfma_f32_16x16x4f32(s, ti, r2, 0, 0, 0);
                i1 = __builtin_amdgcn_mfma_f32_16x16x4f32(c, ti, i1, 0, 0, 0);
                i2 = __builtin_amdgcn_mfma_f32_16x16x4f32(-s, tr, i2, 0, 0, 0);
                idx += step;
                if (idx >= H) idx -= H;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float zr = r1[r] + r2[r], zi = i1[r] + i2[r];
                double p = wk * ((double)zr * (double)zr + (double)zi * (double)zi);
                double* slot = planes + ((long long)pl * a.nky * 16 + kt * 16 + q * 4 + r) * 16 + col;  // this lane's own
                if (f > 0 && f < N) p += *slot;
                *slot = p;
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    // ---- the shells of this tile, once per workgroup
    const int* off = a.csr_off + (long long)tile * (a.n_bins1 + 1);
    const unsigned short* list = a.csr_idx + (long long)tile * H * 16;
    for (int e = tid; e < 4 * a.n_bins1; e += 256) {
        const int p4 = e / a.n_bins1, bin = e - p4 * a.n_bins1;
        const double* plane = planes + (long long)p4 * a.nky * 256;
        double s = 0.0;
        for (int i = off[bin]; i < off[bin + 1]; ++i) s += plane[list[i]];
        a.partials[wg * 4 * a.n_bins1 + e] = s;
    }
#endif
}

// blockIdx.x the channel, blockIdx.y the segment; entry e = plane * (n_bins + 1) + bin.
__global__ __launch_bounds__(256) void power_spectrum_join_kernel(const double* partials, int n_members, int batch, int tiles, int n_bins1,
                                                                  double hw, double* out, double* accum) {
    __shared__ double vals[4 * (POWER_SPECTRUM_MAX_DIM / 2 + 2)];
    const int c = blockIdx.x, channels = gridDim.x;
    const long long per_segment = (long long)batch * channels * tiles;
    for (int e = threadIdx.x; e < 4 * n_bins1; e += 256) {
        double s = 0.0;
        for (int b = 0; b < batch; ++b)
            for (int t = 0; t < tiles; ++t) {
                const long long wg = (long long)blockIdx.y * per_segment + ((long long)b * channels + c) * tiles + t;
                s += partials[wg * 4 * n_bins1 + e];
            }
        const double denom = (double)batch * hw * hw * (e < n_bins1 ? (double)n_members : 1.0);
        vals[e] = s / denom;
    }
    __syncthreads();
    double* o = out + ((long long)blockIdx.y * channels + c) * 4 * n_bins1;
    double* ac = accum ? accum + ((long long)blockIdx.y * channels + c) * 4 * n_bins1 : nullptr;
    for (int e = threadIdx.x; e < 4 * n_bins1; e += 256) {
        const int bin = e % n_bins1;
        double v = vals[e];
        if (bin == n_bins1 - 1) {  // the `total` column: every bin of the plane, the corners last
            v = 0.0;
            for (int k = 0; k < n_bins1; ++k) v += vals[e - bin + k];
        }
        o[e] = v;
        if (ac) ac[e] += v;
    }
}

size_t ps_lds_bytes(int H, int W) {
    const int Hp = (H + 3) / 4 * 4;
    return sizeof(float) * ((size_t)2 * Hp * 16 + 2 * (size_t)W + 2 * (size_t)H + PS_ZROWS * PS_ZCOLS);
}

}  // namespace

int power_spectrum_bin(int H, int W, int ky, int kx) {
    const long long L = H > W ? H : W;
    const long long kyf = ky < H - ky ? ky : H - ky, kxf = kx < W - kx ? kx : W - kx;
    const long long hw2 = (long long)H * H * W * W;
    const long long num = 4 * L * L * (kxf * kxf * H * H + kyf * kyf * W * W);  // < 2^62 for H, W <= 1024
    long long k = (long long)std::floor(std::sqrt((double)num / (4.0 * (double)hw2)) + 0.5);
    // bin = k  <=>  (2k - 1)^2 H^2 W^2 <= num < (2k + 1)^2 H^2 W^2
    while ((2 * k + 1) * (2 * k + 1) * hw2 <= num) ++k;
    while (k > 0 && (2 * k - 1) * (2 * k - 1) * hw2 > num) --k;
    return (int)k;
}

int power_spectrum_plan(int n_segments, int n_members, int batch, int channels, int H, int W, PowerSpectrumPlan* plan) {
    if (n_segments < 1 || n_segments > 65535 || n_members < 1 || n_members > POWER_SPECTRUM_MAX_MEMBERS || batch < 1 || channels < 1 ||
        H < 2 || W < 2 || H > POWER_SPECTRUM_MAX_DIM || W > POWER_SPECTRUM_MAX_DIM)
        return 1;
    if (ps_lds_bytes(H, W) > 160 * 1024) return 1;  // cannot happen within POWER_SPECTRUM_MAX_DIM: 152 KB at 1024 x 1024
    PowerSpectrumPlan p;
    p.tiles = (W / 2 + 1 + 15) / 16;
    p.nky = (H + 15) / 16;
    p.n_bins = (H > W ? H : W) / 2 + 1;
    const long long per_wg = 4LL * p.nky * 256 + 4LL * (p.n_bins + 1) + ((long long)H * W + 1) / 2;  // planes, bins, share of xbar (over-counted)
    // every product below is checked against the cap by division first: nothing overflows
    const long long cap = POWER_SPECTRUM_MAX_WORKSPACE / per_wg / p.tiles / n_segments;  // B x C
    if (batch > cap || channels > cap / batch) return -1;
    p.fields = (long long)batch * channels;
    p.workgroups = (long long)n_segments * p.fields * p.tiles;
    p.mean_doubles = ((long long)n_segments * p.fields * H * W + 1) / 2;
    p.plane_doubles = p.workgroups * 4 * p.nky * 256;
    p.partial_doubles = p.workgroups * 4 * (p.n_bins + 1);
    *plan = p;
    return 0;
}

hipError_t power_spectrum_tables_create(int H, int W, PowerSpectrumTables* t) {
    const int Wh = W / 2 + 1, tiles = (Wh + 15) / 16, n_bins = (H > W ? H : W) / 2 + 1;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<float> tab(3 * (size_t)W + 3 * (size_t)H);
    float* cW = tab.data();
    float *sW = cW + W, *cH = sW + W, *sH = cH + H, *winH = sH + H, *winW = winH + H;
    for (int i = 0; i < W; ++i) {
        cW[i] = (float)std::cos(two_pi * i / W), sW[i] = (float)std::sin(two_pi * i / W);
        winW[i] = (float)(0.5 * (1.0 - std::cos(two_pi * i / W)));
    }
    for (int i = 0; i < H; ++i) {
        cH[i] = (float)std::cos(two_pi * i / H), sH[i] = (float)std::sin(two_pi * i / H);
        winH[i] = (float)(0.5 * (1.0 - std::cos(two_pi * i / H)));
    }
    // per tile: the coefficients (ky < H, kx <= W / 2) sorted by shell, (ky, kx) order inside a shell; the corners are shell n_bins
    std::vector<unsigned short> idx((size_t)tiles * H * 16, 0);
    std::vector<int> off((size_t)tiles * (n_bins + 2), 0);
    std::vector<int> bins((size_t)H * 16);
    for (int tl = 0; tl < tiles; ++tl) {
        int* o = off.data() + (size_t)tl * (n_bins + 2);
        const int cols = std::min(16, Wh - tl * 16);
        for (int ky = 0; ky < H; ++ky)
            for (int x = 0; x < cols; ++x) {
                const int b = std::min(power_spectrum_bin(H, W, ky, tl * 16 + x), n_bins);
                bins[(size_t)ky * 16 + x] = b;
                ++o[b + 1];
            }
        for (int b = 0; b <= n_bins; ++b) o[b + 1] += o[b];
        std::vector<int> at(o, o + n_bins + 1);
        for (int ky = 0; ky < H; ++ky)
            for (int x = 0; x < cols; ++x) idx[(size_t)tl * H * 16 + at[bins[(size_t)ky * 16 + x]]++] = (unsigned short)(ky * 16 + x);
    }
    PowerSpectrumTables r;
    r.H = H, r.W = W;
    hipError_t e = hipMalloc((void**)&r.tables, tab.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&r.csr_idx, idx.size() * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMalloc((void**)&r.csr_off, off.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(r.tables, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r.csr_idx, idx.data(), idx.size() * sizeof(unsigned short), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r.csr_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        power_spectrum_tables_destroy(&r);
        return e;
    }
    *t = r;
    return hipSuccess;
}

void power_spectrum_tables_destroy(PowerSpectrumTables* t) {
    if (t->tables) (void)hipFree(t->tables);
    if (t->csr_idx) (void)hipFree(t->csr_idx);
    if (t->csr_off) (void)hipFree(t->csr_off);
    t->tables = nullptr, t->csr_idx = nullptr, t->csr_off = nullptr;
}

hipError_t launch_power_spectrum(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                 long long member_stride, int batch, int channels, int H, int W, int window,
                                 const PowerSpectrumTables& t, double* workspace, double* out, double* accum, hipStream_t s) {
    PowerSpectrumPlan p;
    if (power_spectrum_plan(n_segments, n_members, batch, channels, H, W, &p) != 0 || t.H != H || t.W != W || (window != 0 && window != 1))
        return hipErrorInvalidValue;
    static bool lds_set = false;  // the kernel's dynamic LDS may exceed the default 64 KB
    if (!lds_set) {
        const hipError_t e = hipFuncSetAttribute((const void*)power_spectrum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        lds_set = true;
    }
    float* xbar = (float*)workspace;
    double* planes = workspace + p.mean_doubles;
    double* partials = planes + p.plane_doubles;
    const long long points = p.fields * H * W;
    dyf_form_note("power_spectrum_kernel:dft16x16x4", 0);
    hipLaunchKernelGGL(power_spectrum_mean_kernel, dim3((unsigned)((points + 255) / 256), (unsigned)n_segments), dim3(256), 0, s, preds_tab,
                       n_members, member_stride, points, xbar);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    PsArgs a;
    a.preds_tab = preds_tab, a.targets_tab = targets_tab, a.xbar = xbar, a.tables = t.tables, a.csr_idx = t.csr_idx, a.csr_off = t.csr_off;
    a.planes = planes, a.partials = partials, a.member_stride = member_stride, a.n_members = n_members, a.channels = channels;
    a.H = H, a.W = W, a.Wh = W / 2 + 1, a.tiles = p.tiles, a.Hp = (H + 3) / 4 * 4, a.nky = p.nky, a.n_bins1 = p.n_bins + 1, a.window = window;
    hipLaunchKernelGGL(power_spectrum_kernel, dim3((unsigned)(p.fields * p.tiles), (unsigned)n_segments), dim3(256), ps_lds_bytes(H, W), s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(power_spectrum_join_kernel, dim3((unsigned)channels, (unsigned)n_segments), dim3(256), 0, s, partials, n_members, batch,
                       p.tiles, p.n_bins + 1, (double)H * (double)W, out, accum);
    return hipGetLastError();
}
