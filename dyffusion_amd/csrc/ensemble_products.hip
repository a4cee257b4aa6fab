// Ensemble forecast products and rank histograms (gfx950): the per-point reductions over the members of an (N, B, C, H, W) forecast
// stack that a user of a probabilistic forecast asks for -- mean, spread, extremes, quantiles, exceedance probabilities
// (dyf_ensemble_products) -- and the Talagrand diagram of the truth among the members (dyf_rank_histogram).  The reference has no
// counterpart; numpy (np.mean / np.std / np.min / np.max / np.quantile "linear" / (x > t).mean()) is what the fields are held to.
#include "kernels.h"

#include <algorithm>

// ------------------------------------------------------------------------------------------------ ensemble products
// Work mapping and staging are those of trajectory_metrics_kernel: every prediction is read once, coalesced (consecutive threads ->
// consecutive points of one member), into LDS, and K planes are written, coalesced.
//   up to 64 members   256 points per workgroup, one thread per point.  The members are staged in fours, xs[quad][thread] as float4
//                      (ensemble_size_metrics_kernel's layout: ds_read_b128 on consecutive 16-byte slots, conflict-free); the slots
//                      past n_members hold NaN, which no comparison below counts.  A thread reads only what it wrote: no barrier.
//   beyond             P = ensemble_tile_points() points per workgroup, T = 256 / P threads per point, xs[member][P]; thread share k
//                      takes the members k, k + T, ...; partial sums / extremes / counts of the T shares are joined by every share
//                      in share order (ensemble_metrics_tiled_kernel's join), so the result does not depend on which thread asks.
// mean = sum * (1 / N) with the sum in member order, var = sum (x - mean)^2 * (1 / N), std = sqrtf(var): the fp32 expressions of
// trajectory_metrics_kernel.  min / max are exact.
//   Selection: rank by counting.  rank(i) = #{j : x_j < x_i} + #{j < i : x_j == x_i} is a permutation of 0..N-1, so each wanted
// order statistic lo / hi of a quantile is held by exactly one member, found with N comparisons straight out of the staged column:
// no LDS writes, no data-dependent control flow, the access pattern of the CRPS pair term.  The one-thread form ranks four members
// at a time against one ds_read_b128 of four others (16 comparisons per LDS read: N^2 bytes of LDS traffic per point, not 4 N^2);
// the tie-break needs no equality test -- members in front of i are compared with <=, those behind with <.  A sort would move the
// column through LDS log^2 N times and needs a power-of-two pad; a selection by partition diverges within the wave.
//   quantile = x_(lo) + frac * (x_(hi) - x_(lo)) without contraction, lo / hi / frac (fp32) from the host ((N - 1) q in double); with
// frac == 0 it is x_(lo) itself.  exceedance = (float)#{x_n > t} / (float)N, one correctly rounded division.
//   NaN: a point with a NaN member gives NaN in every plane but the exceedances, which count the comparisons that are true.
// No atomics, nothing is exchanged between workgroups, a point's outputs depend on its own members alone.
struct products_planes {  // the first plane of each kind (a plane that is not asked for is never written)
    int mean, std, min, max, quantiles, thresholds;
};

__device__ __forceinline__ products_planes products_plane_map(const EnsembleProductsParams& pr) {
    products_planes m;
    int k = 0;
    m.mean = k, k += pr.mean;
    m.std = k, k += pr.std;
    m.min = k, k += pr.min;
    m.max = k, k += pr.max;
    m.quantiles = k, k += pr.n_quantiles;
    m.thresholds = k;
    return m;
}

__device__ __forceinline__ float products_lerp(float lo, float hi, float frac) {
    float v = lo;
    if (frac != 0.0f) {
#pragma clang fp contract(off)  // a product and a sum, each rounded once
        v = lo + frac * (hi - lo);
    }
    return v;
}

__global__ __launch_bounds__(256) void ensemble_products_kernel(const float* const* preds_tab, int n_members, long long n_points,
                                                                long long member_stride, EnsembleProductsParams pr, float* out,
                                                                int n_planes) {
    extern __shared__ float4 products_lds[];  // [quads][256]
    float4* xs = products_lds;
    const int tid = threadIdx.x, n_quads = (n_members + 3) >> 2, nq = pr.n_quantiles;
    const long long p = (long long)blockIdx.x * 256 + tid;
    if (p >= n_points) return;  // no barrier below
    const float* column = preds_tab[blockIdx.y] + p;
    float* dst = out + (long long)blockIdx.y * n_planes * n_points + p;
    const products_planes at = products_plane_map(pr);
    const float nan = __builtin_nanf("");
    float sum = 0.0f, mn = __builtin_inff(), mx = -__builtin_inff();
    bool bad = false;
    for (int q0 = 0; q0 < n_quads; q0 += 4) {  // 16 dword loads in flight per lane, then their four LDS writes
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = column[(long long)min(4 * q0 + i, n_members - 1) * member_stride];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (4 * q0 + i < n_members) {
                sum += v[i];
                mn = fminf(mn, v[i]);
                mx = fmaxf(mx, v[i]);
                bad |= v[i] != v[i];
            } else {
                v[i] = nan;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q0 + u < n_quads) xs[(q0 + u) * 256 + tid] = make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
    }
    const float inv = 1.0f / (float)n_members;
    const float mean = sum * inv;
    if (pr.mean) dst[at.mean * n_points] = mean;  // NaN already where a member is
    if (pr.std) {
        float m2 = 0.0f;
        for (int q = 0; q < n_quads; ++q) {
            const float4 o = xs[q * 256 + tid];
            const float x[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (4 * q + a < n_members) m2 += (x[a] - mean) * (x[a] - mean);
        }
        dst[at.std * n_points] = sqrtf(m2 * inv);
    }
    if (pr.min) dst[at.min * n_points] = bad ? nan : mn;
    if (pr.max) dst[at.max * n_points] = bad ? nan : mx;
    if (nq > 0) {
        float vlo[ENSEMBLE_PRODUCTS_MAX_QUANTILES], vhi[ENSEMBLE_PRODUCTS_MAX_QUANTILES];
#pragma unroll
        for (int k = 0; k < ENSEMBLE_PRODUCTS_MAX_QUANTILES; ++k) vlo[k] = vhi[k] = 0.0f;
        for (int qi = 0; qi < n_quads; ++qi) {
            const float4 me = xs[qi * 256 + tid];
            const float x[4] = {me.x, me.y, me.z, me.w};
            int rank[4] = {0, (int)(x[0] <= x[1]), (int)(x[0] <= x[2]) + (int)(x[1] <= x[2]),
                           (int)(x[0] <= x[3]) + (int)(x[1] <= x[3]) + (int)(x[2] <= x[3])};
            rank[0] += (int)(x[1] < x[0]) + (int)(x[2] < x[0]) + (int)(x[3] < x[0]);
            rank[1] += (int)(x[2] < x[1]) + (int)(x[3] < x[1]);
            rank[2] += (int)(x[3] < x[2]);
            for (int qj = 0; qj < qi; ++qj) {  // members in front: a tie ranks them first
                const float4 o = xs[qj * 256 + tid];
#pragma unroll
                for (int a = 0; a < 4; ++a) rank[a] += ((int)(o.x <= x[a]) + (int)(o.y <= x[a])) + ((int)(o.z <= x[a]) + (int)(o.w <= x[a]));
            }
            for (int qj = qi + 1; qj < n_quads; ++qj) {  // members behind (the NaN slots past n_members count nowhere)
                const float4 o = xs[qj * 256 + tid];
#pragma unroll
                for (int a = 0; a < 4; ++a) rank[a] += ((int)(o.x < x[a]) + (int)(o.y < x[a])) + ((int)(o.z < x[a]) + (int)(o.w < x[a]));
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (4 * qi + a < n_members) {
#pragma unroll
                    for (int k = 0; k < ENSEMBLE_PRODUCTS_MAX_QUANTILES; ++k) {  // static register indices; k < nq is uniform
                        if (k < nq) {
                            if (rank[a] == pr.lo[k]) vlo[k] = x[a];
                            if (rank[a] == pr.hi[k]) vhi[k] = x[a];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < ENSEMBLE_PRODUCTS_MAX_QUANTILES; ++k)
            if (k < nq) dst[(at.quantiles + k) * n_points] = bad ? nan : products_lerp(vlo[k], vhi[k], pr.frac[k]);
    }
    for (int k = 0; k < pr.n_thresholds; ++k) {
        const float t = pr.thresholds[k];
        int count = 0;
        for (int q = 0; q < n_quads; ++q) {
            const float4 o = xs[q * 256 + tid];
            count += ((int)(o.x > t) + (int)(o.y > t)) + ((int)(o.z > t) + (int)(o.w > t));
        }
        dst[(at.thresholds + k) * n_points] = (float)count / (float)n_members;
    }
}

// more than 64 members: P points per workgroup, T = 256 / P threads share a point
__global__ __launch_bounds__(256) void ensemble_products_tiled_kernel(const float* const* preds_tab, int n_members, long long n_points,
                                                                      long long member_stride, EnsembleProductsParams pr, float* out,
                                                                      int n_planes, int P) {
    extern __shared__ float4 products_lds[];  // floats: [n_members][P] members, [4][256] partials, [2 n_quantiles][P] order statistics
    float* xs = (float*)products_lds;
    float* red = xs + (size_t)n_members * P;
    float* sel = red + 4 * 256;
    const float* preds = preds_tab[blockIdx.y];
    const int tid = threadIdx.x, T = 256 / P, nq = pr.n_quantiles;
    const int pi = tid % P, sh = tid / P;
    const long long p0 = (long long)blockIdx.x * P;
    const bool writes = p0 + pi < n_points && sh == 0;
    for (int i = tid; i < n_members * P; i += 256) {  // staging: consecutive threads -> consecutive points of one member
        const int n = i / P, q = i - n * P;
        xs[i] = p0 + q < n_points ? preds[(long long)n * member_stride + p0 + q] : 0.0f;
    }
    __syncthreads();
    const float nan = __builtin_nanf("");
    float sum = 0.0f, mn = __builtin_inff(), mx = -__builtin_inff(), bad = 0.0f;
    for (int n = sh; n < n_members; n += T) {
        const float x = xs[n * P + pi];
        sum += x;
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
        if (x != x) bad = 1.0f;
    }
    red[tid] = sum;
    red[256 + tid] = mn;
    red[512 + tid] = mx;
    red[768 + tid] = bad;
    __syncthreads();
    float tsum = 0.0f, tmn = __builtin_inff(), tmx = -__builtin_inff(), tbad = 0.0f;
    for (int k = 0; k < T; ++k) {  // every share joins the T partials in the same order: all hold the same mean
        tsum += red[k * P + pi];
        tmn = fminf(tmn, red[256 + k * P + pi]);
        tmx = fmaxf(tmx, red[512 + k * P + pi]);
        tbad += red[768 + k * P + pi];
    }
    const float inv = 1.0f / (float)n_members;
    const float mean = tsum * inv;
    __syncthreads();  // the partials are read: the rows are free again
    float m2 = 0.0f;
    for (int n = sh; n < n_members; n += T) {
        const float x = xs[n * P + pi];
        m2 += (x - mean) * (x - mean);
        if (nq > 0) {
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += (int)(xs[j * P + pi] <= x);
            for (int j = n + 1; j < n_members; ++j) rank += (int)(xs[j * P + pi] < x);
            for (int k = 0; k < nq; ++k) {  // one member of the point holds each rank: one writer per slot
                if (rank == pr.lo[k]) sel[(2 * k) * P + pi] = x;
                if (rank == pr.hi[k]) sel[(2 * k + 1) * P + pi] = x;
            }
        }
    }
    red[tid] = m2;
    __syncthreads();
    const products_planes at = products_plane_map(pr);
    float* dst = out + (long long)blockIdx.y * n_planes * n_points + p0 + pi;
    if (writes) {
        if (pr.mean) dst[at.mean * n_points] = mean;
        if (pr.std) {
            float tm2 = 0.0f;
            for (int k = 0; k < T; ++k) tm2 += red[k * P + pi];
            dst[at.std * n_points] = sqrtf(tm2 * inv);
        }
        if (pr.min) dst[at.min * n_points] = tbad != 0.0f ? nan : tmn;
        if (pr.max) dst[at.max * n_points] = tbad != 0.0f ? nan : tmx;
        for (int k = 0; k < nq; ++k)
            dst[(at.quantiles + k) * n_points] = tbad != 0.0f ? nan : products_lerp(sel[(2 * k) * P + pi], sel[(2 * k + 1) * P + pi], pr.frac[k]);
    }
    for (int k = 0; k < pr.n_thresholds; ++k) {  // uniform trip count: the barriers are met by every thread
        const float t = pr.thresholds[k];
        int count = 0;
        for (int n = sh; n < n_members; n += T) count += (int)(xs[n * P + pi] > t);
        red[256 + tid] = (float)count;  // at most 15 360: exact
        __syncthreads();
        if (writes) {
            float total = 0.0f;
            for (int s = 0; s < T; ++s) total += red[256 + s * P + pi];
            dst[(at.thresholds + k) * n_points] = total / (float)n_members;
        }
        __syncthreads();
    }
}

long long ensemble_products_blocks(int n_members, long long n_points) {
    const int P = ensemble_tile_points(n_members);
    return P && n_points >= 1 ? (n_points + P - 1) / P : 0;
}

hipError_t launch_ensemble_products(const float* const* preds_tab, int n_segments, int n_members, long long n_points,
                                    long long member_stride, const EnsembleProductsParams& pr, float* out, hipStream_t s) {
    const int P = ensemble_tile_points(n_members);
    const long long blocks = ensemble_products_blocks(n_members, n_points);
    const int n_planes = pr.mean + pr.std + pr.min + pr.max + pr.n_quantiles + pr.n_thresholds;
    // 256 * blocks threads along x stay below 2^32
    if (P == 0 || blocks < 1 || blocks > ENSEMBLE_PRODUCTS_MAX_BLOCKS || n_segments < 1 || n_segments > 65535 || n_planes < 1 ||
        pr.n_quantiles < 0 || pr.n_quantiles > ENSEMBLE_PRODUCTS_MAX_QUANTILES || pr.n_thresholds < 0 ||
        pr.n_thresholds > ENSEMBLE_PRODUCTS_MAX_THRESHOLDS)
        return hipErrorInvalidValue;
    for (int k = 0; k < pr.n_quantiles; ++k)
        if (pr.lo[k] < 0 || pr.lo[k] >= n_members || pr.hi[k] < pr.lo[k] || pr.hi[k] >= n_members) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)n_segments);
    if (n_members > 64) {
        // at most 60 KB of members, 4 KB of partials and 16 KB of order statistics (16 quantiles at P = 128)
        const size_t lds = ((size_t)n_members * P + 4 * 256 + (size_t)2 * pr.n_quantiles * P) * sizeof(float);
        hipError_t e = hipFuncSetAttribute((const void*)ensemble_products_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        if (e != hipSuccess) return e;
        dyf_form_note("ensemble_products_kernel:tiled", 0);
        hipLaunchKernelGGL(ensemble_products_tiled_kernel, grid, dim3(256), lds, s, preds_tab, n_members, n_points, member_stride, pr,
                           out, n_planes, P);
    } else {
        dyf_form_note("ensemble_products_kernel:quads", 0);
        hipLaunchKernelGGL(ensemble_products_kernel, grid, dim3(256), (size_t)((n_members + 3) / 4) * 256 * sizeof(float4), s, preds_tab,
                           n_members, n_points, member_stride, pr, out, n_planes);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ rank histogram
// The Talagrand diagram per (segment, GROUP), the geometry of ensemble_scores_kernel: a segment's points are row-major (n_outer,
// n_groups, n_inner), point p belongs to group (p / n_inner) % n_groups.  For a point with target y, b = #{x_n < y} and e = #{x_n ==
// y}: each of the bins b .. b + e receives 1 / (e + 1), the uniform split of ties (a boundary-condition pixel, where every member IS
// the target, spreads over all N + 1 bins instead of piling into one).  A point whose target or any member is NaN adds nothing.
//   Work mapping: a group's work items are its (outer, tile) pairs, a tile being 256 consecutive points of one (outer, group) slab;
// blockIdx.x = group * n_chunks + chunk, and chunk c walks the items c, c + n_chunks, ... with n_chunks = min(items, 256), so a
// segment has at most 256 partial histograms per group whatever its size; blockIdx.y is the segment.  One thread per point streams
// the point's members (coalesced, eight loads in flight, nothing staged: b and e need one comparison each) and leaves (b, e, 1 /
// (e + 1)) in LDS; then thread i, the owner of bins i, i + 256, ..., walks the tile's 256 points in point order (every lane reads
// the same address: a broadcast) and adds the weights of those that cover its bins, in fp64, in registers.  No atomics: a bin's
// value is the sum over the chunk's points in (item, point) order, and rank_histogram_finish_kernel adds the chunks in chunk order.
// Without ties every addend is 1.0 and every bin an exact integer.
constexpr int RANK_HISTOGRAM_BINS_PER_THREAD = (RANK_HISTOGRAM_MAX_MEMBERS + 1 + 255) / 256;

__global__ __launch_bounds__(256) void rank_histogram_kernel(const float* const* preds_tab, const float* const* targets_tab, int n_members,
                                                             long long member_stride, long long n_outer, int n_groups, long long n_inner,
                                                             long long tiles_per_slab, int n_chunks, double* partials) {
    __shared__ int pb[256];
    __shared__ int pe[256];
    __shared__ double pw[256];
    const float* preds = preds_tab[blockIdx.y];
    const float* targets = targets_tab[blockIdx.y];
    const int tid = threadIdx.x;
    const int g = blockIdx.x / n_chunks, c = blockIdx.x - g * n_chunks;
    double h[RANK_HISTOGRAM_BINS_PER_THREAD];
#pragma unroll
    for (int s = 0; s < RANK_HISTOGRAM_BINS_PER_THREAD; ++s) h[s] = 0.0;
    const long long items = n_outer * tiles_per_slab;
    for (long long j = c; j < items; j += n_chunks) {
        const long long o = j / tiles_per_slab, t = j - o * tiles_per_slab;
        const long long q = t * 256 + tid;  // within the slab
        int b = 0, e = 0;
        bool counts = q < n_inner;
        if (counts) {
            const long long p = (o * n_groups + g) * n_inner + q;
            const float y = targets[p];
            const float* column = preds + p;
            bool bad = y != y;
            for (int n0 = 0; n0 < n_members; n0 += 8) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = column[(long long)min(n0 + i, n_members - 1) * member_stride];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (n0 + i < n_members) {
                        b += (int)(v[i] < y);
                        e += (int)(v[i] == y);
                        bad |= v[i] != v[i];
                    }
                }
            }
            counts = !bad;
        }
        __syncthreads();  // the walk over the tile before is done
        pb[tid] = counts ? b : 0;
        pe[tid] = counts ? e : 0;
        pw[tid] = counts ? 1.0 / (double)(e + 1) : 0.0;  // a point that does not count adds 0.0 to bin 0
        __syncthreads();
#pragma unroll
        for (int s = 0; s < RANK_HISTOGRAM_BINS_PER_THREAD; ++s) {
            const int i = tid + 256 * s;
            if (i <= n_members) {
                double acc = h[s];
                for (int pt = 0; pt < 256; ++pt) acc += (unsigned)(i - pb[pt]) <= (unsigned)pe[pt] ? pw[pt] : 0.0;
                h[s] = acc;
            }
        }
    }
    double* part = partials + (((long long)blockIdx.y * n_groups + g) * n_chunks + c) * (n_members + 1);
#pragma unroll
    for (int s = 0; s < RANK_HISTOGRAM_BINS_PER_THREAD; ++s) {
        const int i = tid + 256 * s;
        if (i <= n_members) part[i] = h[s];
    }
}

// One workgroup per (segment, group): blockIdx.x the group, blockIdx.y the segment; thread i adds the chunks of bins i, i + 256, ...
// in chunk order.  accum is read and written by this thread alone (ordered by the stream).
__global__ __launch_bounds__(256) void rank_histogram_finish_kernel(const double* partials, int n_chunks, int n_bins, double* out,
                                                                    double* accum) {
    const long long sg = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const double* part = partials + sg * n_chunks * n_bins;
    for (int i = threadIdx.x; i < n_bins; i += 256) {
        double s = 0.0;
        for (int c = 0; c < n_chunks; ++c) s += part[(long long)c * n_bins + i];
        out[sg * n_bins + i] = s;
        if (accum) accum[sg * n_bins + i] += s;
    }
}

int rank_histogram_chunks(int n_members, long long n_outer, int n_groups, long long n_inner) {
    if (n_members < 1 || n_members > RANK_HISTOGRAM_MAX_MEMBERS || n_outer < 1 || n_groups < 1 || n_inner < 1) return 0;
    const long long tiles = (n_inner + 255) / 256;
    if (!ensemble_geometry_fits(n_outer, n_groups, tiles)) return -1;  // the workgroup limit of dyf_ensemble_scores on this geometry
    return (int)std::min<long long>(tiles * n_outer, RANK_HISTOGRAM_MAX_CHUNKS);
}

hipError_t launch_rank_histogram(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                                 long long member_stride, long long n_outer, int n_groups, long long n_inner, double* partials,
                                 double* out, double* accum, hipStream_t s) {
    const int chunks = rank_histogram_chunks(n_members, n_outer, n_groups, n_inner);
    if (chunks < 1 || n_segments < 1 || n_segments > 65535) return hipErrorInvalidValue;
    const long long tiles = (n_inner + 255) / 256;
    dyf_form_note("rank_histogram_kernel:stream", 0);
    hipLaunchKernelGGL(rank_histogram_kernel, dim3((unsigned)((long long)n_groups * chunks), (unsigned)n_segments), dim3(256), 0, s,
                       preds_tab, targets_tab, n_members, member_stride, n_outer, n_groups, n_inner, tiles, chunks, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rank_histogram_finish_kernel, dim3((unsigned)n_groups, (unsigned)n_segments), dim3(256), 0, s, partials, chunks,
                       n_members + 1, out, accum);
    return hipGetLastError();
}
