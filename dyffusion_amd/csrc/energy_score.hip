// Energy score and member-distance matrix of an ensemble (gfx950; dyf_energy_score): per VECTOR of points (one (outer, group) slab of
// the geometry of ensemble_scores_kernel) the Euclidean distances d_i = ||x_i - y|| of every member to the target and D_ij = ||x_i -
// x_j|| between the members, then per (segment, group) their means over outer and the scores built from them.  The reference has no
// counterpart; float64 numpy written from the definition is what the results are held to (tests/energy_score_refs.py).
//   This is an N x N "distance GEMM" over the points of a vector, not a reduction over the members of a point.  The f32-input MFMA
// runs at the vector rate and a Gram-matrix form (|a|^2 + |b|^2 - 2 a.b) cancels for close members, so the differences are taken
// directly on the VALU: diff in fp32, squares accumulated with fmaf over one tile of ENERGY_SCORE_TILE_POINTS points, the tile sums
// added in float64.
//   Mapping (launch 1, energy_score_kernel).  A workgroup owns (segment; vector, block pair (bi <= bj) of 64-member slabs, chunk):
// blockIdx.y is the segment, blockIdx.x = (vector * block_pairs + pair) * chunks + chunk; a chunk walks tiles_per_chunk consecutive
// tiles of the vector.  The 256 threads are 16 x 16, thread (ti, tj) owns the 4 x 4 pairs (64 bi + 4 ti + r, 64 bj + 4 tj + c): 16
// fp32 tile accumulators and 16 float64 running sums.  The two slabs of a tile are staged in LDS transposed to [point][member]: a
// staging thread loads the four members of one quad at one point (consecutive lanes -> consecutive points of a member: coalesced)
// and stores them with one ds_write_b128; with the row pitch of 68 floats the 8 lanes of a store group cover 8 x 4 distinct banks
// (point * 68 + 4 quad -> bank 4 point mod 32 ...).  The next tile's loads are issued before the current tile is computed.  In the
// pair loop every lane of a wave reads the SAME point row: one ds_read_b128 of the thread's four bi-members (the 16 lanes of a
// read group hold 16 different quads of one 64-float row: 64 banks, no conflict) and one of its four bj-members (a broadcast), 32
// VALU operations per two LDS reads.  Diagonal pairs (bi == bj) stage one slab and the target; their threads tj == 0 also
// accumulate d_i.  Slots past n_members and points past the vector's end are staged as 0.0 (never NaN) and masked when the sums
// are written, so up to 64 members every prediction is read from HBM once, and at most ceil(N / 64) times beyond.
//   A vector is split into chunks only where a segment has too few work items to fill the chip (energy_score_plan); every workgroup
// writes its float64 sums of squares to the workspace (partial sums of squares, never of square roots).  Launch 2
// (energy_score_distances_kernel) adds a vector's chunks in chunk order, takes the float64 square root once per vector and the mean
// over outer in outer order; launch 3 (energy_score_finish_kernel) sums members and pairs in index order and writes the planes and
// the optional matrices.  No atomics, nothing is exchanged between workgroups inside a launch: a (segment, group) depends on its
// own data and the geometry alone.
#include "kernels.h"

#include <algorithm>

constexpr int ES_K = ENERGY_SCORE_TILE_POINTS;  // points per tile
constexpr int ES_PITCH4 = 17;                   // float4s per staged point row: 64 members + 4 floats of padding
static_assert(ES_K == 64, "the staging below moves 64 points x 16 quads with 256 threads in four rounds");

struct es_stage {  // one tile of one slab in registers: round r holds (point tid % 64, quad tid / 64 + 4 r)
    float4 v[4];
};

__device__ __forceinline__ es_stage es_load(const float* preds, long long member_stride, int n_members, int m0, long long base,
                                            long long q0, long long n_inner, int tid) {
    es_stage st;
    const int p = tid & 63;
    const bool in_vector = q0 + p < n_inner;
    const float* src = preds + base + q0 + p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + 4 * ((tid >> 6) + 4 * r);
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = in_vector && m + k < n_members ? src[(long long)(m + k) * member_stride] : 0.0f;
        st.v[r] = make_float4(x[0], x[1], x[2], x[3]);
    }
    return st;
}

__device__ __forceinline__ void es_store(float4* slab, const es_stage& st, int tid) {
    const int p = tid & 63;
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[p * ES_PITCH4 + (tid >> 6) + 4 * r] = st.v[r];
}

__global__ __launch_bounds__(256) void energy_score_kernel(const float* const* preds_tab, const float* const* targets_tab, int n_members,
                                                           long long member_stride, long long n_inner, long long vectors, int n_blocks,
                                                           int block_pairs, int chunks, long long tiles, long long tiles_per_chunk,
                                                           double* partials) {
    __shared__ float4 xa[ES_K * ES_PITCH4];
    __shared__ float4 xb[ES_K * ES_PITCH4];
    __shared__ float ys[ES_K];
    const float* preds = preds_tab[blockIdx.y];
    const float* targets = targets_tab[blockIdx.y];
    const int tid = threadIdx.x, ti = tid & 15, tj = tid >> 4;
    const int c = blockIdx.x % chunks;
    const long long vp = blockIdx.x / chunks;
    const long long vec = vp / block_pairs;
    int pair = (int)(vp - vec * block_pairs), bi = 0;
    while (pair >= n_blocks - bi) pair -= n_blocks - bi, ++bi;  // pairs in the order (0,0) (0,1) .. (0,B-1) (1,1) ..
    const int bj = bi + pair;
    const bool diag = bi == bj;
    const long long base = vec * n_inner;  // row-major (outer, group, inner): vector (o, g) starts at (o * n_groups + g) * n_inner
    const long long t0 = (long long)c * tiles_per_chunk, t1 = min(tiles, t0 + tiles_per_chunk);

    float acc[4][4], accy[4];
    double sum[4][4], sumy[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        accy[r] = 0.0f, sumy[r] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[r][k] = 0.0f, sum[r][k] = 0.0;
    }
    const float4* rows_b = diag ? xa : xb;
    es_stage sa, sb;
    float sy = 0.0f;
    sa = es_load(preds, member_stride, n_members, 64 * bi, base, t0 * ES_K, n_inner, tid);
    if (!diag) sb = es_load(preds, member_stride, n_members, 64 * bj, base, t0 * ES_K, n_inner, tid);
    if (diag && tid < ES_K) sy = t0 * ES_K + tid < n_inner ? targets[base + t0 * ES_K + tid] : 0.0f;
    for (long long t = t0; t < t1; ++t) {
        __syncthreads();  // the tile before has been read
        es_store(xa, sa, tid);
        if (!diag) es_store(xb, sb, tid);
        if (diag && tid < ES_K) ys[tid] = sy;
        __syncthreads();
        if (t + 1 < t1) {  // in flight while this tile is computed
            sa = es_load(preds, member_stride, n_members, 64 * bi, base, (t + 1) * ES_K, n_inner, tid);
            if (!diag) sb = es_load(preds, member_stride, n_members, 64 * bj, base, (t + 1) * ES_K, n_inner, tid);
            if (diag && tid < ES_K) sy = (t + 1) * ES_K + tid < n_inner ? targets[base + (t + 1) * ES_K + tid] : 0.0f;
        }
#pragma unroll 4
        for (int p = 0; p < ES_K; ++p) {
            const float4 a4 = xa[p * ES_PITCH4 + ti], b4 = rows_b[p * ES_PITCH4 + tj];
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = a[r] - b[k];
                    acc[r][k] = fmaf(d, d, acc[r][k]);
                }
            if (diag && tj == 0) {
                const float y = ys[p];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = a[r] - y;
                    accy[r] = fmaf(d, d, accy[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sumy[r] += (double)accy[r], accy[r] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) sum[r][k] += (double)acc[r][k], acc[r][k] = 0.0f;
        }
    }
    // entry (i, j), i < j < N: members i and j; entry (i, N): member i and the target.  Every such entry has exactly one writer.
    const int n1 = n_members + 1;
    double* part = partials + (((long long)blockIdx.y * vectors + vec) * chunks + c) * ((long long)n_members * n1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 64 * bi + 4 * ti + r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = 64 * bj + 4 * tj + k;
            if (i < j && j < n_members) part[(long long)i * n1 + j] = sum[r][k];
        }
        if (diag && tj == 0 && i < n_members) part[(long long)i * n1 + n_members] = sumy[r];
    }
}

// blockIdx.y the segment, blockIdx.x = group * entry_blocks + entry block; thread -> entry e = i * (N + 1) + j with j > i: the mean
// over outer (in outer order) of sqrt(sum over the chunks in chunk order).
__global__ __launch_bounds__(256) void energy_score_distances_kernel(const double* partials, int n_members, long long n_outer, int n_groups,
                                                                     int chunks, int entry_blocks, double* means) {
    const int g = blockIdx.x / entry_blocks, eb = blockIdx.x - g * entry_blocks;
    const int n1 = n_members + 1, entries = n_members * n1;
    const int e = eb * 256 + threadIdx.x;
    if (e >= entries) return;
    const int i = e / n1, j = e - i * n1;
    if (j <= i) return;
    const long long vectors = n_outer * n_groups;
    double total = 0.0;
    for (long long o = 0; o < n_outer; ++o) {
        const double* part = partials + (((long long)blockIdx.y * vectors + o * n_groups + g) * chunks) * (long long)entries + e;
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += part[(long long)c * entries];
        total += sqrt(s);
    }
    means[((long long)blockIdx.y * n_groups + g) * entries + e] = total / (double)n_outer;
}

// One workgroup per (segment, group): blockIdx.x the group, blockIdx.y the segment; thread i owns member i (n_members <= 256).
__global__ __launch_bounds__(256) void energy_score_finish_kernel(const double* means, int n_members, double* out, double* member_out,
                                                                  double* pair_out, double* accum) {
    __shared__ double row[ENERGY_SCORE_MAX_MEMBERS];
    __shared__ double dst[ENERGY_SCORE_MAX_MEMBERS];
    const int i = threadIdx.x, n1 = n_members + 1;
    const long long sg = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const double* m = means + sg * n_members * n1;
    if (i < n_members) {
        double s = 0.0;
        for (int j = i + 1; j < n_members; ++j) s += m[(long long)i * n1 + j];
        row[i] = s;
        dst[i] = m[(long long)i * n1 + n_members];
        if (member_out) member_out[sg * n_members + i] = dst[i];
        if (pair_out) {
            double* po = pair_out + (sg * n_members + i) * n_members;
            for (int j = 0; j < n_members; ++j) po[j] = j == i ? 0.0 : j < i ? m[(long long)j * n1 + i] : m[(long long)i * n1 + j];
        }
    }
    __syncthreads();
    if (i == 0) {
        double pairs = 0.0, target = 0.0;
        for (int k = 0; k < n_members; ++k) pairs += row[k], target += dst[k];
        const double n = (double)n_members;
        const double dist_target = target / n;
        const double dist_pair = 2.0 * pairs / (n * (n - 1.0));  // N = 1: 0 / 0 = NaN
        const double v[4] = {n_members > 1 ? dist_target - (n - 1.0) / (2.0 * n) * dist_pair : dist_target, dist_target - 0.5 * dist_pair,
                             dist_target, dist_pair};
        const long long planes = (long long)gridDim.y * gridDim.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            out[k * planes + sg] = v[k];
            if (accum) accum[k * planes + sg] += v[k];
        }
    }
}

int energy_score_plan(int n_segments, int n_members, long long n_outer, int n_groups, long long n_inner, EnergyScorePlan* plan) {
    if (n_segments < 1 || n_members < 1 || n_members > ENERGY_SCORE_MAX_MEMBERS || n_outer < 1 || n_groups < 1 || n_inner < 1) return 1;
    EnergyScorePlan p;
    p.blocks = (n_members + 63) / 64;
    p.block_pairs = p.blocks * (p.blocks + 1) / 2;
    const long long entries = (long long)n_members * (n_members + 1);
    // every product below is checked against the cap by division first: nothing overflows
    const long long cap = ENERGY_SCORE_MAX_WORKSPACE / entries / n_segments;  // vectors x chunks, and groups, per segment
    if (n_outer > cap || (long long)n_groups > cap / n_outer) return -1;
    p.vectors = n_outer * n_groups;
    const long long tiles = (n_inner - 1) / ENERGY_SCORE_TILE_POINTS + 1;
    const long long items = p.vectors * p.block_pairs;  // per segment
    const long long want = std::min<long long>(tiles, std::max<long long>(1, 256 / items));
    p.tiles_per_chunk = (tiles + want - 1) / want;
    p.chunks = (int)((tiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk);  // no empty chunk
    if (p.vectors > cap / p.chunks) return -1;
    p.partial_doubles = (long long)n_segments * p.vectors * p.chunks * entries;
    p.mean_doubles = (long long)n_segments * n_groups * entries;
    if (p.partial_doubles + p.mean_doubles > ENERGY_SCORE_MAX_WORKSPACE) return -1;
    *plan = p;
    return 0;
}

hipError_t launch_energy_score(const float* const* preds_tab, const float* const* targets_tab, int n_segments, int n_members,
                               long long member_stride, long long n_outer, int n_groups, long long n_inner, double* workspace,
                               double* out, double* member_out, double* pair_out, double* accum, hipStream_t s) {
    EnergyScorePlan p;
    if (energy_score_plan(n_segments, n_members, n_outer, n_groups, n_inner, &p) != 0 || n_segments > 65535) return hipErrorInvalidValue;
    // the workspace cap keeps vectors x chunks below 2^27 and with it every grid below 2^31 workgroups along x
    const long long tiles = (n_inner - 1) / ENERGY_SCORE_TILE_POINTS + 1;
    const int entry_blocks = (n_members * (n_members + 1) + 255) / 256;
    double* means = workspace + p.partial_doubles;
    dyf_form_note("energy_score_kernel:pairs4x4", 0);
    hipLaunchKernelGGL(energy_score_kernel, dim3((unsigned)(p.vectors * p.block_pairs * p.chunks), (unsigned)n_segments), dim3(256), 0, s,
                       preds_tab, targets_tab, n_members, member_stride, n_inner, p.vectors, p.blocks, p.block_pairs, p.chunks, tiles,
                       p.tiles_per_chunk, workspace);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(energy_score_distances_kernel, dim3((unsigned)((long long)n_groups * entry_blocks), (unsigned)n_segments), dim3(256),
                       0, s, workspace, n_members, n_outer, n_groups, p.chunks, entry_blocks, means);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(energy_score_finish_kernel, dim3((unsigned)n_groups, (unsigned)n_segments), dim3(256), 0, s, means, n_members, out,
                       member_out, pair_out, accum);
    return hipGetLastError();
}
