// Engine-resident optimizer step: AdamW with global gradient-norm clipping and an EMA shadow of the weights, on the training copy of a
// network (TrainNet, train_internal.h) -- the last third of a training iteration.  Replaces, for the reference's
// torch.optim.AdamW + Lightning `gradient_clip_val` (torch.nn.utils.clip_grad_norm_) + LitEma (src/models/modules/ema.py), the round trip
// "export every gradient, run torch.optim on the module, upload every weight" (~270 repack launches each way per network).
//
// Layout.  TrainNet keeps every gradient in ONE block, g_arena, each parameter's slice at a 256-byte-aligned offset.  exp_avg (m),
// exp_avg_sq (v) and the EMA shadow live in three arenas with the same offsets, so one offset addresses g, m, v and the shadow of an
// element; the master weights stay where the training step reads them (RParam::w, and RParam::wt for convs).  A chunk table on the
// device (built once, and again when dyf_load_weights rebuilds the parameter copy) cuts every parameter into runs of OPT_CHUNK elements.
//
// One step = two launches on the caller's stream, no atomics, and no wait for anything the step itself launches (the host first reads the
// PREVIOUS step's outcome, copied to pinned memory behind that step: it runs at most one step ahead):
//   opt_grad_sumsq   g_arena as one flat array, <= 1024 workgroups, grid-stride, 16-byte loads, one double per workgroup in a fixed slot.
//                    The arena's alignment padding is zero and stays zero: the block is zero-filled when it is allocated (rn_fill_params,
//                    talloc zero = true), dyf_train_zero_grads clears the whole block, and every writer -- the weight-gradient kernels,
//                    the gradient import, the update below -- is handed a parameter's slice and its element count n, never the
//                    padded length.  So the padding adds exact zeros to the sum.
//   opt_adamw_step   every workgroup first sums the partials of launch 1 in ONE fixed order (lane t takes slots t, t + 256, ...; then a
//                    fixed tree), so the norm -- and with it the clip coefficient -- is bitwise the same in every workgroup and in every
//                    run.  A float atomic sum depends on arrival order and differs in the last bits from run to run; that difference
//                    would reach every weight through the clip coefficient.  Then the workgroup walks its chunks.
// The kernel zeroes each gradient after reading it: the resident loop needs no separate memset.
#include "engine_internal.h"
#include "train_internal.h"

using namespace dyf;

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

struct OptArgs {       // every scalar evaluated by the host in double and rounded once, as torch passes Python floats to its kernels
    float lr_decay;      // 1 - lr * weight_decay
    float one_m_b1, beta2, one_m_b2;
    float neg_step;      // -(lr / bc1)
    float bc2_sqrt;      // sqrt(bc2)
    float eps;
    float max_norm;      // <= 0: no clipping
    float ema_omd;       // 1 - ema_decay_now
    int ema;
};

__device__ __forceinline__ double block_sum_fixed(double x, double* red) {  // 256 threads, fixed tree: the same bits in every workgroup
    red[threadIdx.x] = x;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// launch 1: partial[blockIdx.x] = sum of g[i]^2 over the workgroup's grid-stride share (n4 = arena floats / 4; the arena is a multiple of 64)
__global__ __launch_bounds__(256) void opt_grad_sumsq(const float* __restrict__ g, long long n4, double* __restrict__ partial) {
    __shared__ double red[256];
    double s = 0.0;
    const f4* g4 = (const f4*)g;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f4 x = g4[i];
        s += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
    }
    s = block_sum_fixed(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one element: torch.optim.AdamW's single-tensor order -- mul_ (weight decay), lerp_ (exp_avg), mul_ + addcmul_ (exp_avg_sq),
// sqrt / div / add_ (denominator), addcdiv_ -- then LitEma's sub_.  The roundings are those of torch's vectorised fp32 CPU kernels, found
// by comparing against them bit for bit: lerp_ is one fma, addcmul_ is fma((1 - beta2) g, g, beta2 v), addcdiv_ is p + (value m) / denom
// with every operation rounded, the EMA update is unfused.  Contraction is off so that nothing else fuses; divide and sqrt are IEEE.
__device__ __forceinline__ void adamw_one(float& p, float& m, float& v, float& sh, float g, float coef, const OptArgs& a) {
#pragma clang fp contract(off)
    g = g * coef;
    p = p * a.lr_decay;
    m = fmaf(a.one_m_b1, g - m, m);
    const float vb = v * a.beta2, sg = a.one_m_b2 * g;
    v = fmaf(sg, g, vb);
    const float root = sqrtf(v) / a.bc2_sqrt;
    const float denom = root + a.eps;
    const float num = a.neg_step * m;
    const float upd = num / denom;
    p = p + upd;
    if (a.ema) {
        const float d = sh - p, sd = a.ema_omd * d;
        sh = sh - sd;
    }
}

// launch 2: grid-stride over the chunk table
__global__ __launch_bounds__(256) void opt_adamw_step(const OptChunk* __restrict__ chunks, int n_chunks, float* __restrict__ g_arena,
                                                      float* __restrict__ m_arena, float* __restrict__ v_arena, float* __restrict__ s_arena,
                                                      const double* __restrict__ partial, int n_partial, OptArgs a, OptStatus* status) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) s += partial[i];
    const double norm = sqrt(block_sum_fixed(s, red));
    const bool finite = norm <= 1.7976931348623157e308;  // false for inf and NaN
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        status->grad_norm = norm;
        status->skipped = finite ? 0 : 1;
    }
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1, in fp32
    const float coef = a.max_norm > 0.0f ? fminf(1.0f, a.max_norm / ((float)norm + 1e-6f)) : 1.0f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptChunk k = chunks[c];
        float* w = k.w + k.begin;
        float* g = g_arena + k.off + k.begin;
        float* m = m_arena + k.off + k.begin;
        float* v = v_arena + k.off + k.begin;
        float* sh = a.ema ? s_arena + k.off + k.begin : nullptr;
        // the arena slices are 256-byte aligned and chunks start at multiples of OPT_CHUNK: only w's own address decides
        const bool vec = ((((uintptr_t)w) | ((uintptr_t)g)) & 15u) == 0;
        const int n_vec = vec ? k.count / 4 : 0;
        if (!finite) {  // skipped step: the gradients are cleared, nothing else is touched
            for (int i = threadIdx.x; i < n_vec; i += 256) ((f4*)g)[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
            for (int i = n_vec * 4 + threadIdx.x; i < k.count; i += 256) g[i] = 0.0f;
            continue;
        }
        for (int i = threadIdx.x; i < n_vec; i += 256) {
            f4 p4 = ((f4*)w)[i], m4 = ((f4*)m)[i], v4 = ((f4*)v)[i];
            const f4 g4 = ((f4*)g)[i];
            f4 s4 = sh ? ((f4*)sh)[i] : f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p = p4[j], mm = m4[j], vv = v4[j], ss = s4[j];
                adamw_one(p, mm, vv, ss, g4[j], coef, a);
                p4[j] = p; m4[j] = mm; v4[j] = vv; s4[j] = ss;
            }
            ((f4*)w)[i] = p4;
            ((f4*)m)[i] = m4;
            ((f4*)v)[i] = v4;
            if (sh) ((f4*)sh)[i] = s4;
            ((f4*)g)[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
            if (k.wt) {
                const long long e0 = (long long)k.begin + 4ll * i;
#pragma unroll
                for (int j = 0; j < 4; ++j) k.wt[((e0 + j) % k.rest) * k.cout + (e0 + j) / k.rest] = p4[j];
            }
        }
        for (int i = n_vec * 4 + threadIdx.x; i < k.count; i += 256) {
            float p = w[i], mm = m[i], vv = v[i], ss = sh ? sh[i] : 0.0f;
            adamw_one(p, mm, vv, ss, g[i], coef, a);
            w[i] = p;
            m[i] = mm;
            v[i] = vv;
            if (sh) sh[i] = ss;
            g[i] = 0.0f;
            if (k.wt) {
                const long long e0 = (long long)k.begin + i;
                k.wt[(e0 % k.rest) * k.cout + e0 / k.rest] = p;
            }
        }
    }
}

// mode 0: shadow = w (LitEma.__init__); mode 1: w <-> shadow, wt follows w
__global__ __launch_bounds__(256) void opt_shadow(const OptChunk* __restrict__ chunks, int n_chunks, float* __restrict__ s_arena, int mode) {
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptChunk k = chunks[c];
        float* w = k.w + k.begin;
        float* sh = s_arena + k.off + k.begin;
        for (int i = threadIdx.x; i < k.count; i += 256) {
            const float p = w[i];
            if (mode == 0) {
                sh[i] = p;
            } else {
                const float q = sh[i];
                sh[i] = p;
                w[i] = q;
                if (k.wt) {
                    const long long e0 = (long long)k.begin + i;
                    k.wt[(e0 % k.rest) * k.cout + e0 / k.rest] = q;
                }
            }
        }
    }
}

inline unsigned opt_grid(long long work_items) { return (unsigned)std::max<long long>(1, std::min<long long>(work_items, OPT_MAX_PARTIALS)); }

// FNV-1a over every parameter's (name, arena offset, element count), in the map's order: two parameter copies with the same value have
// the same tensors at the same offsets, so m, v and the shadow of one address the other's elements
uint64_t layout_hash(const TrainNet& t) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull; };
    for (auto& kv : t.P) {
        if (kv.second.stat) continue;
        const uint64_t off = (uint64_t)(kv.second.g - t.g_arena), n = (uint64_t)kv.second.n;
        mix(kv.first.data(), kv.first.size() + 1);
        mix(&off, sizeof(off));
        mix(&n, sizeof(n));
    }
    return h;
}

dyf_status build_chunks(dyf_engine* e, TrainNet& t, TrainOptim& o) {
    std::vector<OptChunk> h;
    for (auto& kv : t.P) {
        const RParam& p = kv.second;
        if (p.stat) continue;  // BatchNorm running statistics: no gradient, in no chunk
        if (p.n >= ((size_t)1 << 31)) return fail(e, DYF_ERR_UNSUPPORTED, "optimizer: a parameter of 2^31 elements or more");
        for (size_t b = 0; b < p.n; b += OPT_CHUNK) {
            OptChunk c;
            c.w = p.w;
            c.wt = p.conv ? p.wt : nullptr;
            c.off = (long long)(p.g - t.g_arena);
            c.begin = (int)b;
            c.count = (int)std::min<size_t>(OPT_CHUNK, p.n - b);
            c.cout = p.conv ? p.cout : 1;
            c.rest = p.conv ? p.taps * p.cin : 1;
            if (c.off < 0 || (size_t)c.off + p.n > t.g_arena_floats) return fail(e, DYF_ERR_STATE, "optimizer: a gradient slice outside the arena");
            h.push_back(c);
        }
    }
    if (o.chunks) (void)hipFree(o.chunks);
    o.chunks = nullptr;
    o.n_chunks = (int)h.size();
    if (h.empty()) return fail(e, DYF_ERR_STATE, "optimizer: the network has no parameters");
    HIP_TRY(e, hipMalloc(&o.chunks, h.size() * sizeof(OptChunk)));
    HIP_TRY(e, hipMemcpy(o.chunks, h.data(), h.size() * sizeof(OptChunk), hipMemcpyHostToDevice));
    return DYF_OK;
}

// the optimizer of slot `which`, or null with the error set
TrainOptim* optim_of(dyf_engine* e, int which, TrainNet** net_out = nullptr) {
    TrainNet* t = train_net(e, which);
    if (!t || !t->ready || !t->optim) {
        fail(e, DYF_ERR_STATE, "no optimizer for this network (dyf_optim_create after dyf_load_weights)");
        return nullptr;
    }
    if (net_out) *net_out = t;
    return t->optim;
}

}  // namespace

namespace dyf {

void optim_destroy(TrainNet& t) {
    TrainOptim* o = t.optim;
    if (!o) return;
    if (o->pending && o->status_ready) (void)hipEventSynchronize(o->status_ready);
    if (o->m) (void)hipFree(o->m);
    if (o->chunks) (void)hipFree(o->chunks);
    if (o->partials) (void)hipFree(o->partials);
    if (o->status_dev) (void)hipFree(o->status_dev);
    if (o->status_host) (void)hipHostFree(o->status_host);
    if (o->status_ready) (void)hipEventDestroy(o->status_ready);
    delete o;
    t.optim = nullptr;
}

dyf_status optim_rebind(dyf_engine* e, TrainNet& t) {
    if (!t.optim) return DYF_OK;
    if (t.optim->floats != t.g_arena_floats || t.optim->layout != layout_hash(t)) {  // another network was loaded into the slot: its state means nothing here
        optim_destroy(t);
        return DYF_OK;
    }
    return build_chunks(e, t, *t.optim);
}

dyf_status optim_resolve(dyf_engine* e, TrainOptim& o) {
    if (!o.pending) return DYF_OK;
    HIP_TRY(e, hipEventSynchronize(o.status_ready));
    o.pending = false;
    o.last_norm = o.status_host->grad_norm;
    o.last_skipped = o.status_host->skipped;
    if (!o.last_skipped) ++o.steps;
    return DYF_OK;
}

}  // namespace dyf

extern "C" {

dyf_status dyf_optim_create(dyf_engine* e, int32_t which, const dyf_optim_config* c) {
    if (!e || which < 0 || which > 1 || !c) return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_create: bad arguments");
    if (!(c->beta1 >= 0.0 && c->beta1 < 1.0) || !(c->beta2 >= 0.0 && c->beta2 < 1.0) || !(c->eps >= 0.0) || !(c->weight_decay >= 0.0))
        return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_create: betas in [0, 1), eps >= 0, weight_decay >= 0");
    TrainNet* t = train_net(e, which);
    if (!t || !t->ready || !e->net[which].loaded) return fail(e, DYF_ERR_STATE, "optimizer: the network needs loaded weights (dyf_load_weights)");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    optim_destroy(*t);
    TrainOptim* o = new TrainOptim();
    t->optim = o;
    o->beta1 = c->beta1; o->beta2 = c->beta2; o->eps = c->eps; o->weight_decay = c->weight_decay; o->max_grad_norm = c->max_grad_norm;
    o->ema = c->ema != 0;
    o->floats = t->g_arena_floats;
    o->layout = layout_hash(*t);
    auto bail = [&](dyf_status s) { optim_destroy(*t); return s; };
#define OC(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return bail(fail(e, DYF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e))); } while (0)
    const size_t arenas = o->ema ? 3 : 2;
    OC(hipMalloc(&o->m, arenas * o->floats * sizeof(float)));
    OC(hipMemset(o->m, 0, arenas * o->floats * sizeof(float)));
    o->v = o->m + o->floats;
    o->shadow = o->ema ? o->v + o->floats : nullptr;
    OC(hipMalloc(&o->partials, OPT_MAX_PARTIALS * sizeof(double)));
    OC(hipMalloc(&o->status_dev, sizeof(OptStatus)));
    OC(hipMemset(o->status_dev, 0, sizeof(OptStatus)));
    OC(hipHostMalloc(&o->status_host, sizeof(OptStatus)));
    memset(o->status_host, 0, sizeof(OptStatus));
    OC(hipEventCreateWithFlags(&o->status_ready, hipEventDisableTiming));
    dyf_status s = build_chunks(e, *t, *o);
    if (s != DYF_OK) return bail(s);
    if (o->ema) {
        hipLaunchKernelGGL(opt_shadow, dim3(opt_grid(o->n_chunks)), dim3(256), 0, nullptr, o->chunks, o->n_chunks, o->shadow, 0);
        OC(hipGetLastError());
    }
    OC(hipDeviceSynchronize());
#undef OC
    return DYF_OK;
}

dyf_status dyf_optim_destroy(dyf_engine* e, int32_t which) {
    if (!e || which < 0 || which > 1) return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_destroy: bad arguments");
    TrainNet* t = train_net(e, which);
    if (t && t->optim) {
        HIP_TRY(e, hipSetDevice(e->cfg.device));
        HIP_TRY(e, hipDeviceSynchronize());
        optim_destroy(*t);
    }
    return DYF_OK;
}

dyf_status dyf_optim_step(dyf_engine* e, int32_t which, double lr, double ema_decay_now, void* stream) {
    if (!e || which < 0 || which > 1) return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_step: bad arguments");
    if (!(lr >= 0.0) || !(ema_decay_now >= 0.0 && ema_decay_now <= 1.0))
        return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_step: lr >= 0 and ema_decay_now in [0, 1]");
    TrainNet* t = nullptr;
    TrainOptim* o = optim_of(e, which, &t);
    if (!o) return DYF_ERR_STATE;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    // the previous step's outcome decides this step's count; its copy was queued a whole forward and backward ago
    dyf_status s = optim_resolve(e, *o);
    if (s != DYF_OK) return s;
    hipStream_t st = (hipStream_t)stream;
    const double tstep = (double)(o->steps + 1);
    const double bc1 = 1.0 - std::pow(o->beta1, tstep), bc2 = 1.0 - std::pow(o->beta2, tstep);
    OptArgs a;
    a.lr_decay = (float)(1.0 - lr * o->weight_decay);
    a.one_m_b1 = (float)(1.0 - o->beta1);
    a.beta2 = (float)o->beta2;
    a.one_m_b2 = (float)(1.0 - o->beta2);
    a.neg_step = (float)(-(lr / bc1));
    a.bc2_sqrt = (float)std::sqrt(bc2);
    a.eps = (float)o->eps;
    a.max_norm = (float)o->max_grad_norm;
    a.ema_omd = (float)(1.0 - ema_decay_now);
    a.ema = o->ema ? 1 : 0;
    const long long n4 = (long long)(t->g_arena_floats / 4);
    const unsigned parts = opt_grid((n4 + 255) / 256);
    hipLaunchKernelGGL(opt_grad_sumsq, dim3(parts), dim3(256), 0, st, t->g_arena, n4, o->partials);
    hipLaunchKernelGGL(opt_adamw_step, dim3(opt_grid(o->n_chunks)), dim3(256), 0, st, o->chunks, o->n_chunks, t->g_arena, o->m, o->v, o->shadow,
                       o->partials, (int)parts, a, o->status_dev);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemcpyAsync(o->status_host, o->status_dev, sizeof(OptStatus), hipMemcpyDeviceToHost, st));
    HIP_TRY(e, hipEventRecord(o->status_ready, st));
    o->pending = true;
    return DYF_OK;
}

dyf_status dyf_optim_last(dyf_engine* e, int32_t which, double* grad_norm_out, int32_t* skipped_out) {
    if (!e || which < 0 || which > 1) return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_last: bad arguments");
    TrainOptim* o = optim_of(e, which);
    if (!o) return DYF_ERR_STATE;
    dyf_status s = optim_resolve(e, *o);
    if (s != DYF_OK) return s;
    if (grad_norm_out) *grad_norm_out = o->last_norm;
    if (skipped_out) *skipped_out = o->last_skipped;
    return DYF_OK;
}

dyf_status dyf_optim_get_step(dyf_engine* e, int32_t which, int64_t* step_out) {
    if (!e || which < 0 || which > 1 || !step_out) return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_get_step: bad arguments");
    TrainOptim* o = optim_of(e, which);
    if (!o) return DYF_ERR_STATE;
    dyf_status s = optim_resolve(e, *o);
    if (s != DYF_OK) return s;
    *step_out = o->steps;
    return DYF_OK;
}

dyf_status dyf_optim_set_step(dyf_engine* e, int32_t which, int64_t step) {
    if (!e || which < 0 || which > 1 || step < 0) return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_set_step: bad arguments");
    TrainOptim* o = optim_of(e, which);
    if (!o) return DYF_ERR_STATE;
    dyf_status s = optim_resolve(e, *o);
    if (s != DYF_OK) return s;
    o->steps = step;
    return DYF_OK;
}

dyf_status dyf_optim_swap_ema(dyf_engine* e, int32_t which, void* stream) {
    if (!e || which < 0 || which > 1) return fail(e, DYF_ERR_INVALID_ARGUMENT, "dyf_optim_swap_ema: bad arguments");
    TrainOptim* o = optim_of(e, which);
    if (!o) return DYF_ERR_STATE;
    if (!o->ema) return fail(e, DYF_ERR_STATE, "dyf_optim_swap_ema: the optimizer keeps no EMA shadow");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    hipLaunchKernelGGL(opt_shadow, dim3(opt_grid(o->n_chunks)), dim3(256), 0, (hipStream_t)stream, o->chunks, o->n_chunks, o->shadow, 1);
    HIP_TRY(e, hipGetLastError());
    return DYF_OK;
}

}  // extern "C"
