// Shared between train.hip (the recorded forward / backward of arch unet_simple) and train_gemm.hip (its convolutions on the
// fp32 matrix cores).
#pragma once
#include "common.h"

#include <algorithm>

// ---- the 16-bit operand format of the TRAINING convs: always bf16, in both builds of the library (the fp16 build too).
// Training tensors, master weights, accumulators and statistics are fp32; only the MFMA operands are rounded while they are staged,
// so the format is independent of the engine's inference storage type.  fp16 operands would need the reference's GradScaler
// (Lightning precision=16): with mean-reduced losses dL/dout is ~1e-6..1e-7 at real batch sizes, below fp16's normal range, and the
// rounded gradient operand keeps a few bits or flushes to zero.  bf16 has fp32's exponent: no loss scale, no skipped steps.
typedef __bf16 t16_native_t;
typedef t16_native_t t16x8_t __attribute__((ext_vector_type(8)));
typedef t16_native_t t16x2_native_t __attribute__((ext_vector_type(2)));
typedef uint16_t t16_t;
#define T16_MFMA_32x32x16(a, b, c, x, y, z) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, x, y, z)
__device__ __host__ __forceinline__ t16_t f32_to_t16(float f) {  // round-to-nearest-even, NaN preserved
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (t16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (t16_t)(u >> 16);
}
__device__ __host__ __forceinline__ float t16_to_f32(t16_t v) { return __builtin_bit_cast(float, ((uint32_t)v) << 16); }
__device__ __forceinline__ uint32_t pack_t16x2(float lo, float hi) {  // one v_cvt_pk_bf16_f32
#if defined(__HIP_DEVICE_COMPILE__)
    const f32x2_native_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, t16x2_native_t));
#else
    return (uint32_t)f32_to_t16(lo) | ((uint32_t)f32_to_t16(hi) << 16);
#endif
}

// bf16x3: the lo image of a value whose hi image (its bf16 rounding) is `hi`: bf16(v - hi), the subtraction exact in fp32
__device__ __forceinline__ uint32_t pack_t16x2_lo(float a, float b, uint32_t hi) {
    return pack_t16x2(a - __builtin_bit_cast(float, hi << 16), b - __builtin_bit_cast(float, hi & 0xffff0000u));
}
__device__ __host__ __forceinline__ t16_t f32_to_t16_lo(float v, t16_t hi) { return f32_to_t16(v - t16_to_f32(hi)); }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE attribute: the training launchers that need more than the 64 KB
// default raise it once per (kernel, device) -- a process-wide flag left the second GPU of a process at the default, and its first
// launch failed.  Returns false (and the launcher declines the shape) when the attribute cannot be set.
// The kernel is the template ARGUMENT, so every kernel has a state of its own (keyed on the type of a function-pointer parameter, two
// kernels of one signature -- two instantiations of one kernel template -- would share it, and the second would launch unraised).
#include <atomic>
template <auto Kernel>
static inline bool train_raise_dynamic_lds(int bytes) {
    static std::atomic<unsigned char> done[64];  // per kernel; 0 not tried, 1 set, 2 failed
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
    unsigned char st = done[dev].load(std::memory_order_acquire);
    if (st == 0) {
        st = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 1 : 2;
        done[dev].store(st, std::memory_order_release);
    }
    return st == 1;
}

#include <map>
#include <string>
#include <vector>

#include "../../include/dyffusion_hip.h"  // dyf_status, dyf_engine

namespace dyf {

struct RParam {              // one parameter in its training layout, and its gradient (same layout)
    float* w = nullptr;      // conv: [cout][tap][cin]; Linear: [out][in]; vectors as stored
    float* wt = nullptr;     // every conv: [tap][cin][cout] (forward layout; a weight-standardised conv derives its own pair per use)
    float* g = nullptr;
    size_t n = 0;
    int conv = 0, cout = 0, cin = 0, taps = 0;   // conv: any 4-d weight as (cout, cin, kh, kw) -- a ConvTranspose2d (dim, C, 4, 4) is [dim][tap][C]
    bool stat = false;       // a BatchNorm running statistic: no gradient; what leaves by its name is the (updated) statistic itself
};

struct TrainOptim;  // engine-resident AdamW / EMA state of one network (train_optim.hip)

struct TrainNet {
    std::map<std::string, RParam> P;
    std::vector<void*> owned;
    float* g_arena = nullptr;     // every parameter's gradient buffer is a 256-byte-aligned slice of ONE block: zeroing the gradients is
    size_t g_arena_floats = 0;    // one memset instead of one per parameter (~270 per network and step)
    bool ready = false;
    TrainOptim* optim = nullptr;  // dyf_optim_create; survives a reload of the weights (optim_rebind), destroyed with the engine
};

// ---- engine-resident optimizer (train_optim.hip)
// One entry of the update kernel's chunk table: OPT_CHUNK consecutive elements (fewer at a tensor's end) of ONE parameter.
struct OptChunk {
    float* w;            // the parameter's master weights (training layout)
    float* wt;           // its [tap][cin][cout] copy, or null
    long long off;       // offset of the parameter's slice in g_arena -- and in the m, v and shadow arenas, which share its offsets
    int begin, count;    // the chunk's element range inside the parameter
    int cout, rest;      // wt: element i of w is wt[(i % rest) * cout + i / rest], rest = taps * cin
};
constexpr int OPT_CHUNK = 4096;        // elements per chunk: 16 KB of each of w, g, m, v, shadow
constexpr int OPT_MAX_PARTIALS = 1024; // workgroups of the sum-of-squares launch = partial sums the update launch re-reduces

struct OptStatus {       // what a step leaves for the host: written by workgroup 0 of the update launch
    double grad_norm;
    int skipped, pad;
};

struct TrainOptim {
    double beta1 = 0.9, beta2 = 0.999, eps = 1e-8, weight_decay = 0.0, max_grad_norm = 0.0;  // doubles, as torch.optim holds them
    bool ema = false;
    size_t floats = 0;               // = TrainNet::g_arena_floats the arenas below were sized for
    uint64_t layout = 0;             // hash of every parameter's (name, arena offset, n): the state belongs to exactly this layout
    float *m = nullptr, *v = nullptr, *shadow = nullptr;   // one block: [m | v | shadow]
    OptChunk* chunks = nullptr;      // device
    int n_chunks = 0;
    double* partials = nullptr;      // device [OPT_MAX_PARTIALS]
    OptStatus* status_dev = nullptr;
    OptStatus* status_host = nullptr;  // pinned: copied behind every step, read when the host next needs the outcome
    hipEvent_t status_ready = nullptr;
    bool pending = false;            // a step was launched whose outcome (skipped or not) the host has not read yet
    long long steps = 0;             // applied steps the host knows of (torch's state["step"])
    double last_norm = 0.0;
    int last_skipped = 0;
};

void optim_destroy(TrainNet& t);                      // frees everything; t.optim = nullptr
dyf_status optim_rebind(dyf_engine* e, TrainNet& t);   // after the parameter copy was rebuilt: new chunk table over the new pointers
dyf_status optim_resolve(dyf_engine* e, TrainOptim& o);  // waits for the pending step's status and books it
TrainNet* train_net(dyf_engine* e, int which);         // train.hip: the network's training copy, or null

struct TConv {  // geometry of one nn.Conv2d on NHWC fp32 tensors: x (n, h, w, cin) -> y (n, ho, wo, cout), k x k / stride s / pad p
    int n, h, w, cin, ho, wo, cout, k, s, p;
};

// fp32 MFMA implicit-GEMM forms (train_gemm.hip); return false when the shape is not covered (caller falls back to the VALU kernel)
// ws / ws_floats: workspace for the split-K partial sums of launches with few output tiles (null: never split)
// Operand format of the training convs for the calls of THIS thread: set by the training entry points from the engine's
// dyf_train_set_precision (0 = the DYF_TRAIN_OPERANDS environment variable decides: unset / fp32 -> fp32 operands).
extern thread_local int g_train_precision;
bool train_operands16();
// bf16x3 (dyf_train_set_precision(48), or DYF_TRAIN_OPERANDS=bf16x3 where the engine did not say): the convs the 16-bit dispatch takes stage
// every operand as hi = bf16(v), lo = bf16(v - hi) and compute a_lo b_hi + a_hi b_lo + a_hi b_hi (train_gemm.hip, train_halo16.hip)
bool train_operands_split();
struct TrainPrecisionScope {
    int prev;
    explicit TrainPrecisionScope(int p) : prev(g_train_precision) { g_train_precision = p; }
    ~TrainPrecisionScope() { g_train_precision = prev; }
};
// "The convs of THIS thread are launched by a sampling forward" (f32_net_forward under dyf_set_sample_precision(48), and the op seam's
// DYF_TOP_SAMPLE): the dispatchers have no engine pointer, so forms that only sampling takes read this -- the fused bf16x3 halo forward
// of train_halo16.hip.  Recorded (training) forwards and every backward run with it clear and keep their forms bit for bit.
extern thread_local int g_sample_forward;
struct SampleForwardScope {
    int prev;
    explicit SampleForwardScope(int on) : prev(g_sample_forward) { g_sample_forward = on; }
    ~SampleForwardScope() { g_sample_forward = prev; }
};

// Deterministic training mode for the calls of THIS thread: set by the training entry points from the engine's
// dyf_train_set_deterministic (the reference's trainer.deterministic).  On: no launcher may merge a floating-point sum with atomics --
// every cross-workgroup sum writes one slab of partial sums per contributor to the split-K workspace, and det_reduce adds the slabs in
// index order to the destination (a second launch: no tickets, no waiting between workgroups).  Sampling never reads it (scope 0).
extern thread_local int g_train_det;
inline bool train_det() { return g_train_det != 0; }
struct TrainDetScope {
    int prev;
    explicit TrainDetScope(int on) : prev(g_train_det) { g_train_det = on; }
    ~TrainDetScope() { g_train_det = prev; }
};
// dst[i] += ws[0 * stride + i] + ws[1 * stride + i] + ... + ws[(splits - 1) * stride + i], i < n, summed in that order (train_gemm.hip)
void det_reduce(const float* ws, int splits, long long stride, long long n, float* dst, hipStream_t st);
void det_reduce(const double* ws, int splits, long long stride, long long n, double* dst, hipStream_t st);

bool tgemm_conv_fwd(const TConv& g, const float* x, const float* wt, const float* bias, float* y, float* ws, size_t ws_floats,
                    hipStream_t st);
bool tgemm_conv_dgrad(const TConv& g, const float* dz, const float* w, const float* bias, float* dx, float* ws, size_t ws_floats,
                      hipStream_t st);
// (ws / ws_floats: the slabs of the deterministic mode; unused otherwise)
bool tgemm_conv_wgrad(const TConv& g, const float* dz, const float* x, float* dw, float* ws, size_t ws_floats, hipStream_t st);

// 3 x 3 / stride 1 / pad 1 layers with 16-bit operands, tile + halo staged once (train_halo16.hip); false: shape not covered.
// mode 0: forward (A = x, W = wt[tap][ci][co]); mode 1: data gradient (A = dz, W = w[co][tap][ci]); ws receives the 16-bit weights
bool thalo_conv3x3(const TConv& g, int mode, const float* A, const float* W, const float* bias, float* C, float* ws, size_t ws_floats,
                   hipStream_t st);
bool thalo_wgrad3x3(const TConv& g, const float* dz, const float* x, float* dw, float* ws, size_t ws_floats, hipStream_t st);

}  // namespace dyf
