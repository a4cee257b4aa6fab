// The epilogue step of the MFMA conv forms, defined once (device code only).
//
// Every MFMA conv form swaps its operands (D^T = W X^T), so lane (l31, hi) of a 32 x 32 accumulator holds PIXEL l31 and, in
// register r, CHANNEL 8 * (r >> 2) + 4 * hi + (r & 3) of the tile's 32 channels.  One step takes the 8 registers r0 .. r0 + 7
// (r0 = 8 * g2: register groups 2 g2 and 2 g2 + 1, i.e. the lane's channels c + {0..3} and c + 8 + {0..3}, c = 16 g2 + 4 hi) through
//     v = acc * A + C  ->  activation  ->  dropout  (-> + residual)  ->  16-bit pack  ->  exchange with lane l ^ 32,
// after which the lane holds 8 CONSECUTIVE channels of its pixel: one 16-byte row.  No LDS round trip, no barrier.  What a form adds
// around the step -- addressing, LDS staging, the sparse column map, the fused GroupNorm, where its loads are issued -- stays with
// the form.
#pragma once
#include "common.h"

#include <type_traits>

// (A, C) of the step's 8 channels: a0 / c0 = the table entries of channels c + {0..3}, a1 / c1 = those of c + 8 + {0..3}; ps = the
// dropout scale folded into the affine (drop_prescale; 1 for tables that are already scaled or never are)
__device__ __forceinline__ void epi_coef(const float4 a0, const float4 a1, const float4 c0, const float4 c1, const float ps, float (&ca)[8],
                                         float (&cc)[8]) {
    ca[0] = a0.x * ps; ca[1] = a0.y * ps; ca[2] = a0.z * ps; ca[3] = a0.w * ps;
    ca[4] = a1.x * ps; ca[5] = a1.y * ps; ca[6] = a1.z * ps; ca[7] = a1.w * ps;
    cc[0] = c0.x * ps; cc[1] = c0.y * ps; cc[2] = c0.z * ps; cc[3] = c0.w * ps;
    cc[4] = c1.x * ps; cc[5] = c1.y * ps; cc[6] = c1.z * ps; cc[7] = c1.w * ps;
}
// ... loaded here: A / C point at the lane's first channel (c) of the two tables (global memory or LDS)
__device__ __forceinline__ void epi_coef(const float* A, const float* C, const float ps, float (&ca)[8], float (&cc)[8]) {
    epi_coef(*(const float4*)A, *(const float4*)(A + 8), *(const float4*)C, *(const float4*)(C + 8), ps, ca, cc);
}

// 8 fp32 values -> 16-bit pairs -> exchange between lanes l and l + 32 -> one 16-byte row.  Before the exchange a lane holds
// p = channels c + {0..3} (group 2 g2) and q = channels c + 8 + {0..3} (group 2 g2 + 1).  v_permlane32_swap hands the low lanes' q
// to the high lanes and the high lanes' p to the low lanes, so afterwards
//   lanes  0-31 hold {own p, partner's p} = channels 16 g2 + 0..7,
//   lanes 32-63 hold {partner's q, own q} = channels 16 g2 + 8..15:
// every lane stores at channel offset 16 g2 + 8 * hi.
__device__ __forceinline__ uint4 epi_pack_swap(const float (&v)[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t p0 = pack_el16x2(v[0], v[1]), p1 = pack_el16x2(v[2], v[3]);
    const uint32_t q0 = pack_el16x2(v[4], v[5]), q1 = pack_el16x2(v[6], v[7]);
    const auto s0 = __builtin_amdgcn_permlane32_swap(p0, q0, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(p1, q1, false, false);
    uint4 o;
    o.x = s0[0]; o.y = s1[0]; o.z = s0[1]; o.w = s1[1];
    return o;
#else
    return make_uint4(0u, 0u, 0u, 0u);  // the exchange exists in the device pass only
#endif
}

// residual: r0 = the 16-bit values of channels c + {0..3}, r1 = those of c + 8 + {0..3}, added in fp32
__device__ __forceinline__ void epi_add_residual(float (&v)[8], const uint2 r0, const uint2 r1) {
    const uint32_t rw[4] = {r0.x, r0.y, r1.x, r1.y};
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] += (t & 1) ? el16_hi(rw[t >> 1]) : el16_lo(rw[t >> 1]);
}

// affine -> activation -> dropout of accumulator registers r0 .. r0 + 7; e0 = element index of channel c in the launch's dense NHWC
// output (the dropout stream position, whatever the storage layout), row0 = index of the sample's first element.  Hands back the
// fp32 values: for the sites that add a residual or store fp32 before packing.
template <int ACT, int MODE, class Acc>
__device__ __forceinline__ void epi_values(const Acc& acc, const int r0, const float (&ca)[8], const float (&cc)[8], const uint32_t e0,
                                           const uint32_t row0, const DropSpec& drop, const RngKey key, float (&v)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = fmaf(acc[r0 + t], ca[t], cc[t]);
    act_drop_fixed<4, ACT, MODE, true>(v, e0, row0, drop, key);
    act_drop_fixed<4, ACT, MODE, true>(v + 4, e0 + 8, row0, drop, key);
}

// the whole plain step
template <int ACT, int MODE, class Acc>
__device__ __forceinline__ uint4 epi_step(const Acc& acc, const int r0, const float (&ca)[8], const float (&cc)[8], const uint32_t e0,
                                          const uint32_t row0, const DropSpec& drop, const RngKey key) {
    float v[8];
    epi_values<ACT, MODE>(acc, r0, ca, cc, e0, row0, drop, key, v);
    return epi_pack_swap(v);
}

// (activation, dropout mode) are wave-uniform: the epilogue is instantiated per pair and dispatched once, with scalar branches.
// f(integral_constant<int, ACT>, integral_constant<int, MODE>) for none / ReLU / LeakyReLU / SiLU (the MFMA forms do not take GELU:
// conv_mfma_supported) x dropout off / generated / injected.
template <class F>
__device__ __forceinline__ void epi_dispatch(const int act, const int mode, F&& f) {
    auto by_mode = [&](auto act_c) {
        if (mode == 0) f(act_c, std::integral_constant<int, 0>{});
        else if (mode == 1) f(act_c, std::integral_constant<int, 1>{});
        else f(act_c, std::integral_constant<int, 2>{});
    };
    if (act == ACT_RELU) by_mode(std::integral_constant<int, ACT_RELU>{});
    else if (act == ACT_LEAKY) by_mode(std::integral_constant<int, ACT_LEAKY>{});
    else if (act == ACT_SILU) by_mode(std::integral_constant<int, ACT_SILU>{});
    else by_mode(std::integral_constant<int, ACT_NONE>{});
}
