// lk_common.hpp -- device helpers shared by the pyramidal LK kernels (kernels_lk3.hip: two keypoints per wavefront, 4 lanes per
// target; lk4_kernel.hpp: one keypoint per wavefront, 8 lanes per target; lk_plain.hpp: the plain body of the cross-check and of
// the forward-backward check): fixed-point bilinear weights, DPP sums inside a group, exact integer sums, the Scharr window's way
// into LDS.  Arithmetic follows oracle/pc_oracle.c (OpenCV's LKTrackerInvoker).
#pragma once

#include "kernels.hpp"

namespace pc {

constexpr int W_BITS = 14;

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
// all-reduce (sum) across a group of GL lanes (GL = 8 or 16, groups are aligned)
template <int GL>
__device__ __forceinline__ int group_allreduce_add(int v) {
    v += dpp_i32<0xB1>(v);    // quad_perm [1,0,3,2]  (lane ^ 1)
    v += dpp_i32<0x4E>(v);    // quad_perm [2,3,0,1]  (lane ^ 2)
    v += dpp_i32<0x141>(v);   // row_half_mirror      (other quad of the 8-lane half)
    if (GL == 16) v += dpp_i32<0x140>(v);  // row_mirror (other half of the row)
    return v;
}

// exact float of (hi * 2^16 + lo): each term is exactly representable (|hi| < 2^24, |lo| < 2^24),
// so the single fp32 add rounds the exact integer once (== (float)(int64) of the oracle).
__device__ __forceinline__ float exact_sum_to_float(int hi, int lo) {
    return (float)hi * 65536.f + (float)lo;
}

struct Weights {
    int w00, w01, w10, w11;   // w11 may be -1 (rounding of the other three), never smaller
    uint32_t r0, r1;          // signed 16-bit pairs (w00, w01) and (w10, w11) for v_dot2_i32_i16
    bool neg11;
};
__device__ __forceinline__ Weights bilinear_weights(float a, float b) {
    Weights w;
    w.w00 = __float2int_rn((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
    w.w01 = __float2int_rn(a * (1.f - b) * (float)(1 << W_BITS));
    w.w10 = __float2int_rn((1.f - a) * b * (float)(1 << W_BITS));
    w.w11 = (1 << W_BITS) - w.w00 - w.w01 - w.w10;
    w.neg11 = w.w11 < 0;
    w.r0 = (uint32_t)w.w00 | ((uint32_t)w.w01 << 16);             // 0 <= w00, w01, w10 <= 2^14
    w.r1 = (uint32_t)w.w10 | ((uint32_t)w.w11 << 16);             // w11 == -1 -> 0xffff in the high half
    return w;
}

typedef short pc_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int sdot2(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(pc_short2, a), __builtin_bit_cast(pc_short2, b), c, false);
}

// Raw Scharr window ((WIN+1)^2 dwords at `Dbase`, row pitch `pitch` dwords) -> LDS with NL lanes.  load() only
// issues the loads, so the caller can put the I-window staging between load() and store() and pay one memory
// latency for both.
template <int WIN, int NL>
struct DerivWindow {
    static constexpr int TOTAL = (WIN + 1) * (WIN + 1);
    static constexpr int TRIPS = (TOTAL + NL - 1) / NL;
    int32_t v[TRIPS];
    __device__ __forceinline__ void load(const int32_t* __restrict__ Dbase, int pitch, int l) {
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const int i = min(l + NL * k, TOTAL - 1);   // lanes past the end repeat the last item (same address, same value): no branch
            const int r = i / (WIN + 1), c = i - r * (WIN + 1);
            v[k] = Dbase[r * pitch + c];
        }
    }
    __device__ __forceinline__ void store(int32_t* dbuf, int l) const {
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            dbuf[min(l + NL * k, TOTAL - 1)] = v[k];
        }
    }
};

// wave-wide exact integer sum -> fp32: DPP inside each 16-lane row, then the 4 row results
// (lanes 0,16,32,48) through readlane
__device__ __forceinline__ int wave_sum_i32(int v) {
    v = group_allreduce_add<16>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ float wave_exact_sum(int partial) {
    return exact_sum_to_float(wave_sum_i32(partial >> 16), wave_sum_i32(partial & 0xffff));
}

}  // namespace pc
