// lk_pair.hpp -- what the kernels around the forward LK launch share beyond the body of lk_plain.hpp: who a lane is (one wavefront
// per keypoint in visiting order, one group of 8 lanes per target, records at rec[slot * 8 + target]), OpenCV's bounds test of a
// window, the 64-lane walk of a window, the exact 64-bit sums of a group and of a wavefront, the Newton step with its two exits,
// and the launch of a kernel in the plain geometry.  Used by lk_plain.hpp, lk_norm.hpp, lk_fb.hpp and the kernels of
// kernels_lk.hip, kernels_lk_fb.hip, kernels_lk_norm.hip, kernels_lk_search.hip, kernels_lk_wmask.hip, kernels_lk_affine.hip and
// kernels_lk_corr.hip; the product kernels (kernels_lk3.hip, lk4_kernel.hpp) have their own mapping and stay on lk_common.hpp.
// Every function is inlined and takes its state by reference: no kernel built from them holds more registers than when it spelled
// them out (tests/test_lk_normalized_cpu.py; profiles/lk_pair_helpers.json has every figure).
#pragma once

#include <algorithm>

#include "../../../include/polychase_hip.h"
#include "lk_common.hpp"

namespace pc {

// ---- who a lane is ----
struct LKPair {
    int wave, lane;    // the wavefront in its workgroup, the lane in its wavefront
    int grp, lg;       // the target (the group of 8 lanes), the lane in its group
    int slot, feat;    // the keypoint in visiting order and in keypoint order
    bool tgt_active;   // the group has a target
    float4 rec;        // the pair's record; zero until lk_pair_record has run for an active group
    bool fwd_ok;       // ... and whether its status is 1: uniform in the group
    // the pair's place in the [target][n] side arrays; computed where it is used, not carried through the tracking
    __device__ __forceinline__ size_t side(int n) const { return (size_t)grp * (size_t)n + (size_t)feat; }
};
// the record of an active group, re-read where a launch in between may have changed it
__device__ __forceinline__ void lk_pair_record(LKPair& q, const float4* rec) {
    if (q.tgt_active) q.rec = rec[(size_t)q.slot * kRecStride + q.grp];
    q.fwd_ok = q.tgt_active && __float_as_uint(q.rec.w) == 1u;
}
// the keypoint of the slot: the one load of the visiting order
__device__ __forceinline__ void lk_pair_keypoint(LKPair& q, const uint32_t* perm) { q.feat = perm ? (int)perm[q.slot] : q.slot; }
// -> false: the wavefront has no keypoint (whole wavefronts, nothing of q is to be used).  p: the kernel's parameters (n,
// n_targets, perm, and rec with RECORD), read here and in this order, not where the call stands.  WAVES: wavefronts per
// workgroup, 0: as launched.  RECORD: with the record; false for a kernel that loads its record later or not at all.
// KEYPOINT: false for a kernel that has an exit of its own in front of the load of perm[slot] and calls lk_pair_keypoint behind
// it.  Nothing else is loaded, and a field the kernel does not use costs nothing.
template <bool RECORD, int WAVES = 0, bool KEYPOINT = true, class Params>
__device__ __forceinline__ bool lk_pair_prologue(LKPair& q, const Params& p) {
    q.wave = threadIdx.x >> 6;
    q.lane = threadIdx.x & 63;
    q.grp = q.lane >> 3;
    q.lg = q.lane & 7;
    q.slot = (int)blockIdx.x * (WAVES ? WAVES : (int)(blockDim.x >> 6)) + q.wave;
    if (q.slot >= p.n) return false;
    q.tgt_active = q.grp < p.n_targets;
    q.rec = make_float4(0.f, 0.f, 0.f, 0.f);
    q.fwd_ok = false;
    if constexpr (RECORD) lk_pair_record(q, p.rec);
    if constexpr (KEYPOINT) lk_pair_keypoint(q, p.perm);
    return true;
}

// OpenCV's bounds test of a win x win window whose origin floors to (ix, iy) in a w x h level: a window that passes lies inside
// the planes' padding (win rows, >= win columns)
__device__ __forceinline__ bool lk_window_outside(int ix, int iy, int win, int w, int h) { return ix < -win || ix >= w || iy < -win || iy >= h; }

// the 64 lanes of a wavefront walk a window: pixel i = lane + 64 k at (y, x) = (i / win, i % win), f(i, y, x); <= 16 pixels per lane
template <class F>
__device__ __forceinline__ void for_each_window_pixel(int lane, int win, const F& f) {
    const int n = win * win;
    const int dy = 64 / win, dx = 64 - dy * win;   // what 64 pixels further means in rows and columns
    int y = lane / win, x = lane - y * win;
    for (int i = lane; i < n; i += 64) {
        f(i, y, x);
        x += dx;
        y += dy;
        if (x >= win) {
            x -= win;
            y++;
        }
    }
}

// ---- exact sums ----
// over the group, of per-lane signed 64-bit partials (|total| < 2^47): v = (v >> 32) 2^32 + ((v >> 16) & 0xffff) 2^16 +
// (v & 0xffff) in two's complement, three DPP sums of 16-bit-wide pieces
__device__ __forceinline__ long long group8_sum_s64(long long v) {
    const int c0 = group_allreduce_add<8>((int)(v & 0xffff));
    const int c1 = group_allreduce_add<8>((int)((v >> 16) & 0xffff));
    const int c2 = group_allreduce_add<8>((int)(v >> 32));
    return (long long)c2 * 4294967296ll + (long long)c1 * 65536ll + (long long)c0;
}
// the same over the wavefront (|partial| < 2^47, and so the total for the <= 64 partials the callers have)
__device__ __forceinline__ long long wave_sum_s64(long long v) {
    const int c0 = wave_sum_i32((int)(v & 0xffff));
    const int c1 = wave_sum_i32((int)((v >> 16) & 0xffff));
    const int c2 = wave_sum_i32((int)(v >> 32));
    return (long long)c2 * 4294967296ll + (long long)c1 * 65536ll + (long long)c0;
}
// the 32-bit shortcuts over the wavefront, exact in 64 bits: two sums instead of three
__device__ __forceinline__ long long wave_sum_s32(int v) {
    return (long long)wave_sum_i32(v >> 16) * 65536ll + (long long)wave_sum_i32(v & 0xffff);
}
__device__ __forceinline__ long long wave_sum_u32(uint32_t v) {
    return (long long)wave_sum_i32((int)(v >> 16)) * 65536ll + (long long)wave_sum_i32((int)(v & 0xffffu));
}
// the group's sum (|total| < 2^40) as ONE rounding of the exact integer: hi * 2^16 + lo with both terms exact in fp32
__device__ __forceinline__ float group8_exact_sum_i64(long long v) {
    const long long t = group8_sum_s64(v);
    return exact_sum_to_float((int)(t >> 16), (int)(t & 0xffff));
}

// ---- the Newton step of an iteration: (dx, dy) from A, b and D = 1 / det A, the search position q and the result n = q +
// half_win moved by it; -> true when the iteration ends here: the step is below eps_sq (fp64, as OpenCV compares), or it
// undoes the previous one (the oscillation exit: half a step back).  (pdx, pdy) carry the step to the next call. ----
__device__ __forceinline__ bool lk_newton_step(float A11, float A12, float A22, float D, float b1, float b2, float half_win, int j, double eps_sq,
                                               float& qx, float& qy, float& nx, float& ny, float& pdx, float& pdy) {
    const float dx = (A12 * b2 - A22 * b1) * D;
    const float dy = (A12 * b1 - A11 * b2) * D;
    qx += dx;
    qy += dy;
    nx = qx + half_win;
    ny = qy + half_win;
    if ((double)dx * (double)dx + (double)dy * (double)dy <= eps_sq) return true;
    if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
        nx -= dx * 0.5f;
        ny -= dy * 0.5f;
        return true;
    }
    pdx = dx;
    pdy = dy;
    return false;
}

// ---- launchers ----
// what every kernel of the family asks of its window and its number of targets
inline bool lk_pair_args_ok(int win, int n_targets) { return win >= 3 && win <= PC_MAX_WINDOW && n_targets >= 1 && n_targets <= kRecStride; }

// The plain geometry: dynamic LDS of 8 groups x win^2 x 8 bytes per wavefront, 1..4 wavefronts per workgroup, as many as fit
// below 64 KiB (window 16: 3 wavefronts, 49152 bytes, not 4, exactly 64 KiB; window 31: 1).
struct PlainLKLaunch {
    int waves;
    unsigned blocks;
    size_t lds_bytes;
};
inline PlainLKLaunch plain_lk_launch(int n, int win) {
    static_assert((size_t)kRecStride * PC_MAX_WINDOW * PC_MAX_WINDOW * sizeof(uint2) < 65536, "one wavefront's templates must fit below 64 KiB");
    const size_t wave_bytes = (size_t)kRecStride * win * win * sizeof(uint2);   // <= 61504
    const int waves = (int)std::min<size_t>(4, 65535 / wave_bytes);
    return {waves, (unsigned)((n + waves - 1) / waves), waves * wave_bytes};
}
// a kernel in that geometry, n > 0; a kernel with one instance per arithmetic order: x86_order ? kernel<true> : kernel<false>
template <class... Params, class... Args>
inline void launch_plain_geometry(void (*kernel)(Params...), int n, int win, hipStream_t s, const Args&... args) {
    const PlainLKLaunch g = plain_lk_launch(n, win);
    hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(64 * g.waves), g.lds_bytes, s, args...);
}

}  // namespace pc
