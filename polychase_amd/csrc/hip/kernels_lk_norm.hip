// kernels_lk_norm.hip -- brightness-normalised LK on gfx950 (include/polychase_hip.h: pc_lk_track_normalized has the rule;
// DESIGN.md section 4 "Brightness normalisation"): the forward launch and the backward launch of the forward-backward check when
// the option is on.  Both leave exactly what the kernels they stand in for leave -- the raw records
// out_rec[slot * 8 + target] = (q, err, status_f), the back arrays --, so everything downstream is unchanged.  The body is
// norm_lk_pair (lk_norm.hpp).
#include "lk_norm.hpp"

namespace pc {

constexpr int kNormWaves = 4;   // wavefronts (keypoints) per workgroup of the forward launch, at every window

// Forward: one wavefront per keypoint in the visiting order p.perm, one group of 8 lanes per target.  The template is the same for
// the eight targets: all 64 lanes evaluate it once per level into the wavefront's slice of LDS (8 bytes per pixel, <= 7688 bytes)
// and the template sums are wave reductions; each group then gathers its J window straight from the padded u8 plane, a lane
// walking whole columns.  All groups read the same LDS addresses (broadcasts, one 8-byte access per pixel).  Nothing crosses
// wavefronts: no barrier.  No window is read before it passed OpenCV's bounds test on the same floats, so every read lies inside
// the padding (win rows, >= win columns).
__global__ __launch_bounds__(64 * kNormWaves) void lk_norm_kernel(const LKParams p, const int win) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 3;
    lk_signal_dispatched(p);
    const int slot = (int)blockIdx.x * kNormWaves + wave;
    if (slot >= p.n) return;   // whole wavefronts
    const bool active = grp < p.n_targets;
    const float2 pt = p.pts[p.perm ? (int)p.perm[slot] : slot];
    const auto level_of = [&](int level) {
        const Level L = p.src[level];
        return PlainLKLevel{L.w, L.h, L.pitch, L.img, L.der, p.tgt[grp][level]};
    };
    const PlainLKResult r = norm_lk_pair<true, true>(level_of, pt.x, pt.y, win, lane, active, p.max_level, p.max_iters, p.eps_sq,
                                                     p.min_eig_thr, s_tmpl + (size_t)wave * (win * win));
    // one 16-byte record per (slot, target): the wavefront's results are contiguous
    if ((lane & 7) == 0 && active) p.out_rec[(size_t)slot * kRecStride + grp] = make_float4(r.nx, r.ny, r.err, __uint_as_float(r.status ? 1u : 0u));
}

// Backward: lk_fb_kernel's mapping and parameters with the normalised body; the template of every pair comes from the target's
// planes at the forward end point (per group), the searched image is frame1.
__global__ __launch_bounds__(256) void lk_norm_fb_kernel(const LKFBParams p) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 3, lg = lane & 7;
    const int slot = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (slot >= p.n) return;   // whole wavefronts
    const bool tgt_active = grp < p.n_targets;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tgt_active) rec = p.rec[(size_t)slot * kRecStride + grp];
    const bool fwd_ok = tgt_active && __float_as_uint(rec.w) == 1u;   // uniform in the group
    const int feat = p.perm ? (int)p.perm[slot] : slot;

    float nx = 0.f, ny = 0.f;
    bool status = false;
    if (fwd_ok) {
        const auto level_of = [&](int level) {
            const Level L = p.f1[level];
            return PlainLKLevel{L.w, L.h, L.pitch, p.timg[grp][level], p.tder[grp][level], L.img};
        };
        const PlainLKResult r = norm_lk_pair<false, false>(level_of, rec.x, rec.y, p.win, lane, true, p.max_level, p.max_iters, p.eps_sq,
                                                           p.min_eig_thr, s_tmpl + (size_t)(wave * 8 + grp) * (p.win * p.win));
        nx = r.nx;
        ny = r.ny;
        status = r.status;
    }

    if (lg == 0 && tgt_active) {
        if (fwd_ok) {
            const float2 pt = p.pts[feat];
            const float dx = nx - pt.x, dy = ny - pt.y;
            const float d2 = dx * dx + dy * dy;
            const bool keep = status && (d2 <= p.thr2);   // a NaN fails
            if (!keep) p.rec[(size_t)slot * kRecStride + grp].w = __uint_as_float(0u);
        }
        const size_t o = (size_t)grp * (size_t)p.n + (size_t)feat;
        if (p.back_xy) p.back_xy[o] = fwd_ok ? make_float2(nx, ny) : make_float2(0.f, 0.f);
        if (p.back_status) p.back_status[o] = (fwd_ok && status) ? (uint8_t)1 : (uint8_t)0;
    }
}

bool launch_lk_norm(const LKParams& p, int win, hipStream_t s) {
    if (win < 3 || win > PC_MAX_WINDOW || p.n_targets < 1 || p.n_targets > kRecStride) return false;
    if (p.n <= 0) return true;
    const size_t lds_bytes = (size_t)kNormWaves * win * win * sizeof(uint2);   // <= 30752
    hipLaunchKernelGGL(lk_norm_kernel, dim3((unsigned)((p.n + kNormWaves - 1) / kNormWaves)), dim3(64 * kNormWaves), lds_bytes, s, p, win);
    return true;
}

bool launch_lk_norm_fb(const LKFBParams& p, hipStream_t s) {
    if (p.win < 3 || p.win > PC_MAX_WINDOW || p.n_targets < 1 || p.n_targets > kRecStride) return false;
    if (p.n <= 0) return true;
    const PlainLKLaunch g = plain_lk_launch(p.n, p.win);
    hipLaunchKernelGGL(lk_norm_fb_kernel, dim3(g.blocks), dim3(64 * g.waves), g.lds_bytes, s, p);
    return true;
}

}  // namespace pc
