// kernels_lk_norm.hip -- brightness-normalised LK on gfx950 (include/polychase_hip.h: pc_lk_track_normalized has the rule;
// DESIGN.md section 4 "Brightness normalisation"): the forward launch and the backward launch of the forward-backward check when
// the option is on.  Both leave exactly what the kernels they stand in for leave -- the raw records
// out_rec[slot * 8 + target] = (q, err, status_f), the back arrays --, so everything downstream is unchanged.  The body is
// norm_lk_pair (lk_norm.hpp); the backward launch's decision is lk_fb_body (lk_fb.hpp).
#include "lk_fb.hpp"
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
    lk_signal_dispatched(p);
    LKPair q;
    if (!lk_pair_prologue<false, kNormWaves>(q, p)) return;   // whole wavefronts
    const float2 pt = p.pts[q.feat];
    const auto level_of = [&](int level) {
        const Level L = p.src[level];
        return PlainLKLevel{L.w, L.h, L.pitch, L.img, L.der, p.tgt[q.grp][level]};
    };
    const PlainLKResult r = norm_lk_pair<true, true>(level_of, pt.x, pt.y, win, q.lane, q.tgt_active, p.max_level, p.max_iters, p.eps_sq,
                                                     p.min_eig_thr, s_tmpl + (size_t)q.wave * (win * win));
    // one 16-byte record per (slot, target): the wavefront's results are contiguous
    if (q.lg == 0 && q.tgt_active)
        p.out_rec[(size_t)q.slot * kRecStride + q.grp] = make_float4(r.nx, r.ny, r.err, __uint_as_float(r.status ? 1u : 0u));
}

// Backward: lk_fb_kernel's mapping, parameters, decision and side arrays (lk_fb.hpp) with the normalised body; it owns every
// row.  The template of every pair comes from the target's planes at the forward end point (per group), the searched image is
// frame1.
__global__ __launch_bounds__(256) void lk_norm_fb_kernel(const LKFBParams p) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    lk_fb_body<FBRows::All>(p, s_tmpl, [&](const LKPair& q, uint2* tm) {
        const auto level_of = [&](int level) { return lk_fb_level(p, q.grp, level); };
        return norm_lk_pair<false, false>(level_of, q.rec.x, q.rec.y, p.win, q.lane, true, p.max_level, p.max_iters, p.eps_sq, p.min_eig_thr, tm);
    });
}

bool launch_lk_norm(const LKParams& p, int win, hipStream_t s) {
    if (!lk_pair_args_ok(win, p.n_targets)) return false;
    if (p.n <= 0) return true;
    const size_t lds_bytes = (size_t)kNormWaves * win * win * sizeof(uint2);   // <= 30752
    hipLaunchKernelGGL(lk_norm_kernel, dim3((unsigned)((p.n + kNormWaves - 1) / kNormWaves)), dim3(64 * kNormWaves), lds_bytes, s, p, win);
    return true;
}

bool launch_lk_norm_fb(const LKFBParams& p, hipStream_t s) {
    if (!lk_pair_args_ok(p.win, p.n_targets)) return false;
    if (p.n <= 0) return true;
    launch_plain_geometry(lk_norm_fb_kernel, p.n, p.win, s, p);
    return true;
}

}  // namespace pc
