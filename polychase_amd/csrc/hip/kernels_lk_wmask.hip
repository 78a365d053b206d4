// kernels_lk_wmask.hip -- masked LK windows on gfx950: template samples outside the mask carry no weight
// (include/polychase_hip.h: pc_lk_track_window_masked has the rule; DESIGN.md section 4 "Masked windows").
//
// Both kernels are the MASKED instances of plain_lk_pair (lk_plain.hpp), mapped like the kernels around them: one wavefront per
// keypoint in the visiting order of the forward launch, one group of 8 lanes per target, the group's template in its own slice of
// LDS, no barrier.
//
// lk_wmask_kernel   ONE launch directly after the forward launch.  Whether a keypoint is touched -- its template window has an
//                   off sample at some level that passes the bounds test -- depends on frame1's weight planes and the keypoint
//                   alone, not on the target, so the test is wave-uniform: the 64 lanes scan the (win + 1)^2 taps of each level's
//                   window, a ballot decides, and the wavefront of an untouched keypoint leaves before it builds a template and
//                   writes nothing: its records stay the product kernel's.  A touched keypoint is tracked again into every target
//                   under the rule and its records are overwritten.
// lk_wmask_fb_kernel   lk_fb_kernel (the same lk_fb_body, lk_fb.hpp) with the weights of the template image, the target; a target
//                   without weights takes the same body with every sample on, which is the plain pass bit for bit.
#include "lk_fb.hpp"

namespace pc {

template <bool X86>
__global__ __launch_bounds__(256) void lk_wmask_kernel(const LKWMaskParams p) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    LKPair q;   // the record is only written
    if (!lk_pair_prologue<false>(q, p)) return;   // whole wavefronts
    const int win = p.win;
    const float2 pt = p.pts[q.feat];

    // the touched test: the template origins of plain_lk_pair, expression for expression
    const float half_win = (float)(win - 1) * 0.5f;
    const int side = win + 1, taps = side * side;
    bool off = false;
    for (int level = p.max_level; level >= 0; --level) {
        const Level L = p.src[level];
        const float lscale = 1.f / (float)(1 << level);
        float px = pt.x * lscale, py = pt.y * lscale;
        px -= half_win;
        py -= half_win;
        const int ipx = (int)floorf(px), ipy = (int)floorf(py);
        if (lk_window_outside(ipx, ipy, win, L.w, L.h)) continue;
        // a window that passed the bounds test lies inside the plane's padding, as in the image planes
        const uint8_t* __restrict__ wt = p.swt[level] + (ptrdiff_t)ipy * L.pitch + ipx;
        for (int i = q.lane; i < taps; i += 64) {
            const int y = i / side, x = i - y * side;
            off = off || wt[(ptrdiff_t)y * L.pitch + x] == 0;
        }
    }
    if (__ballot(off) == 0ull) return;   // untouched: the whole wavefront
    if (q.lane == 0 && p.touched) p.touched[q.feat] = 1;
    if (!q.tgt_active) return;   // whole groups

    const auto level_of = [&](int level) {
        const Level L = p.src[level];
        return PlainLKLevel{L.w, L.h, L.pitch, L.img, L.der, p.tgt[q.grp][level], p.swt[level]};
    };
    const PlainLKResult r = plain_lk_pair<X86, true, false, true>(level_of, pt.x, pt.y, win, q.lg, p.max_level, p.max_iters, p.eps_sq,
                                                                  p.min_eig_thr, s_tmpl + (size_t)(q.wave * 8 + q.grp) * (win * win));
    if (q.lg == 0) p.rec[(size_t)q.slot * kRecStride + q.grp] = make_float4(r.nx, r.ny, r.err, __uint_as_float(r.status ? 1u : 0u));
}

bool launch_lk_wmask(const LKWMaskParams& p, hipStream_t s) {
    if (!lk_pair_args_ok(p.win, p.n_targets)) return false;
    if (p.n <= 0) return true;
    launch_plain_geometry(p.x86_order ? lk_wmask_kernel<true> : lk_wmask_kernel<false>, p.n, p.win, s, p);
    return true;
}

static_assert(sizeof(LKWMaskFBParams) <= 4096, "the parameters travel as kernel arguments");

// it owns every row: the launcher refuses a job with a search prepass
template <bool X86>
__global__ __launch_bounds__(256) void lk_wmask_fb_kernel(const LKWMaskFBParams m) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    const LKFBParams& p = m.fb;
    lk_fb_body<FBRows::All>(p, s_tmpl, [&](const LKPair& q, uint2* tm) {
        const auto level_of = [&](int level) { return lk_fb_level(p, q.grp, level, m.twt[q.grp][level]); };
        return plain_lk_pair<X86, false, false, true>(level_of, q.rec.x, q.rec.y, p.win, q.lg, p.max_level, p.max_iters, p.eps_sq, p.min_eig_thr, tm);
    });
}

bool launch_lk_wmask_fb(const LKWMaskFBParams& m, hipStream_t s) {
    const LKFBParams& p = m.fb;
    if (!lk_pair_args_ok(p.win, p.n_targets) || p.search_state) return false;
    if (p.n <= 0) return true;
    launch_plain_geometry(p.x86_order ? lk_wmask_fb_kernel<true> : lk_wmask_fb_kernel<false>, p.n, p.win, s, m);
    return true;
}

}  // namespace pc
