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
// lk_wmask_fb_kernel   lk_fb_kernel with the weights of the template image, the target; a target without weights takes the same
//                   body with every sample on, which is the plain pass bit for bit.
#include "lk_plain.hpp"

namespace pc {

template <bool X86>
__global__ __launch_bounds__(256) void lk_wmask_kernel(const LKWMaskParams p) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 3, lg = lane & 7;
    const int slot = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (slot >= p.n) return;   // whole wavefronts
    const int win = p.win;
    const int feat = p.perm ? (int)p.perm[slot] : slot;
    const float2 pt = p.pts[feat];

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
        if (ipx < -win || ipx >= L.w || ipy < -win || ipy >= L.h) continue;
        // a window that passed the bounds test lies inside the plane's padding, as in the image planes
        const uint8_t* __restrict__ wt = p.swt[level] + (ptrdiff_t)ipy * L.pitch + ipx;
        for (int i = lane; i < taps; i += 64) {
            const int y = i / side, x = i - y * side;
            off = off || wt[(ptrdiff_t)y * L.pitch + x] == 0;
        }
    }
    if (__ballot(off) == 0ull) return;   // untouched: the whole wavefront
    if (lane == 0 && p.touched) p.touched[feat] = 1;
    if (grp >= p.n_targets) return;      // whole groups

    const auto level_of = [&](int level) {
        const Level L = p.src[level];
        return PlainLKLevel{L.w, L.h, L.pitch, L.img, L.der, p.tgt[grp][level], p.swt[level]};
    };
    const PlainLKResult r = plain_lk_pair<X86, true, false, true>(level_of, pt.x, pt.y, win, lg, p.max_level, p.max_iters, p.eps_sq,
                                                                  p.min_eig_thr, s_tmpl + (size_t)(wave * 8 + grp) * (win * win));
    if (lg == 0) p.rec[(size_t)slot * kRecStride + grp] = make_float4(r.nx, r.ny, r.err, __uint_as_float(r.status ? 1u : 0u));
}

bool launch_lk_wmask(const LKWMaskParams& p, hipStream_t s) {
    if (p.win < 3 || p.win > PC_MAX_WINDOW || p.n_targets < 1 || p.n_targets > kRecStride) return false;
    if (p.n <= 0) return true;
    const PlainLKLaunch g = plain_lk_launch(p.n, p.win);
    if (p.x86_order) hipLaunchKernelGGL((lk_wmask_kernel<true>), dim3(g.blocks), dim3(64 * g.waves), g.lds_bytes, s, p);
    else hipLaunchKernelGGL((lk_wmask_kernel<false>), dim3(g.blocks), dim3(64 * g.waves), g.lds_bytes, s, p);
    return true;
}

static_assert(sizeof(LKWMaskFBParams) <= 4096, "the parameters travel as kernel arguments");

template <bool X86>
__global__ __launch_bounds__(256) void lk_wmask_fb_kernel(const LKWMaskFBParams q) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    const LKFBParams& p = q.fb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 3, lg = lane & 7;
    const int slot = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (slot >= p.n) return;   // whole wavefronts
    const bool tgt_active = grp < p.n_targets;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tgt_active) rec = p.rec[(size_t)slot * kRecStride + grp];
    const int feat = p.perm ? (int)p.perm[slot] : slot;
    const bool fwd_ok = tgt_active && __float_as_uint(rec.w) == 1u;   // uniform in the group

    float nx = 0.f, ny = 0.f;
    bool status = false;
    if (fwd_ok) {
        const auto level_of = [&](int level) {
            const Level L = p.f1[level];
            return PlainLKLevel{L.w, L.h, L.pitch, p.timg[grp][level], p.tder[grp][level], L.img, q.twt[grp][level]};
        };
        const PlainLKResult r = plain_lk_pair<X86, false, false, true>(level_of, rec.x, rec.y, p.win, lg, p.max_level, p.max_iters, p.eps_sq,
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

bool launch_lk_wmask_fb(const LKWMaskFBParams& q, hipStream_t s) {
    const LKFBParams& p = q.fb;
    if (p.win < 3 || p.win > PC_MAX_WINDOW || p.n_targets < 1 || p.n_targets > kRecStride || p.search_state) return false;
    if (p.n <= 0) return true;
    const PlainLKLaunch g = plain_lk_launch(p.n, p.win);
    if (p.x86_order) hipLaunchKernelGGL((lk_wmask_fb_kernel<true>), dim3(g.blocks), dim3(64 * g.waves), g.lds_bytes, s, q);
    else hipLaunchKernelGGL((lk_wmask_fb_kernel<false>), dim3(g.blocks), dim3(64 * g.waves), g.lds_bytes, s, q);
    return true;
}

}  // namespace pc
