// kernels_lk_fb.hip -- forward-backward consistency check of the LK flow (Kalal et al., 2010) on gfx950.
//
// After the forward launch (kernels_lk*.hip) has left its raw records out_rec[slot * 8 + target] = (q, err, status_f), ONE
// launch tracks every surviving q back from its target into frame1 -- calcOpticalFlowPyrLK(prev = target, next = frame1,
// pts = {q}), bit for bit oracle/pc_oracle.c's pco_lk in the context's arithmetic mode -- and clears the status of a row whose
// backward pass fails or lands further than the threshold from the keypoint it started at.  Everything downstream of the
// records (compaction, unpacking) is unchanged.
//
// Mapping: one wavefront per keypoint (visiting order of the forward launch), one group of 8 lanes per target.  The decision and
// the side arrays are those of lk_fb_body (lk_fb.hpp), which the backward kernels of the options are built from; the pass itself is plain_lk_pair
// (lk_plain.hpp) with the roles of the images swapped: the template of every pair comes from the target's planes at the forward
// end point, the searched image is frame1.  Pairs with status_f == 0 do no work; a wavefront without a surviving pair only writes
// its zeros to the side arrays.
#include "lk_fb.hpp"

namespace pc {

// lk_fb_body<FBRows::NotReplaced> written out: built from the shared body the x86-order instance allocates 79 VGPRs instead of its
// 78, whichever way the body is spelled, so this one kernel keeps its text.  What it decides and writes is what lk_fb_body does.
template <bool X86>
__global__ __launch_bounds__(256) void lk_fb_kernel(const LKFBParams p) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 3, lg = lane & 7;
    const int slot = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (slot >= p.n) return;   // whole wavefronts
    const bool tgt_active = grp < p.n_targets;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tgt_active) rec = p.rec[(size_t)slot * kRecStride + grp];
    const int feat = p.perm ? (int)p.perm[slot] : slot;
    // search prepass: a row it replaced (state 1) is lk_search_fb_kernel's, this launch neither tracks nor writes it
    const bool guided = p.search_state && tgt_active && p.search_state[(size_t)grp * (size_t)p.n + (size_t)feat] == 1;
    const bool fwd_ok = tgt_active && !guided && __float_as_uint(rec.w) == 1u;   // uniform in the group

    float nx = 0.f, ny = 0.f;
    bool status = false;
    if (fwd_ok) {
        const auto level_of = [&](int level) { return lk_fb_level(p, grp, level); };
        const PlainLKResult r = plain_lk_pair<X86, false>(level_of, rec.x, rec.y, p.win, lg, p.max_level, p.max_iters, p.eps_sq, p.min_eig_thr,
                                                          s_tmpl + (size_t)(wave * 8 + grp) * (p.win * p.win));
        nx = r.nx;
        ny = r.ny;
        status = r.status;
    }

    if (lg == 0 && tgt_active && !guided) {
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

bool launch_lk_fb(const LKFBParams& p, hipStream_t s) {
    if (!lk_pair_args_ok(p.win, p.n_targets)) return false;
    if (p.n <= 0) return true;
    launch_plain_geometry(p.x86_order ? lk_fb_kernel<true> : lk_fb_kernel<false>, p.n, p.win, s, p);
    return true;
}

}  // namespace pc
