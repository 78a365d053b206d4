// lk_fb.hpp -- the backward launch of the forward-backward check, whatever body tracks the pair: who owns a row, what "within
// the threshold" means, and what the side arrays hold.  lk_norm_fb_kernel (kernels_lk_norm.hip), lk_search_fb_kernel
// (kernels_lk_search.hip) and lk_wmask_fb_kernel (kernels_lk_wmask.hip) are this body with their row filter and their way of
// tracking one pair; lk_fb_kernel (kernels_lk_fb.hip) is FBRows::NotReplaced written out, for a register (see there).
#pragma once

#include "lk_plain.hpp"

namespace pc {

// which rows a backward kernel owns; a row it does not own it neither tracks nor writes
enum class FBRows {
    All,           // every (keypoint, target) pair
    NotReplaced,   // all but the rows the search prepass replaced (state 1); p.search_state may be null: then all
    Replaced       // only those, p.search_state is not null; the group of any other row leaves before it loads its record
};

// s_tmpl: the workgroup's dynamic LDS in the plain geometry; track(q, tm) -> PlainLKResult tracks the pair q back from (q.rec.x,
// q.rec.y) with the group's slice tm and is called for the rows whose forward status is 1.  A row is kept when the backward pass
// succeeds and ends within the threshold of the keypoint -- fp32, each operation rounded on its own, a NaN fails --, otherwise the
// status word of its record is cleared.  back_xy / back_status: the backward end point and status, zeros for a row whose forward
// pass had failed already.
template <FBRows ROWS, class Track>
__device__ __forceinline__ void lk_fb_body(const LKFBParams& p, uint2* const s_tmpl, const Track& track) {
    LKPair q;
    if (!lk_pair_prologue<ROWS != FBRows::Replaced>(q, p)) return;   // whole wavefronts
    bool owned = q.tgt_active;
    if constexpr (ROWS == FBRows::Replaced) {
        if (!owned || p.search_state[q.side(p.n)] != 1) return;   // whole groups; nothing below crosses a group
        lk_pair_record(q, p.rec);                                 // only now: a check in between may have dropped the row
    } else if constexpr (ROWS == FBRows::NotReplaced) {
        const bool replaced = p.search_state && owned && p.search_state[q.side(p.n)] == 1;   // lk_search_fb_kernel's row
        owned = owned && !replaced;
    }
    const bool fwd_ok = owned && __float_as_uint(q.rec.w) == 1u;   // uniform in the group

    float nx = 0.f, ny = 0.f;
    bool status = false;
    if (fwd_ok) {
        const PlainLKResult r = track(q, s_tmpl + (size_t)(q.wave * 8 + q.grp) * (p.win * p.win));
        nx = r.nx;
        ny = r.ny;
        status = r.status;
    }

    if (q.lg == 0 && owned) {
        if (fwd_ok) {
            const float2 pt = p.pts[q.feat];
            const float dx = nx - pt.x, dy = ny - pt.y;
            const float d2 = dx * dx + dy * dy;
            const bool keep = status && (d2 <= p.thr2);   // a NaN fails
            if (!keep) p.rec[(size_t)q.slot * kRecStride + q.grp].w = __uint_as_float(0u);
        }
        const size_t o = q.side(p.n);
        if (p.back_xy) p.back_xy[o] = fwd_ok ? make_float2(nx, ny) : make_float2(0.f, 0.f);
        if (p.back_status) p.back_status[o] = (fwd_ok && status) ? (uint8_t)1 : (uint8_t)0;
    }
}

// the template of every backward pair comes from its target's planes, the searched image is frame1
__device__ __forceinline__ PlainLKLevel lk_fb_level(const LKFBParams& p, int grp, int level, const uint8_t* wt = nullptr) {
    const Level L = p.f1[level];
    return PlainLKLevel{L.w, L.h, L.pitch, p.timg[grp][level], p.tder[grp][level], L.img, wt};
}

}  // namespace pc
