// kernels_lk_search.hip -- search prepass of the LK flow rows on gfx950 (include/polychase_hip.h: pc_lk_track_search has the rule;
// DESIGN.md section 4 "Search prepass"; the rule restated in numpy: tests/lk_search_ref.py).
//
// After the forward launch (kernels_lk*.hip) has left its raw records out_rec[slot * 8 + target] = (q, err, status_f), ONE launch
// does three things per (keypoint, target) pair: it finds an integer displacement d by matching the 8 x 8 block around the keypoint
// against the target's plane at pyramid level s (at most 33 x 33 candidates, sum of absolute differences), runs the canonical
// plain LK pass (lk_plain.hpp, with the patch error) once more with the top level's search started at p + d, and keeps whichever
// of the two results has the smaller stored patch error.  A pair whose best candidate is the zero displacement, or is not 25 %
// better than it, does nothing more and leaves its record untouched.
//
// Mapping (lk_affine_kernel's): one wavefront per keypoint in the visiting order of the forward launch, one group of 8 lanes per
// target.  The template block is the same for the eight targets: the 64 lanes fetch one byte each into 64 bytes of LDS, and every
// lane keeps the 16 dwords in registers.  Each group stages its target's search region, (8 + 2 r) rows, in its own slice of LDS
// as the ALIGNED dwords of the plane that cover it (the interior origin and the pitch are multiples of 4): a dword is read only
// when its row and its first byte lie inside the interior, so at most three bytes of the right padding travel along, and they are
// never compared -- a candidate exists only where its whole block is inside; everything else is stored as 0.  A lane then owns
// the candidates dx = lo + lg, lo + lg + 8, ...: for each it walks the region's rows ONCE, builds the row's eight bytes from three
// dwords with v_alignbyte_b32, and adds them to the eight candidates dy the row belongs to (two v_sad_u8 each, template row
// k = row - dy), the running sums in eight registers that rotate as candidates complete.  The smallest key (SAD, dx^2 + dy^2,
// dy, dx) goes through the group as one 64-bit minimum.  The guided pass reuses the group's slice for its template (8 bytes per window pixel): every lane of the group is past its last read of the region by then (the
// minimum is a cross-lane operation in between).  Nothing crosses wavefronts: no barrier.  Window, level and radius are RUNTIME
// values and the arithmetic mode plays no part: one instance.
//
// lk_search_fb_kernel: the backward pass of the forward-backward check for the rows the search replaced (state 1), the same
// canonical body with the roles of the images swapped and the top level started at q - d; lk_fb_kernel (kernels_lk_fb.hip) leaves
// those rows to it, and the decision and the side arrays are the ones both share (lk_fb.hpp: lk_fb_body).
#include "lk_fb.hpp"

namespace pc {

constexpr int kSearchBlock = 8;     // the block is 8 x 8 pixels
constexpr int kSearchMaxR = 16;     // |dx|, |dy| <= 16 at the search level

// bytes of LDS per group: the search region (rows of whole dwords: up to 3 bytes in front of the region's first column, one dword
// of slack for the third aligned read of a row) or the template of the guided pass, whichever is larger; a multiple of 16
__host__ __device__ __forceinline__ int search_region_pitch(int r) { return ((kSearchBlock + 2 * r + 3 + 3) / 4 + 1) * 4; }
__host__ __device__ __forceinline__ int search_slice_bytes(int r, int win) {
    const int region = (kSearchBlock + 2 * r) * search_region_pitch(r), tmpl = win * win * (int)sizeof(uint2);
    return ((region > tmpl ? region : tmpl) + 15) & ~15;
}
__host__ __device__ __forceinline__ int search_wave_bytes(int r, int win) { return 64 + kRecStride * search_slice_bytes(r, win); }

__device__ __forceinline__ unsigned long long search_key(uint32_t sad, int dx, int dy) {
    return ((unsigned long long)sad << 32) | (unsigned long long)(uint32_t)(((dx * dx + dy * dy) << 16) | ((dy + kSearchMaxR) << 8) | (dx + kSearchMaxR));
}

// The smallest key among the candidates (dx, dy), dy = c - r for c_lo <= c <= c_hi, whose blocks start at byte `xoff` of the region's
// rows (rpd dwords per row): rows c_lo .. c_hi + 7 are walked once, row ry adds its eight bytes to the candidates c = ry - k under
// template row k; acc[(c - c_lo) & 7] is candidate c's running sum, complete and handed on with its eighth row.
__device__ __forceinline__ unsigned long long column_best(const uint32_t* __restrict__ region, int rpd, int xoff, int dx, int r, int c_lo, int c_hi,
                                                          int last_row, const uint32_t (&t)[16], unsigned long long best) {
    const uint32_t* const col = region + (xoff >> 2);
    const uint32_t sh = (uint32_t)xoff & 3u;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = c_lo; base <= c_hi + 7; base += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int ry = base + j;
            const uint32_t* const rp = col + min(ry, last_row) * rpd;   // rows past c_hi + 7 only feed sums that are never looked at
            const uint32_t w0 = rp[0], w1 = rp[1], w2 = rp[2];
            const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh), hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
#pragma unroll
            for (int k = 0; k < 8; k++)
                acc[(j - k) & 7] = __builtin_amdgcn_sad_u8(hi, t[2 * k + 1], __builtin_amdgcn_sad_u8(lo, t[2 * k], acc[(j - k) & 7]));
            const int c = ry - 7;   // complete with this row: its sum is in acc[(j + 1) & 7]
            if (c >= c_lo && c <= c_hi) {
                const unsigned long long key = search_key(acc[(j + 1) & 7], dx, c - r);
                best = key < best ? key : best;
            }
            acc[(j + 1) & 7] = 0;
        }
    }
    return best;
}

__device__ __forceinline__ unsigned long long group8_min_u64(unsigned long long v) {
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        const unsigned long long o = __shfl_xor(v, m, 8);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void lk_search_kernel(const SearchParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_search[];
    LKPair q;   // the record is read last, by one lane
    if (!lk_pair_prologue<false>(q, p)) return;   // whole wavefronts
    const int wave = q.wave, lane = q.lane, grp = q.grp, lg = q.lg, slot = q.slot, feat = q.feat;
    const bool tgt_active = q.tgt_active;
    const size_t o = q.side(p.n);
    const int r = p.r, s = p.s;
    uint8_t* const wmem = s_search + (size_t)wave * search_wave_bytes(r, p.win);
    uint8_t* const slice = wmem + 64 + grp * search_slice_bytes(r, p.win);

    // ---- template block: uniform in the wavefront ----
    const float2 pt = p.pts[feat];
    const Level Ls = p.src[s];
    const int ws = Ls.w, hs = Ls.h, pitch = Ls.pitch;
    const float lscale = 1.f / (float)(1 << s);
    const float fcx = floorf(pt.x * lscale + 0.5f), fcy = floorf(pt.y * lscale + 0.5f);
    // in fp32 first (a NaN or an infinity fails; the values that pass are small integers, exact in fp32 and in int)
    const bool inside = fcx - 4.f >= 0.f && fcx + 4.f <= (float)ws && fcy - 4.f >= 0.f && fcy + 4.f <= (float)hs;
    if (!inside) {
        if (lg == 0 && tgt_active) {
            if (p.search_d) p.search_d[o] = make_short2(0, 0);
            if (p.search_state) p.search_state[o] = 0;
        }
        return;
    }
    const int ox = (int)fcx - 4, oy = (int)fcy - 4;
    wmem[lane] = Ls.img[(ptrdiff_t)(oy + (lane >> 3)) * pitch + ox + (lane & 7)];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // every lane reads what the whole wavefront wrote
    uint32_t t[16];
#pragma unroll
    for (int k = 0; k < 16; k++) t[k] = reinterpret_cast<const uint32_t*>(wmem)[k];

    if (!tgt_active) return;   // whole groups; nothing below crosses a group

    // ---- the target's search region: region row ry is plane row oy - r + ry, its dword k the plane's aligned dword at x = ax + 4 k,
    // ax = ox - r rounded down to a multiple of 4; a dword whose row or first byte lies outside the interior is 0 ----
    const uint8_t* __restrict__ const Js = p.tgt[grp][s];
    const int rpd = search_region_pitch(r) >> 2, rows = kSearchBlock + 2 * r;
    const int ax = (ox - r) & ~3, lead = (ox - r) - ax;   // 0 .. 3 bytes in front of the region's first column
    uint32_t* const region = reinterpret_cast<uint32_t*>(slice);
    for (int i = lg; i < rows * rpd; i += 8) {
        const int ry = i / rpd, k = i - ry * rpd;
        const int y = oy - r + ry, x = ax + 4 * k;
        uint32_t v = 0;
        if (y >= 0 && y < hs && x >= 0 && x < ws) v = *reinterpret_cast<const uint32_t*>(Js + (ptrdiff_t)y * pitch + x);
        region[i] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the group reads what its eight lanes wrote

    // ---- candidates: the displacements whose block lies inside the interior; (0, 0) is one of them ----
    const int dx_lo = max(-r, -ox), dx_hi = min(r, ws - kSearchBlock - ox);
    const int dy_lo = max(-r, -oy), dy_hi = min(r, hs - kSearchBlock - oy);
    unsigned long long best = ~0ull;
    for (int dx = dx_lo + lg; dx <= dx_hi; dx += 8) best = column_best(region, rpd, lead + dx + r, dx, r, dy_lo + r, dy_hi + r, rows - 1, t, best);
    best = group8_min_u64(best);
    const uint32_t sad_zero = (uint32_t)(column_best(region, rpd, lead + r, 0, r, r, r, rows - 1, t, ~0ull) >> 32);
    const uint32_t sad_best = (uint32_t)(best >> 32);
    int ddx = (int)(best & 0xffu) - kSearchMaxR, ddy = (int)((best >> 8) & 0xffu) - kSearchMaxR;
    if (!(4u * sad_best <= 3u * sad_zero)) ddx = ddy = 0;
    ddx *= 1 << s;
    ddy *= 1 << s;
    if (ddx == 0 && ddy == 0) {   // uniform in the group
        if (lg == 0) {
            if (p.search_d) p.search_d[o] = make_short2(0, 0);
            if (p.search_state) p.search_state[o] = 0;
        }
        return;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the region's last read precedes the template's first write

    // ---- guided pass: the canonical body with the top level started at p + d, and the better of the two records ----
    const auto level_of = [&](int level) {
        const Level L = p.src[level];
        return PlainLKLevel{L.w, L.h, L.pitch, L.img, L.der, p.tgt[grp][level]};
    };
    const PlainLKResult g = plain_lk_pair<false, true, true>(level_of, pt.x, pt.y, p.win, lg, p.max_level, p.max_iters, p.eps_sq, p.min_eig_thr,
                                                             reinterpret_cast<uint2*>(slice), pt.x + (float)ddx, pt.y + (float)ddy);
    if (lg == 0) {
        const float4 rec = p.rec[(size_t)slot * kRecStride + grp];
        const bool take = g.status && (__float_as_uint(rec.w) != 1u || g.err < rec.z);   // a NaN fails
        if (take) p.rec[(size_t)slot * kRecStride + grp] = make_float4(g.nx, g.ny, g.err, __uint_as_float(1u));
        if (p.search_d) p.search_d[o] = make_short2((short)ddx, (short)ddy);
        if (p.search_state) p.search_state[o] = take ? (uint8_t)1 : (uint8_t)2;
    }
}

__global__ __launch_bounds__(256) void lk_search_fb_kernel(const LKFBParams p) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    lk_fb_body<FBRows::Replaced>(p, s_tmpl, [&](const LKPair& q, uint2* tm) {
        const short2 d = p.search_d[q.side(p.n)];
        const auto level_of = [&](int level) { return lk_fb_level(p, q.grp, level); };
        return plain_lk_pair<false, false, true>(level_of, q.rec.x, q.rec.y, p.win, q.lg, p.max_level, p.max_iters, p.eps_sq, p.min_eig_thr, tm,
                                                 q.rec.x - (float)d.x, q.rec.y - (float)d.y);
    });
}

void search_level_radius(int search_radius, int top_level, int* s, int* r) {
    int level = 0;
    while (level < top_level && ((search_radius + (1 << level) - 1) >> level) > kSearchMaxR) level++;
    *s = level;
    *r = std::min(kSearchMaxR, (search_radius + (1 << level) - 1) >> level);
}

bool launch_lk_search(const SearchParams& p, hipStream_t s) {
    if (!lk_pair_args_ok(p.win, p.n_targets)) return false;
    if (p.r < 1 || p.r > kSearchMaxR || p.s < 0 || p.s > p.max_level) return false;
    // the region is staged in aligned dwords
    if (p.src[p.s].pitch & 3) return false;
    for (int t = 0; t < p.n_targets; t++)
        if (reinterpret_cast<uintptr_t>(p.tgt[t][p.s]) & 3) return false;
    if (p.n <= 0) return true;
    const size_t wave_bytes = (size_t)search_wave_bytes(p.r, p.win);   // <= 64 + 8 * 7696 = 61632
    static_assert(64 + kRecStride * ((PC_MAX_WINDOW * PC_MAX_WINDOW * 8 + 15) & ~15) < 65536, "one wavefront's slices must fit below 64 KiB");
    const int waves = (int)std::min<size_t>(4, 65535 / wave_bytes);
    hipLaunchKernelGGL(lk_search_kernel, dim3((unsigned)((p.n + waves - 1) / waves)), dim3(64 * waves), waves * wave_bytes, s, p);
    return true;
}

bool launch_lk_search_fb(const LKFBParams& p, hipStream_t s) {
    if (!lk_pair_args_ok(p.win, p.n_targets)) return false;
    if (!p.search_d || !p.search_state) return false;
    if (p.n <= 0) return true;
    launch_plain_geometry(lk_search_fb_kernel, p.n, p.win, s, p);
    return true;
}

}  // namespace pc
