// kernels_lk_corr.hip -- minimum correlation between the reference patch and the matched patch of the LK flow rows on gfx950
// (include/polychase_hip.h: pc_lk_track_correlated has the rule; DESIGN.md section 4 "Minimum correlation").
//
// After the forward launch (kernels_lk*.hip) has left its raw records out_rec[slot * 8 + target] = (q, err, status_f), ONE launch
// evaluates, for every record with status_f == 1, the two win x win windows LK itself compared at level 0 -- the I window of the
// template pass at p - half in frame1's u8 plane, the J window of the error pass at q - half in the target's -- takes their five
// integer sums and clears the status of a row whose normalised cross-correlation lies below the threshold.  The decision is made
// on exact integers and separately rounded fp64 products: no division, no root.  Everything downstream of the records
// (forward-backward check, compaction, unpacking) is unchanged.
//
// Mapping (lk_fb_kernel's): one wavefront per keypoint in the visiting order of the forward launch, one group of 8 lanes per
// target.  The I window is the same for the eight targets: all 64 lanes evaluate it once into the wavefront's slice of LDS
// (int16 per pixel, <= 1922 bytes) and sum it; each group then gathers its own J window straight from the padded u8 plane, a lane
// walking whole window columns so that the bottom taps of a row are the top taps of the next.  No window is read before it passed
// OpenCV's bounds test on the same floats, so every read lies inside the padding (win rows, >= win columns).  Nothing crosses
// wavefronts: no barrier.  The window is a RUNTIME value (3 .. PC_MAX_WINDOW) and the arithmetic mode plays no part: one instance.
// Who a lane is, the bounds test, the walk of the I window and the exact sums are lk_pair.hpp's.
#include "lk_plain.hpp"

namespace pc {

constexpr int kCorrWaves = 4;                                              // wavefronts (keypoints) per workgroup
constexpr int kCorrSlice = (PC_MAX_WINDOW * PC_MAX_WINDOW + 1) & ~1;       // int16 entries per wavefront, a whole number of dwords

__global__ __launch_bounds__(64 * kCorrWaves) void lk_corr_kernel(const CorrParams p) {
    __shared__ int16_t s_win[kCorrWaves][kCorrSlice];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 3, lg = lane & 7;
    const int slot = (int)blockIdx.x * kCorrWaves + wave;
    if (slot >= p.n) return;   // whole wavefronts
    const bool tgt_active = grp < p.n_targets;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tgt_active) rec = p.rec[(size_t)slot * kRecStride + grp];
    const bool fwd_ok = tgt_active && __float_as_uint(rec.w) == 1u;   // uniform in the group
    const bool any_ok = __ballot(fwd_ok) != 0ull;                     // uniform in the wavefront
    const int feat = p.perm ? (int)p.perm[slot] : slot;

    const int win = p.win, n = win * win;
    const int w = p.f1.w, h = p.f1.h, pitch = p.f1.pitch;
    const float half_win = (float)(win - 1) * 0.5f;
    int16_t* const iwin = s_win[wave];

    // ---- I window: all 64 lanes, pixel i at (y, x) = (i / win, i % win) ----
    bool i_ok = false;
    int sI = 0;
    long long sII = 0;
    if (any_ok) {
        const float2 pt = p.pts[feat];
        const float px = pt.x - half_win, py = pt.y - half_win;
        const int ipx = (int)floorf(px), ipy = (int)floorf(py);
        i_ok = !lk_window_outside(ipx, ipy, win, w, h);
        if (i_ok) {
            const Weights wI = bilinear_weights(px - (float)ipx, py - (float)ipy);
            const uint8_t* const ib = p.f1.img + (ptrdiff_t)ipy * pitch + ipx;
            uint32_t s1 = 0u, s2 = 0u;                      // <= 16 pixels per lane: 16 * 8160^2 < 2^31
            for_each_window_pixel(lane, win, [&](int i, int y, int x) {
                const uint8_t* const s = ib + (ptrdiff_t)y * pitch + x;
                const int v = interp_u8(s[0], s[1], s[pitch], s[pitch + 1], wI);   // 0 .. 8160
                iwin[i] = (int16_t)v;
                s1 += (uint32_t)v;
                s2 += (uint32_t)(v * v);
            });
            sI = wave_sum_i32((int)s1);                     // <= 961 * 8160 < 2^23
            sII = wave_sum_u32(s2);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the groups read what the whole wavefront wrote

    // ---- J window and the decision: one group per target, lane l owns columns l, l + 8, ... ----
    bool keep = false;
    float score = 0.f;
    if (fwd_ok && i_ok) {
        const float qx = rec.x - half_win, qy = rec.y - half_win;
        const int iqx = (int)floorf(qx), iqy = (int)floorf(qy);
        if (!lk_window_outside(iqx, iqy, win, w, h)) {
            const Weights wJ = bilinear_weights(qx - (float)iqx, qy - (float)iqy);
            const uint8_t* const jb = p.timg[grp] + (ptrdiff_t)iqy * pitch + iqx;
            int sJ = 0;
            long long sJJ = 0, sIJ = 0;   // non-negative
            for (int x = lg; x < win; x += 8) {
                const uint8_t* s = jb + x;
                int t0 = s[0], t1 = s[1];
                uint32_t cJJ = 0u, cIJ = 0u;                // one column: 31 * 8160^2 < 2^31
                for (int y = 0; y < win; y++) {
                    s += pitch;
                    const int u0 = s[0], u1 = s[1];
                    const int vj = interp_u8(t0, t1, u0, u1, wJ);
                    const int vi = (int)iwin[y * win + x];
                    sJ += vj;
                    cJJ += (uint32_t)(vj * vj);
                    cIJ += (uint32_t)(vi * vj);
                    t0 = u0;
                    t1 = u1;
                }
                sJJ += cJJ;
                sIJ += cIJ;
            }
            const long long SJ = (long long)group_allreduce_add<8>(sJ);   // <= 961 * 8160
            const long long SJJ = group8_sum_s64(sJJ), SIJ = group8_sum_s64(sIJ);   // 961 * 8160^2 < 2^47
            const long long nn = (long long)n, SI = (long long)sI;
            const long long cov = nn * SIJ - SI * SJ;                     // |.| <= 961 * 961 * 8160^2 < 2^46
            const long long vI = nn * sII - SI * SI, vJ = nn * SJJ - SJ * SJ;
            const double dc = (double)cov;                                // exact
            const double dv = (double)vI * (double)vJ;
            const double lhs = dc * dc, rhs = dv * p.t2;
            keep = cov > 0 && lhs >= rhs;
            if (p.corr && vI != 0 && vJ != 0) score = (float)(dc / sqrt(dv));
        }
    }

    if (lg == 0 && tgt_active) {
        if (fwd_ok && p.drop && !keep) p.rec[(size_t)slot * kRecStride + grp].w = __uint_as_float(0u);
        if (p.corr) p.corr[(size_t)grp * (size_t)p.n + (size_t)feat] = score;
    }
}

bool launch_lk_corr(const CorrParams& p, hipStream_t s) {
    if (!lk_pair_args_ok(p.win, p.n_targets)) return false;
    if (p.n <= 0) return true;
    hipLaunchKernelGGL(lk_corr_kernel, dim3((unsigned)((p.n + kCorrWaves - 1) / kCorrWaves)), dim3(64 * kCorrWaves), 0, s, p);
    return true;
}

}  // namespace pc
