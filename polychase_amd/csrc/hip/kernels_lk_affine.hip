// kernels_lk_affine.hip -- affine refinement of the LK flow rows on gfx950 (include/polychase_hip.h: pc_lk_track_affine has the
// rule; DESIGN.md section 4 "Affine refinement"; the rule restated in numpy: tests/lk_affine_ref.py).
//
// After the forward launch (kernels_lk*.hip) has left its raw records out_rec[slot * 8 + target] = (q, err, status_f), ONE launch
// refines, for every record with status_f == 1, the end point at level 0 under a 6-parameter warp of the window: Gauss-Newton on
// J(c + M (x - centre)) - I(x) from c = q, M = identity, with the template's 6 x 6 matrix H = sum g g^T factored once per keypoint.
// A record is overwritten with (cx, cy, err_a) only when the refined window matches its patch no worse than the stored one and the
// warp stayed near the identity; the status never changes, and everything downstream of the records is unchanged.
//
// Mapping (lk_corr_kernel's): one wavefront per keypoint in the visiting order of the forward launch, one group of 8 lanes per
// target.  The template is the same for the eight targets: all 64 lanes evaluate it once into the wavefront's slice of LDS
// (pack_template's 8 bytes per pixel, <= 7688 bytes), the 21 entries of H are exact wave reductions, and the fp64 Cholesky factor
// (uniform over the wavefront) goes to 168 bytes of LDS beside it.  Each group then runs its row: a lane owns whole window columns,
// computes every pixel's position and weights, gathers its four bytes from the padded u8 plane and accumulates the six b_i in
// int64.  No pixel is read before its own floor passed the bounds test of the rule, which keeps all four taps inside the padding
// (win rows, >= win columns), whatever the kernel is handed.  fp64 appears only in the factor, the two triangular solves and the
// stop test.  Nothing crosses wavefronts: no barrier.  The window is a RUNTIME value (3 .. PC_MAX_WINDOW) and the arithmetic mode
// plays no part: one instance.  Who a lane is, the walk of the window and the exact sums are lk_pair.hpp's.
#include "lk_plain.hpp"

namespace pc {

constexpr int kAffWaves = 4;                                  // wavefronts (keypoints) per workgroup
constexpr int kAffSlice = PC_MAX_WINDOW * PC_MAX_WINDOW;      // template entries per wavefront

// index of L[i][j], j <= i, in the packed lower triangle
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// The warped J window of one group at (cx, cy, m), a lane walking columns lg, lg + 8, ...  SOLVE: the six b_i = sum e g_i;
// otherwise sum |e| in b[0].  -> false (uniform in the group) when a pixel fails the bounds test; then nothing of b is valid.
template <bool SOLVE>
__device__ __forceinline__ bool affine_window(const uint8_t* __restrict__ J, int pitch, int w, int h, int win, int lg, const uint2* tm,
                                              float cx, float cy, float m11, float m12, float m21, float m22, long long (&b)[6]) {
    const float lo = (float)(-win), hix = (float)(w + win - 2), hiy = (float)(h + win - 2);
    long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
    int failed = 0;
    for (int c = lg; c < win && !failed; c += 8) {
        const int U = 2 * c - (win - 1);
        const float u = (float)U * 0.5f;
        const float xc = cx + m11 * u, yc = cy + m21 * u;
        int V = -(win - 1);
        for (int r = 0; r < win; r++, V += 2) {
            const float v = (float)V * 0.5f;
            const float xj = xc + m12 * v, yj = yc + m22 * v;
            const float fx = floorf(xj), fy = floorf(yj);
            if (!(fx >= lo && fx <= hix && fy >= lo && fy <= hiy)) {   // a NaN fails
                failed = 1;
                break;
            }
            const Weights wJ = bilinear_weights(xj - fx, yj - fy);
            const uint8_t* const s = J + (ptrdiff_t)(int)fy * pitch + (int)fx;
            const int jv = interp_u8(s[0], s[1], s[pitch], s[pitch + 1], wJ);   // 0 .. 8160
            const uint2 t = tm[r * win + c];
            const int e = jv - (int)t.x;                                         // |e| <= 8160
            if constexpr (SOLVE) {
                const int ex = e * (int)(int16_t)(t.y & 0xffffu), ey = e * ((int)t.y >> 16);   // |.| < 2^26
                s0 += (long long)ex * U;
                s1 += (long long)ex * V;
                s2 += (long long)ey * U;
                s3 += (long long)ey * V;
                s4 += ex;
                s5 += ey;
            } else {
                s0 += e < 0 ? -e : e;
            }
        }
    }
    if (group_allreduce_add<8>(failed) != 0) return false;
    b[0] = group8_sum_s64(s0);   // |.| <= 961 * 2^26 * 30 < 2^47
    if constexpr (SOLVE) {
        b[1] = group8_sum_s64(s1);
        b[2] = group8_sum_s64(s2);
        b[3] = group8_sum_s64(s3);
        b[4] = group8_sum_s64(s4);
        b[5] = group8_sum_s64(s5);
    }
    return true;
}

__global__ __launch_bounds__(64 * kAffWaves) void lk_affine_kernel(const AffineParams p) {
    __shared__ uint2 s_tm[kAffWaves][kAffSlice];
    __shared__ double s_L[kAffWaves][24];
    LKPair q;
    if (!lk_pair_prologue<true, kAffWaves, false>(q, p)) return;   // whole wavefronts
    if (__ballot(q.fwd_ok) == 0ull) return;                                  // uniform in the wavefront
    lk_pair_keypoint(q, p.perm);
    const int wave = q.wave, lane = q.lane, grp = q.grp, lg = q.lg;
    const float4 rec = q.rec;

    const int win = p.win, n = win * win;
    const int w = p.f1.w, h = p.f1.h, pitch = p.f1.pitch;
    const float half_win = (float)(win - 1) * 0.5f;
    uint2* const tm = s_tm[wave];
    double* const Ls = s_L[wave];

    // ---- template: all 64 lanes, pixel i at (r, c) = (i / win, i % win); H = sum g g^T, exact ----
    const float2 pt = p.pts[q.feat];
    const float px = pt.x - half_win, py = pt.y - half_win;
    const int ipx = (int)floorf(px), ipy = (int)floorf(py);
    bool can = !lk_window_outside(ipx, ipy, win, w, h);   // uniform in the wavefront
    if (can) {
        const Weights wI = bilinear_weights(px - (float)ipx, py - (float)ipy);
        const ptrdiff_t oI = (ptrdiff_t)ipy * pitch + ipx;
        long long hs[21];
#pragma unroll
        for (int k = 0; k < 21; k++) hs[k] = 0;
        for_each_window_pixel(lane, win, [&](int i, int r, int c) {
            const TemplatePixel t = template_pixel(p.f1.img, p.f1.der, pitch, oI + (ptrdiff_t)r * pitch + c, wI);
            tm[i] = pack_template(t);
            const int U = 2 * c - (win - 1), V = 2 * r - (win - 1);
            const long long g[6] = {(long long)(t.ix * U), (long long)(t.ix * V), (long long)(t.iy * U), (long long)(t.iy * V),
                                    (long long)t.ix, (long long)t.iy};   // |g| < 2^20, <= 16 pixels per lane: partials < 2^44
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int bb = 0; bb <= a; bb++) hs[tri(a, bb)] += g[a] * g[bb];
        });
        // ---- factor: lower Cholesky of (double)H, column by column, the same in every lane ----
        double L[21];
#pragma unroll
        for (int k = 0; k < 21; k++) L[k] = (double)wave_sum_s64(hs[k]);   // partials < 2^44; below 2^53: exact
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double s = L[tri(j, j)];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - L[tri(j, k)] * L[tri(j, k)];
            if (!(s > 0.0)) can = false;
            const double d = sqrt(s);
            L[tri(j, j)] = d;
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double t = L[tri(i, j)];
#pragma unroll
                for (int k = 0; k < j; k++) t = t - L[tri(i, k)] * L[tri(j, k)];
                L[tri(i, j)] = t / d;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 21; k++) Ls[k] = L[k];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the groups read what the whole wavefront wrote

    if (!q.fwd_ok) return;   // whole groups; nothing below crosses a group

    // ---- the row: one group per target ----
    float cx = rec.x, cy = rec.y, m11 = 1.f, m12 = 0.f, m21 = 0.f, m22 = 1.f;
    bool accepted = false;
    float err_a = 0.f;
    if (can) {
        const uint8_t* const J = p.timg[grp];
        const double scale = (double)((win - 1) * (win - 1));
        long long b[6];
        bool ok = true;
        for (int it = 0; it < p.max_iters; it++) {
            ok = affine_window<true>(J, pitch, w, h, win, lg, tm, cx, cy, m11, m12, m21, m22, b);
            if (!ok) break;
            // L L^T t = -b
            double t[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double s = -(double)b[i];
#pragma unroll
                for (int k = 0; k < i; k++) s = s - Ls[tri(i, k)] * t[k];
                t[i] = s / Ls[tri(i, i)];
            }
#pragma unroll
            for (int i = 5; i >= 0; i--) {
                double s = t[i];
#pragma unroll
                for (int k = i + 1; k < 6; k++) s = s - Ls[tri(k, i)] * t[k];
                t[i] = s / Ls[tri(i, i)];
            }
            m11 += (float)(2.0 * t[0]);
            m12 += (float)(2.0 * t[1]);
            m21 += (float)(2.0 * t[2]);
            m22 += (float)(2.0 * t[3]);
            cx += (float)t[4];
            cy += (float)t[5];
            if ((t[4] * t[4] + t[5] * t[5]) + scale * (((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + t[3] * t[3]) <= p.eps_sq) break;
        }
        if (ok) ok = affine_window<false>(J, pitch, w, h, win, lg, tm, cx, cy, m11, m12, m21, m22, b);
        if (ok) {
            err_a = (float)b[0] / (float)(32 * n);   // <= 961 * 8160 < 2^24: the conversion is exact
            const float det = m11 * m22 - m12 * m21;
            const float ddx = cx - rec.x, ddy = cy - rec.y;
            accepted = err_a <= rec.z && det >= 0.5f && det <= 2.0f && fabsf(m11 - 1.f) <= 0.5f && fabsf(m12) <= 0.5f &&
                       fabsf(m21) <= 0.5f && fabsf(m22 - 1.f) <= 0.5f && ddx * ddx + ddy * ddy <= half_win * half_win;
        }
    }

    if (lg == 0) {
        if (accepted) p.rec[(size_t)q.slot * kRecStride + grp] = make_float4(cx, cy, err_a, __uint_as_float(1u));
        if (p.affine_m) p.affine_m[q.side(p.n)] = make_float4(m11, m12, m21, m22);
        if (p.affine_state) p.affine_state[q.side(p.n)] = accepted ? (uint8_t)1 : (uint8_t)2;
    }
}

bool launch_lk_affine(const AffineParams& p, hipStream_t s) {
    if (!lk_pair_args_ok(p.win, p.n_targets)) return false;
    if (p.n <= 0) return true;
    hipLaunchKernelGGL(lk_affine_kernel, dim3((unsigned)((p.n + kAffWaves - 1) / kAffWaves)), dim3(64 * kAffWaves), 0, s, p);
    return true;
}

}  // namespace pc
