// lk_norm.hpp -- brightness-normalised pyramidal Lucas-Kanade of ONE point (include/polychase_hip.h: pc_lk_track_normalized has
// the rule; tests/lk_normalized_ref.py restates it in numpy).  It is plain_lk_pair (lk_plain.hpp) level by level -- bounds tests,
// bilinear weights, template_pixel, interp_u8, the 2x2 solve, the epsilon test, the oscillation exit and the level-0 L1 patch
// error are the same fp32 / integer expressions, the shared ones the same functions (lk_pair.hpp) -- with two replacements: the structure tensor is the CENTRED Gram matrix of the
// template's gradients, and the mismatch vector is that of g (J - mean J) - (I - mean I), g the ratio of the two windows'
// standard deviations.  All window sums are exact integers; fp64 appears only in the handful of scalars per level / iteration,
// every operation rounded on its own.  The arithmetic mode plays no part: one instance.
//
// Two kernels are built from it (kernels_lk_norm.hip): WAVE = true, the forward launch -- the template is the same for the eight
// targets of a keypoint, so all 64 lanes evaluate it once per level into the wavefront's LDS slice and the template sums are wave
// reductions; WAVE = false, the backward launch of the forward-backward check -- the template comes from the group's own target, so
// the group's 8 lanes evaluate it (lane l owns columns l, l + 8, ...) into the group's slice, as plain_lk_pair does.
#pragma once

#include "lk_plain.hpp"

namespace pc {

// what a level's template leaves for its iterations
struct NormTemplate {
    long long Sx, Sy;      // sums of ix, iy
    long long CIx, CIy;    // n S_Ix - S_I S_x, n S_Iy - S_I S_y
    long long vI;          // n S_II - S_I^2
    float A11, A12, A22;   // the centred Gram matrix / n, times FLT_SCALE
};
// every product and difference below stays under 2^53 (n <= 961, I <= 8160, |ix|, |iy| <= 4080): the conversions are exact
__device__ __forceinline__ NormTemplate norm_template(int n, long long SI, long long SII, long long Sx, long long Sy, long long Sxx,
                                                      long long Sxy, long long Syy, long long SIx, long long SIy) {
    const float FLT_SCALE = 1.f / (float)(1 << 20);
    const long long nn = (long long)n;
    const double dn = (double)n;
    NormTemplate T;
    T.Sx = Sx;
    T.Sy = Sy;
    T.CIx = nn * SIx - SI * Sx;
    T.CIy = nn * SIy - SI * Sy;
    T.vI = nn * SII - SI * SI;
    T.A11 = (float)((double)(nn * Sxx - Sx * Sx) / dn) * FLT_SCALE;
    T.A12 = (float)((double)(nn * Sxy - Sx * Sy) / dn) * FLT_SCALE;
    T.A22 = (float)((double)(nn * Syy - Sy * Sy) / dn) * FLT_SCALE;
    return T;
}

// level_of(level) -> PlainLKLevel (J: this lane's group's searched plane); lane: the lane's index in its wavefront; tm: the
// wavefront's (WAVE) or the group's LDS slice, win * win entries.  WAVE: all 64 lanes call, `active` says whether the lane's
// group has a pair to track (the others only help with the template).  !WAVE: the lanes of one group call, active is true.
// Every lane of a group returns the same result.  ERR: as in plain_lk_pair.
template <bool WAVE, bool ERR, class LevelOf>
__device__ __forceinline__ PlainLKResult norm_lk_pair(const LevelOf& level_of, float start_x, float start_y, int win, int lane, bool active,
                                                      int max_level, int max_iters, double eps_sq, float min_eig_thr, uint2* const tm) {
    const int lg = lane & 7;
    const int n = win * win;
    const float half_win = (float)(win - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (float)(1 << 20);
    float nx = 0.f, ny = 0.f, err = 0.f;
    bool status = true;
    for (int level = max_level; level >= 0; --level) {
        const PlainLKLevel L = level_of(level);
        const uint8_t* __restrict__ I = L.I;
        const int32_t* __restrict__ dI = L.dI;
        const uint8_t* __restrict__ J = L.J;
        const int pitch = L.pitch;
        const float lscale = 1.f / (float)(1 << level);
        float px = start_x * lscale, py = start_y * lscale;
        float qx, qy;
        if (level == max_level) {
            qx = px;
            qy = py;
        } else {
            qx = nx * 2.f;
            qy = ny * 2.f;
        }
        nx = qx;
        ny = qy;

        // ---- template ----
        px -= half_win;
        py -= half_win;
        const int ipx = (int)floorf(px), ipy = (int)floorf(py);
        if (lk_window_outside(ipx, ipy, win, L.w, L.h)) {
            if (level == 0) status = false;
            continue;
        }
        const Weights wI = bilinear_weights(px - (float)ipx, py - (float)ipy);
        const ptrdiff_t oI = (ptrdiff_t)ipy * pitch + ipx;
        NormTemplate T;
        if constexpr (WAVE) {
            // <= 16 pixels per lane: 16 * 8160^2 < 2^31
            int sI = 0, sx = 0, sy = 0, sxy = 0, sIx = 0, sIy = 0;
            uint32_t sII = 0u, sxx = 0u, syy = 0u;
            for_each_window_pixel(lane, win, [&](int i, int y, int x) {
                const TemplatePixel t = template_pixel(I, dI, pitch, oI + (ptrdiff_t)y * pitch + x, wI);
                tm[i] = pack_template(t);
                sI += t.ival;
                sII += (uint32_t)(t.ival * t.ival);
                sx += t.ix;
                sy += t.iy;
                sxx += (uint32_t)(t.ix * t.ix);
                sxy += t.ix * t.iy;
                syy += (uint32_t)(t.iy * t.iy);
                sIx += t.ival * t.ix;
                sIy += t.ival * t.iy;
            });
            T = norm_template(n, (long long)wave_sum_i32(sI), wave_sum_u32(sII), (long long)wave_sum_i32(sx), (long long)wave_sum_i32(sy),
                              wave_sum_u32(sxx), wave_sum_s32(sxy), wave_sum_u32(syy), wave_sum_s32(sIx), wave_sum_s32(sIy));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the groups read what the whole wavefront wrote
        } else {
            int sI = 0, sx = 0, sy = 0;   // <= 124 pixels per lane
            long long sII = 0, sxx = 0, sxy = 0, syy = 0, sIx = 0, sIy = 0;
            for (int x = lg; x < win; x += 8) {
                for (int y = 0; y < win; y++) {
                    const TemplatePixel t = template_pixel(I, dI, pitch, oI + (ptrdiff_t)y * pitch + x, wI);
                    tm[y * win + x] = pack_template(t);
                    sI += t.ival;
                    sII += t.ival * t.ival;
                    sx += t.ix;
                    sy += t.iy;
                    sxx += t.ix * t.ix;
                    sxy += t.ix * t.iy;
                    syy += t.iy * t.iy;
                    sIx += t.ival * t.ix;
                    sIy += t.ival * t.iy;
                }
            }
            T = norm_template(n, (long long)group_allreduce_add<8>(sI), group8_sum_s64(sII), (long long)group_allreduce_add<8>(sx),
                              (long long)group_allreduce_add<8>(sy), group8_sum_s64(sxx), group8_sum_s64(sxy), group8_sum_s64(syy),
                              group8_sum_s64(sIx), group8_sum_s64(sIy));
        }
        const float A11 = T.A11, A12 = T.A12, A22 = T.A22;
        float D = A11 * A22 - A12 * A12;
        const float tdiff = A11 - A22;
        const float min_eig = (A22 + A11 - sqrtf(tdiff * tdiff + 4.f * A12 * A12)) / (float)(2 * win * win);
        if (min_eig < min_eig_thr || D < 1.1920928955078125e-07f /* FLT_EPSILON */) {
            if (level == 0) status = false;
            continue;
        }
        D = 1.f / D;

        if (active) {
            // ---- iterations on the searched plane: lane l of the group owns columns l, l + 8, ... ----
            const long long nn = (long long)n;
            const double dn = (double)n;
            qx -= half_win;
            qy -= half_win;
            float pdx = 0.f, pdy = 0.f;
            for (int j = 0; j < max_iters; j++) {
                const int iqx = (int)floorf(qx), iqy = (int)floorf(qy);
                if (lk_window_outside(iqx, iqy, win, L.w, L.h)) {
                    if (level == 0) status = false;
                    break;
                }
                const Weights wJ = bilinear_weights(qx - (float)iqx, qy - (float)iqy);
                const uint8_t* const jb = J + (ptrdiff_t)iqy * pitch + iqx;
                int tJ = 0;
                long long tJJ = 0, tJx = 0, tJy = 0;
                for (int x = lg; x < win; x += 8) {
                    const uint8_t* s = jb + x;
                    int t0 = s[0], t1 = s[1];   // the bottom taps of a row are the top taps of the next
                    uint32_t cJJ = 0u;          // one column: 31 * 8160^2 < 2^32, 31 * 8160 * 4080 < 2^31
                    int cJx = 0, cJy = 0;
                    for (int y = 0; y < win; y++) {
                        s += pitch;
                        const int u0 = s[0], u1 = s[1];
                        const uint2 t = tm[y * win + x];
                        const int vj = interp_u8(t0, t1, u0, u1, wJ);   // 0 .. 8160
                        tJ += vj;
                        cJJ += (uint32_t)(vj * vj);
                        cJx += vj * (int)(int16_t)(t.y & 0xffffu);
                        cJy += vj * ((int)t.y >> 16);
                        t0 = u0;
                        t1 = u1;
                    }
                    tJJ += cJJ;
                    tJx += cJx;
                    tJy += cJy;
                }
                const long long TJ = (long long)group_allreduce_add<8>(tJ);   // <= 961 * 8160
                const long long TJJ = group8_sum_s64(tJJ), TJx = group8_sum_s64(tJx), TJy = group8_sum_s64(tJy);
                const long long vJ = nn * TJJ - TJ * TJ;
                const long long CJx = nn * TJx - TJ * T.Sx, CJy = nn * TJy - TJ * T.Sy;
                float g = 1.f;
                if (T.vI > 0 && vJ > 0) g = fminf(fmaxf((float)sqrt((double)T.vI / (double)vJ), 0.25f), 4.f);
                const float b1 = (float)(((double)g * (double)CJx - (double)T.CIx) / dn) * FLT_SCALE;
                const float b2 = (float)(((double)g * (double)CJy - (double)T.CIy) / dn) * FLT_SCALE;
                if (lk_newton_step(A11, A12, A22, D, b1, b2, half_win, j, eps_sq, qx, qy, nx, ny, pdx, pdy)) break;
            }

            // ---- L1 patch error at level 0: OpenCV's, un-normalised ----
            if (status && level == 0) {
                const float ex = nx - half_win, ey = ny - half_win;
                const int iex = (int)floorf(ex), iey = (int)floorf(ey);
                if (lk_window_outside(iex, iey, win, L.w, L.h)) {
                    status = false;
                } else if constexpr (ERR) {
                    const Weights wE = bilinear_weights(ex - (float)iex, ey - (float)iey);
                    const uint8_t* const eb = J + (ptrdiff_t)iey * pitch + iex;
                    int se = 0;
                    for (int x = lg; x < win; x += 8) {
                        const uint8_t* s = eb + x;
                        int t0 = s[0], t1 = s[1];
                        for (int y = 0; y < win; y++) {
                            s += pitch;
                            const int u0 = s[0], u1 = s[1];
                            const int diff = interp_u8(t0, t1, u0, u1, wE) - (int)tm[y * win + x].x;
                            se += diff < 0 ? -diff : diff;
                            t0 = u0;
                            t1 = u1;
                        }
                    }
                    se = group_allreduce_add<8>(se);   // <= 31^2 * 8160 < 2^24: exact in fp32 too
                    err = ((float)se * 1.f) / (float)(32 * win * win);
                }
            }
        }
        if constexpr (WAVE) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next level's template overwrites the slice
    }
    PlainLKResult r;
    r.nx = nx;
    r.ny = ny;
    r.status = status;
    r.err = status ? err : 0.f;
    return r;
}

}  // namespace pc
