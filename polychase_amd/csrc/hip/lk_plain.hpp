// lk_plain.hpp -- pyramidal Lucas-Kanade of ONE point by ONE group of 8 lanes, written the way oracle/pc_oracle.c's pco_lk reads:
// calcOpticalFlowPyrLK(prev = the template image, next = the searched image, pts = {start}), bit for bit in either arithmetic
// order.  Ten kernel instances are built from it:
//   lk_plain_kernel<X86>      kernels_lk.hip        the forward cross-check of the product kernels: template = frame1, searched = a
//                                                   target, with the patch error
//   lk_fb_kernel<X86>         kernels_lk_fb.hip     the backward pass of the forward-backward check (lk_fb.hpp): template = a target,
//                                                   searched = frame1, no patch error
//   lk_search_kernel          kernels_lk_search.hip the guided pass of the search prepass (GUESS), and
//   lk_search_fb_kernel                             the backward pass of the rows it replaced
//   lk_wmask_kernel<X86>      kernels_lk_wmask.hip  the MASKED instances (include/polychase_hip.h: pc_lk_track_window_masked has the
//   lk_wmask_fb_kernel<X86>                         rule), forward and backward
// and lk_norm.hpp restates it level by level for the brightness-normalised pair.  Who a lane is, the bounds test, the exact sums,
// the Newton step and the launch geometry are lk_pair.hpp's, shared with the kernels that only read the records.
//
// The group evaluates its own win x win template (patch value + Scharr pair per pixel) per level and keeps it in its own slice of
// LDS, 8 bytes per pixel; the searched image is gathered straight from the padded u8 plane: a window that passed OpenCV's bounds
// test lies inside the padding (win rows, >= win columns), and no window is read before it passed that test.  Nothing is shared
// with another group, so there is no barrier and no fence: a lane reads back only what it wrote itself (it owns whole window
// COLUMNS in every phase).  The window is a RUNTIME value (3 .. PC_MAX_WINDOW): one instance per arithmetic order.
#pragma once

#include "lk_pair.hpp"

namespace pc {

// one pyramid level of a pair: the geometry both images share, the template's u8 and Scharr planes, the searched u8 plane
// (interior origins)
struct PlainLKLevel {
    int w, h, pitch;
    const uint8_t* I;
    const int32_t* dI;
    const uint8_t* J;
    const uint8_t* Wt = nullptr;   // MASKED: the template image's weight plane (geometry of I), null: every sample on
};
struct PlainLKResult {
    float nx, ny;
    bool status;
    float err;   // ERR only; 0 where status is false
};

struct TemplatePixel {
    int ival, ix, iy;
};

// patch value (CV_DESCALE by W_BITS - 5) and Scharr pair (CV_DESCALE by W_BITS) of one template pixel at the window origin o
__device__ __forceinline__ TemplatePixel template_pixel(const uint8_t* __restrict__ I, const int32_t* __restrict__ dI, int pitch, ptrdiff_t o,
                                                        const Weights& w) {
    const uint8_t* s = I + o;
    const int32_t* d = dI + o;
    TemplatePixel t;
    t.ival = PC_DESCALE((int)s[0] * w.w00 + (int)s[1] * w.w01 + (int)s[pitch] * w.w10 + (int)s[pitch + 1] * w.w11, W_BITS - 5);
    const int d00 = d[0], d01 = d[1], d10 = d[pitch], d11 = d[pitch + 1];
    t.ix = PC_DESCALE((int)(int16_t)(d00 & 0xffff) * w.w00 + (int)(int16_t)(d01 & 0xffff) * w.w01 + (int)(int16_t)(d10 & 0xffff) * w.w10 +
                          (int)(int16_t)(d11 & 0xffff) * w.w11,
                      W_BITS);
    t.iy = PC_DESCALE((d00 >> 16) * w.w00 + (d01 >> 16) * w.w01 + (d10 >> 16) * w.w10 + (d11 >> 16) * w.w11, W_BITS);
    return t;
}
__device__ __forceinline__ uint2 pack_template(const TemplatePixel& t) {
    return make_uint2((uint32_t)t.ival, (uint32_t)(t.ix & 0xffff) | ((uint32_t)t.iy << 16));
}
// MASKED: a sample is on iff its four taps are on in the weight plane (255 / 0); the flag rides above ival (0 .. 8160) in the
// entry's first word, and an off sample carries a zero Scharr pair
constexpr uint32_t kTemplateOnBit = 1u << 16;
__device__ __forceinline__ bool template_sample_on(const uint8_t* __restrict__ Wt, int pitch, ptrdiff_t o) {
    const uint8_t* m = Wt + o;
    return (m[0] & m[1] & m[pitch] & m[pitch + 1]) != 0;
}
template <bool MASKED>
__device__ __forceinline__ uint32_t template_ival(uint32_t word) {
    if constexpr (MASKED) return word & 0xffffu;
    else return word;
}
__device__ __forceinline__ int interp_u8(int a, int b, int c, int d, const Weights& w) {
    return PC_DESCALE(a * w.w00 + b * w.w01 + c * w.w10 + d * w.w11, W_BITS - 5);
}
// interpolated J value minus the template's patch value
__device__ __forceinline__ int pixel_diff(const uint8_t* __restrict__ s, int pitch, const Weights& w, uint32_t ival) {
    return interp_u8(s[0], s[1], s[pitch], s[pitch + 1], w) - (int)ival;
}

// level_of(level) -> PlainLKLevel; lg: the lane's index in its group; tm: the group's LDS slice, win * win entries.
// Every lane of the group returns the same result.
//
// X86: the fp32 lane sums of LKTrackerInvoker's CV_SIMD128 path (PC_ARITH_LK_X86_ORDER, pco_lk under PCO_EMU_LK_SIMD): lane
// c < 4 of the group is vector lane c -- columns c, c + 4, ... below SIMD_W = (win / 8) * 8, row by row --, lane 4 the scalar
// accumulator over the remaining columns, lanes 5-7 idle.  Otherwise lane l owns columns l, l + 8, ... and the sums are exact integers.
// ERR: also the level-0 patch error; without it only that error's bounds test, which decides the status like any other.
// GUESS: the search of the top level starts at (guess_x, guess_y) * lscale instead of at the template's position -- OpenCV's
// OPTFLOW_USE_INITIAL_FLOW, the guided pass of the search prepass (kernels_lk_search.hip); nothing else changes, and without it
// the two arguments are not looked at.
// MASKED: the masked windows -- PlainLKLevel::Wt decides which template samples take part; the four places the rule changes are
// marked below, and an instance without the switch is the code it was.
template <bool X86, bool ERR, bool GUESS = false, bool MASKED = false, class LevelOf>
__device__ __forceinline__ PlainLKResult plain_lk_pair(const LevelOf& level_of, float start_x, float start_y, int win, int lg, int max_level,
                                                       int max_iters, double eps_sq, float min_eig_thr, uint2* const tm,
                                                       float guess_x = 0.f, float guess_y = 0.f) {
    const int simd_w = (win / 8) * 8;
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
            if constexpr (GUESS) {
                qx = guess_x * lscale;
                qy = guess_y * lscale;
            } else {
                qx = px;
                qy = py;
            }
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
        [[maybe_unused]] const uint8_t* __restrict__ Wt = nullptr;
        [[maybe_unused]] int n_on = win * win;
        [[maybe_unused]] int lane_on = 0;
        if constexpr (MASKED) Wt = L.Wt;
        // MASKED (1): ix and iy of an off sample are 0, ival is kept
        auto masked_template = [&](TemplatePixel& t, ptrdiff_t o) -> uint2 {
            uint2 e;
            if constexpr (MASKED) {
                const bool on = !Wt || template_sample_on(Wt, pitch, o);
                if (!on) t.ix = t.iy = 0;
                lane_on += on ? 1 : 0;
                e = pack_template(t);
                e.x |= on ? kTemplateOnBit : 0u;
            } else {
                e = pack_template(t);
            }
            return e;
        };
        float A11, A12, A22;
        if constexpr (X86) {
            float q11 = 0.f, q12 = 0.f, q22 = 0.f;
            const int xb = lg < 4 ? lg : simd_w, xe = lg < 4 ? simd_w : (lg == 4 ? win : 0), xs = lg < 4 ? 4 : 1;
            for (int y = 0; y < win; y++) {
                for (int x = xb; x < xe; x += xs) {
                    TemplatePixel t = template_pixel(I, dI, pitch, oI + (ptrdiff_t)y * pitch + x, wI);
                    tm[y * win + x] = masked_template(t, oI + (ptrdiff_t)y * pitch + x);
                    if (lg < 4) {
                        const float fx = (float)t.ix, fy = (float)t.iy;
                        q22 = fy * fy + q22;
                        q12 = fx * fy + q12;
                        q11 = fx * fx + q11;
                    } else {
                        q11 += (float)(t.ix * t.ix);
                        q12 += (float)(t.ix * t.iy);
                        q22 += (float)(t.iy * t.iy);
                    }
                }
            }
            auto combine = [](float q) {
                const float s = ((__shfl(q, 0, 8) + __shfl(q, 1, 8)) + __shfl(q, 2, 8)) + __shfl(q, 3, 8);
                return __shfl(q, 4, 8) + s;
            };
            A11 = combine(q11) * FLT_SCALE;
            A12 = combine(q12) * FLT_SCALE;
            A22 = combine(q22) * FLT_SCALE;
        } else {
            long long s11 = 0, s12 = 0, s22 = 0;
            for (int x = lg; x < win; x += 8) {
                for (int y = 0; y < win; y++) {
                    TemplatePixel t = template_pixel(I, dI, pitch, oI + (ptrdiff_t)y * pitch + x, wI);
                    tm[y * win + x] = masked_template(t, oI + (ptrdiff_t)y * pitch + x);
                    s11 += t.ix * t.ix;   // |ix|, |iy| <= 4080
                    s12 += t.ix * t.iy;
                    s22 += t.iy * t.iy;
                }
            }
            A11 = group8_exact_sum_i64(s11) * FLT_SCALE;
            A12 = group8_exact_sum_i64(s12) * FLT_SCALE;
            A22 = group8_exact_sum_i64(s22) * FLT_SCALE;
        }
        if constexpr (MASKED) {
            // MASKED (2): a window with fewer than a quarter of its samples on fails like the min-eig test
            n_on = group_allreduce_add<8>(lane_on);
            if (4 * n_on < win * win) {
                if (level == 0) status = false;
                continue;
            }
        }
        float D = A11 * A22 - A12 * A12;
        const float tdiff = A11 - A22;
        // MASKED (3): the divisor counts the on samples
        const float min_eig = (A22 + A11 - sqrtf(tdiff * tdiff + 4.f * A12 * A12)) / (float)(2 * (MASKED ? n_on : win * win));
        if (min_eig < min_eig_thr || D < 1.1920928955078125e-07f /* FLT_EPSILON */) {
            if (level == 0) status = false;
            continue;
        }
        D = 1.f / D;

        // ---- iterations on the searched plane ----
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
            float b1, b2;
            if constexpr (X86) {
                float q1 = 0.f, q2 = 0.f;
                for (int y = 0; y < win; y++) {
                    const uint8_t* const jr = jb + (ptrdiff_t)y * pitch;
                    const uint2* const tr = tm + y * win;
                    if (lg < 4) {
                        // the products of columns (c, c + 4) of a block of 8 are added as int32 before the conversion
                        for (int x0 = lg; x0 < simd_w; x0 += 8) {
                            const uint2 ta = tr[x0], tb = tr[x0 + 4];
                            const int da = pixel_diff(jr + x0, pitch, wJ, template_ival<MASKED>(ta.x)),
                                      db = pixel_diff(jr + x0 + 4, pitch, wJ, template_ival<MASKED>(tb.x));
                            const int p1 = da * (int)(int16_t)(ta.y & 0xffffu) + db * (int)(int16_t)(tb.y & 0xffffu);
                            const int p2 = da * ((int)ta.y >> 16) + db * ((int)tb.y >> 16);
                            q1 += (float)p1;
                            q2 += (float)p2;
                        }
                    } else if (lg == 4) {
                        for (int x = simd_w; x < win; x++) {
                            const uint2 t = tr[x];
                            const int d = pixel_diff(jr + x, pitch, wJ, template_ival<MASKED>(t.x));
                            q1 += (float)(d * (int)(int16_t)(t.y & 0xffffu));
                            q2 += (float)(d * ((int)t.y >> 16));
                        }
                    }
                }
                auto combine = [](float q) {
                    const float v = (__shfl(q, 0, 8) + __shfl(q, 2, 8)) + (__shfl(q, 1, 8) + __shfl(q, 3, 8));
                    return __shfl(q, 4, 8) + v;
                };
                b1 = combine(q1) * FLT_SCALE;
                b2 = combine(q2) * FLT_SCALE;
            } else {
                long long sb1 = 0, sb2 = 0;
                for (int x = lg; x < win; x += 8) {
                    const uint8_t* s = jb + x;
                    int t0 = s[0], t1 = s[1];   // the bottom taps of a row are the top taps of the next
                    for (int y = 0; y < win; y++) {
                        s += pitch;
                        const int u0 = s[0], u1 = s[1];
                        const uint2 t = tm[y * win + x];
                        const int diff = interp_u8(t0, t1, u0, u1, wJ) - (int)template_ival<MASKED>(t.x);   // |diff| <= 8160
                        sb1 += diff * (int)(int16_t)(t.y & 0xffffu);
                        sb2 += diff * ((int)t.y >> 16);
                        t0 = u0;
                        t1 = u1;
                    }
                }
                b1 = group8_exact_sum_i64(sb1) * FLT_SCALE;
                b2 = group8_exact_sum_i64(sb2) * FLT_SCALE;
            }
            if (lk_newton_step(A11, A12, A22, D, b1, b2, half_win, j, eps_sq, qx, qy, nx, ny, pdx, pdy)) break;
        }

        // ---- L1 patch error at level 0 ----
        if (status && level == 0) {
            const float ex = nx - half_win, ey = ny - half_win;
            const int iex = (int)floorf(ex), iey = (int)floorf(ey);
            if (lk_window_outside(iex, iey, win, L.w, L.h)) {
                status = false;
            } else if constexpr (ERR) {
                const Weights wE = bilinear_weights(ex - (float)iex, ey - (float)iey);
                const uint8_t* const eb = J + (ptrdiff_t)iey * pitch + iex;
                // the columns whose template values this lane wrote
                const int xb = !X86 || lg < 4 ? lg : simd_w, xe = !X86 ? win : (lg < 4 ? simd_w : (lg == 4 ? win : 0));
                const int xs = !X86 ? 8 : (lg < 4 ? 4 : 1);
                int se = 0;
                for (int y = 0; y < win; y++) {
                    for (int x = xb; x < xe; x += xs) {
                        const uint32_t tw = tm[y * win + x].x;
                        const int diff = pixel_diff(eb + (ptrdiff_t)y * pitch + x, pitch, wE, template_ival<MASKED>(tw));
                        // MASKED (4): the error is that of the on samples
                        if (!MASKED || (tw & kTemplateOnBit)) se += diff < 0 ? -diff : diff;
                    }
                }
                se = group_allreduce_add<8>(se);   // <= 31^2 * 8160 < 2^24: exact in fp32 too
                err = ((float)se * 1.f) / (float)(32 * (MASKED ? n_on : win * win));
            }
        }
    }
    PlainLKResult r;
    r.nx = nx;
    r.ny = ny;
    r.status = status;
    r.err = status ? err : 0.f;
    return r;
}

}  // namespace pc
