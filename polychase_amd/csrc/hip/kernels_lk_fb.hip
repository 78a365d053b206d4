// kernels_lk_fb.hip -- forward-backward consistency check of the LK flow (Kalal et al., 2010) on gfx950.
//
// After the forward launch (kernels_lk*.hip) has left its raw records out_rec[slot * 8 + target] = (q, err, status_f), ONE
// launch tracks every surviving q back from its target into frame1 -- calcOpticalFlowPyrLK(prev = target, next = frame1,
// pts = {q}), bit for bit oracle/pc_oracle.c's pco_lk in the context's arithmetic mode -- and clears the status of a row whose
// backward pass fails or lands further than the threshold from the keypoint it started at.  Everything downstream of the
// records (compaction, unpacking) is unchanged.
//
// Mapping: one wavefront per keypoint (visiting order of the forward launch), one group of 8 lanes per target, DPP sums
// inside the group -- the forward generic kernel's layout.  What differs from the forward kernels:
//   * the template (I side) of every pair comes from a DIFFERENT image, the target's, at a sub-pixel position: each group
//     evaluates its own WIN x WIN template (patch value + Scharr pair per pixel) per level and keeps it in its own slice of
//     LDS, 8 bytes per pixel; nothing is shared across the wavefront, so the kernel has no barrier and no fence: a lane reads
//     back only what it wrote itself (a lane owns whole window COLUMNS in both phases);
//   * the window is a RUNTIME value (3 .. PC_MAX_WINDOW): one instance per arithmetic order instead of one per window, LDS sized
//     at launch (8 groups x WIN^2 x 8 bytes per wavefront; 1..4 wavefronts per workgroup, as many as fit below 64 KiB);
//   * the searched image (frame1) is gathered straight from the padded u8 plane: a window that passed OpenCV's bounds test
//     lies inside the padding (win rows, >= win columns), and no window is read before it passed that test.
// Pairs with status_f == 0 do no work; a wavefront without a surviving pair only writes its zeros to the side arrays.
#include <algorithm>

#include "../../../include/polychase_hip.h"
#include "lk_common.hpp"

namespace pc {

namespace {

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
__device__ __forceinline__ int interp_u8(int a, int b, int c, int d, const Weights& w) {
    return PC_DESCALE(a * w.w00 + b * w.w01 + c * w.w10 + d * w.w11, W_BITS - 5);
}
// interpolated J value minus the template's patch value
__device__ __forceinline__ int pixel_diff(const uint8_t* __restrict__ s, int pitch, const Weights& w, uint32_t ival) {
    return interp_u8(s[0], s[1], s[pitch], s[pitch + 1], w) - (int)ival;
}

// Sum over the group of per-lane 64-bit partials (|total| < 2^40) as ONE rounding of the exact integer: three 16-bit-wide
// DPP sums, the total rebuilt in 64 bits, then hi * 2^16 + lo with both terms exact in fp32.
__device__ __forceinline__ float group8_exact_sum_i64(long long v) {
    const int c0 = group_allreduce_add<8>((int)(v & 0xffff));
    const int c1 = group_allreduce_add<8>((int)((v >> 16) & 0xffff));
    const int c2 = group_allreduce_add<8>((int)(v >> 32));
    const long long t = (long long)c2 * 4294967296ll + (long long)c1 * 65536ll + (long long)c0;
    return exact_sum_to_float((int)(t >> 16), (int)(t & 0xffff));
}

}  // namespace

// X86: the fp32 lane sums of LKTrackerInvoker's CV_SIMD128 path (lk_kernel<WIN, true> in kernels_lk.hip): lane c < 4 of a
// group is vector lane c -- columns c, c + 4, ... below SIMD_W = (win / 8) * 8, row by row --, lane 4 the scalar accumulator
// over the remaining columns, lanes 5-7 idle.  Otherwise lane l owns columns l, l + 8, ... and the sums are exact integers.
template <bool X86>
__global__ __launch_bounds__(256) void lk_fb_kernel(const LKFBParams p) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    const int win = p.win, npx = win * win;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 3, lg = lane & 7;
    const int slot = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (slot >= p.n) return;   // whole wavefronts
    const bool tgt_active = grp < p.n_targets;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tgt_active) rec = p.rec[(size_t)slot * kRecStride + grp];
    const bool fwd_ok = tgt_active && __float_as_uint(rec.w) == 1u;   // uniform in the group
    const int feat = p.perm ? (int)p.perm[slot] : slot;

    float nx = 0.f, ny = 0.f;
    bool status = false;
    if (fwd_ok) {
        uint2* const tm = s_tmpl + (size_t)(wave * 8 + grp) * npx;
        const int simd_w = (win / 8) * 8;
        const float half_win = (float)(win - 1) * 0.5f;
        const float FLT_SCALE = 1.f / (float)(1 << 20);
        status = true;
        for (int level = p.max_level; level >= 0; --level) {
            const Level L = p.f1[level];
            const uint8_t* __restrict__ I = p.timg[grp][level];
            const int32_t* __restrict__ dI = p.tder[grp][level];
            const uint8_t* __restrict__ J = L.img;
            const int pitch = L.pitch;
            const float lscale = 1.f / (float)(1 << level);
            float px = rec.x * lscale, py = rec.y * lscale;
            float qx, qy;
            if (level == p.max_level) {
                qx = px;
                qy = py;
            } else {
                qx = nx * 2.f;
                qy = ny * 2.f;
            }
            nx = qx;
            ny = qy;

            // ---- template on the target's planes ----
            px -= half_win;
            py -= half_win;
            const int ipx = (int)floorf(px), ipy = (int)floorf(py);
            if (ipx < -win || ipx >= L.w || ipy < -win || ipy >= L.h) {
                if (level == 0) status = false;
                continue;
            }
            const Weights wI = bilinear_weights(px - (float)ipx, py - (float)ipy);
            const ptrdiff_t oI = (ptrdiff_t)ipy * pitch + ipx;
            float A11, A12, A22;
            if constexpr (X86) {
                float q11 = 0.f, q12 = 0.f, q22 = 0.f;
                const int xb = lg < 4 ? lg : simd_w, xe = lg < 4 ? simd_w : (lg == 4 ? win : 0), xs = lg < 4 ? 4 : 1;
                for (int y = 0; y < win; y++) {
                    for (int x = xb; x < xe; x += xs) {
                        const TemplatePixel t = template_pixel(I, dI, pitch, oI + (ptrdiff_t)y * pitch + x, wI);
                        tm[y * win + x] = pack_template(t);
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
                        const TemplatePixel t = template_pixel(I, dI, pitch, oI + (ptrdiff_t)y * pitch + x, wI);
                        tm[y * win + x] = pack_template(t);
                        s11 += t.ix * t.ix;   // |ix|, |iy| <= 4080
                        s12 += t.ix * t.iy;
                        s22 += t.iy * t.iy;
                    }
                }
                A11 = group8_exact_sum_i64(s11) * FLT_SCALE;
                A12 = group8_exact_sum_i64(s12) * FLT_SCALE;
                A22 = group8_exact_sum_i64(s22) * FLT_SCALE;
            }
            float D = A11 * A22 - A12 * A12;
            const float tdiff = A11 - A22;
            const float min_eig = (A22 + A11 - sqrtf(tdiff * tdiff + 4.f * A12 * A12)) / (float)(2 * win * win);
            if (min_eig < p.min_eig_thr || D < 1.1920928955078125e-07f /* FLT_EPSILON */) {
                if (level == 0) status = false;
                continue;
            }
            D = 1.f / D;

            // ---- iterations on frame1's plane ----
            qx -= half_win;
            qy -= half_win;
            float pdx = 0.f, pdy = 0.f;
            for (int j = 0; j < p.max_iters; j++) {
                const int iqx = (int)floorf(qx), iqy = (int)floorf(qy);
                if (iqx < -win || iqx >= L.w || iqy < -win || iqy >= L.h) {
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
                                const int da = pixel_diff(jr + x0, pitch, wJ, ta.x), db = pixel_diff(jr + x0 + 4, pitch, wJ, tb.x);
                                const int p1 = da * (int)(int16_t)(ta.y & 0xffffu) + db * (int)(int16_t)(tb.y & 0xffffu);
                                const int p2 = da * ((int)ta.y >> 16) + db * ((int)tb.y >> 16);
                                q1 += (float)p1;
                                q2 += (float)p2;
                            }
                        } else if (lg == 4) {
                            for (int x = simd_w; x < win; x++) {
                                const uint2 t = tr[x];
                                const int d = pixel_diff(jr + x, pitch, wJ, t.x);
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
                            const int diff = interp_u8(t0, t1, u0, u1, wJ) - (int)t.x;   // |diff| <= 8160
                            sb1 += diff * (int)(int16_t)(t.y & 0xffffu);
                            sb2 += diff * ((int)t.y >> 16);
                            t0 = u0;
                            t1 = u1;
                        }
                    }
                    b1 = group8_exact_sum_i64(sb1) * FLT_SCALE;
                    b2 = group8_exact_sum_i64(sb2) * FLT_SCALE;
                }
                const float dx = (A12 * b2 - A22 * b1) * D;
                const float dy = (A12 * b1 - A11 * b2) * D;
                qx += dx;
                qy += dy;
                nx = qx + half_win;
                ny = qy + half_win;
                if ((double)dx * (double)dx + (double)dy * (double)dy <= p.eps_sq) break;
                if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
                    nx -= dx * 0.5f;
                    ny -= dy * 0.5f;
                    break;
                }
                pdx = dx;
                pdy = dy;
            }

            // the patch error itself is not an output of the check; its bounds test decides the status like any other
            if (status && level == 0) {
                const int iex = (int)floorf(nx - half_win), iey = (int)floorf(ny - half_win);
                if (iex < -win || iex >= L.w || iey < -win || iey >= L.h) status = false;
            }
        }
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

bool launch_lk_fb(const LKFBParams& p, hipStream_t s) {
    if (p.win < 3 || p.win > PC_MAX_WINDOW || p.n_targets < 1 || p.n_targets > kRecStride) return false;
    if (p.n <= 0) return true;
    const size_t wave_bytes = (size_t)kRecStride * p.win * p.win * sizeof(uint2);   // <= 61504
    static_assert((size_t)kRecStride * PC_MAX_WINDOW * PC_MAX_WINDOW * sizeof(uint2) < 65536, "one wavefront's templates must fit below 64 KiB");
    const int waves = (int)std::min<size_t>(4, 65535 / wave_bytes);   // window 16: 3 wavefronts (49152 bytes), not 4 (exactly 64 KiB)
    const unsigned blocks = (unsigned)((p.n + waves - 1) / waves);
    if (p.x86_order) hipLaunchKernelGGL((lk_fb_kernel<true>), dim3(blocks), dim3(64 * waves), waves * wave_bytes, s, p);
    else hipLaunchKernelGGL((lk_fb_kernel<false>), dim3(blocks), dim3(64 * waves), waves * wave_bytes, s, p);
    return true;
}

}  // namespace pc
