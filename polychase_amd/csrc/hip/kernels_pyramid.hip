// kernels_pyramid.hip -- one fused, LDS-tiled kernel per pyramid level (K1 + K6 + K7 of DESIGN.md section 4).
//
// Replaces, per level l of cv::buildOpticalFlowPyramid (reference cpp/opticalflow.cc:180-187) and the
// cv::cvtColor(COLOR_RGB2GRAY) in front of it (cpp/opticalflow.cc:259,:298):
//     level 0:  RGB / gray / float RGB(A) frame  -> gray tile                      (RGB2Gray, 15-bit coefficients; or the
//               context's gray conversion: channel weights, a transfer table for float channels; or a u8 RGBA, uint16 or
//               float16 RGB(A) frame, each channel made a byte by its rule of pixel_rules.hpp)
//     level l:  parent level's padded plane      -> pyrDown tile (5x5, (sum + 128) >> 8, REFLECT_101)
//   and then, from that tile in LDS (64 x 16 pixels + a 1-px halo), in the same kernel:
//     the u8 image plane, its REFLECT_101 padding of `win` pixels (copyMakeBorder), the uint16 (pixel << 7) plane
//     the LK kernel reads (with the same padding) and the Scharr derivative plane (ScharrDerivInvoker).
// Round 1 ran three kernels per level over global memory (pyrDown, border, Scharr; 18 single-byte loads per lane in
// the last one) plus a gray kernel; here every plane is written once with 4/8/16-byte stores and the level's pixels are
// read from HBM once.  Pure integer arithmetic: bit-exact against oracle/pc_oracle.c and against the unfused
// kernels of kernels_image.hip, which stay as the cross-check (POLYCHASE_PYRAMID_VARIANT=1).
#include "kernels.hpp"

namespace pc {

static thread_local int tl_helper_prio = 0;
int helper_prio_arg() { return tl_helper_prio; }
void set_helper_prio(int hi) { tl_helper_prio = hi ? 1 : 0; }

namespace {

constexpr int TW = 64, TH = 16;                   // output tile
constexpr int CW = TW + 2, CH = TH + 2;           // + 1-px halo for the Scharr stencil
constexpr int C_X0 = 3;                           // LDS column of the halo column x0 - 1 (interior starts 4-byte aligned)
constexpr int C_PITCH = 72;
constexpr int P_H = 2 * TH + 7;                   // parent rows a tile + halo needs (5x5 taps, stride 2)
constexpr int H_Q = (CW + 3) / 4;                 // horizontal pass: quads of outputs per row (17)
constexpr int H_PITCH = 4 * H_Q;                  // uint16 per row (68)

__device__ __forceinline__ uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b) {
    return (r * 9798u + g * 19235u + b * 3735u + (1u << 14)) >> 15;
}
// numpy `(x * 255).astype(uint8)` of the addon (blender_addon/operators/analysis.py:221-233); see kernels_image.hip
__device__ __forceinline__ uint32_t float_channel_to_u8(float v) {
    const float s = v * 255.0f;
    const int i = (s >= -2147483648.0f && s < 2147483648.0f) ? (int)s : (int)0x80000000;
    return (uint32_t)i & 0xffu;
}

// the gray conversions other than the default (pc_context_set_gray_conversion): channel weights from the launch's arguments
// and, for SRC_RGBF32_T, float channels through the transfer table -- a pure look-up in global memory (20 KiB that every
// workgroup of the launch shares: it stays in the L1 / L2; DESIGN.md section 4, "Grey conversion")
template <int SRC>
__device__ __forceinline__ uint32_t gray_src(const LevelSource& in, uint32_t r, uint32_t g, uint32_t b) {
    if constexpr (SRC == SRC_RGB8_W || SRC == SRC_RGBF32_W || SRC == SRC_RGBF32_T || SRC >= SRC_RGBA8_W)
        return (r * in.wr + g * in.wg + b * in.wb + (1u << 14)) >> 15;
    else return gray_of(r, g, b);
}
// the sources of 16-bit channels (pixel_rules.hpp): uint16, and float16 widened to the float32 it equals
template <int SRC>
constexpr bool kSrc16 = SRC == SRC_RGB16_W || SRC == SRC_RGBF16_W || SRC == SRC_RGBF16_T;
template <int SRC>
__device__ __forceinline__ uint32_t channel16(const LevelSource& in, uint32_t v) {
    if constexpr (SRC == SRC_RGB16_W) return u16_to_u8(v);
    else if constexpr (SRC == SRC_RGBF16_T) return in.table[transfer_index(f16_bits_to_f32_bits(v))];
    else return f32_bits_to_u8(f16_bits_to_f32_bits(v));
}
// four pixels of C 16-bit channels each from the 2 C aligned dwords that hold them (x a multiple of 4)
template <int SRC, int C>
__device__ __forceinline__ void quad16(const LevelSource& in, const uint8_t* row, int x, uint32_t px[4]) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(row) + 2 * C * (x >> 2);
    uint32_t d[2 * C];
#pragma unroll
    for (int k = 0; k < 2 * C; k++) d[k] = s[k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t c[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int i = k * C + j;
            c[j] = channel16<SRC>(in, (i & 1) ? d[i >> 1] >> 16 : d[i >> 1] & 0xffffu);
        }
        px[k] = gray_src<SRC>(in, c[0], c[1], c[2]);
    }
}
template <int SRC>
__device__ __forceinline__ uint32_t float_channel(const LevelSource& in, const float* s) {
    if constexpr (SRC == SRC_RGBF32_T) return in.table[transfer_index(*reinterpret_cast<const uint32_t*>(s))];
    else return float_channel_to_u8(*s);
}

template <int SRC>
__device__ __forceinline__ uint32_t source_gray(const LevelSource& in, int x, int y) {
    const uint8_t* row = in.src + (size_t)y * in.src_pitch;
    if (SRC == SRC_RGB8 || SRC == SRC_RGB8_W) {
        const uint8_t* s = row + 3 * (size_t)x;
        return gray_src<SRC>(in, s[0], s[1], s[2]);
    } else if (SRC == SRC_GRAY8) {
        return row[x];
    } else if (SRC == SRC_RGBA8_W) {
        const uint8_t* s = row + 4 * (size_t)x;
        return gray_src<SRC>(in, s[0], s[1], s[2]);
    } else if (kSrc16<SRC>) {
        // 16-bit loads: such a frame is 2-byte aligned, whatever else
        const uint16_t* s = reinterpret_cast<const uint16_t*>(row) + (size_t)x * in.channels;
        return gray_src<SRC>(in, channel16<SRC>(in, s[0]), channel16<SRC>(in, s[1]), channel16<SRC>(in, s[2]));
    } else {
        const float* s = reinterpret_cast<const float*>(row) + (size_t)x * in.channels;
        return gray_src<SRC>(in, float_channel<SRC>(in, s), float_channel<SRC>(in, s + 1), float_channel<SRC>(in, s + 2));
    }
}

// where pixel coordinate v of a `len`-long axis is mirrored to by a REFLECT_101 border of `win` pixels:
// m[0] = itself, m[1] = the pad position below 0 (or INT_MIN), m[2] = the pad position above len - 1 (or INT_MIN)
constexpr int kNone = -(1 << 30);
__device__ __forceinline__ void mirrors(int v, int len, int win, int m[3]) {
    m[0] = v;
    m[1] = (v >= 1 && v <= win) ? -v : kNone;
    m[2] = (v <= len - 2 && v >= len - 1 - win) ? 2 * (len - 1) - v : kNone;
}

}  // namespace

template <int SRC>
__global__ __launch_bounds__(256) void level_kernel(const LevelSource in, const Level out, const int win, int hi_prio) {
    helper_priority(hi_prio);
    __shared__ __attribute__((aligned(16))) uint8_t s_c[CH][C_PITCH];           // the level's tile + halo
    __shared__ __attribute__((aligned(16))) uint16_t s_h[SRC == SRC_PYR ? P_H : 1][H_PITCH];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int w = out.w, h = out.h;
    if (in.clear) {
        const int stride = (int)(gridDim.x * gridDim.y) * 256;
        for (int i = (int)(blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid; i < in.clear_words; i += stride) in.clear[i] = 0u;
    }

    // ---- phase A: every in-image pixel of [x0 - 1, x0 + TW] x [y0 - 1, y0 + TH] into s_c ----
    if constexpr (SRC == SRC_PYR) {
        const Level& P = in.parent;
        const int px0 = 2 * x0 - 4, py0 = 2 * y0 - 4;     // parent position of the first byte the tile reads; px0 is 4-byte aligned
        const int ymin = -win, ymax = P.h + win - 1, xmax = P.pitch - kPadX - 4;
        // horizontal [1 4 6 4 1] at stride 2, straight from the parent plane: output c (level column x0 - 1 + c) reads parent bytes
        // 2c .. 2c + 4 of the row, a quad of outputs the three aligned dwords at bytes 8q .. 8q + 11.  (Staging the parent rows in
        // LDS first -- 39 rows of 36 dwords -- cost a pass of address arithmetic and a barrier to save half a dword load per
        // output: the quads' dwords overlap by one in three, and the L1 serves that.)
        for (int i = tid; i < P_H * H_Q; i += 256) {
            const int r = i / H_Q, q = i - r * H_Q;
            // clamped positions are never consumed by an in-image output (they lie beyond the parent's 2-px reach)
            const int yy = min(max(py0 + r, ymin), ymax);
            const uint8_t* prow = P.img + (ptrdiff_t)yy * P.pitch;
            const uint32_t a = *reinterpret_cast<const uint32_t*>(prow + min(px0 + 8 * q, xmax));
            const uint32_t b = *reinterpret_cast<const uint32_t*>(prow + min(px0 + 8 * q + 4, xmax));
            const uint32_t c = *reinterpret_cast<const uint32_t*>(prow + min(px0 + 8 * q + 8, xmax));
            int v[11];
            v[0] = a & 0xff; v[1] = (a >> 8) & 0xff; v[2] = (a >> 16) & 0xff; v[3] = a >> 24;
            v[4] = b & 0xff; v[5] = (b >> 8) & 0xff; v[6] = (b >> 16) & 0xff; v[7] = b >> 24;
            v[8] = c & 0xff; v[9] = (c >> 8) & 0xff; v[10] = (c >> 16) & 0xff;
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = (uint32_t)(v[2 * k + 2] * 6 + (v[2 * k + 1] + v[2 * k + 3]) * 4 + v[2 * k] + v[2 * k + 4]);
            *reinterpret_cast<uint2*>(&s_h[r][4 * q]) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
        }
        __syncthreads();
        // vertical [1 4 6 4 1] at stride 2, two columns per lane
        for (int i = tid; i < CH * (H_PITCH / 2); i += 256) {
            const int cy = i / (H_PITCH / 2), cp = i - cy * (H_PITCH / 2);
            const int c = 2 * cp;
            if (c >= CW) continue;
            uint32_t t[5];
#pragma unroll
            for (int k = 0; k < 5; k++) t[k] = *reinterpret_cast<const uint32_t*>(&s_h[2 * cy + k][c]);
            const uint32_t lo = ((t[0] & 0xffff) + (t[4] & 0xffff) + ((t[1] & 0xffff) + (t[3] & 0xffff)) * 4 + (t[2] & 0xffff) * 6 + 128) >> 8;
            const uint32_t hi = ((t[0] >> 16) + (t[4] >> 16) + ((t[1] >> 16) + (t[3] >> 16)) * 4 + (t[2] >> 16) * 6 + 128) >> 8;
            s_c[cy][C_X0 + c] = (uint8_t)lo;
            if (c + 1 < CW) s_c[cy][C_X0 + c + 1] = (uint8_t)hi;
        }
    } else {
        // interior of the tile: 4 pixels per lane
        const int r = tid >> 4, g = tid & 15;
        const int x = x0 + 4 * g, y = y0 + r;
        if (y < h && x < w) {
            uint32_t px[4] = {0, 0, 0, 0};
            if (in.aligned && x + 3 < w) {
                const uint8_t* row = in.src + (size_t)y * in.src_pitch;
                if (SRC == SRC_RGB8 || SRC == SRC_RGB8_W) {
                    const uint32_t* s = reinterpret_cast<const uint32_t*>(row) + 3 * (x >> 2);
                    const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
                    px[0] = gray_src<SRC>(in, d0 & 0xff, (d0 >> 8) & 0xff, (d0 >> 16) & 0xff);
                    px[1] = gray_src<SRC>(in, d0 >> 24, d1 & 0xff, (d1 >> 8) & 0xff);
                    px[2] = gray_src<SRC>(in, (d1 >> 16) & 0xff, d1 >> 24, d2 & 0xff);
                    px[3] = gray_src<SRC>(in, (d2 >> 8) & 0xff, (d2 >> 16) & 0xff, d2 >> 24);
                } else if (SRC == SRC_GRAY8) {
                    const uint32_t d = *reinterpret_cast<const uint32_t*>(row + x);
                    px[0] = d & 0xff; px[1] = (d >> 8) & 0xff; px[2] = (d >> 16) & 0xff; px[3] = d >> 24;
                } else if (SRC == SRC_RGBA8_W) {
                    const uint32_t* s = reinterpret_cast<const uint32_t*>(row) + x;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t d = s[k];
                        px[k] = gray_src<SRC>(in, d & 0xff, (d >> 8) & 0xff, (d >> 16) & 0xff);
                    }
                } else if (kSrc16<SRC>) {
                    if (in.channels == 4) quad16<SRC, 4>(in, row, x, px);
                    else quad16<SRC, 3>(in, row, x, px);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) px[k] = source_gray<SRC>(in, x + k, y);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (x + k < w) px[k] = source_gray<SRC>(in, x + k, y);
            }
            *reinterpret_cast<uint32_t*>(&s_c[r + 1][C_X0 + 1 + 4 * g]) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        }
        // halo ring: neighbours that belong to the adjacent tiles (in-image positions only)
        if (tid < 2 * CW + 2 * TH) {
            int cx, cy;
            if (tid < 2 * CW) {
                cy = tid < CW ? 0 : CH - 1;
                cx = tid < CW ? tid : tid - CW;
            } else {
                const int k = tid - 2 * CW;
                cy = 1 + (k >> 1);
                cx = (k & 1) ? CW - 1 : 0;
            }
            const int ax = x0 - 1 + cx, ay = y0 - 1 + cy;
            if (ax >= 0 && ax < w && ay >= 0 && ay < h) s_c[cy][C_X0 + cx] = (uint8_t)source_gray<SRC>(in, ax, ay);
        }
    }
    __syncthreads();
    // positions one pixel outside the image take the REFLECT_101 value (the Scharr stencil's border, and the first
    // ring of the padding); only tiles that touch the image edge have any
    const bool edge_tile = x0 == 0 || y0 == 0 || x0 + TW >= w || y0 + TH >= h;
    if (edge_tile) {
        for (int i = tid; i < CW * CH; i += 256) {
            const int cy = i / CW, cx = i - cy * CW;
            const int ax = x0 - 1 + cx, ay = y0 - 1 + cy;
            if ((ax < 0 || ax >= w || ay < 0 || ay >= h) && ax >= -1 && ax <= w && ay >= -1 && ay <= h) {
                // the source is an in-image position of this tile's block: written in phase A, not by this pass
                const int sx = reflect101(ax, w) - (x0 - 1), sy = reflect101(ay, h) - (y0 - 1);
                if (sx >= 0 && sx < CW && sy >= 0 && sy < CH) s_c[cy][C_X0 + cx] = s_c[sy][C_X0 + sx];
            }
        }
        __syncthreads();
    }

    // ---- phase B: the level's planes, 4 pixels per lane ----
    const int r = tid >> 4, g = tid & 15;
    const int x = x0 + 4 * g, y = y0 + r;
    if (y >= h || x >= w) return;
    // bytes x - 1 .. x + 4 of the three rows: the dwords at columns 4g, 4g + 4, 4g + 8 (aligned)
    uint32_t rows[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(&s_c[r + k][4 * g]);
        rows[k][0] = p[0];
        rows[k][1] = p[1];
        rows[k][2] = p[2];
    }
    const uint32_t centre = rows[1][1];                  // pixels x .. x + 3
    // Scharr on pairs of columns in packed 16-bit lanes: every intermediate fits 16 bits ((a + b) * 3 + c * 10 <= 4080, the
    // differences +-4080) and only the low 16 bits of dx and dy are stored, so wrapping 16-bit arithmetic gives the same bits as
    // the 32-bit form at half the instructions.  pr[k][j]: columns x - 1 + 2j, x + 2j of row k (bytes 3 + 2j, 4 + 2j of the 12).
    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
    u16x2 pr[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        pr[k][0] = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(rows[k][1], rows[k][0], 0x0c040c03u));
        pr[k][1] = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(0u, rows[k][1], 0x0c020c01u));
        pr[k][2] = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(rows[k][2], rows[k][1], 0x0c040c03u));
    }
    const u16x2 k3 = {3, 3}, k10 = {10, 10};
    u16x2 t0[3], t1[3];                                  // columns x - 1 + 2j, x + 2j: (a + b) * 3 + c * 10 and b - a
#pragma unroll
    for (int j = 0; j < 3; j++) {
        t0[j] = (pr[0][j] + pr[2][j]) * k3 + pr[1][j] * k10;
        t1[j] = pr[2][j] - pr[0][j];
    }
    int32_t d[4];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        // pixels x + 2j, x + 2j + 1: dx = t0[i + 2] - t0[i], dy = (t1[i + 2] + t1[i]) * 3 + t1[i + 1] * 10
        const u16x2 dx = t0[j + 1] - t0[j];
        const u16x2 mid = __builtin_bit_cast(u16x2, __builtin_amdgcn_alignbit(__builtin_bit_cast(uint32_t, t1[j + 1]), __builtin_bit_cast(uint32_t, t1[j]), 16u));
        const u16x2 dy = (t1[j + 1] + t1[j]) * k3 + mid * k10;
        const uint32_t dxu = __builtin_bit_cast(uint32_t, dx), dyu = __builtin_bit_cast(uint32_t, dy);
        d[2 * j] = (int32_t)__builtin_amdgcn_perm(dyu, dxu, 0x05040100u);       // dx | dy << 16 of the even pixel
        d[2 * j + 1] = (int32_t)__builtin_amdgcn_perm(dyu, dxu, 0x07060302u);   // ... of the odd one
    }
    const uint32_t w16lo = __builtin_amdgcn_perm(0u, centre, 0x0c010c00u) << 7;   // (p0, p1) << 7 as 16-bit lanes
    const uint32_t w16hi = __builtin_amdgcn_perm(0u, centre, 0x0c030c02u) << 7;
    uint8_t* img = out.img + (ptrdiff_t)y * out.pitch + x;
    uint16_t* img16 = out.img16 + (ptrdiff_t)y * out.pitch + x;
    int32_t* der = out.der + (ptrdiff_t)y * out.pitch + x;
    if (x + 3 < w) {
        *reinterpret_cast<uint32_t*>(img) = centre;
        *reinterpret_cast<uint2*>(img16) = make_uint2(w16lo, w16hi);
        *reinterpret_cast<int4*>(der) = make_int4(d[0], d[1], d[2], d[3]);
    } else {
        for (int i = 0; i < 4 && x + i < w; i++) {
            const uint32_t v = (centre >> (8 * i)) & 0xff;
            img[i] = (uint8_t)v;
            img16[i] = (uint16_t)(v << 7);
            der[i] = d[i];
        }
    }
    // REFLECT_101 padding (copyMakeBorder in buildOpticalFlowPyramid): every pixel writes its own mirror images, so
    // no tile depends on a neighbour's data however the tiles fall on the image edge
    if (x <= win || x + 3 >= w - 1 - win || y <= win || y >= h - 1 - win) {
        int my[3];
        mirrors(y, h, win, my);
        for (int i = 0; i < 4 && x + i < w; i++) {
            const uint32_t v = (centre >> (8 * i)) & 0xff;
            int mx[3];
            mirrors(x + i, w, win, mx);
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    if ((a | b) == 0 || my[a] == kNone || mx[b] == kNone) continue;
                    const ptrdiff_t o = (ptrdiff_t)my[a] * out.pitch + mx[b];
                    out.img[o] = (uint8_t)v;
                    out.img16[o] = (uint16_t)(v << 7);
                }
        }
    }
}

void launch_level(const LevelSource& in, const Level& out, int win, hipStream_t s) {
    dim3 grid((out.w + TW - 1) / TW, (out.h + TH - 1) / TH);
    switch (in.kind) {
        case SRC_PYR: hipLaunchKernelGGL(level_kernel<SRC_PYR>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGB8: hipLaunchKernelGGL(level_kernel<SRC_RGB8>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_GRAY8: hipLaunchKernelGGL(level_kernel<SRC_GRAY8>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGB8_W: hipLaunchKernelGGL(level_kernel<SRC_RGB8_W>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGBF32_W: hipLaunchKernelGGL(level_kernel<SRC_RGBF32_W>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGBF32_T: hipLaunchKernelGGL(level_kernel<SRC_RGBF32_T>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGBA8_W: hipLaunchKernelGGL(level_kernel<SRC_RGBA8_W>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGB16_W: hipLaunchKernelGGL(level_kernel<SRC_RGB16_W>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGBF16_W: hipLaunchKernelGGL(level_kernel<SRC_RGBF16_W>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        case SRC_RGBF16_T: hipLaunchKernelGGL(level_kernel<SRC_RGBF16_T>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
        default: hipLaunchKernelGGL(level_kernel<SRC_RGBF32>, grid, dim3(256), 0, s, in, out, win, helper_prio_arg()); break;
    }
}

}  // namespace pc
