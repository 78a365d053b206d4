// kernels_lens.hip -- lens undistortion at ingest: the gray plane of a frame resampled through the context's lens map
// (include/polychase_hip.h: pc_context_set_lens_map has the rule; not in the reference, whose frames are taken as pinhole).
//
// A gather: the map is the stream (8 B per output pixel, read once as two 16-byte loads per lane), the taps are single bytes
// of the gray plane.  Neighbouring lanes read neighbouring source pixels -- a lens map is smooth --, so the 16 byte loads of a lane
// hit cache lines its neighbours have brought into the L1; nothing is staged in LDS, nothing is shared between lanes, no atomics.
// One lane makes four adjacent output pixels and stores them as one dword.  Pure integer arithmetic: bit-exact against the
// restatement in tests/lens_ref.py.
#include "kernels.hpp"

namespace pc {

namespace {

// one output pixel: bilinear blend of the four clamped taps with 8-bit weights, rounded once; an invalid entry gives 0
__device__ __forceinline__ uint32_t lens_tap(const uint8_t* __restrict__ src, int spitch, int w, int h, int qx, int qy) {
    const int ix = qx >> kLensFracBits, iy = qy >> kLensFracBits;
    const uint32_t wx = (uint32_t)qx & 255u, wy = (uint32_t)qy & 255u;
    const int x0 = min(max(ix, 0), w - 1), x1 = min(max(ix + 1, 0), w - 1);
    const int y0 = min(max(iy, 0), h - 1), y1 = min(max(iy + 1, 0), h - 1);
    const uint8_t* r0 = src + (size_t)y0 * spitch;
    const uint8_t* r1 = src + (size_t)y1 * spitch;
    const uint32_t a = r0[x0], b = r0[x1], c = r1[x0], d = r1[x1];
    const uint32_t top = a * (256u - wx) + b * wx, bot = c * (256u - wx) + d * wx;
    const uint32_t v = (top * (256u - wy) + bot * wy + 32768u) >> 16;
    return (qx == kLensInvalid || qy == kLensInvalid) ? 0u : v;
}

}  // namespace

// map: h rows of map_pitch entries (a multiple of 4, so a lane's eight words are two aligned int4s and the last lane of a row
// stays inside it); dst rows are 4-byte aligned
__global__ __launch_bounds__(256) void lens_remap_kernel(const uint8_t* __restrict__ src, int spitch, int w, int h,
                                                         const int32_t* __restrict__ map, int map_pitch, uint8_t* __restrict__ dst,
                                                         int dpitch, int hi_prio) {
    helper_priority(hi_prio);
    const int gx = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int x = 4 * gx;
    if (x >= w) return;
    const int4* m = reinterpret_cast<const int4*>(map + ((size_t)y * map_pitch + x) * 2);
    const int4 e0 = m[0], e1 = m[1];
    uint32_t px[4];
    px[0] = lens_tap(src, spitch, w, h, e0.x, e0.y);
    px[1] = lens_tap(src, spitch, w, h, e0.z, e0.w);
    px[2] = lens_tap(src, spitch, w, h, e1.x, e1.y);
    px[3] = lens_tap(src, spitch, w, h, e1.z, e1.w);
    uint8_t* d = dst + (size_t)y * dpitch + x;
    if (x + 3 < w) {
        *reinterpret_cast<uint32_t*>(d) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    } else {
        for (int i = 0; i < 4 && x + i < w; i++) d[i] = (uint8_t)px[i];
    }
}

void launch_lens_remap(const uint8_t* src, int src_pitch, int w, int h, const int32_t* map, int map_pitch, uint8_t* dst, int dst_pitch,
                       hipStream_t s) {
    const int groups = (w + 3) / 4;
    dim3 grid((groups + 255) / 256, h);
    hipLaunchKernelGGL(lens_remap_kernel, grid, dim3(256), 0, s, src, src_pitch, w, h, map, map_pitch, dst, dst_pitch, helper_prio_arg());
}

}  // namespace pc
