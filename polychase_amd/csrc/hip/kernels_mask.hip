// kernels_mask.hip -- the detection mask's plane (kernels_gftt.hip: the MASKED variants read it) rasterised on gfx950 from
// polygon outlines (include/polychase_hip.h: pc_frame_set_mask_polygons states the fill rule; DESIGN.md section 4 "Polygon
// masks").
//
// The rule is integer.  Vertices arrive snapped to sixteenths of a pixel (|X|, |Y| <= 2^19); pixel (px, py) is the point
// P = (16 px, 16 py).  An edge A -> B is crossed at P when (Ay <= Py) != (By <= Py), and lies to the right of P when
// d = (Bx - Ax)(Py - Ay) - (Px - Ax)(By - Ay) has the sign of By - Ay (64-bit: the terms reach 2^41).  A pixel is inside a
// polygon that has an odd number of crossed edges to its right (even-odd), on when it is inside any polygon, flipped by
// `invert`; on = 255, off = 0.
//
// Mapping.  A 256-lane workgroup owns a tile of kPolyTileW x kPolyTileH pixels; a lane owns a quad of 4 adjacent pixels in
// each of the tile's rows: 16 pixels, whose state is one bit each of two registers (parity in the polygon at hand, union of
// the polygons done).  The workgroup walks the vertex list 256 edges at a time and keeps, in input order (ballot + prefix,
// no atomics), the edges that can be crossed to the right of a pixel of the tile: those whose y-span meets the tile's rows
// and that are not wholly left of it.  Kept edges wait in LDS with their polygon's index; when kPolyEdgeCap of them could be
// exceeded the lanes consume what is there and the list starts again, so any outline fits.  Edges stay ordered by polygon:
// when the index changes, the finished polygon's parity is folded into the union.  Every edge read in the consuming loop
// is wave-uniform, so "crossed" is a scalar branch; along a row d is linear in Px: one product per row, then adds.
// Every loop is bounded by the vertex count, no workgroup waits for another, and each byte of the plane is written once.
#include "kernels.hpp"

namespace pc {

constexpr int kPolyTileW = 1024, kPolyTileH = 4;   // 256 lanes x 4 pixels, 4 rows
constexpr int kPolyEdgeCap = 512;                  // 8 KB of edges + 512 B of polygon indices in LDS
static_assert(kPolyTileH * 4 <= 32, "a lane's pixels are the bits of one register");
static_assert(kPolyEdgeCap >= 256 && kPolyEdgeCap % 256 == 0, "a batch of 256 edges must fit an empty list");

__global__ __launch_bounds__(256) void polygon_mask_kernel(const int32_t* __restrict__ starts, const int2* __restrict__ verts, int nv, int np,
                                                           int invert, uint8_t* __restrict__ mask, int w, int h, int hi_prio) {
    helper_priority(hi_prio);
    __shared__ int4 s_edge[kPolyEdgeCap];       // Ax, Ay, Bx, By
    __shared__ uint8_t s_poly[kPolyEdgeCap];
    __shared__ int s_start[kPolyMaxPolygons + 1];
    __shared__ int s_wave[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kPolyTileW + tid * 4, y0 = blockIdx.y * kPolyTileH;
    const int tile_px = 16 * blockIdx.x * kPolyTileW;                              // P.x of the tile's leftmost pixels
    const int py_first = 16 * y0, py_last = 16 * (y0 + kPolyTileH - 1);
    np = min(np, kPolyMaxPolygons);
    if (tid <= np) s_start[tid] = tid < np ? min(max(starts[tid], 0), nv) : nv;
    __syncthreads();

    uint32_t par = 0, on = 0;   // bit 4 r + k: pixel (x0 + k, y0 + r)
    int cur = -1;               // polygon of `par` (uniform)
    auto consume = [&](int n) {
        for (int e = 0; e < n; e++) {
            const int4 E = s_edge[e];
            const int p = s_poly[e];
            if (p != cur) {
                on |= par;
                par = 0;
                cur = p;
            }
            const int dy = E.w - E.y;
            const long long dx = E.z - E.x;
            const long long left = (long long)(16 * x0 - E.x) * dy;
#pragma unroll
            for (int r = 0; r < kPolyTileH; r++) {
                const int py = py_first + 16 * r;
                if ((E.y <= py) == (E.w <= py)) continue;
                long long d = dx * (py - E.y) - left, step = 16ll * dy;
                if (dy < 0) {
                    d = -d;
                    step = -step;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) par ^= (uint32_t)(d - k * step > 0) << (4 * r + k);
            }
        }
    };

    int n = 0;   // edges in LDS (uniform)
    for (int base = 0, it = 0; base < nv; base += 256, it++) {
        if (n + 256 > kPolyEdgeCap) {
            __syncthreads();
            consume(n);
            n = 0;
            __syncthreads();
        }
        const int i = base + tid;
        bool keep = false;
        int4 E = make_int4(0, 0, 0, 0);
        int p = 0;
        if (i < nv) {
            while (p + 1 < np && i >= s_start[p + 1]) p++;
            const int j = i + 1 < s_start[p + 1] ? i + 1 : s_start[p];
            const int2 A = verts[i], B = verts[j];
            E = make_int4(A.x, A.y, B.x, B.y);
            keep = min(A.y, B.y) <= py_last && max(A.y, B.y) > py_first && max(A.x, B.x) > tile_px;
        }
        const unsigned long long ballot = __ballot(keep);
        if (lane == 0) s_wave[it & 1][wave] = __popcll(ballot);
        __syncthreads();
        int at = n, total = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = s_wave[it & 1][k];
            if (k < wave) at += c;
            total += c;
        }
        if (keep) {
            at += __popcll(ballot & ((1ull << lane) - 1ull));
            s_edge[at] = E;
            s_poly[at] = (uint8_t)p;
        }
        n += total;
    }
    __syncthreads();
    consume(n);
    on |= par;
    if (invert) on = ~on;

    if (x0 >= w) return;
#pragma unroll
    for (int r = 0; r < kPolyTileH; r++) {
        const int y = y0 + r;
        if (y >= h) break;
        const uint32_t bits = (on >> (4 * r)) & 15u;
        // bit k -> byte k = 255
        const uint32_t word = ((bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21)) * 255u;
        const size_t at = (size_t)y * w + x0;
        if (x0 + 3 < w && (at & 3) == 0) {
            *reinterpret_cast<uint32_t*>(mask + at) = word;
        } else {
            for (int k = 0; k < 4 && x0 + k < w; k++) mask[at + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

void launch_polygon_mask(const int32_t* poly, int n_vertices, int n_polygons, int invert, uint8_t* mask, int w, int h, hipStream_t s) {
    const dim3 grid((w + kPolyTileW - 1) / kPolyTileW, (h + kPolyTileH - 1) / kPolyTileH);
    hipLaunchKernelGGL(polygon_mask_kernel, grid, dim3(256), 0, s, poly, reinterpret_cast<const int2*>(poly + kPolyVertsAt), n_vertices, n_polygons,
                       invert, mask, w, h, helper_prio_arg());
}

}  // namespace pc
