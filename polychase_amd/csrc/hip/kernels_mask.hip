// kernels_mask.hip -- the detection mask's plane (kernels_gftt.hip: the MASKED variants read it) rasterised on gfx950 from
// polygon outlines (include/polychase_hip.h: pc_frame_set_mask_polygons states the fill rule; DESIGN.md section 4 "Polygon
// masks").  Further down: the choked plane of a mask and the test of the forward records against it ("Target-side masks"), and
// the weight planes of the masked windows ("Masked windows").
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

// ---- target-side masks (DESIGN.md section 4 "Target-side masks") ----
//
// mask_choke_kernel: the choked plane C_r of a mask plane -- out(x, y) = 255 when every pixel of the frame within r of (x, y) in
// both axes is on (byte != 0), else 0; pixels outside the frame count as on.  The structuring element is a square, so the erosion
// is a row pass followed by a column pass, and both run on BITS:
//   row pass     a wavefront takes one row of the tile with its halo, kChokeTileW + 2 r <= 126 pixels.  Two ballots turn the
//                row's bytes into a 128-bit word X (bit k: column x0 - r + k); Y = AND over k in [0, 2 r] of X >> k, by doubling
//                (a handful of wave-uniform shifts), has in bit i the answer for column x0 + i.  Its low 64 bits go to LDS, one
//                word per row: (kChokeTileH + 62) * 8 = 752 bytes.  The zeros a right shift brings in at bit 127 travel 2 r <= 62
//                bits down and never reach bit 63.
//   column pass  the lane of output row t and byte octet q ANDs the 2 r + 1 words of rows t .. t + 2 r (eight lanes read one
//                address: a broadcast) and expands its eight bits to bytes.
// One launch, every loop bounded by r, no workgroup waits for another, each byte of the output written exactly once.  r = 0 is
// accepted as well and gives the on/off image of the input.
constexpr int kChokeTileW = 64, kChokeTileH = 32;   // one ballot wide; 256 lanes x 8 pixels
constexpr int kChokeMaxMargin = 31;
static_assert(kChokeTileW == 64, "a row of the tile is one ballot");
static_assert(kChokeTileW + 2 * kChokeMaxMargin <= 128, "a row of the tile with its halo is two ballots");
static_assert(kChokeTileH * (kChokeTileW / 8) == 256, "a lane owns eight pixels of one row");

__device__ __forceinline__ void shr128(unsigned long long& hi, unsigned long long& lo, int k) {   // 0 <= k < 64
    if (k == 0) return;
    lo = (lo >> k) | (hi << (64 - k));
    hi >>= k;
}

__global__ __launch_bounds__(256) void mask_choke_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int w, int h, int r,
                                                         int hi_prio) {
    helper_priority(hi_prio);
    __shared__ unsigned long long s_row[kChokeTileH + 2 * kChokeMaxMargin];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kChokeTileW, y0 = blockIdx.y * kChokeTileH;
    r = min(max(r, 0), kChokeMaxMargin);
    const int rows_in = kChokeTileH + 2 * r, window = 2 * r + 1;

    for (int j = wave; j < rows_in; j += 4) {   // whole wavefronts: j is uniform
        const int y = y0 - r + j;
        const bool row_in = y >= 0 && y < h;
        const int c0 = x0 - r + lane, c1 = c0 + 64;
        bool on0 = true, on1 = true;            // outside the frame: on
        if (row_in && c0 >= 0 && c0 < w) on0 = in[(size_t)y * w + c0] != 0;
        if (row_in && lane < 2 * r && c1 < w) on1 = in[(size_t)y * w + c1] != 0;   // c1 >= 64 - r > 0
        unsigned long long lo = __ballot(on0), hi = __ballot(on1);
        int len = 1;
        while (2 * len <= window) {
            unsigned long long h2 = hi, l2 = lo;
            shr128(h2, l2, len);
            hi &= h2;
            lo &= l2;
            len *= 2;
        }
        if (len < window) {
            unsigned long long h2 = hi, l2 = lo;
            shr128(h2, l2, window - len);
            lo &= l2;
        }
        if (lane == 0) s_row[j] = lo;
    }
    __syncthreads();

    const int t = tid >> 3, q = tid & 7;
    const int x = x0 + 8 * q, y = y0 + t;
    if (x >= w || y >= h) return;
    unsigned long long z = s_row[t];
    for (int k = 1; k < window; k++) z &= s_row[t + k];
    const uint32_t bits8 = (uint32_t)(z >> (8 * q)) & 255u;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const uint32_t bits = (bits8 >> (4 * half)) & 15u;
        // bit k -> byte k = 255
        const uint32_t word = ((bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21)) * 255u;
        const int xq = x + 4 * half;
        const size_t at = (size_t)y * w + xq;
        if (xq + 3 < w && (at & 3) == 0) {
            *reinterpret_cast<uint32_t*>(out + at) = word;
        } else {
            for (int k = 0; k < 4 && xq + k < w; k++) out[at + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

void launch_mask_choke(const uint8_t* mask, uint8_t* choked, int w, int h, int margin, hipStream_t s) {
    const dim3 grid((w + kChokeTileW - 1) / kChokeTileW, (h + kChokeTileH - 1) / kChokeTileH);
    hipLaunchKernelGGL(mask_choke_kernel, grid, dim3(256), 0, s, mask, choked, w, h, margin, helper_prio_arg());
}

// lk_target_mask_kernel: one lane per raw record of the forward launch.  A record with status 1 whose target holds a plane is
// judged by the plane's byte at its end point's pixel (include/polychase_hip.h: pc_lk_track_masked has the rounding); a zero
// clears the status word, as lk_fb_kernel does.  End point and error stay.
__global__ __launch_bounds__(256) void lk_target_mask_kernel(const TargetMaskParams p) {
    helper_priority(p.hi_prio);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.n * kRecStride) return;
    const int tgt = (int)(i & (kRecStride - 1));
    if (tgt >= p.n_targets) return;
    const uint8_t* const plane = p.plane[tgt];
    if (!plane) return;
    const float4 rec = p.rec[i];
    if (__float_as_uint(rec.w) != 1u) return;
    const int ix = (int)fminf(fmaxf(floorf(rec.x + 0.5f), 0.f), (float)(p.w - 1));   // a NaN lands on 0
    const int iy = (int)fminf(fmaxf(floorf(rec.y + 0.5f), 0.f), (float)(p.h - 1));
    if (plane[(size_t)iy * p.w + ix] == 0) p.rec[i].w = __uint_as_float(0u);
}

void launch_lk_target_mask(TargetMaskParams p, hipStream_t s) {
    if (p.n <= 0 || p.n_targets <= 0) return;
    p.hi_prio = helper_prio_arg();
    const size_t lanes = (size_t)p.n * kRecStride;
    hipLaunchKernelGGL(lk_target_mask_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, p);
}

// ---- masked windows: the weight planes of a frame (DESIGN.md section 4 "Masked windows") ----
//
// mask_down_kernel: M_l from M_{l-1}, one lane per pixel of level l: the AND of the 5 x 5 pixels pyrDown read to make it, through
// the REFLECT_101 index map.  Both planes are packed; any non-zero byte of the input is on (level 1 reads the mask plane itself).
// window_weight_kernel: W_l of every level in one launch (blockIdx.z = level), one lane per 4 adjacent pixels: the AND of M_l over
// the Scharr support, neighbours outside the level counting as on, written to the interior of the padded plane.  Every read is
// bounds-tested against the level, every write against its interior; no lane waits for another.
__global__ __launch_bounds__(256) void mask_down_kernel(const uint8_t* __restrict__ in, int pw, int ph, uint8_t* __restrict__ out, int w, int h,
                                                        int hi_prio) {
    helper_priority(hi_prio);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    bool on = true;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const uint8_t* const row = in + (size_t)reflect101(2 * y + dy, ph) * pw;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) on = on && row[reflect101(2 * x + dx, pw)] != 0;
    }
    out[(size_t)y * w + x] = on ? 255 : 0;
}

__global__ __launch_bounds__(256) void window_weight_kernel(const WindowWeightParams p) {
    helper_priority(p.hi_prio);
    const int l = blockIdx.z;
    const int w = p.w[l], h = p.h[l];
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= w || y >= h) return;
    const uint8_t* __restrict__ m = l == 0 ? p.mask : p.m[l];
    uint32_t col = 0;   // bit k: every pixel of column x0 - 1 + k in rows y - 1 .. y + 1 is on (outside the level: on)
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int x = x0 - 1 + k;
        bool on = true;
        if (x >= 0 && x < w) {
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int yy = y + dy;
                if (yy >= 0 && yy < h) on = on && m[(size_t)yy * w + x] != 0;
            }
        }
        col |= (uint32_t)on << k;
    }
    const uint32_t bits = col & (col >> 1) & (col >> 2) & 15u;
    // bit k -> byte k = 255
    const uint32_t word = ((bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21)) * 255u;
    uint8_t* const out = p.wt[l] + (size_t)y * p.pitch[l] + x0;   // interior rows start 4-byte aligned (kPadX, pitch)
    if (x0 + 3 < w) {
        *reinterpret_cast<uint32_t*>(out) = word;
    } else {
        for (int k = 0; k < 4 && x0 + k < w; k++) out[k] = (uint8_t)(word >> (8 * k));
    }
}

void launch_window_weights(WindowWeightParams p, hipStream_t s) {
    if (p.nlevels < 1) return;
    p.hi_prio = helper_prio_arg();
    for (int l = 1; l < p.nlevels; l++) {
        const dim3 grid((p.w[l] + 63) / 64, (p.h[l] + 3) / 4);
        hipLaunchKernelGGL(mask_down_kernel, grid, dim3(256), 0, s, l == 1 ? p.mask : p.m[l - 1], p.w[l - 1], p.h[l - 1], p.m[l], p.w[l], p.h[l],
                           p.hi_prio);
    }
    const dim3 grid((p.w[0] + 255) / 256, (p.h[0] + 3) / 4, p.nlevels);
    hipLaunchKernelGGL(window_weight_kernel, grid, dim3(256), 0, s, p);
}

}  // namespace pc
