// kernels_render.hip -- image-order render of a mesh through its LBVH (DESIGN.md section 4 "Mesh render"): per pixel the index
// of the closest triangle, the t of that hit and the on/off byte of a silhouette mask.  The headless counterpart of the
// triangle-index buffer the reference's addon draws with OpenGL (blender_addon/operators/pin_mode/masking_3d.py:17-45).
//
// Pixel (px, py) casts the ray pc_raycast_pixels casts for xy = ((float)px, (float)py): the unprojection below is the one of
// raycast_bvh_kernel / raycast_sweep_kernel (kernels_tracker.hip), the per-triangle test and the tie rule are bvh_closest_hit's
// (bvh.hpp).  A lane's result is min (t, index) over every triangle that passes the test, and the hierarchy only prunes what the
// ray cannot reach, so the planes equal raycast_sweep_kernel evaluated at the pixel grid in every bit.
//
// Mapping.  One lane per pixel, one wavefront (= one workgroup) per tile of kRenderTileW x kRenderTileH pixels: the rays of a
// tile leave one origin in nearly one direction, so its lanes walk nearly the same nodes and a BvhNode fetch (one 64-byte line)
// is nearly uniform; a row of the tile is 64 B of the int32 plane and 16 B of the byte plane.  Each lane keeps its stack column
// in LDS, kBvhStack entries, as raycast_bvh_kernel does: 16 KB per wavefront, ten wavefronts per CU.  Tile shape and traversal
// were picked by measurement (DESIGN_HISTORY.md "Mesh render"): 16 x 4 over 8 x 8, 32 x 2 and 64 x 1, and the per-lane stacks
// over one stack per wavefront, which tests the union of 64 rays' triangles and took 1.57 x the time on a 980 k-triangle mesh.
// No lane waits for another; the traversal ends when the stack is empty and the stack is capped at kBvhStack; every store is
// bounds-tested against the frame, and a null plane is never touched.
#include "bvh.hpp"
#include "kernels.hpp"

namespace pc {

constexpr int kRenderTileW = 16, kRenderTileH = 4;
static_assert(kRenderTileW * kRenderTileH == 64, "a tile is one wavefront");

__global__ __launch_bounds__(64) void mesh_render_kernel(BvhView B, const uint32_t* __restrict__ tri_mask, int check_mask, RayCamera cam,
                                                         int w, int h, int invert, int32_t* __restrict__ prim, float* __restrict__ depth,
                                                         uint8_t* __restrict__ plane) {
    __shared__ int s_stack[kBvhStack][64];
    const int lane = threadIdx.x;
    const int px = blockIdx.x * kRenderTileW + lane % kRenderTileW, py = blockIdx.y * kRenderTileH + lane / kRenderTileW;
    if (px >= w || py >= h) return;
    // CameraIntrinsics::Unproject (cpp/pnp/types.h:95-98) then rotate into object space, as raycast_bvh_kernel
    const float fx = (float)px, fy = (float)py;
    const float ux = cam.sign * ((fx - cam.cx) / cam.fx), uy = cam.sign * ((fy - cam.cy) / cam.fy), uz = cam.sign;
    const float dx = cam.m[0] * ux + cam.m[1] * uy + cam.m[2] * uz;
    const float dy = cam.m[3] * ux + cam.m[4] * uy + cam.m[5] * uz;
    const float dz = cam.m[6] * ux + cam.m[7] * uy + cam.m[8] * uz;
    float best_t, best_u, best_v;
    const int best = bvh_closest_hit(B, cam.origin[0], cam.origin[1], cam.origin[2], dx, dy, dz, &s_stack[0][lane], 64, &best_t, &best_u,
                                     &best_v);
    const size_t at = (size_t)py * (size_t)w + (size_t)px;
    if (prim) prim[at] = best;                                  // the ids do not look at the triangle mask
    if (depth) depth[at] = best >= 0 ? best_t : 0.0f;
    if (plane) {
        // a masked closest triangle is a miss, not a pass-through (ray_casting.cc:104-106)
        bool on = best >= 0 && !(check_mask && ((tri_mask[best >> 5] >> (best & 31)) & 1u));
        if (invert) on = !on;
        plane[at] = on ? 255 : 0;
    }
}

void launch_mesh_render(const BvhView& bvh, const uint32_t* tri_mask, int check_mask, const RayCamera& cam, int w, int h, int invert,
                        int32_t* prim, float* depth, uint8_t* plane, hipStream_t s) {
    if (w <= 0 || h <= 0 || (!prim && !depth && !plane)) return;
    const dim3 grid((unsigned)((w + kRenderTileW - 1) / kRenderTileW), (unsigned)((h + kRenderTileH - 1) / kRenderTileH));
    hipLaunchKernelGGL(mesh_render_kernel, grid, dim3(64), 0, s, bvh, tri_mask, check_mask, cam, w, h, invert, prim, depth, plane);
}

}  // namespace pc
