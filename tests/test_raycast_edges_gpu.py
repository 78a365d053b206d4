"""GPU: the LBVH and the ray-cast kernels where the tracker tests never feed them.
(a) pc_raycast_pixels (hierarchy) against pc_raycast_pixels_sweep (every triangle), bit for bit, on meshes picked for a line of
    kernels_bvh.hip / bvh.hpp each: triangle counts around the 64 / 256 edges of the build kernels, equal Morton codes (one
    centroid, exact copies, a stray far vertex), zero extent in one and in two axes, coordinates far from the origin and small,
    a camera inside a closed box, and rays with an exactly zero direction component (1 / 0 = inf and 0 * inf = NaN in the slab
    test) -- under both unproject signs, with and without the triangle mask.
(b) the sweep through polychase_core (the host's (view * model)^-1) against float64 Moeller-Trumbore (tests/tracker_ref.py) under
    rotated / sheared / mirrored model matrices; gates = 4 x the float32 restatement's own error, measured in
    tests/test_tracker_ref_cpu.py and recorded in profiles/tracker_raycast_gates.txt."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from polychase_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
VP = C.c_void_p
W, H, F = 640.0, 480.0, 500.0
N_RAYS = 4096


class RayCamera(C.Structure):
    _fields_ = [("dir_matrix", C.c_float * 9), ("origin", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("unproject_sign", C.c_float)]


def _p(a):
    return a.ctypes.data_as(VP)


@pytest.fixture(scope="module")
def env():
    L = hip.load()
    ctx = hip.Context(0)
    L.pc_mesh_create.argtypes = [VP, VP, C.c_int, VP, C.c_int, C.POINTER(VP)]
    L.pc_mesh_set_mask.argtypes = [VP, VP, VP, C.c_int]
    L.pc_mesh_destroy.argtypes = [VP]
    for fn in (L.pc_raycast_pixels, L.pc_raycast_pixels_sweep):
        fn.argtypes = [VP, VP, C.POINTER(RayCamera), VP, C.c_int, C.c_int, VP, VP, VP, VP]
    yield L, ctx
    ctx.close()


def _cast(env, mesh, cam, xy, check_mask, sweep):
    L, ctx = env
    n = len(xy)
    hit, pos = np.full(n, 7, np.uint8), np.full((n, 3), np.nan, np.float32)
    prim, uvt = np.full(n, 12345, np.uint32), np.full((n, 3), np.nan, np.float32)
    fn = L.pc_raycast_pixels_sweep if sweep else L.pc_raycast_pixels
    assert fn(ctx._h, mesh, C.byref(cam), _p(xy), n, check_mask, _p(hit), _p(pos), _p(prim), _p(uvt)) == 0, L.pc_last_error()
    return hit, pos, prim, uvt


def _camera(R, origin, sign, f=F, cx=W / 2, cy=H / 2):
    """f > 0: with sign = -1 the OpenGL intrinsics are (-f, -f)"""
    cam = RayCamera()
    cam.dir_matrix[:] = [float(v) for v in np.asarray(R, np.float32).ravel()]
    cam.origin[:] = [float(v) for v in np.asarray(origin, np.float32)]
    cam.fx = cam.fy = f * sign
    cam.cx, cam.cy, cam.unproject_sign = cx, cy, sign
    return cam


def _look_at(center, dist, sign, R):
    """a camera `dist` away from `center`, looking at it along its own forward axis (+z for sign = +1, -z for -1)"""
    fwd = np.asarray(R, float) @ [0, 0, sign]
    return _camera(R, np.asarray(center, float) - dist * fwd, sign)


def _same_as_sweep(env, verts, tris, cams, xy=None, seed=0):
    """hierarchy == sweep in every output word, for every camera, with and without the mask (every seventh triangle);
    returns the unmasked sweep results per camera"""
    L, ctx = env
    verts, tris = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.uint32)
    mesh = VP()
    assert L.pc_mesh_create(ctx._h, _p(verts), len(verts), _p(tris), len(tris), C.byref(mesh)) == 0, L.pc_last_error()
    words = np.zeros((len(tris) + 31) // 32, np.uint32)
    for t in range(0, len(tris), 7):
        words[t >> 5] |= np.uint32(1 << (t & 31))
    assert L.pc_mesh_set_mask(ctx._h, mesh, _p(words), len(words)) == 0
    if xy is None:
        rng = np.random.default_rng(seed)
        xy = rng.uniform([-40, -40], [W + 40, H + 40], (N_RAYS, 2)).astype(np.float32)      # some outside the image
        xy[:64] = np.floor(xy[:64])
    out = []
    for cam in cams:
        for check_mask in (0, 1):
            a = _cast(env, mesh, cam, xy, check_mask, sweep=False)
            b = _cast(env, mesh, cam, xy, check_mask, sweep=True)
            assert set(np.unique(b[0])) <= {0, 1}
            for ga, gb in zip(a, b):
                assert np.array_equal(ga.view(np.uint8), gb.view(np.uint8))
            hit = b[0] == 1
            assert np.all(b[2][hit] < len(tris)) and np.all(b[2][~hit] == 0xffffffff)
            if check_mask:                                   # a masked closest triangle is a miss, not a pass-through
                free = out[-1]
                masked = (free[0] == 1) & (free[2] % 7 == 0)
                assert np.array_equal(hit, (free[0] == 1) & ~masked)
                assert np.array_equal(b[3][hit], free[3][hit])
            else:
                out.append(b)
    L.pc_mesh_destroy(mesh)
    return out


R_TILT = tr._rot([0.4, 1.0, 0.2], 0.35)


def _cams(center, dist):
    return [_look_at(center, dist, s, R_TILT) for s in (1.0, -1.0)]


def _soup(n, rng):
    """triangles of very different size all over [-2, 2]^3; number 0 is large and central, so that every prefix is hit"""
    c = rng.uniform(-2, 2, (n, 1, 3))
    size = 10 ** rng.uniform(-1.5, 0.0, (n, 1, 1))
    c[0], size[0] = 0.0, 1.5
    verts = (c + rng.normal(0, 1, (n, 3, 3)) * size).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def _flat_grid(nx, ny, axis):
    """nx x ny cells in [0, 1]^2, lying exactly in the plane `axis` = 0"""
    gx, gy = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1))
    plane = np.stack([gx.ravel(), gy.ravel()], 1)
    verts = np.insert(plane, axis, 0.0, axis=1).astype(np.float32)
    a = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    tris = np.stack([np.stack([a, a + 1, a + nx + 2], 1), np.stack([a, a + nx + 2, a + nx + 1], 1)], 1).reshape(-1, 3)
    return verts, tris.astype(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_soup_prefixes_around_the_build_kernels_edges(env, n):
    verts, tris = _soup(1000, np.random.default_rng(11))
    res = _same_as_sweep(env, verts, tris[:n], _cams([0, 0, 0], 7.0), seed=n)
    assert all(r[0].sum() > 30 for r in res)
    if n >= 63:
        assert all(len(np.unique(r[2][r[0] == 1])) > 10 for r in res)


def test_many_triangles_around_one_centroid(env):
    """equal Morton codes: the index half of the key alone decides the topology"""
    rng = np.random.default_rng(12)
    n = 300
    p = rng.normal(0, 1, (n, 2, 3)) * 10 ** rng.uniform(-1.0, 0.3, (n, 1, 1))
    p = p.astype(np.float32)
    verts = np.concatenate([p, -(p[:, :1] + p[:, 1:2])], 1)          # a + b + c == 0 exactly, in the kernel's order too
    assert not ((verts[:, 0] + verts[:, 1]) + verts[:, 2]).any()
    res = _same_as_sweep(env, verts.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), _cams([0, 0, 0], 6.0))
    assert all(len(np.unique(r[2][r[0] == 1])) > 30 for r in res)


def test_exact_copies_of_one_triangle_the_lowest_index_wins(env):
    tri = np.array([[-1.5, -1.2, 0.1], [1.6, -1.0, -0.2], [0.1, 1.4, 0.3]], np.float32)
    n = 300
    res = _same_as_sweep(env, np.tile(tri, (n, 1)), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), _cams([0, 0, 0], 6.0))
    for r in res:
        assert r[0].sum() > 200 and np.all(r[2][r[0] == 1] == 0)
    # the same with shared vertices, the copies only in the index array
    res = _same_as_sweep(env, tri, np.tile(np.array([[0, 1, 2]], np.uint32), (n, 1)), _cams([0, 0, 0], 6.0))
    for r in res:
        assert r[0].sum() > 200 and np.all(r[2][r[0] == 1] == 0)


def test_a_stray_far_vertex_collapses_the_morton_cells(env):
    gx, gy = np.meshgrid(np.linspace(0, 1, 41), np.linspace(0, 1, 26))
    z = 0.5 + 0.2 * np.sin(5 * gx) * np.cos(4 * gy)
    verts = np.stack([gx.ravel(), gy.ravel(), z.ravel()], 1)
    a = (np.arange(25)[:, None] * 41 + np.arange(40)[None, :]).ravel()
    tris = np.stack([np.stack([a, a + 1, a + 42], 1), np.stack([a, a + 42, a + 41], 1)], 1).reshape(-1, 3)
    assert len(tris) == 2000
    far = np.array([[1e4, 1e4, 1e4], [1e4 + 1, 1e4, 1e4], [1e4, 1e4 + 1, 1e4]])
    verts = np.concatenate([verts, far]).astype(np.float32)
    tris = np.concatenate([tris, [[len(verts) - 3, len(verts) - 2, len(verts) - 1]]]).astype(np.uint32)
    res = _same_as_sweep(env, verts, tris, _cams([0.5, 0.5, 0.5], 1.2))
    assert all(r[0].sum() > 800 and len(np.unique(r[2][r[0] == 1])) > 300 for r in res)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_flat_grid_with_zero_extent_in_one_axis(env, axis):
    verts, tris = _flat_grid(12, 10, axis)
    center = np.insert([0.5, 0.5], axis, 0.0)
    res = _same_as_sweep(env, verts, tris, _cams(center, 1.8) + [_look_at(center, 1.8, 1.0, tr._rot([1, 1, 1], 2.0 * (axis + 1)))])
    assert sum(r[0].sum() for r in res) > 500


def test_a_row_of_triangles_with_two_zero_extents(env):
    """congruent triangles along x: the centroids differ in x only"""
    n = 40
    tri = np.array([[0, -0.3, 0], [0.2, 0.3, 0.1], [-0.1, 0.3, -0.1]])
    verts = (tri[None] + np.arange(n)[:, None, None] * np.array([0.125, 0, 0])).reshape(-1, 3).astype(np.float32)
    c = verts.reshape(n, 3, 3)
    cen = (c[:, 0] + c[:, 1] + c[:, 2]) * np.float32(1 / 3)
    assert np.ptp(cen[:, 1]) == 0 and np.ptp(cen[:, 2]) == 0 and np.ptp(cen[:, 0]) > 0
    res = _same_as_sweep(env, verts, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), _cams([2.5, 0, 0], 4.0))
    assert all(len(np.unique(r[2][r[0] == 1])) > 20 for r in res)


@pytest.mark.parametrize("kind", ["plain", "translated_1e3", "scaled_1e-2"])
def test_grid_far_from_the_origin_and_small(env, kind):
    """pad = 1e-5 * extent has to cover the float32 error of Moeller-Trumbore at these coordinates; not below 1e-2: the
    absolute 1e-10 determinant gate would reject the triangles in the reference too"""
    verts, tris = tr.grid_mesh()
    shift, scale = (np.float32(1e3) if kind == "translated_1e3" else np.float32(0)), (np.float32(1e-2) if kind == "scaled_1e-2" else np.float32(1))
    verts = verts * scale + shift
    res = _same_as_sweep(env, verts, tris, _cams(np.full(3, float(shift)), 6.0 * float(scale)))
    assert all(r[0].sum() > 800 and len(np.unique(r[2][r[0] == 1])) > 300 for r in res)


def test_camera_inside_a_closed_box(env):
    """back faces are hit; triangles behind the origin are not"""
    faces_v, faces_t = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            v, t = _flat_grid(4, 4, axis)
            v[:, axis] = side
            faces_t.append(t + sum(len(x) for x in faces_v))
            faces_v.append(v)
    verts, tris = np.concatenate(faces_v), np.concatenate(faces_t)
    assert len(tris) == 192
    origin = np.array([0.4, 0.55, 0.3])
    cams = [_camera(R, origin, s) for s in (1.0, -1.0) for R in (R_TILT, tr._rot([1, 0.2, 0], 1.7))]
    res = _same_as_sweep(env, verts, tris, cams)
    for cam, r in zip(cams, res):
        hit = r[0] == 1
        assert hit.mean() > 0.995                                     # closed: (all but a ray through a crack) end on a wall
        assert np.all(r[3][hit, 2] > 0)
        fwd = np.array(cam.dir_matrix[:]).reshape(3, 3) @ [0, 0, cam.unproject_sign]
        assert np.all((r[1][hit] - origin) @ fwd > 0)                    # ... on a wall in front of the camera


@pytest.mark.parametrize("place", ["on_vertex", "on_box_low_face", "on_box_high_face"])
def test_axis_parallel_rays(env, place):
    """dir_matrix = identity and an integer principal point: the row y = cy has dy == 0, the column x = cx has dx == 0, the
    centre both -- 1 / d = +-inf in the traversal.  The origin's x and y equal a vertex's, or a padded box face's (pad as
    pc_mesh_create computes it), where (lo - o) * inf = 0 * inf = NaN."""
    verts, tris = tr.grid_mesh()
    xs = np.unique(verts[:, 0])
    ext = (verts.max(0) - verts.min(0)).max()
    pad = np.float32(1e-5) * ext + np.float32(1e-30)
    off = {"on_vertex": np.float32(0), "on_box_low_face": -pad, "on_box_high_face": pad}[place]
    ox, oy = xs[7] + off, xs[12] + off
    cx, cy = 300.0, 200.0
    xy = np.concatenate([np.stack([np.arange(W), np.full(int(W), cy)], 1), np.stack([np.full(int(H), cx), np.arange(H)], 1), [[cx, cy]]])
    xy = xy.astype(np.float32)
    cams, zero_signs = [], set()
    for sign, fy_sign in ((1.0, 1.0), (-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0)):
        cam = _camera(np.eye(3), [ox, oy, -6.0 * sign], sign, cx=cx, cy=cy)
        cam.fy = F * fy_sign
        cams.append(cam)
        # the directions as the kernels form them
        s = np.float32(sign)
        ux, uy = s * ((xy[:, 0] - np.float32(cx)) / np.float32(cam.fx)), s * ((xy[:, 1] - np.float32(cy)) / np.float32(cam.fy))
        z = np.float32(0)
        d = np.stack([ux + z * uy + z * s, z * ux + uy + z * s], 1)
        zero_signs |= {bool(b) for b in np.signbit(d[d == 0])}
    assert zero_signs == {False, True}                                # +0 and -0 components both occur
    res = _same_as_sweep(env, verts, tris, cams, xy=xy)
    nW = int(W)
    for r in res:                                                     # at least one ray of each kind hits
        assert r[0][:nW].sum() > 100 and r[0][nW:-1].sum() > 100 and r[0][-1] == 1


# ---- (b) the sweep through polychase_core against float64 ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@pytest.fixture(scope="module")
def gates():
    return tr.raycast_gates()


@pytest.mark.parametrize("name", list(tr.raycast_scene_specs()))
def test_sweep_equals_float64_under_general_model_matrices(core, gates, name):
    sc, r64, _, _ = tr.raycast_reference(name)
    amb = tr.raycast_ambiguous(r64, gates)
    assert amb.mean() <= 0.01                                         # before the GPU result is looked at
    k = core.CameraIntrinsics(fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, aspect_ratio=1.07, width=tr.RC_W, height=tr.RC_H,
                              convention=core.CameraConvention.OpenCV if sc.opencv else core.CameraConvention.OpenGL)
    mesh = core.AcceleratedMesh(sc.verts, sc.tris)
    hits = core._ray_cast_pixels(mesh, core.SceneTransformations(sc.model, sc.view, k), sc.xy, False, exhaustive=True)
    got = np.array([h is not None for h in hits])
    ok = ~amb
    assert np.array_equal(got[ok], r64.hit[ok])
    idx = np.nonzero(ok & r64.hit)[0]
    assert len(idx) > 500
    assert np.array_equal(np.array([hits[i].primitive_id for i in idx]), r64.prim[idx])
    uv = np.array([hits[i].barycentric_coordinate for i in idx], np.float64)
    t = np.array([hits[i].t for i in idx], np.float64)
    pos = np.array([hits[i].pos for i in idx], np.float64)
    worst = (max(np.abs(uv[:, 0] - r64.u[idx]).max(), np.abs(uv[:, 1] - r64.v[idx]).max()) / gates[0],
             np.abs(t - r64.t[idx]).max() / gates[1], np.abs(pos - r64.pos[idx]).max() / gates[2])
    print(f"{name}: worst |gpu - f64| / gate: bary {worst[0]:.4f} t {worst[1]:.4f} pos {worst[2]:.4f}; ambiguous {int(amb.sum())}")
    assert max(worst) <= 1.0
