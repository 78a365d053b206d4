"""GPU: pc_mesh_render through the C ABI.
(a) bit parity: prim, depth and the un-inverted, un-eroded mask equal pc_raycast_pixels_sweep evaluated at the pixel grid in every
    byte -- prim and depth against the sweep WITHOUT the triangle mask (the ids do not look at it), mask against the sweep's hit
    under the same check_mask -- on the soup, a one-triangle mesh, a flat grid lying in a coordinate plane and a camera inside a
    closed box, at frame sizes that are no multiple of any tile, under both unproject signs;
(b) the scene whose planes are known in closed form, and float64 on the pixels float32 can decide;
(c) erosion and polarity against tests/mesh_render_ref.py applied to the GPU's own un-eroded plane; host and device pointers;
    null planes; (d) every refusal, and the resource counts after the run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from polychase_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_ref as mr  # noqa: E402
import test_raycast_edges_gpu as edges  # noqa: E402
import tracker_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
VP = C.c_void_p
RayCamera = edges.RayCamera
SIZES = [(67, 45), (131, 70), (1, 1), (200, 3), (3, 200)]
PC_E_INVALID = -1


def _p(a):
    return a.ctypes.data_as(VP)


@pytest.fixture(scope="module")
def env():
    L = hip.load()
    ctx = hip.Context(0)
    L.pc_mesh_create.argtypes = [VP, VP, C.c_int, VP, C.c_int, C.POINTER(VP)]
    L.pc_mesh_set_mask.argtypes = [VP, VP, VP, C.c_int]
    L.pc_mesh_destroy.argtypes = [VP]
    L.pc_raycast_pixels_sweep.argtypes = [VP, VP, C.POINTER(RayCamera), VP, C.c_int, C.c_int, VP, VP, VP, VP]
    L.pc_mesh_render.argtypes = [VP, VP, C.POINTER(RayCamera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP, VP, VP]
    L.pc_peer_buffer_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(VP)]
    L.pc_peer_buffer_free.argtypes = [C.c_int, VP]
    L.pc_context_download.argtypes = [VP, VP, VP, C.c_size_t]
    yield L, ctx
    ctx.close()


def _cam(c):
    """the ctypes camera of a mesh_render_ref camera"""
    cam = RayCamera()
    cam.dir_matrix[:] = [float(v) for v in c.R.ravel()]
    cam.origin[:] = [float(v) for v in c.origin]
    cam.fx, cam.fy, cam.cx, cam.cy, cam.unproject_sign = c.fx, c.fy, c.cx, c.cy, c.sign
    return cam


class Mesh:
    def __init__(self, env, verts, tris, every_seventh_masked=True):
        L, ctx = env
        self.L, self.ctx = L, ctx
        self.verts, self.tris = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.uint32)
        self.h = VP()
        assert L.pc_mesh_create(ctx._h, _p(self.verts), len(self.verts), _p(self.tris), len(self.tris), C.byref(self.h)) == 0, L.pc_last_error()
        self.masked = np.zeros(len(self.tris), bool)
        if every_seventh_masked:
            self.masked[::7] = True
            words = np.zeros((len(self.tris) + 31) // 32, np.uint32)
            for t in np.nonzero(self.masked)[0]:
                words[t >> 5] |= np.uint32(1 << (t & 31))
            assert L.pc_mesh_set_mask(ctx._h, self.h, _p(words), len(words)) == 0

    def close(self):
        self.L.pc_mesh_destroy(self.h)

    def render(self, cam, w, h, check_mask=0, invert=0, margin=0, planes="pdm"):
        """host pointers; the planes not asked for come back as None"""
        prim = np.full((h, w), 12345, np.int32) if "p" in planes else None
        depth = np.full((h, w), np.nan, np.float32) if "d" in planes else None
        mask = np.full((h, w), 7, np.uint8) if "m" in planes else None
        rc = self.L.pc_mesh_render(self.ctx._h, self.h, C.byref(cam), w, h, check_mask, invert, margin, 0,
                                   _p(prim) if prim is not None else None, _p(depth) if depth is not None else None,
                                   _p(mask) if mask is not None else None)
        assert rc == 0, self.L.pc_last_error()
        return prim, depth, mask

    def sweep(self, cam, w, h, check_mask):
        xy = mr.pixel_grid(w, h)
        n = len(xy)
        hit, pos = np.full(n, 7, np.uint8), np.full((n, 3), np.nan, np.float32)
        prim, uvt = np.full(n, 12345, np.uint32), np.full((n, 3), np.nan, np.float32)
        assert self.L.pc_raycast_pixels_sweep(self.ctx._h, self.h, C.byref(cam), _p(xy), n, check_mask, _p(hit), _p(pos), _p(prim),
                                              _p(uvt)) == 0, self.L.pc_last_error()
        return hit.reshape(h, w), prim.reshape(h, w), uvt[:, 2].copy().reshape(h, w)


def _same_as_sweep(mesh, cam, w, h):
    """every byte of the three planes, with and without the triangle mask; returns the planes of check_mask = 0"""
    free_hit, free_prim, free_t = mesh.sweep(cam, w, h, 0)
    out = None
    for check_mask in (0, 1):
        prim, depth, mask = mesh.render(cam, w, h, check_mask)
        hit = free_hit if check_mask == 0 else mesh.sweep(cam, w, h, 1)[0]
        assert np.array_equal(prim.view(np.uint32), free_prim)                 # 0xffffffff <-> -1; masked triangles still show
        assert np.array_equal(depth.view(np.uint32), free_t.view(np.uint32))
        assert np.array_equal(mask, hit * np.uint8(255))
        if check_mask:
            seen_masked = (prim >= 0) & mesh.masked[np.maximum(prim, 0)]
            assert np.array_equal(mask == 255, (prim >= 0) & ~seen_masked)
        else:
            out = (prim, depth, mask)
    return out


def _soup_cams(w, h, f):
    return [_cam(mr.look_at([0, 0, 0], 6.0, s, edges.R_TILT, f, w // 2, h // 2)) for s in (1.0, -1.0)]


@pytest.fixture(scope="module")
def soup(env):
    m = Mesh(env, *mr.soup_mesh())
    yield m
    m.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_soup_equals_the_sweep_at_the_pixel_grid(soup, w, h):
    for cam in _soup_cams(w, h, 50.0 if w < 100 else 100.0):
        prim, _, mask = _same_as_sweep(soup, cam, w, h)
        assert (mask == 255).any()                                          # triangle 0 is large and central
    if w * h > 1000:
        assert len(np.unique(prim[prim >= 0])) > 30 and (prim[prim >= 0] % 7 == 0).any()


@pytest.mark.parametrize("w,h", SIZES)
def test_one_triangle_equals_the_sweep(env, w, h):
    tri = np.array([[-1.5, -1.2, 0.1], [1.6, -1.0, -0.2], [0.1, 1.4, 0.3]], np.float32)
    m = Mesh(env, tri, [[0, 1, 2]], every_seventh_masked=False)
    for cam in _soup_cams(w, h, 50.0):
        prim, _, mask = _same_as_sweep(m, cam, w, h)
        assert set(np.unique(prim)) <= {-1, 0} and (prim == 0).any()
    m.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_flat_grid_in_a_coordinate_plane_equals_the_sweep(env, axis):
    m = Mesh(env, *edges._flat_grid(12, 10, axis))
    center = np.insert([0.5, 0.5], axis, 0.0)
    hits = 0
    for w, h in ((67, 45), (3, 200)):
        for s in (1.0, -1.0):
            cam = _cam(mr.look_at(center, 1.8, s, edges.R_TILT, 50.0, w // 2, h // 2))
            hits += (_same_as_sweep(m, cam, w, h)[2] == 255).sum()
    assert hits > 100                                                       # the scene is not empty (seen edge-on under one axis)
    m.close()


def test_camera_inside_a_closed_box_equals_the_sweep(env):
    faces_v, faces_t = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            v, t = edges._flat_grid(4, 4, axis)
            v[:, axis] = side
            faces_t.append(t + sum(len(x) for x in faces_v))
            faces_v.append(v)
    m = Mesh(env, np.concatenate(faces_v), np.concatenate(faces_t))
    for w, h in ((67, 45), (131, 70)):
        for s in (1.0, -1.0):
            cam = _cam(mr.camera(edges.R_TILT, [0.4, 0.55, 0.3], s, 50.0, w // 2, h // 2))
            prim, depth, mask = _same_as_sweep(m, cam, w, h)
            assert (prim >= 0).mean() > 0.995 and np.all(depth[prim >= 0] > 0)   # closed: every ray ends on a wall in front
    m.close()


def test_empty_mesh_renders_all_miss(env):
    m = Mesh(env, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), every_seventh_masked=False)
    prim, depth, mask = m.render(_soup_cams(67, 45, 50.0)[0], 67, 45)
    assert np.all(prim == -1) and np.all(depth == 0) and np.all(mask == 0)
    assert np.all(m.render(_soup_cams(67, 45, 50.0)[0], 67, 45, invert=1, planes="m")[2] == 255)
    m.close()


def test_exact_scene(env):
    verts, tris, c = mr.exact_scene()
    m = Mesh(env, verts, tris, every_seventh_masked=False)
    prim, depth, mask = m.render(_cam(c), mr.EXACT_W, mr.EXACT_H)
    assert np.array_equal(mask, mr.rect_plane(mr.EXACT_W, mr.EXACT_H, *mr.EXACT_RECT))
    assert (prim == 0).sum() == 300 and (prim == 1).sum() == 300
    assert np.abs(depth[mask == 255] - 4.0).max() <= mr.GATE_T and np.all(depth[mask == 0] == 0)
    assert np.array_equal(m.render(_cam(c), mr.EXACT_W, mr.EXACT_H, margin=3, planes="m")[2],
                          mr.rect_plane(mr.EXACT_W, mr.EXACT_H, 14, 37, 9, 22))
    assert np.array_equal(m.render(_cam(c), mr.EXACT_W, mr.EXACT_H, invert=1, margin=3, planes="m")[2],
                          mr.rect_plane(mr.EXACT_W, mr.EXACT_H, 8, 43, 3, 28, inside=0, outside=255))
    m.close()


@pytest.mark.parametrize("name", list(mr.SOUP_SCENES))
def test_soup_equals_float64_where_float32_can_decide(soup, name):
    w, h, c, prim64, hit64, amb = mr.soup_reference(name)
    assert amb.mean() <= 0.005                                              # before the GPU result is looked at
    prim, _, mask = soup.render(_cam(c), w, h)
    ok = ~amb
    assert np.array_equal((mask == 255)[ok], hit64[ok])
    assert np.array_equal(prim[ok], prim64[ok])


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("margin", [0, 1, 5, 31])
def test_erosion_and_polarity_follow_the_rule(soup, margin, invert):
    w, h = 131, 70
    cam = _soup_cams(w, h, 100.0)[0]
    plain = soup.render(cam, w, h, 1, planes="m")[2]
    got = soup.render(cam, w, h, 1, invert, margin, planes="m")[2]
    assert np.array_equal(got, mr.mask_from_hit(plain, invert, margin))
    if margin <= 5:
        assert (got == 255).any() and (got == 0).any()


def test_device_pointers_give_the_same_bytes_and_null_planes_are_left_alone(env, soup):
    import torch

    L, ctx = env
    w, h = 131, 70
    n = w * h
    cam = _soup_cams(w, h, 100.0)[1]
    want = soup.render(cam, w, h, 1, 1, 5)
    want_plain = soup.render(cam, w, h, 1)
    # one device block: canary | prim | canary | depth | canary | mask | canary (every start 4-byte aligned)
    guard = 256
    offs = [0]
    for size in (guard, 4 * n, guard, 4 * n, guard, n, guard):
        offs.append((offs[-1] + size + 3) // 4 * 4)
    total = offs[-1]
    for planes in ("pdm", "p", "d", "m", "pm"):
        block = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        at = lambda k: VP(block.data_ptr() + offs[k])   # noqa: E731
        inv, mar = (1, 5) if "m" in planes else (0, 0)
        rc = L.pc_mesh_render(ctx._h, soup.h, C.byref(cam), w, h, 1, inv, mar, 1, at(1) if "p" in planes else None,
                              at(3) if "d" in planes else None, at(5) if "m" in planes else None)
        assert rc == 0, L.pc_last_error()
        host = block.cpu().numpy()
        for k, (key, ref) in enumerate(zip("pdm", want)):
            lo, hi = offs[2 * k + 1], offs[2 * k + 1] + ref.nbytes
            if key in planes:
                assert np.array_equal(host[lo:hi], ref.view(np.uint8).ravel())
            else:
                assert np.all(host[lo:hi] == 0xA5)
            assert np.all(host[offs[2 * k]:lo] == 0xA5) and np.all(host[hi:offs[2 * k + 2]] == 0xA5)
    # host pointers: asking for one plane gives that plane's bytes
    for planes in ("p", "d", "m"):
        got = soup.render(cam, w, h, 1, planes=planes)
        for g, ref in zip(got, want_plain):
            assert g is None or np.array_equal(g.view(np.uint8), ref.view(np.uint8))


def test_refusals(env, soup):
    L, ctx = env
    cam = _soup_cams(67, 45, 50.0)[0]
    w, h = 67, 45
    prim, depth, mask = np.zeros((h, w), np.int32), np.zeros((h, w), np.float32), np.zeros((h, w), np.uint8)

    def call(c=ctx._h, m=soup.h, k=C.byref(cam), w=w, h=h, check=0, invert=0, margin=0, p=_p(prim), d=_p(depth), b=_p(mask)):
        return L.pc_mesh_render(c, m, k, w, h, check, invert, margin, 0, p, d, b)

    assert call() == 0
    assert call(c=None) == PC_E_INVALID and call(m=None) == PC_E_INVALID and call(k=None) == PC_E_INVALID
    assert call(p=None, d=None, b=None) == PC_E_INVALID
    assert call(w=0) == PC_E_INVALID and call(h=0) == PC_E_INVALID and call(w=-3) == PC_E_INVALID
    assert call(w=65537) == PC_E_INVALID and call(h=65537) == PC_E_INVALID   # PC_MESH_RENDER_MAX_SIDE, refused before anything is touched
    assert call(margin=-1) == PC_E_INVALID and call(margin=32) == PC_E_INVALID and call(margin=31) == 0
    assert call(b=None, invert=1) == PC_E_INVALID and call(b=None, margin=1) == PC_E_INVALID and call(b=None) == 0
    other = hip.Context(0)
    try:
        assert call(c=other._h) == PC_E_INVALID
        assert b"context" in L.pc_last_error()
    finally:
        other.close()


def test_resources_balance_after_the_mesh_is_destroyed():
    """the scratch planes live with the mesh: a run with a margin and with host pointers allocates all four, destroy frees them"""
    before = hip.live_resources()
    ctx = hip.Context(0)
    m = Mesh((hip.load(), ctx), *mr.soup_mesh())
    cam = _soup_cams(67, 45, 50.0)[0]
    m.render(cam, 67, 45, 1, 1, 5)
    assert hip.live_resources()[0] > before[0]
    m.close()
    ctx.close()
    assert hip.live_resources() == before
