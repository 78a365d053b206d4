"""Plain numpy restatement of the mesh render (include/polychase_hip.h: pc_mesh_render; DESIGN.md section 4 "Mesh render") and
the scenes its tests share.  No GPU.

  render       tracker_ref.mt_closest over the pixel grid -- pixel (px, py) casts the ray of xy = (px, py) -- then the triangle
               mask (a masked closest triangle is a miss), the polarity, the erosion
  erode        the choke rule: a square of 2 margin + 1 pixels, pixels outside the frame count as on
  exact_scene  a frame and a quad of dyadic coordinates whose planes are known in closed form
  soup_scene   the 300-triangle soup of tests/test_raycast_edges_gpu.py under its tilted camera, 6 units back
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_ref as tr  # noqa: E402

# the gates of profiles/tracker_raycast_gates.txt: a float64 decision closer to a boundary than this is one float32 cannot tell
GATE_BARY, GATE_T = 4.165e-05, 1.325e-05
MAX_MARGIN = 31


def pixel_grid(w, h):
    """xy [h * w, 2] float32 in row-major pixel order: pixel centres sit at integer coordinates"""
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    return np.stack([px.ravel(), py.ravel()], 1).astype(np.float32)


def grid_rays(dtype, cam, w, h):
    """(origin, dirs) of every pixel as the kernels form them: Unproject, then the rotation into object space"""
    dtype = np.dtype(dtype).type
    xy = pixel_grid(w, h).astype(dtype)
    s = dtype(cam.sign)
    ux, uy = s * ((xy[:, 0] - dtype(cam.cx)) / dtype(cam.fx)), s * ((xy[:, 1] - dtype(cam.cy)) / dtype(cam.fy))
    uz = np.full(len(xy), s, dtype)
    m = np.asarray(cam.R, np.float32).astype(dtype).reshape(3, 3)
    dirs = np.stack([m[k, 0] * ux + m[k, 1] * uy + m[k, 2] * uz for k in range(3)], 1)
    return np.asarray(cam.origin, np.float32).astype(dtype), dirs


def erode(plane, margin):
    """on/off image of `plane` eroded by a (2 margin + 1)-pixel square; outside the frame counts as on.  uint8 255 / 0"""
    on = np.asarray(plane) != 0
    h, w = on.shape
    pad = np.ones((h + 2 * margin, w + 2 * margin), bool)
    pad[margin:margin + h, margin:margin + w] = on
    out = np.ones((h, w), bool)
    for dy in range(2 * margin + 1):
        for dx in range(2 * margin + 1):
            out &= pad[dy:dy + h, dx:dx + w]
    return np.where(out, 255, 0).astype(np.uint8)


def mask_from_hit(hit, invert, margin):
    """steps 2 and 3 of the rule on an (h, w) on/off plane: polarity first, erosion second"""
    on = np.asarray(hit) != 0
    if invert:
        on = ~on
    return erode(on, margin)


def render(dtype, verts, tris, cam, w, h, masked=None, check_mask=False, invert=False, margin=0):
    """(prim int32 (h, w), depth (h, w), mask uint8 (h, w), the mt_closest result with its float64 margins)"""
    r = tr.mt_closest(dtype, verts, tris, *grid_rays(dtype, cam, w, h))
    prim = r.prim.astype(np.int32).reshape(h, w)
    depth = np.where(r.hit, r.t, 0).reshape(h, w)
    on = r.hit.copy()
    if check_mask and masked is not None:
        on &= ~np.asarray(masked, bool)[np.maximum(r.prim, 0)]
    return prim, depth, mask_from_hit(on.reshape(h, w), invert, margin), r


def ambiguous(r64):
    return (r64.m_bary < GATE_BARY) | (r64.m_t < GATE_T)


def camera(R, origin, sign, f, cx, cy):
    """f > 0: with sign = -1 the OpenGL intrinsics are (-f, -f)"""
    return SimpleNamespace(R=np.asarray(R, np.float32).reshape(3, 3), origin=np.asarray(origin, np.float32), sign=float(sign),
                           fx=float(f * sign), fy=float(f * sign), cx=float(cx), cy=float(cy))


def look_at(center, dist, sign, R, f, cx, cy):
    fwd = np.asarray(R, float) @ [0, 0, sign]
    return camera(R, np.asarray(center, float) - dist * fwd, sign, f, cx, cy)


# ---- the exact scene -------------------------------------------------------------------------------------------------------
EXACT_W, EXACT_H = 67, 45
EXACT_RECT = (11, 40, 6, 25)          # mask on exactly for 11 <= px <= 40, 6 <= py <= 25


def exact_scene():
    """Identity camera at the origin, fx = fy = 64, cx = 32, cy = 20; a two-triangle quad at z = 4 whose projection is the
    rectangle x in [10.5, 40.5], y in [5.5, 25.5] (x = 16 X + 32, y = 16 Y + 20).  Every coordinate is dyadic; no pixel centre
    lies within 0.5 px of an outline, nor on the shared diagonal 2 x - 3 y = 4.5 (no integer solution)."""
    x0, x1 = (10.5 - 32) / 16, (40.5 - 32) / 16
    y0, y1 = (5.5 - 20) / 16, (25.5 - 20) / 16
    verts = np.array([[x0, y0, 4], [x1, y0, 4], [x1, y1, 4], [x0, y1, 4]], np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return verts, tris, camera(np.eye(3), [0, 0, 0], 1.0, 64.0, 32.0, 20.0)


def rect_plane(w, h, x_lo, x_hi, y_lo, y_hi, inside=255, outside=0):
    out = np.full((h, w), outside, np.uint8)
    out[y_lo:y_hi + 1, x_lo:x_hi + 1] = inside
    return out


# ---- the soup scenes -------------------------------------------------------------------------------------------------------
SOUP_SCENES = {"67x45": (67, 45, 50.0), "131x70": (131, 70, 100.0)}


def soup_mesh():
    import test_raycast_edges_gpu as edges

    return edges._soup(300, np.random.default_rng(3))


def soup_camera(name, sign=1.0):
    import test_raycast_edges_gpu as edges

    w, h, f = SOUP_SCENES[name]
    return look_at([0, 0, 0], 6.0, sign, edges.R_TILT, f, w // 2, h // 2)


_soup_cache = {}


def soup_reference(name, sign=1.0):
    """(w, h, camera, float64 prim, float64 hit, ambiguous) of a soup scene, planes of shape (h, w); once per process"""
    key = (name, sign)
    if key not in _soup_cache:
        w, h, _ = SOUP_SCENES[name]
        verts, tris = soup_mesh()
        cam = soup_camera(name, sign)
        prim, _, _, r64 = render(np.float64, verts, tris, cam, w, h)
        _soup_cache[key] = (w, h, cam, prim, r64.hit.reshape(h, w), ambiguous(r64).reshape(h, w))
    return _soup_cache[key]
