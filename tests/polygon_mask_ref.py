"""Reference for polygon detection masks: the fill rule of include/polychase_hip.h (pc_frame_set_mask_polygons) restated in
numpy int64, and the named shapes the tests rasterise.

The rule: snap every coordinate to X = rint(x * 16) (float32 multiply, round-half-to-even); with P = (16 px, 16 py) an edge
A -> B is crossed when (Ay <= Py) != (By <= Py) and lies to the right of P when d = (Bx - Ax)(Py - Ay) - (Px - Ax)(By - Ay) is
> 0 for By > Ay, < 0 for By < Ay; a pixel is inside a polygon with an odd number of crossed edges to its right, on when inside
any polygon, flipped by invert; on = 255."""
import numpy as np

MAX_POLYGONS, MAX_VERTICES, SUBPIXEL = 32, 4096, 16


def snap(poly):
    """(K, 2) array-like -> int64 (K, 2) in sixteenths of a pixel; ValueError for what the rule calls an error"""
    p = np.asarray(poly, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 2 or len(p) < 3:
        raise ValueError("a polygon is (K, 2) with K >= 3")
    if not np.all(np.isfinite(p)) or np.any(np.abs(p) > 32768):
        raise ValueError("coordinate not finite or out of range")
    return np.rint(p * np.float32(SUBPIXEL)).astype(np.int64)


def inside(poly, w, h):
    """bool (h, w): the even-odd interior of one polygon by the rule"""
    v = snap(poly)
    px = 16 * np.arange(w, dtype=np.int64)[None, :]
    py = 16 * np.arange(h, dtype=np.int64)
    par = np.zeros((h, w), bool)
    for (ax, ay), (bx, by) in zip(v, np.roll(v, -1, axis=0)):
        rows = np.nonzero((ay <= py) != (by <= py))[0]          # the rows on which the edge is crossed
        if len(rows) == 0:
            continue
        d = (bx - ax) * (py[rows, None] - ay) - (px - ax) * (by - ay)
        par[rows] ^= (d > 0) if by > ay else (d < 0)
    return par


def plane(polys, w, h, invert=False):
    """uint8 (h, w), 255 / 0: the mask plane of a polygon mask"""
    polys = list(polys)
    if len(polys) > MAX_POLYGONS or sum(len(p) for p in polys) > MAX_VERTICES:
        raise ValueError("too many polygons or vertices")
    on = np.zeros((h, w), bool)
    for p in polys:
        on |= inside(p, w, h)
    return np.where(on != bool(invert), 255, 0).astype(np.uint8)


def inside_float64(poly, w, h):
    """an independent crossing test in float64 on the snapped vertices (x of the crossing point against the pixel's x)"""
    v = snap(poly).astype(np.float64) / 16.0
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    par = np.zeros((h, w), bool)
    for (ax, ay), (bx, by) in zip(v, np.roll(v, -1, axis=0)):
        if ay == by:
            continue
        crossed = (ay <= y) != (by <= y)
        xc = ax + (y - ay) * (bx - ax) / (by - ay)
        par ^= crossed & (xc > x)
    return par


# ---- shapes: name -> f(w, h) -> list of (K, 2) float32 arrays ----
def _f32(points):
    return np.asarray(points, dtype=np.float32)


def triangle(w, h):
    return [_f32([(0.13 * w + 0.3, 0.1 * h + 0.7), (0.9 * w - 0.45, 0.45 * h + 0.2), (0.3 * w + 0.15, 0.93 * h - 0.6)])]


def star(w, h):
    """concave, 10 vertices, about a third of the frame"""
    a = np.pi * np.arange(10) / 5 + 0.1
    r = np.where(np.arange(10) % 2 == 0, 0.48, 0.2) * min(w, h)
    return [_f32(np.stack([w / 2 + 0.37 + 1.3 * r * np.cos(a), h / 2 - 0.21 + r * np.sin(a)], axis=1))]


def bow_tie(w, h):
    return [_f32([(0.1 * w, 0.1 * h), (0.9 * w, 0.9 * h), (0.9 * w, 0.1 * h), (0.1 * w, 0.9 * h)])]


def across_borders(w, h):
    """a diamond that leaves the frame through all four borders"""
    return [_f32([(0.5 * w, -0.3 * h), (1.2 * w, 0.5 * h), (0.5 * w, 1.3 * h), (-0.2 * w, 0.5 * h)])]


def rectangle(w, h):
    return [_f32([(10, 5), (20, 5), (20, 15), (10, 15)])]


def quads32(w, h):
    rng = np.random.default_rng(32)
    out = []
    for _ in range(32):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        s = rng.uniform(3, 0.2 * min(w, h))
        out.append(_f32([(cx - s, cy - 0.6 * s), (cx + 0.8 * s, cy - s), (cx + s, cy + 0.7 * s), (cx - 0.9 * s, cy + s)]))
    return out


def circle4096(w, h):
    a = 2 * np.pi * np.arange(4096) / 4096
    r = 0.4 * min(w, h)
    return [_f32(np.stack([w / 2 + 0.3 + r * np.cos(a), h / 2 - 0.2 + r * np.sin(a)], axis=1))]


def closing_and_horizontal(w, h):
    """the closing vertex repeated (a zero-length edge) and horizontal edges through pixel centres"""
    return [_f32([(5, 7), (30, 7), (30, 20.5), (5, 20.5), (5, 7)])]


def sub_pixel(w, h):
    return [_f32([(10.1, 10.1), (10.9, 10.2), (10.5, 10.9)])]


def empty(w, h):
    return []


def ties(w, h):
    """coordinates whose sixteenths end in .5: 160.5 -> 160 and 48.5 -> 48 keep column 10 and row 3 in, 641.5 -> 642"""
    return [_f32([(10.03125, 3.03125), (40.09375, 3.03125), (40.09375, 20.03125), (10.03125, 20.03125)])]


def comb(w, h):
    """1100 teeth-edges that each span every row: every workgroup keeps more edges than its LDS list holds at once"""
    n = 1100
    x = np.linspace(-3.3, w + 2.7, n)
    y = np.where(np.arange(n) % 2 == 0, -4.5, h + 3.25)
    return [_f32(np.stack([x, y], axis=1))]


def two_combs(w, h):
    """two such polygons one after the other: the list is emptied in the middle of a polygon and between polygons"""
    a = comb(w, h)[0]
    b = a.copy()
    b[:, 0] = b[:, 0] * 0.5 + 0.31 * w
    return [a[:700], b[:600]]


def outside(w, h):
    return [_f32([(w + 10, 5), (w + 50, 5), (w + 30, 40)]), _f32([(-40, -30), (-5, -20), (-20, -2.5)]), _f32([(3, h + 2), (40, h + 9), (9, h + 30)])]


def degenerate(w, h):
    return [_f32([(3, 3), (9, 9), (6, 6)]), _f32([(4, 4), (4, 4), (4, 4)]), _f32([(2, 8), (12, 8), (7, 8)])]


def frame_covering(w, h):
    return [_f32([(-1, -1), (w + 1, -1), (w + 1, h + 1), (-1, h + 1)])]


# the shapes of the GPU plane test
SHAPES = {"triangle": triangle, "star": star, "bow_tie": bow_tie, "across_borders": across_borders, "rectangle": rectangle,
          "quads32": quads32, "circle4096": circle4096, "closing_and_horizontal": closing_and_horizontal, "sub_pixel": sub_pixel,
          "empty": empty, "ties": ties, "comb": comb, "two_combs": two_combs}
# shapes that turn nothing on / everything on
NOTHING = {"sub_pixel": sub_pixel, "outside": outside, "degenerate": degenerate, "empty": empty}
EVERYTHING = {"frame_covering": frame_covering}


def moving(fid, w, h):
    """a pentagon with fractional vertices that moves with the frame; frame 4 has no mask (None), frame 9 an empty one"""
    if fid == 4:
        return None
    if fid == 9:
        return []
    a = 2 * np.pi * np.arange(5) / 5 + 0.3 * fid
    return [_f32(np.stack([60.3 + 15.25 * fid + 70 * np.cos(a), 55.7 + 6.5 * fid + 60 * np.sin(a)], axis=1))]
