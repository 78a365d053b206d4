"""The affine refinement rule of include/polychase_hip.h (pc_lk_track_affine), restated in numpy.  TEST INFRASTRUCTURE ONLY.

A forward record (keypoint p, stored float32 end point q, patch error err, status 1) is refined at level 0 under a 6-parameter
warp of the window: pixel (c, r) of the template at p - half is compared with the target at
    (cx + m11 u + m12 v, cy + m21 u + m22 v),   u = c - half, v = r - half,
starting from (cx, cy) = q and m = identity.  Gauss-Newton on J - I with the 6 x 6 matrix H = sum g g^T of the template,
g = (ix U, ix V, iy U, iy V, ix, iy), U = 2c - (win - 1), V = 2r - (win - 1): every sum an exact Python integer, the Cholesky factor
and the two triangular solves in float64, the state in float32, every operation rounded on its own.  The template, the bilinear
weights and the interpolation are tests/lk_normalized_ref.py's (oracle/pc_oracle.c's), so the final evaluation at the identity is
the oracle's patch error.  The refined (cx, cy, err_a) replaces (q, err) iff err_a <= err and the warp stayed near the identity;
otherwise the record stays as it was, bit for bit.  The status never changes."""
from __future__ import annotations

import math

import numpy as np

import lk_normalized_ref as nref
from lk_normalized_ref import Planes, W_BITS, f32, f64

NOT_RUN, ACCEPTED, UNCHANGED = 0, 1, 2


class Template:
    """what a keypoint's level-0 template leaves for its rows: ival, the six columns of g, and the factor L (or None: s <= 0)"""

    def __init__(self, P: Planes, x, y):
        win = P.win
        w, h, I, dIx, dIy = P.levels[0]
        half = f32(win - 1) * f32(0.5)
        px, py = f32(x) - half, f32(y) - half
        ipx, ipy = nref._floor(px), nref._floor(py)
        self.ok = not nref._outside(ipx, ipy, w, h, win)
        self.L = None
        if not self.ok:
            return
        wI = nref._weights(px - f32(ipx), py - f32(ipy))
        self.ival = nref._interp(I, win, ipx, ipy, wI, W_BITS - 5)
        ix = nref._interp(dIx, win, ipx, ipy, wI, W_BITS)
        iy = nref._interp(dIy, win, ipx, ipy, wI, W_BITS)
        U = (2 * np.arange(win, dtype=np.int64) - (win - 1))[None, :] + np.zeros((win, 1), np.int64)      # [r, c]: columns
        V = U.T
        self.U, self.V = U, V
        self.g = [ix * U, ix * V, iy * U, iy * V, ix, iy]
        H = [[int((self.g[i] * self.g[j]).sum()) for j in range(6)] for i in range(6)]
        assert max(abs(v) for row in H for v in row) < 1 << 53
        self.H = H
        self.L = _cholesky(H)


def _cholesky(H):
    """lower Cholesky of float64(H), column by column; None unless every pivot's s > 0"""
    L = [[f64(0.0)] * 6 for _ in range(6)]
    for j in range(6):
        s = f64(H[j][j])
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0:
            return None
        L[j][j] = f64(math.sqrt(s))
        for i in range(j + 1, 6):
            s = f64(H[i][j])
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    return L


def _solve(L, b):
    """t with L L^T t = -b"""
    y = [f64(0.0)] * 6
    for i in range(6):
        s = -f64(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    t = [f64(0.0)] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * t[k]
        t[i] = s / L[i][i]
    return t


def warped_window(Jplane, w, h, win, U, V, cx, cy, m):
    """int64 (win, win) values of the target's padded level-0 plane under the warp, or None when a pixel fails the bounds test"""
    u, v = U.astype(np.float32) * f32(0.5), V.astype(np.float32) * f32(0.5)
    xj = (cx + m[0] * u) + m[1] * v
    yj = (cy + m[2] * u) + m[3] * v
    fx, fy = np.floor(xj), np.floor(yj)
    ok = (fx >= -win) & (fx <= w + win - 2) & (fy >= -win) & (fy <= h + win - 2)       # a NaN fails
    if not ok.all():
        return None
    a, b = xj - fx, yj - fy
    one, s = f32(1.0), f32(1 << W_BITS)
    w00 = np.rint((one - a) * (one - b) * s).astype(np.int64)
    w01 = np.rint(a * (one - b) * s).astype(np.int64)
    w10 = np.rint((one - a) * b * s).astype(np.int64)
    w11 = (1 << W_BITS) - w00 - w01 - w10
    X, Y = fx.astype(np.int64) + win, fy.astype(np.int64) + win
    val = Jplane[Y, X] * w00 + Jplane[Y, X + 1] * w01 + Jplane[Y + 1, X] * w10 + Jplane[Y + 1, X + 1] * w11
    return (val + (1 << (W_BITS - 5 - 1))) >> (W_BITS - 5)


def refine_row(T: Template, N: Planes, q, err, max_iters, eps):
    """one row -> (x, y, err, m [4], state); T.ok and T.L is not None"""
    win = N.win
    w, h, J = N.levels[0][:3]
    half = f32(win - 1) * f32(0.5)
    qx, qy, err = f32(q[0]), f32(q[1]), f32(err)
    cx, cy = qx, qy
    m = [f32(1.0), f32(0.0), f32(0.0), f32(1.0)]

    def unchanged():      # the record as it was; affine_m reports the matrix the refinement ended with
        return qx, qy, err, np.array(m, np.float32), UNCHANGED

    eps2 = f64(eps) * f64(eps)
    scale = f64((win - 1) * (win - 1))
    for _ in range(max_iters):
        jv = warped_window(J, w, h, win, T.U, T.V, cx, cy, m)
        if jv is None:
            return unchanged()
        e = jv - T.ival
        b = [int((e * g).sum()) for g in T.g]
        t = _solve(T.L, b)
        for k in range(4):
            m[k] = m[k] + f32(f64(2.0) * t[k])
        cx, cy = cx + f32(t[4]), cy + f32(t[5])
        if (t[4] * t[4] + t[5] * t[5]) + scale * (((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + t[3] * t[3]) <= eps2:
            break
    jv = warped_window(J, w, h, win, T.U, T.V, cx, cy, m)
    if jv is None:
        return unchanged()
    err_a = f32(int(np.abs(jv - T.ival).sum())) / f32(32 * win * win)
    det = m[0] * m[3] - m[1] * m[2]
    dx, dy = cx - qx, cy - qy
    accept = (err_a <= err and f32(0.5) <= det <= f32(2.0)
              and abs(m[0] - f32(1.0)) <= f32(0.5) and abs(m[1]) <= f32(0.5) and abs(m[2]) <= f32(0.5) and abs(m[3] - f32(1.0)) <= f32(0.5)
              and dx * dx + dy * dy <= half * half)
    if not accept:
        return unchanged()
    return cx, cy, err_a, np.array(m, np.float32), ACCEPTED


def refine(P: Planes, targets, pts, forward, opt):
    """P: frame1's planes; targets: a list of Planes; pts [N, 2]; forward: per target (next_xy [N, 2], status [N], err [N]); opt: an
    oracle.FlowOptions -> per target (next_xy, status, err, affine_m [N, 4], affine_state [N]).  The template and its factor are
    evaluated once per keypoint."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    max_iters = min(max(opt.term_max_iters, 0), 100)
    eps = min(max(opt.term_epsilon, 0.0), 10.0)
    n = len(pts)
    out = [(np.array(f[0], np.float32), np.array(f[1], np.uint8), np.array(f[2], np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.uint8))
           for f in forward]
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            if not any(o[1][i] == 1 for o in out):
                continue
            T = Template(P, pts[i, 0], pts[i, 1])
            for N, (xy, st, err, m, state) in zip(targets, out):
                if st[i] != 1:
                    continue
                if not T.ok or T.L is None:
                    m[i], state[i] = (1.0, 0.0, 0.0, 1.0), UNCHANGED
                    continue
                x, y, e, mm, s = refine_row(T, N, xy[i], err[i], max_iters, eps)
                xy[i], err[i], m[i], state[i] = (x, y), e, mm, s
    return out
