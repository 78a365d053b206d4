"""The brightness-normalised LK rule of include/polychase_hip.h (pc_lk_track_normalized), restated in numpy.  TEST INFRASTRUCTURE
ONLY.

track() is oracle/pc_oracle.c's lk_range (OpenCV's LKTrackerInvoker, canonical accumulation) on the oracle's own padded image and
derivative planes, one point at a time and vectorised over the window: the bounds tests, the 14-bit bilinear weights, the template
values ival / ix / iy, the interpolation of the searched plane, the 2x2 solve, the epsilon test, the oscillation exit and the
level-0 L1 patch error are that file's float32 / integer expressions, each operation rounded on its own.  With normalize=True two
lines change (n = win * win, all sums exact Python integers, every float64 operation rounded on its own):

    template, per level   S_I, S_II, S_x, S_y, S_xx, S_xy, S_yy, S_Ix, S_Iy over the window (x = ix, y = iy, I = ival)
                          A11 = f32(f64(n S_xx - S_x^2) / f64(n)) * FLT_SCALE, A12 and A22 likewise   (plain: f32(S_xx) * FLT_SCALE)
    each iteration        T_J, T_JJ, T_Jx, T_Jy over the J window; vI = n S_II - S_I^2, vJ = n T_JJ - T_J^2
                          g = f32(sqrt(f64(vI) / f64(vJ))) clamped to [0.25, 4] when vI > 0 and vJ > 0, else 1
                          b1 = f32((f64(g) f64(n T_Jx - T_J S_x) - f64(n S_Ix - S_I S_x)) / f64(n)) * FLT_SCALE, b2 likewise
                          (plain: f32(sum (J - I) ix) * FLT_SCALE)

With normalize=False it must reproduce oracle.lk under canonical emulation bit for bit (tests/test_lk_normalized_cpu.py), which
pins every line the rule did not change."""
from __future__ import annotations

import math

import numpy as np

W_BITS = 14
f32, f64 = np.float32, np.float64
FLT_SCALE = f32(1.0) / f32(1 << 20)
FLT_EPSILON = f32(1.1920928955078125e-07)


class Planes:
    """the padded int64 planes of an oracle.Pyramid, level by level: (w, h, img [h + 2 win, w + 2 win], ix, iy)"""

    def __init__(self, pyr):
        self.win = pyr.win
        self.levels = []
        for l in range(pyr.num_levels):
            w, h = pyr.level_size(l)
            d = pyr.deriv(l).astype(np.int64)
            self.levels.append((w, h, pyr.image(l).astype(np.int64), np.ascontiguousarray(d[:, :, 0]), np.ascontiguousarray(d[:, :, 1])))
        self.num_levels = len(self.levels)


def _weights(a, b):
    one, s = f32(1.0), f32(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * s))      # lrintf: to nearest, ties to even
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _interp(plane, win, ix, iy, wts, bits):
    """DESCALE(., bits) of the bilinear taps of the win x win window whose first tap is interior pixel (ix, iy)"""
    s = plane[iy + win:iy + 2 * win + 1, ix + win:ix + 2 * win + 1]
    v = s[:-1, :-1] * wts[0] + s[:-1, 1:] * wts[1] + s[1:, :-1] * wts[2] + s[1:, 1:] * wts[3]
    return (v + (1 << (bits - 1))) >> bits


def _floor(v):
    return int(np.floor(v)) if np.isfinite(v) else (1 << 31) - 1      # (the device's conversion saturates; fails every bounds test)


def _outside(ix, iy, w, h, win):
    return ix < -win or ix >= w or iy < -win or iy >= h


def _isum(a):
    return int(a.sum())


def track_point(P: Planes, N: Planes, x, y, max_level, max_iters, eps_sq, min_eig_thr, normalize):
    """-> (nx, ny) float32, status, err float32"""
    win = P.win
    n = win * win
    half = f32(win - 1) * f32(0.5)
    x, y = f32(x), f32(y)
    nx = ny = f32(0.0)
    status, err = True, f32(0.0)
    for level in range(max_level, -1, -1):
        w, h, I, dIx, dIy = P.levels[level]
        J = N.levels[level][2]
        lscale = f32(1.0 / (1 << level))
        px, py = x * lscale, y * lscale
        if level == max_level:
            qx, qy = px, py
        else:
            qx, qy = nx * f32(2.0), ny * f32(2.0)
        nx, ny = qx, qy
        px, py = px - half, py - half
        ipx, ipy = _floor(px), _floor(py)
        if _outside(ipx, ipy, w, h, win):
            if level == 0:
                status = False
            continue
        wI = _weights(px - f32(ipx), py - f32(ipy))
        ival = _interp(I, win, ipx, ipy, wI, W_BITS - 5)
        ix = _interp(dIx, win, ipx, ipy, wI, W_BITS)
        iy = _interp(dIy, win, ipx, ipy, wI, W_BITS)
        if normalize:
            S_I, S_II, S_x, S_y = _isum(ival), _isum(ival * ival), _isum(ix), _isum(iy)
            S_Ix, S_Iy = _isum(ival * ix), _isum(ival * iy)
            G11, G12, G22 = n * _isum(ix * ix) - S_x * S_x, n * _isum(ix * iy) - S_x * S_y, n * _isum(iy * iy) - S_y * S_y
            C_Ix, C_Iy, vI = n * S_Ix - S_I * S_x, n * S_Iy - S_I * S_y, n * S_II - S_I * S_I
            assert max(abs(v) for v in (G11, G12, G22, C_Ix, C_Iy, vI)) < 1 << 53
            A11 = f32(f64(G11) / f64(n)) * FLT_SCALE
            A12 = f32(f64(G12) / f64(n)) * FLT_SCALE
            A22 = f32(f64(G22) / f64(n)) * FLT_SCALE
        else:
            A11 = f32(_isum(ix * ix)) * FLT_SCALE
            A12 = f32(_isum(ix * iy)) * FLT_SCALE
            A22 = f32(_isum(iy * iy)) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        tdiff = A11 - A22
        min_eig = (A22 + A11 - np.sqrt(tdiff * tdiff + f32(4.0) * A12 * A12)) / f32(2 * win * win)
        if min_eig < min_eig_thr or D < FLT_EPSILON:
            if level == 0:
                status = False
            continue
        D = f32(1.0) / D

        qx, qy = qx - half, qy - half
        pdx = pdy = f32(0.0)
        for j in range(max_iters):
            iqx, iqy = _floor(qx), _floor(qy)
            if _outside(iqx, iqy, w, h, win):
                if level == 0:
                    status = False
                break
            jv = _interp(J, win, iqx, iqy, _weights(qx - f32(iqx), qy - f32(iqy)), W_BITS - 5)
            if normalize:
                T_J, T_JJ, T_Jx, T_Jy = _isum(jv), _isum(jv * jv), _isum(jv * ix), _isum(jv * iy)
                vJ, C_Jx, C_Jy = n * T_JJ - T_J * T_J, n * T_Jx - T_J * S_x, n * T_Jy - T_J * S_y
                g = f32(1.0)
                if vI > 0 and vJ > 0:
                    g = min(max(f32(np.sqrt(f64(vI) / f64(vJ))), f32(0.25)), f32(4.0))
                b1 = f32((f64(g) * f64(C_Jx) - f64(C_Ix)) / f64(n)) * FLT_SCALE
                b2 = f32((f64(g) * f64(C_Jy) - f64(C_Iy)) / f64(n)) * FLT_SCALE
            else:
                diff = jv - ival
                b1 = f32(_isum(diff * ix)) * FLT_SCALE
                b2 = f32(_isum(diff * iy)) * FLT_SCALE
            dx = (A12 * b2 - A22 * b1) * D
            dy = (A12 * b1 - A11 * b2) * D
            qx, qy = qx + dx, qy + dy
            nx, ny = qx + half, qy + half
            if f64(dx) * f64(dx) + f64(dy) * f64(dy) <= eps_sq:
                break
            if j > 0 and abs(f64(dx + pdx)) < 0.01 and abs(f64(dy + pdy)) < 0.01:
                nx, ny = nx - dx * f32(0.5), ny - dy * f32(0.5)
                break
            pdx, pdy = dx, dy

        if status and level == 0:
            ex, ey = nx - half, ny - half
            iex, iey = _floor(ex), _floor(ey)
            if _outside(iex, iey, w, h, win):
                status = False
                continue
            diff = _interp(J, win, iex, iey, _weights(ex - f32(iex), ey - f32(iey)), W_BITS - 5) - ival
            err = (f32(_isum(np.abs(diff))) * f32(1.0)) / f32(32 * win * win)
    return nx, ny, status, (err if status else f32(0.0))


def track(P: Planes, N: Planes, pts, opt, normalize=True, only=None):
    """calcOpticalFlowPyrLK(prev = P, next = N, pts) under the rule -> next_xy [n, 2] float32, status uint8, err float32; `opt`: an
    oracle.FlowOptions (the window is the planes' padding); only: a boolean mask, the other rows stay zero and are not tracked"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    max_level = max(0, min(opt.max_level, P.num_levels - 1, N.num_levels - 1))
    max_iters = min(max(opt.term_max_iters, 0), 100)
    eps = min(max(opt.term_epsilon, 0.0), 10.0)
    thr = f32(opt.min_eigen_threshold)
    xy, st, err = np.zeros((len(pts), 2), np.float32), np.zeros(len(pts), np.uint8), np.zeros(len(pts), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, (x, y) in enumerate(pts):
            if only is not None and not only[i]:
                continue
            nx, ny, s, e = track_point(P, N, x, y, max_level, max_iters, eps * eps, thr, normalize)
            xy[i], st[i], err[i] = (nx, ny), int(s), e
    return xy, st, err


def forward_backward(P: Planes, N: Planes, pts, opt, thr, normalize=True, forward=None):
    """the forward-backward check (include/polychase_hip.h: pc_lk_track_fb) with both passes under the rule -> next_xy, final status,
    err, back_xy, back_status; forward: the forward pass's (next_xy, status, err) when it is already known"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    xy, st, err = forward if forward is not None else track(P, N, pts, opt, normalize)
    bxy, bst, _ = track(N, P, xy, opt, normalize, only=st == 1)
    dx, dy = bxy[:, 0] - pts[:, 0], bxy[:, 1] - pts[:, 1]
    d2 = dx * dx + dy * dy
    thr2 = f32(f64(thr) * f64(thr))
    with np.errstate(invalid="ignore"):
        final = ((st == 1) & (bst == 1) & (d2 <= thr2)).astype(np.uint8)
    return xy, final, err, bxy, bst
