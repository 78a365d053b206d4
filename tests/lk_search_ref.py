"""The search prepass of include/polychase_hip.h (pc_lk_track_search), restated in numpy.  TEST INFRASTRUCTURE ONLY.

Three parts, as in the rule:

    level_radius(R, T)        the level the blocks are matched at and the radius there
    match(I, J, w, h, ...)    the block matching of one keypoint: every candidate's SAD in one vectorised expression, the smallest
                              key (SAD, dx^2 + dy^2, dy, dx), the 25 % acceptance -> d in level-0 pixels
    track_point(..., gx, gy)  tests/lk_normalized_ref.py's canonical track_point (normalize=False) with ONE change: at the top level
                              the search starts at (gx, gy) * lscale instead of at (x, y) * lscale.  With (gx, gy) == (x, y) it must
                              reproduce oracle.lk under canonical emulation bit for bit (tests/test_lk_search_cpu.py), which pins every
                              line the rule did not change.

search() applies them to the forward rows of every target and keeps the better record; backward() is the forward-backward variant:
rows in state 1 are tracked back by track_point from q, started at q - d, every other row by the caller's plain backward pass."""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from lk_normalized_ref import FLT_EPSILON, FLT_SCALE, W_BITS, Planes, _floor, _interp, _isum, _outside, _weights, f32, f64

__all__ = ["Planes", "level_radius", "match", "track_point", "search", "backward", "NONE", "REPLACED", "KEPT"]

NONE, REPLACED, KEPT = 0, 1, 2
BLOCK, MAX_R = 8, 16


def level_radius(R: int, T: int):
    """-> (s, r): s = the smallest level with ceil(R / 2^s) <= 16, clamped to T; r = min(16, ceil(R / 2^s))"""
    s = 0
    while s < T and -(-R // (1 << s)) > MAX_R:
        s += 1
    return s, min(MAX_R, -(-R // (1 << s)))


def block_origin(x, y, s):
    """(ox, oy) of the 8 x 8 template block at level s, or None for a non-finite position"""
    lscale = f32(1.0) / f32(1 << s)
    with np.errstate(over="ignore", invalid="ignore"):
        fx, fy = np.floor(f32(x) * lscale + f32(0.5)), np.floor(f32(y) * lscale + f32(0.5))
    if not (np.isfinite(fx) and np.isfinite(fy)):
        return None
    return int(fx) - 4, int(fy) - 4


def _inside(ox, oy, w, h):
    return 0 <= ox and ox + BLOCK <= w and 0 <= oy and oy + BLOCK <= h


def match(I: np.ndarray, J: np.ndarray, x, y, s: int, r: int):
    """I, J: the INTERIOR u8 planes [h, w] of frame1 and of the target at level s -> (dx, dy) in level-0 pixels, (0, 0) when the
    keypoint is not searched, when the best candidate is the zero displacement or when it is not 25 % better than it"""
    h, w = I.shape
    o = block_origin(x, y, s)
    if o is None or not _inside(o[0], o[1], w, h):
        return 0, 0
    ox, oy = o
    tmpl = I[oy:oy + BLOCK, ox:ox + BLOCK].astype(np.int64)
    dx_lo, dx_hi = max(-r, -ox), min(r, w - BLOCK - ox)
    dy_lo, dy_hi = max(-r, -oy), min(r, h - BLOCK - oy)
    blocks = sliding_window_view(J, (BLOCK, BLOCK))[oy + dy_lo:oy + dy_hi + 1, ox + dx_lo:ox + dx_hi + 1].astype(np.int64)
    sad = np.abs(blocks - tmpl).sum(axis=(2, 3))          # [dy, dx], exact integers <= 16320
    dy, dx = np.meshgrid(np.arange(dy_lo, dy_hi + 1), np.arange(dx_lo, dx_hi + 1), indexing="ij")
    order = np.lexsort((dx.ravel(), dy.ravel(), (dx * dx + dy * dy).ravel(), sad.ravel()))      # the last key is the primary one
    k = order[0]
    best, zero = int(sad.ravel()[k]), int(sad[-dy_lo, -dx_lo])
    if not 4 * best <= 3 * zero:
        return 0, 0
    return int(dx.ravel()[k]) * (1 << s), int(dy.ravel()[k]) * (1 << s)


def track_point(P: Planes, N: Planes, x, y, gx, gy, max_level, max_iters, eps_sq, min_eig_thr, want_err=True):
    """the canonical plain pass, template at (x, y) in P, searched in N, the top level started at (gx, gy) * lscale
    -> (nx, ny) float32, status, err float32"""
    win = P.win
    half = f32(win - 1) * f32(0.5)
    x, y, gx, gy = f32(x), f32(y), f32(gx), f32(gy)
    nx = ny = f32(0.0)
    status, err = True, f32(0.0)
    for level in range(max_level, -1, -1):
        w, h, I, dIx, dIy = P.levels[level]
        J = N.levels[level][2]
        lscale = f32(1.0 / (1 << level))
        px, py = x * lscale, y * lscale
        if level == max_level:
            qx, qy = gx * lscale, gy * lscale          # <- the one change
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
            if want_err:
                diff = _interp(J, win, iex, iey, _weights(ex - f32(iex), ey - f32(iey)), W_BITS - 5) - ival
                err = (f32(_isum(np.abs(diff))) * f32(1.0)) / f32(32 * win * win)
    return nx, ny, status, (err if status else f32(0.0))


def _terms(P, targets, opt):
    T = max(0, min([opt.max_level, P.num_levels - 1] + [N.num_levels - 1 for N in targets]))
    max_iters = min(max(opt.term_max_iters, 0), 100)
    eps = min(max(opt.term_epsilon, 0.0), 10.0)
    return T, max_iters, eps * eps, f32(opt.min_eigen_threshold)


def _interior(planes: Planes, s: int) -> np.ndarray:
    w, h, img = planes.levels[s][:3]
    win = planes.win
    return np.ascontiguousarray(img[win:win + h, win:win + w])


def search(P: Planes, targets, pts, forward, opt, R: int):
    """P: frame1's planes; targets: a list of Planes; pts [N, 2]; forward: per target (next_xy [N, 2], status [N], err [N]), the
    forward launch's rows; opt: an oracle.FlowOptions; R: search_radius, 1..256
    -> per target (next_xy, status, err, search_d [N, 2] int16, search_state [N])"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    T, max_iters, eps_sq, thr = _terms(P, targets, opt)
    s, r = level_radius(R, T)
    I = _interior(P, s)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for N, f in zip(targets, forward):
            xy, st, err = np.array(f[0], np.float32), np.array(f[1], np.uint8), np.array(f[2], np.float32)
            d, state = np.zeros((n, 2), np.int16), np.zeros(n, np.uint8)
            J = _interior(N, s)
            for i, (x, y) in enumerate(pts):
                dx, dy = match(I, J, x, y, s, r)
                if dx == 0 and dy == 0:
                    continue
                d[i] = (dx, dy)
                gx, gy, sg, eg = track_point(P, N, x, y, f32(x) + f32(dx), f32(y) + f32(dy), T, max_iters, eps_sq, thr)
                if sg and (st[i] == 0 or eg < err[i]):
                    xy[i], st[i], err[i], state[i] = (gx, gy), 1, eg, REPLACED
                else:
                    state[i] = KEPT
            out.append((xy, st, err, d, state))
    return out


def backward(P: Planes, N: Planes, pts, row, opt, thr, plain_back):
    """the forward-backward check of one target's rows (next_xy, status, err, search_d, search_state): rows in state 1 with status 1
    are tracked back by track_point from q, started at q - d; the other rows with status 1 by plain_back(q [k, 2]) -> (back_xy,
    back_status), the usual backward pass.  -> (final status, back_xy, back_status)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    xy, st, _, d, state = row
    n = len(pts)
    T, max_iters, eps_sq, mthr = _terms(P, [N], opt)
    bxy, bst = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    usual = np.nonzero((st == 1) & (state != REPLACED))[0]
    if len(usual):
        b, sb = plain_back(xy[usual])
        bxy[usual], bst[usual] = b, sb
    with np.errstate(over="ignore", invalid="ignore"):
        for i in np.nonzero((st == 1) & (state == REPLACED))[0]:
            qx, qy = xy[i]
            bx, by, sb, _ = track_point(N, P, qx, qy, qx - f32(d[i, 0]), qy - f32(d[i, 1]), T, max_iters, eps_sq, mthr, want_err=False)
            bxy[i], bst[i] = (bx, by), int(sb)
        dx, dy = bxy[:, 0] - pts[:, 0], bxy[:, 1] - pts[:, 1]
        d2 = dx * dx + dy * dy
        final = ((st == 1) & (bst == 1) & (d2 <= f32(f64(thr) * f64(thr)))).astype(np.uint8)
    return final, bxy, bst
