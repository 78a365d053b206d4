"""The masked-window rule of include/polychase_hip.h (pc_lk_track_window_masked), restated in numpy.  TEST INFRASTRUCTURE ONLY.

weight_pyramid() builds the planes W_l of a mask: M_0 = on; M_l = the AND of the 5 x 5 pixels of M_{l-1} that pyrDown read, through
the BORDER_REFLECT_101 index map; W_l = the AND of M_l over the Scharr support, with everything outside the level on.

track_point() is oracle/pc_oracle.c's pco_lk, one point at a time and vectorised over the window, on the oracle's own padded planes
(the helpers are those of tests/lk_normalized_ref.py), in EITHER accumulation order:

    canonical   every sum an exact integer, rounded to fp32 once
    x86         the fp32 lane sums of OpenCV's SSE path as lk_plain.hpp states them: vector lane c < 4 owns columns c, c + 4, ..
                below SIMD_W = (win / 8) * 8, row by row -- in the b sums the products of columns (c, c + 4) of a block of 8 are
                added as integers first --, a scalar accumulator owns the columns from SIMD_W on; the A sums combine as
                s + (((q0 + q1) + q2) + q3), the b sums as s + ((q0 + q2) + (q1 + q3))

and with `weights` (the template image's planes) the four changes of the rule:

    1. ix and iy of an off sample are 0 (a sample is on iff its four taps are on in W_l); ival is kept
    2. 4 * n_on < win * win: the level fails like the min-eig test
    3. the min-eig divisor is f32(2 * n_on)
    4. the level-0 patch error sums |diff| over the on samples and divides by f32(32 * n_on)

Without weights, and with all-on weights, it must reproduce oracle.lk bit for bit under both emulations
(tests/test_lk_window_mask_cpu.py), which pins every line the rule did not change."""
from __future__ import annotations

import numpy as np

from lk_normalized_ref import FLT_EPSILON, FLT_SCALE, W_BITS, Planes, _floor, _interp, _outside, _weights, f32, f64  # noqa: F401


def level_sizes(w, h, win, max_level):
    """buildOpticalFlowPyramid's levels: it stops where the next level would be <= the window"""
    out = [(w, h)]
    while len(out) <= max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            break
        out.append((w, h))
    return out


def _reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def weight_pyramid(mask, win, sizes):
    """mask: (H, W) bytes, non-zero = on; sizes: [(w_l, h_l)] -> [W_l with its padding, bool (h_l + 2 win, w_l + 2 win)]"""
    M = np.asarray(mask) != 0
    assert M.shape == (sizes[0][1], sizes[0][0])
    out = []
    for l, (w, h) in enumerate(sizes):
        if l > 0:
            pw, ph = sizes[l - 1]
            xi = np.array([[_reflect101(2 * x + d, pw) for d in range(-2, 3)] for x in range(w)])
            yi = np.array([[_reflect101(2 * y + d, ph) for d in range(-2, 3)] for y in range(h)])
            Mn = np.ones((h, w), bool)
            for dy in range(5):
                for dx in range(5):
                    Mn &= M[yi[:, dy]][:, xi[:, dx]]
            M = Mn
        Pd = np.pad(M, 1, constant_values=True)
        W = np.ones((h, w), bool)
        for dy in range(3):
            for dx in range(3):
                W &= Pd[dy:dy + h, dx:dx + w]
        out.append(np.pad(W, win, constant_values=True))
    return out


def _sample_on(Wl, win, ipx, ipy):
    """the on flags of the win x win samples of the window whose first tap is interior pixel (ipx, ipy)"""
    s = Wl[ipy + win:ipy + 2 * win + 1, ipx + win:ipx + 2 * win + 1]
    return s[:-1, :-1] & s[:-1, 1:] & s[1:, :-1] & s[1:, 1:]


def _seq(v):
    """q = 0; q += v[0]; q += v[1]; ... in fp32, along axis 0"""
    v = np.asarray(v, f32)
    if v.shape[0] == 0:
        return np.zeros(v.shape[1:], f32)
    return np.add.accumulate(v, axis=0, dtype=f32)[-1]


def _x86_A(p, win):
    """p: the integer products of the window, [win, win] -> the fp32 sum in the lane order of the A sums"""
    sw = (win // 8) * 8
    q = _seq(p[:, :sw].astype(f32).reshape(win * (sw // 4), 4)) if sw else np.zeros(4, f32)
    s = _seq(p[:, sw:].astype(f32).reshape(-1))
    return s + (((q[0] + q[1]) + q[2]) + q[3])


def _x86_b(p, win):
    """... of the b sums: the products of columns (c, c + 4) of a block of 8 are added as integers before the conversion"""
    sw = (win // 8) * 8
    if sw:
        blk = p[:, :sw].reshape(win, sw // 8, 8)
        q = _seq((blk[:, :, :4] + blk[:, :, 4:]).astype(f32).reshape(win * (sw // 8), 4))
    else:
        q = np.zeros(4, f32)
    s = _seq(p[:, sw:].astype(f32).reshape(-1))
    return s + ((q[0] + q[2]) + (q[1] + q[3]))


def _isum(a):
    return int(a.sum())


def track_point(P: Planes, N: Planes, x, y, max_level, max_iters, eps_sq, min_eig_thr, weights=None, x86=False):
    """-> (nx, ny) float32, status, err float32, touched"""
    win = P.win
    half = f32(win - 1) * f32(0.5)
    x, y = f32(x), f32(y)
    nx = ny = f32(0.0)
    status, err, touched = True, f32(0.0), False
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
        n_on = win * win
        on = None
        if weights is not None:
            on = _sample_on(weights[level], win, ipx, ipy)
            touched = touched or not on.all()
            ix, iy = ix * on, iy * on                                   # (1)
            n_on = int(on.sum())
        if x86:
            A11, A12, A22 = (_x86_A(p, win) * FLT_SCALE for p in (ix * ix, ix * iy, iy * iy))
        else:
            A11, A12, A22 = (f32(_isum(p)) * FLT_SCALE for p in (ix * ix, ix * iy, iy * iy))
        if 4 * n_on < win * win:                                        # (2)
            if level == 0:
                status = False
            continue
        D = A11 * A22 - A12 * A12
        tdiff = A11 - A22
        min_eig = (A22 + A11 - np.sqrt(tdiff * tdiff + f32(4.0) * A12 * A12)) / f32(2 * n_on)   # (3)
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
            diff = _interp(J, win, iqx, iqy, _weights(qx - f32(iqx), qy - f32(iqy)), W_BITS - 5) - ival
            if x86:
                b1, b2 = _x86_b(diff * ix, win) * FLT_SCALE, _x86_b(diff * iy, win) * FLT_SCALE
            else:
                b1, b2 = f32(_isum(diff * ix)) * FLT_SCALE, f32(_isum(diff * iy)) * FLT_SCALE
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
            if on is not None:
                diff = diff * on                                        # (4)
            err = (f32(_isum(np.abs(diff))) * f32(1.0)) / f32(32 * n_on)
    return nx, ny, status, (err if status else f32(0.0)), touched


def _criteria(P, N, opt):
    max_level = max(0, min(opt.max_level, P.num_levels - 1, N.num_levels - 1))
    max_iters = min(max(opt.term_max_iters, 0), 100)
    eps = min(max(opt.term_epsilon, 0.0), 10.0)
    return max_level, max_iters, eps * eps, f32(opt.min_eigen_threshold)


def track(P: Planes, N: Planes, pts, opt, weights=None, x86=False, only=None):
    """calcOpticalFlowPyrLK(prev = P, next = N, pts) under the rule -> next_xy [n, 2] float32, status uint8, err float32, touched
    uint8; `opt`: an oracle.FlowOptions (the window is the planes' padding); weights: weight_pyramid() of P's mask, or None; only: a
    boolean mask, the other rows stay zero and are not tracked"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    crit = _criteria(P, N, opt)
    n = len(pts)
    xy, st, err, tch = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, (x, y) in enumerate(pts):
            if only is not None and not only[i]:
                continue
            nx, ny, s, e, t = track_point(P, N, x, y, *crit, weights=weights, x86=x86)
            xy[i], st[i], err[i], tch[i] = (nx, ny), int(s), e, int(t)
    return xy, st, err, tch


def forward_backward(P: Planes, N: Planes, pts, opt, thr, weights_p=None, weights_n=None, x86=False, forward=None):
    """the forward-backward check (include/polychase_hip.h: pc_lk_track_fb) with each pass under the weights of its template image
    -> next_xy, final status, err, back_xy, back_status; forward: the forward pass's (next_xy, status, err) when it is known"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    xy, st, err = forward if forward is not None else track(P, N, pts, opt, weights_p, x86)[:3]
    bxy, bst, _, _ = track(N, P, xy, opt, weights_n, x86, only=st == 1)
    dx, dy = bxy[:, 0] - pts[:, 0], bxy[:, 1] - pts[:, 1]
    d2 = dx * dx + dy * dy
    thr2 = f32(f64(thr) * f64(thr))
    with np.errstate(invalid="ignore"):
        final = ((st == 1) & (bst == 1) & (d2 <= thr2)).astype(np.uint8)
    return xy, final, err, bxy, bst
