"""CPU: the masked-window rule restated in numpy (tests/lk_window_mask_ref.py) -- pinned to the oracle where the rule changes
nothing, its weight pyramid on hand-checkable masks, and its effect on the two-layer scene."""
import numpy as np
import pytest

import lk_window_mask_ref as ref
import lk_window_mask_scene as scene
import oracle

MODES = {"canonical": (oracle.EMU_CANONICAL, False), "x86": (oracle.EMU_LK_SIMD, True)}


@pytest.fixture(scope="module")
def pair():
    (g0, g1), _ = scene.frames()
    return g0[:119, :161].copy(), g1[:119, :161].copy()      # odd sizes


def _points(w, h):
    rs = np.random.RandomState(3)
    inside = np.stack([rs.uniform(0, w - 1, 24), rs.uniform(0, h - 1, 24)], axis=1)
    edge = [(0.0, 0.0), (w - 1.0, h - 1.0), (0.37, h - 1.2), (w - 0.6, 2.25), (1.5, 1.5), (w / 2 + 0.5, 0.25)]
    outside = [(-3.5, 10.25), (w + 4.2, 20.0), (30.5, -6.75), (40.0, h + 2.5), (-40.0, -40.0), (w + 60.0, h / 2)]
    return np.concatenate([inside, np.array(edge), np.array(outside)]).astype(np.float32)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("win", [3, 8, 10, 21])
def test_restatement_is_the_oracle_without_a_mask_and_under_an_all_on_mask(pair, win, mode):
    emu, x86 = MODES[mode]
    g0, g1 = pair
    h, w = g0.shape
    pts = _points(w, h)
    opt = oracle.flow_options(window_size=win, max_level=3)
    with oracle.emulation(emu):
        p0, p1 = oracle.Pyramid(g0, win, 3), oracle.Pyramid(g1, win, 3)
        want = oracle.lk(p0, p1, pts, opt)
    P, N = ref.Planes(p0), ref.Planes(p1)
    sizes = [p0.level_size(l) for l in range(p0.num_levels)]
    all_on = ref.weight_pyramid(np.full((h, w), 255, np.uint8), win, sizes)
    for weights in (None, all_on):
        xy, st, err, touched = ref.track(P, N, pts, opt, weights=weights, x86=x86)
        assert np.array_equal(st, want[1])
        assert st.sum() >= 20 and (st == 0).sum() >= 2, "the points must exercise both outcomes"   # (-40, -40) and (w + 60, .) at least
        assert np.array_equal(xy.view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(err.view(np.uint32), want[2].view(np.uint32))
        assert not touched.any()


# ---- the weight pyramid ----

def _brute_force(mask, win, sizes):
    """the definition, pixel by pixel"""
    M = [np.asarray(mask) != 0]
    for l in range(1, len(sizes)):
        (w, h), (pw, ph) = sizes[l], sizes[l - 1]
        m = np.ones((h, w), bool)
        for y in range(h):
            for x in range(w):
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        yy, xx = 2 * y + dy, 2 * x + dx
                        yy = -yy if yy < 0 else (2 * (ph - 1) - yy if yy >= ph else yy)      # BORDER_REFLECT_101, one reflection
                        xx = -xx if xx < 0 else (2 * (pw - 1) - xx if xx >= pw else xx)
                        m[y, x] &= M[l - 1][yy, xx]
        M.append(m)
    out = []
    for (w, h), m in zip(sizes, M):
        W = np.ones((h + 2 * win, w + 2 * win), bool)
        for y in range(h):
            for x in range(w):
                W[y + win, x + win] = m[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].all()
        out.append(W)
    return out


def _off_box(shape, win, x0, x1, y0, y1):
    """all on but the interior pixels x0..x1, y0..y1 (clipped to the level)"""
    h, w = shape[0] - 2 * win, shape[1] - 2 * win
    W = np.ones(shape, bool)
    W[win + max(y0, 0):win + min(y1, h - 1) + 1, win + max(x0, 0):win + min(x1, w - 1) + 1] = False
    return W


def test_weight_pyramid_of_one_off_pixel():
    win, sizes = 5, ref.level_sizes(40, 30, 5, 2)
    assert sizes == [(40, 30), (20, 15), (10, 8)]
    mask = np.full((30, 40), 255, np.uint8)
    mask[12, 21] = 0
    W = ref.weight_pyramid(mask, win, sizes)
    # level 0: the Scharr support of the pixel.  Level 1: pixel x reads 2x - 2 .. 2x + 2, so x in 10..11 and y in 5..7 are off in
    # M_1, and W_1 is that box grown by one.  Level 2: M_2 is off where 2x - 2 .. 2x + 2 meets 10..11 (x in 4..6) and 2y - 2 .. 2y + 2
    # meets 5..7 (y in 2..4)
    assert np.array_equal(W[0], _off_box(W[0].shape, win, 20, 22, 11, 13))
    assert np.array_equal(W[1], _off_box(W[1].shape, win, 9, 12, 4, 8))
    assert np.array_equal(W[2], _off_box(W[2].shape, win, 3, 7, 1, 5))


def test_weight_pyramid_of_an_off_pixel_on_the_frame_border():
    win, sizes = 3, ref.level_sizes(41, 31, 3, 1)
    assert sizes == [(41, 31), (21, 16)]
    mask = np.full((31, 41), 255, np.uint8)
    mask[30, 40] = 0        # the last pixel of both axes: level 1 reads it from x in 19..20 (2x + 2 >= 40) and y in 14..15
    mask[0, 1] = 0          # column 1 is read by x = 0 (directly and as the reflection of -1) and x = 1, row 0 by y = 0 and y = 1
    W = ref.weight_pyramid(mask, win, sizes)
    want0 = _off_box(W[0].shape, win, 39, 40, 29, 30) & _off_box(W[0].shape, win, 0, 2, 0, 1)
    want1 = _off_box(W[1].shape, win, 18, 20, 13, 15) & _off_box(W[1].shape, win, 0, 2, 0, 2)
    assert np.array_equal(W[0], want0)
    assert np.array_equal(W[1], want1)
    for a, b in zip(W, _brute_force(mask, win, sizes)):
        assert np.array_equal(a, b)


def test_weight_pyramid_at_odd_level_sizes_is_the_definition():
    win, sizes = 10, ref.level_sizes(161, 119, 10, 2)
    assert sizes == [(161, 119), (81, 60), (41, 30)]
    _, (m0, _) = scene.frames()
    mask = m0[:119, :161].copy()
    mask[:, 160] = 0        # an outline that leaves through the border
    mask[118, 30:50] = 255
    for a, b in zip(ref.weight_pyramid(mask, win, sizes), _brute_force(mask, win, sizes)):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_weight_pyramid_all_on_and_all_off():
    win, sizes = 8, ref.level_sizes(161, 119, 8, 3)
    for W in ref.weight_pyramid(np.full((119, 161), 1, np.uint8), win, sizes):
        assert W.all()
    for (w, h), W in zip(sizes, ref.weight_pyramid(np.zeros((119, 161), np.uint8), win, sizes)):
        assert not W[win:-win, win:-win].any()
        pad = W.copy()
        pad[win:-win, win:-win] = True
        assert pad.all() and W.shape == (h + 2 * win, w + 2 * win)


# ---- the effect ----

# Median end-point error against the foreground's motion, status-1 rows, 40 keypoints per band inside the disc's outline, 3 levels:
# (window, band) -> (unweighted = the parent's behaviour, weighted), pixels, measured with this restatement on scene.frames(7)
MEASURED = {
    (10, "outer"): (0.854, 0.026),
    (10, "inner"): (0.337, 0.016),
    (21, "outer"): (0.712, 0.009),
    (21, "inner"): (0.192, 0.008),
}


@pytest.mark.parametrize("win", [10, 21])
def test_weights_remove_the_background_from_keypoints_near_the_outline(win):
    (g0, g1), (m0, _) = scene.frames()
    p0, p1 = oracle.Pyramid(g0, win, 2), oracle.Pyramid(g1, win, 2)
    assert p0.num_levels == 3
    P, N = ref.Planes(p0), ref.Planes(p1)
    weights = ref.weight_pyramid(m0, win, [p0.level_size(l) for l in range(3)])
    opt = oracle.flow_options(window_size=win, max_level=2)
    for band, (lo, hi) in (("outer", (0.0, win / 4)), ("inner", (win / 4, win / 2))):
        pts = scene.ring_keypoints(lo, hi)
        want = scene.truth(pts)
        med = []
        for wts in (None, weights):
            xy, st, _, touched = ref.track(P, N, pts, opt, weights=wts)
            ok = st == 1
            assert ok.mean() >= 0.9
            assert wts is None or touched.all()
            med.append(float(np.median(np.linalg.norm(xy[ok] - want[ok], axis=1))))
        m_un, m_w = MEASURED[(win, band)]
        print(f"window {win} {band} band: unweighted {med[0]:.3f} px, weighted {med[1]:.3f} px (measured {m_un} -> {m_w})")
        # the factor 2 covers seed-to-seed spread and nothing else
        assert med[1] <= med[0] * 2.0 * (m_w / m_un)
        if (win, band) == (21, "outer"):
            assert med[1] < 0.5 * med[0]
