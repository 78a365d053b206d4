"""CPU: the search prepass rule as restated in tests/lk_search_ref.py -- what it leaves of plain LK, its level / radius table, the
tie-break and the acceptance on hand-made planes, and the quality claims the option is built for, asserted on the reference before
any GPU result is compared with it.  No GPU.

Scene of the quality claims: 256 x 192 crops of fb_scene.to_u8(fb_scene.texture(W + 320, H + 320, 11)); frame1 is the crop at
(160, 160), a target the crop displaced by an integer vector, so the analytic end point of keypoint p is p + (dx, dy).  Window 10,
max_level 3, R = 64, every fourth oracle.gftt keypoint.  "Good": status 1 and within 0.5 px of the analytic end point; "inside":
the analytic end point lies inside the frame."""
import numpy as np
import pytest

import fb_scene
import lk_search_ref as ref
import oracle

W, H, WIN, MAX_LEVEL, R = 256, 192, 10, 3, 64


@pytest.fixture(scope="module")
def big():
    return fb_scene.to_u8(fb_scene.texture(W + 320, H + 320, 11))


def crop(big, dx=0, dy=0):
    return np.ascontiguousarray(big[160 - dy:160 - dy + H, 160 - dx:160 - dx + W])


@pytest.fixture(scope="module")
def frame1(big):
    with oracle.emulation(oracle.EMU_CANONICAL):
        g = crop(big)
        kps = oracle.gftt(g)[::4]
        pyr = oracle.Pyramid(g, WIN, MAX_LEVEL)
        return g, kps, pyr, ref.Planes(pyr)


_RUNS = {}


def run(big, frame1, d):
    """plain rows (the oracle's, canonical) and searched rows of the displacement d, computed once"""
    if d not in _RUNS:
        _, kps, pyr, P = frame1
        opt = oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
        with oracle.emulation(oracle.EMU_CANONICAL):
            pt = oracle.Pyramid(crop(big, *d), WIN, MAX_LEVEL)
            plain = oracle.lk(pyr, pt, kps, opt)
            found = ref.search(P, [ref.Planes(pt)], kps, [plain], opt, R)[0]
        _RUNS[d] = (plain, found)
    return _RUNS[d]


def counts(kps, d, rows):
    end = kps + np.array(d, np.float32)
    inside = (end[:, 0] >= 0) & (end[:, 0] <= W - 1) & (end[:, 1] >= 0) & (end[:, 1] <= H - 1)
    good = (rows[1] == 1) & (np.hypot(*(rows[0] - end).T) <= 0.5)
    return int(inside.sum()), int(good.sum())


def test_with_the_guess_at_the_keypoint_the_guided_pass_is_the_oracle_bit_for_bit(big, frame1):
    _, kps, pyr, P = frame1
    extra = np.array([[0.25, 0.5], [W - 1.0, H - 1.0], [-30.0, 20.0], [W + 40.0, 5.5], [100.5, 77.75]], np.float32)
    pts = np.concatenate([kps[:60], extra])
    opt = oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    for d in ((3, -2), (19, -11)):
        with oracle.emulation(oracle.EMU_CANONICAL):
            pt = oracle.Pyramid(crop(big, *d), WIN, MAX_LEVEL)
            want = oracle.lk(pyr, pt, pts, opt)
        N = ref.Planes(pt)
        with np.errstate(over="ignore", invalid="ignore"):
            got = [ref.track_point(P, N, x, y, x, y, MAX_LEVEL, 30, 0.01 * 0.01, np.float32(opt.min_eigen_threshold)) for x, y in pts]
        assert want[1].sum() >= 30 and (want[1] == 0).any()
        assert np.array_equal(np.array([g[2] for g in got], np.uint8), want[1])
        assert np.array_equal(np.array([g[:2] for g in got], np.float32).view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(np.array([g[3] for g in got], np.float32).view(np.uint32), want[2].view(np.uint32))


@pytest.mark.parametrize("R_, T, want", [(5, 2, (0, 5)), (16, 2, (0, 16)), (40, 2, (2, 10)), (200, 2, (2, 16)), (64, 3, (2, 16)),
                                          (1, 0, (0, 1)), (256, 0, (0, 16)), (256, 8, (4, 16)), (17, 3, (1, 9))])
def test_level_and_radius(R_, T, want):
    assert ref.level_radius(R_, T) == want


def _planes(seed=5, w=64, h=48):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def test_tie_break_and_acceptance_on_hand_made_planes():
    I = _planes()
    x, y = 30.0, 20.0                      # block origin (26, 16) at level 0
    tmpl = I[16:24, 26:34]
    # an exact copy at (+5, -3): found, and scaled by the level
    J = _planes(6)
    J[13:21, 31:39] = tmpl
    assert ref.match(I, J, x, y, 0, 8) == (5, -3)
    assert ref.match(I, J, 4 * x, 4 * y, 2, 8) == (20, -12)  # the same planes read as level 2: p and d in level-0 pixels
    assert ref.match(I, J, x, y, 0, 4) != (5, -3)            # outside the radius
    # two equal minima at the same distance, (+5, -3) and (-5, 3): the smaller dy wins; (3, 5) against (-5, 3): dy again
    J[19:27, 21:29] = tmpl
    assert ref.match(I, J, x, y, 0, 8) == (5, -3)
    J2 = _planes(6)
    J2[21:29, 29:37] = tmpl
    J2[19:27, 21:29] = tmpl
    assert ref.match(I, J2, x, y, 0, 8) == (-5, 3)
    # same dy, same distance, (-4, 0) and (4, 0): the smaller dx wins
    J3 = _planes(6)
    J3[16:24, 22:30] = tmpl
    J3[16:24, 30:38] = tmpl
    assert ref.match(I, J3, x, y, 0, 8) == (-4, 0)
    # a nearer minimum beats a farther equal one
    J4 = _planes(6)
    J4[9:17, 26:34] = tmpl           # (0, -7)
    J4[17:25, 28:36] = tmpl          # (2, 1): nearer
    assert ref.match(I, J4, x, y, 0, 8) == (2, 1)
    # acceptance: a best candidate that is not 25 % better than the zero displacement is refused
    flat = np.full((48, 64), 100, np.uint8)
    If = flat.copy()
    If[16:24, 26:34] = 140                                   # template: 64 pixels of 140
    Jz = flat.copy()
    Jz[16:24, 26:34] = 130                                   # at zero: SAD 640
    Jz[30:38, 40:48] = 132                                   # at (14, 14): SAD 512 > 480 = 3/4 of 640
    assert ref.match(If, Jz, x, y, 0, 16) == (0, 0)
    Jz[30:38, 40:48] = 133                                   # SAD 448 <= 480
    assert ref.match(If, Jz, x, y, 0, 16) == (14, 14)
    Jz[30:38, 40:48] = 132
    Jz[31, 41] = 140                                         # SAD 512 - 8 = 504 > 480: still refused
    assert ref.match(If, Jz, x, y, 0, 16) == (0, 0)
    # a keypoint whose block is not inside, or that is not finite, is not searched; candidates stop at the border
    assert ref.match(I, J, 3.0, 20.0, 0, 8) == (0, 0)
    assert ref.match(I, J, np.nan, 20.0, 0, 8) == (0, 0) and ref.match(I, J, np.inf, 20.0, 0, 8) == (0, 0)
    assert ref.match(I, J, 60.5, 20.0, 0, 8) == (0, 0)       # cx = 61: the block ends at 65 > 64
    Je = _planes(7)
    Je[0:8, 56:64] = I[4:12, 50:58]                          # keypoint (54, 8): the copy sits in the very corner, (6, -4)
    assert ref.match(I, Je, 54.0, 8.0, 0, 16) == (6, -4)


def test_quality_at_a_long_displacement(big, frame1):
    """measured on this scene at (37, -22): 181 rows end inside the frame, plain LK keeps 10 good ones, the rule 137 (states: 91 not
    displaced, 152 replaced, 21 kept); the conditions are the proposal's (5 x the plain good rows, 60 % of the inside rows)"""
    kps = frame1[1]
    plain, found = run(big, frame1, (37, -22))
    inside, good_plain = counts(kps, (37, -22), plain)
    _, good = counts(kps, (37, -22), found)
    print("(37, -22): inside", inside, "plain good", good_plain, "with the search", good, "states", np.bincount(found[4], minlength=3).tolist())
    assert good >= 5 * good_plain and good >= 0.6 * inside and good >= 50
    # a rescue, not a check: a record is never replaced by one with a larger patch error
    rep = found[4] == ref.REPLACED
    assert rep.any() and ((plain[1][rep] == 0) | (found[2][rep] < plain[2][rep])).all()
    assert ((plain[1] == 0) & rep).any(), "some forward status-0 row is rescued"
    keep = ~rep
    assert found[0][keep].tobytes() == plain[0][keep].tobytes() and np.array_equal(found[1][keep], plain[1][keep])


@pytest.mark.parametrize("d", [(9, 5), (0, 0)])
def test_no_good_row_is_lost_at_short_displacements(big, frame1, d):
    kps = frame1[1]
    plain, found = run(big, frame1, d)
    inside, good_plain = counts(kps, d, plain)
    _, good = counts(kps, d, found)
    print(d, "inside", inside, "plain good", good_plain, "with the search", good, "states", np.bincount(found[4], minlength=3).tolist())
    assert good_plain >= 0.9 * inside and good >= good_plain
    if d == (0, 0):
        assert not found[4].any() and not found[3].any()
        assert all(found[k].tobytes() == plain[k].tobytes() for k in range(3))
