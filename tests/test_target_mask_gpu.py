"""GPU: target-side masks at stage level.  The choked plane (kernels_mask.hip: mask_choke_kernel through
pc_frame_download_choked_mask) against tests/target_mask_ref.py, byte for byte; pc_lk_track_masked against the CPU oracle
composed with the reference's plane test (tests/fb_scene.py, tests/target_mask_ref.py), bit for bit, in both arithmetic modes."""
import functools

import numpy as np
import pytest

import fb_scene
import oracle
import polygon_mask_ref
import target_mask_ref as ref
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "opencv_x86": (hip.ARITH_OPENCV_X86, oracle.EMU_OPENCV_X86)}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


# ---- the choked plane ----
SIZES = [(1, 1), (37, 29), (67, 5), (64, 64), (333, 211), (1027, 9)]     # (w, h)
MARGINS = [1, 2, 7, 31]


def _corners(w, h):
    m = np.full((h, w), 255, np.uint8)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 0
    return m


def _random(w, h, off, seed):
    rng = np.random.default_rng(seed + 1000 * w + h)
    on = rng.random((h, w)) >= off
    return np.where(on, rng.integers(1, 255, (h, w)), 0).astype(np.uint8)     # the on bytes: anything but 0 and 255


PLANES = {
    "random_50": lambda w, h: _random(w, h, 0.5, 1),
    "random_2": lambda w, h: _random(w, h, 0.02, 2),
    "all_on": lambda w, h: np.full((h, w), 7, np.uint8),
    "all_off": lambda w, h: np.zeros((h, w), np.uint8),
    "corners": _corners,
}


@pytest.mark.parametrize("plane", sorted(PLANES))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_choked_plane_matches_the_reference(ctx, size, plane):
    w, h = size
    m = PLANES[plane](w, h)
    f = hip.Frame(ctx, w, h, 3, 0)
    f.set_mask(m)
    assert np.array_equal(f.mask(), m)
    for r in [0] + MARGINS:
        got, want = f.choked_mask(r), ref.choke(m, r)
        assert got.shape == want.shape and np.array_equal(got, want), (size, plane, r, int((got != want).sum()))
    f.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_choked_polygon_mask_matches_the_reference(ctx, size):
    """an inverted rectangle, rasterised on the GPU: the plane the choke reads was never on the host"""
    w, h = size
    polys = [np.array([(0.3 * w, 0.3 * h), (0.3 * w + w / 3, 0.3 * h), (0.3 * w + w / 3, 0.3 * h + h / 3), (0.3 * w, 0.3 * h + h / 3)],
                      np.float32)]
    m = polygon_mask_ref.plane(polys, w, h, invert=True)
    f = hip.Frame(ctx, w, h, 3, 0)
    f.set_mask_polygons(polys, invert=True)
    assert np.array_equal(f.mask(), m)
    for r in [0] + MARGINS:
        assert np.array_equal(f.choked_mask(r), ref.choke(m, r)), (size, r)
    f.close()


def test_the_plane_download_needs_a_mask_and_a_margin_in_range(ctx):
    f = hip.Frame(ctx, 37, 29, 3, 0)
    with pytest.raises(hip.PolychaseHipError, match="no mask"):
        f.choked_mask(1)
    f.set_mask(np.ones((29, 37), np.uint8))
    for bad in (-1, 32):
        with pytest.raises(hip.PolychaseHipError, match="margin"):
            f.choked_mask(bad)
    assert f.choked_mask(31).all()
    f.set_mask(None)
    with pytest.raises(hip.PolychaseHipError, match="no mask"):
        f.choked_mask(0)
    f.close()


# ---- pc_lk_track_masked ----
# name: (width, height, window, max_level, target kinds): the scenes of tests/test_lk_fb_gpu.py
CASES = {
    "131x97_w10_l3": (131, 97, 10, 3, ("shift", "same", "border")),
    "160x120_w15_l2": (160, 120, 15, 2, ("shift", "same", "unrelated", "border", "shift", "shift", "border", "shift")),
    "96x80_w5_l1": (96, 80, 5, 1, ("shift",)),
    "64x64_w3_l2": (64, 64, 3, 2, ("shift", "unrelated", "border")),
    "160x120_w31_l2": (160, 120, 31, 2, ("shift",)),
}
TRACK_MARGINS = (0, 2, 5)
FB_THRESHOLDS = (0.0, 1.0)
# the one target of each case that carries NO mask: it must come out as pc_lk_track_fb leaves it
UNMASKED = {"131x97_w10_l3": None, "160x120_w15_l2": 5, "96x80_w5_l1": None, "64x64_w3_l2": None, "160x120_w31_l2": None}


@functools.lru_cache(maxsize=None)
def _scene(case):
    w, h, win, ml, kinds = CASES[case]
    far = win > 10
    base = fb_scene.texture(w, h, 11 + win, 2 if far else 3)
    g1 = fb_scene.to_u8(base)
    targets = [fb_scene.target(base, k, 100 + 7 * i, far) for i, k in enumerate(kinds)]
    return g1, targets, oracle.gftt(g1)


@functools.lru_cache(maxsize=None)
def _mask(case, t):
    """off exactly over target t's occluder rectangle (fb_scene.occluded); on bytes other than 255; None: no mask"""
    w, h, win, ml, kinds = CASES[case]
    if UNMASKED[case] == t:
        return None
    m = np.full((h, w), 1 + 17 * t, np.uint8)
    x0, y0 = (0.1, 0.5) if kinds[t] == "border" else (0.3, 0.3)
    rx, ry = int(w * x0), int(h * y0)
    m[ry:ry + h // 3, rx:rx + w // 3] = 0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _composed(case, arith, thr):
    """the oracle's forward pass and its composition with the backward pass, once per (case, arithmetic, threshold)"""
    w, h, win, ml, kinds = CASES[case]
    g1, targets, kps = _scene(case)
    opt = oracle.flow_options(window_size=win, max_level=ml)
    with oracle.emulation(ARITH[arith][1]):
        p1 = oracle.Pyramid(g1, win, ml)
        out = []
        for t in targets:
            pt = oracle.Pyramid(t, win, ml)
            if thr > 0:
                c = fb_scene.composed(p1, pt, kps, opt, thr)
            else:
                q, sf, err = oracle.lk(p1, pt, kps, opt)
                c = {"next_xy": q, "status_f": sf, "err": err, "status": sf.copy()}
            out.append(c)
    for c in out:
        for v in c.values():
            v.setflags(write=False)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.fixture(scope="module", params=sorted(ARITH))
def actx(request):
    c = hip.Context(0)
    c.set_arithmetic(ARITH[request.param][0])
    yield request.param, c
    c.close()


def _frames(ctx, case):
    w, h, win, ml, kinds = CASES[case]
    g1, targets, kps = _scene(case)
    fr = []
    for g in [g1] + list(targets):
        f = hip.Frame(ctx, w, h, win, ml)
        f.set_gray(g)
        fr.append(f)
    fr[0].set_keypoints(kps)
    for t in range(len(targets)):
        if _mask(case, t) is not None:
            fr[1 + t].set_mask(_mask(case, t))
    return fr


@pytest.mark.parametrize("thr", FB_THRESHOLDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_masked_call_matches_the_oracle_and_the_reference_plane(actx, case, thr):
    arith, ctx = actx
    w, h, win, ml, kinds = CASES[case]
    exp = _composed(case, arith, thr)
    fwd = _composed(case, arith, 0.0)
    # the scene must exercise both outcomes: asserted on the ORACLE's result, before anything is compared with it
    for t, kind in enumerate(kinds):
        if _mask(case, t) is None:
            continue
        for r in TRACK_MARGINS:
            sf = fwd[t]["status_f"]
            kept = ref.keep(fwd[t]["next_xy"], sf, _mask(case, t), r)
            dropped = int(sf.sum()) - int(kept.sum())
            print(case, arith, kind, "margin", r, "forward", int(sf.sum()), "dropped by the mask", dropped, "kept", int(kept.sum()))
            assert dropped >= 2 and int(kept.sum()) >= 10, (case, t, kind, r, dropped, int(kept.sum()))
    if case in ("131x97_w10_l3", "160x120_w15_l2"):   # forward rows of the border targets end outside the frame, and are judged there
        for t, kind in enumerate(kinds):
            if kind == "border":
                q = fwd[t]["next_xy"][fwd[t]["status_f"] == 1]
                px, py = np.floor(q[:, 0] + np.float32(0.5)), np.floor(q[:, 1] + np.float32(0.5))     # the pixel before the clamp
                outside = (px < 0) | (px > w - 1) | (py < 0) | (py > h - 1)
                print(case, arith, "border target", t, "rows that end outside the frame:", int(outside.sum()))
                assert outside.any(), (case, t)
    fr = _frames(ctx, case)
    opt = hip.flow_options(window_size=win, max_level=ml)
    plain_xy, plain_st, plain_err, _, _ = hip.lk_track_fb(ctx, fr[0], fr[1:], thr, opt)
    off_xy, off_st, off_err = hip.lk_track_masked(ctx, fr[0], fr[1:], thr, -1, opt)
    assert off_xy.tobytes() == plain_xy.tobytes() and off_st.tobytes() == plain_st.tobytes() and off_err.tobytes() == plain_err.tobytes()
    for r in TRACK_MARGINS:
        xy, st, err = hip.lk_track_masked(ctx, fr[0], fr[1:], thr, r, opt)
        for t, c in enumerate(exp):
            assert np.array_equal(_bits(xy[t]), _bits(c["next_xy"])), (r, t, "next_xy")
            assert np.array_equal(_bits(err[t]), _bits(c["err"])), (r, t, "err")
            want = ref.keep(c["next_xy"], c["status"], _mask(case, t), r)
            assert np.array_equal(st[t], want), (r, t, "status", int((st[t] != want).sum()))
            if _mask(case, t) is None:
                assert np.array_equal(st[t], plain_st[t]), (r, t, "a target without a mask keeps its rows")
    for f in fr:
        f.close()


def test_bad_margins_raise_and_a_cleared_mask_is_no_mask(actx):
    arith, ctx = actx
    case = "96x80_w5_l1"
    w, h, win, ml, kinds = CASES[case]
    fr = _frames(ctx, case)
    opt = hip.flow_options(window_size=win, max_level=ml)
    for bad in (-2, 32):
        with pytest.raises(hip.PolychaseHipError, match="margin"):
            hip.lk_track_masked(ctx, fr[0], fr[1:], 0.0, bad, opt)
    xy0, st0, err0 = hip.lk_track(ctx, fr[0], fr[1:], opt)
    xy, st, err = hip.lk_track_masked(ctx, fr[0], fr[1:], 0.0, 2, opt)
    assert xy.tobytes() == xy0.tobytes() and err.tobytes() == err0.tobytes() and int(st.sum()) < int(st0.sum())
    fr[1].set_mask(None)
    xy, st, err = hip.lk_track_masked(ctx, fr[0], fr[1:], 0.0, 2, opt)
    assert xy.tobytes() == xy0.tobytes() and st.tobytes() == st0.tobytes() and err.tobytes() == err0.tobytes()
    # neither new kernel belongs to a timed class: the call counts what the plain call counts
    fr[1].set_mask(_mask(case, 0))
    ctx.enable_timing(True)
    counts = []
    for margin in (-1, 2):
        ctx.reset_timing()
        hip.lk_track_masked(ctx, fr[0], fr[1:], 0.0, margin, opt)
        counts.append({k: v[0] for k, v in ctx.timing().items()})
    ctx.enable_timing(False)
    assert counts[0] == counts[1] and counts[0]["lk"] == 1, counts
    for f in fr:
        f.close()


# ---- pc_analyzer_set_target_mask_margin ----
def test_each_target_is_judged_by_the_mask_and_margin_it_was_put_under(ctx):
    """frames put with will_detect = 0 take the mask as targets only: frame 1 is still detected WITHOUT it; frames 2..5 are put
    under a host mask with margin 2, a device mask with margin 0, no mask, and a polygon mask with margin 31"""
    import torch
    w, h, win, ml = 160, 120, 10, 2
    frames = fb_scene.clip(w, h, 5)
    gray = [oracle.rgb2gray(f) for f in frames]
    m = np.full((h, w), 9, np.uint8)
    rx, ry = int(0.3 * w), int(0.3 * h)
    m[ry:ry + h // 3, rx:rx + w // 3] = 0
    rect = [np.array([(rx, ry), (rx + w // 3, ry), (rx + w // 3, ry + h // 3), (rx, ry + h // 3)], np.float32)]
    assert np.array_equal(polygon_mask_ref.plane(rect, w, h, invert=True) != 0, m != 0)
    dev = torch.from_numpy(m).cuda()
    an = hip.Analyzer(ctx, w, h, hip.gftt_options(), hip.flow_options(window_size=win, max_level=ml), ring_frames=17, max_jobs=3)
    an.set_mask(m)
    an.set_target_mask_margin(2)
    an.put_frame(1, frames[0], will_detect=False)
    an.put_frame(2, frames[1], will_detect=False)
    an.set_mask(dev)
    an.set_target_mask_margin(0)
    an.put_frame(3, frames[2], will_detect=False)
    an.set_mask(None)
    an.put_frame(4, frames[3], will_detect=False)
    an.set_mask_polygons(rect, invert=True)
    an.set_target_mask_margin(31)
    an.put_frame(5, frames[4], will_detect=False)
    an.set_target_mask_margin(-1)             # frames already put keep what they were put under
    judged = {2: (m, 2), 3: (m, 0), 4: (None, 0), 5: (m, 31)}
    an.submit(1, [2, 3, 4, 5])
    frame1, kps, detected, flows = an.collect()
    okps = oracle.gftt(gray[0])
    assert frame1 == 1 and detected and np.array_equal(kps, okps), "frame 1 is detected without the mask"
    assert (m[okps[:, 1].astype(int), okps[:, 0].astype(int)] == 0).any(), "some of its keypoints lie where the mask is off"
    opt = oracle.flow_options(window_size=win, max_level=ml)
    p1 = oracle.Pyramid(gray[0], win, ml)
    for t, (mask, r) in judged.items():
        q, sf, err = oracle.lk(p1, oracle.Pyramid(gray[t - 1], win, ml), okps, opt)
        keep = np.nonzero(ref.keep(q, sf, mask, r) == 1)[0].astype(np.uint32)
        print("target", t, "margin", r, "forward", int(sf.sum()), "kept", len(keep))
        assert (len(keep) < int(sf.sum())) == (mask is not None) and len(keep) >= 10
        idx, xy, e = flows[t]
        assert np.array_equal(idx, keep) and np.array_equal(_bits(xy), _bits(q[keep])) and np.array_equal(_bits(e), _bits(err[keep]))
    # reset keeps the margin and clears the mask: with no mask in force nothing is judged
    an.set_target_mask_margin(5)
    an.reset()
    an.put_frame(1, frames[0], will_detect=False)
    an.put_frame(2, frames[1], will_detect=False)
    an.submit(1, [2])
    _, kps, _, flows = an.collect()
    q, sf, err = oracle.lk(p1, oracle.Pyramid(gray[1], win, ml), okps, opt)
    assert np.array_equal(kps, okps) and np.array_equal(flows[2][0], np.nonzero(sf == 1)[0].astype(np.uint32))
    an.close()
