"""GPU: one LK job with every pass behind the forward launch switched on, through both callers of the sequence -- the stage call
(pc_lk_track_search) and the analyzer, configured through its setters -- which must leave the same rows, byte for byte.

Scene (tests/lk_search_scene.py): 160 x 120 frames, max_level 2, frame1 against three displaced crops of the same texture -- by 19
pixels where the search prepass is there to find them, by less than LK's own reach where it is not; the first and the last carry
a target-side mask (the rectangle of tests/test_target_mask_gpu.py, margin 2), the middle one none.  200 keypoints:
detected corners, some off the pixel grid, and the scene's border and out-of-frame points; 200 leaves the last workgroup of every
launch partly filled.  Windows 10 (two keypoints per wavefront) and 11 (one), canonical arithmetic and PC_ARITH_LK_X86_ORDER.

  case "constancy"    search radius 40, affine refinement, masks with margin 2, min_correlation 0.75, fb threshold 1
  case "normalized"   normalize, masks with margin 2, min_correlation 0.75, fb threshold 1

The mask and the correlation test judge a row by its end point alone and leave it otherwise untouched, so the job's final status is
the status of the same job without the two, filtered on the host by tests/target_mask_ref.py and tests/lk_correlation_ref.py: that
is asserted, and on the filtered status that every target keeps rows and loses rows, the masked ones to their mask."""
import functools

import numpy as np
import pytest

import lk_affine_ref as aff_ref
import lk_correlation_ref as corr_ref
import lk_search_ref as search_ref
import lk_search_scene as scene
import oracle
import target_mask_ref as mask_ref
from polychase_amd import hip

pytestmark = pytest.mark.gpu

W, H, MAX_LEVEL = scene.W, scene.H, scene.MAX_LEVEL
MASKED = (True, False, True)
MARGIN, MIN_CORRELATION, FB, RADIUS = 2, 0.75, 1.0, 40
ARITH = {"canonical": hip.ARITH_CANONICAL, "lk_x86_order": hip.ARITH_LK_X86_ORDER}
# name: (search_radius, affine, normalize, the displacements of the three targets)
CASES = {"constancy": (RADIUS, 1, 0, ((5, -3), (19, -11), (-19, 11))), "normalized": (0, 0, 1, ((5, -3), (9, -6), (-7, 4)))}


@functools.lru_cache(maxsize=None)
def _rgb(shifts):
    return [np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) for g in [scene.frame1()] + [scene.target(s) for s in shifts]]


@functools.lru_cache(maxsize=None)
def _gray(shifts):
    return [oracle.rgb2gray(f) for f in _rgb(shifts)]


@functools.lru_cache(maxsize=None)
def _keypoints() -> np.ndarray:
    with oracle.emulation(oracle.EMU_CANONICAL):
        det = oracle.gftt(_gray(())[0])
    extra = scene.keypoints()[49:]          # the scene's border and out-of-frame points
    det = det[:200 - len(extra)].copy()
    det[::3] += np.float32([0.25, 0.625])
    det[1::5] -= np.float32([0.5, 0.125])
    pts = np.concatenate([det, extra]).astype(np.float32)
    assert len(pts) == 200, len(pts)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _mask(t):
    """off over a rectangle of a third of each side (tests/test_target_mask_gpu.py: _mask); None: target t carries no mask"""
    if not MASKED[t]:
        return None
    m = np.full((H, W), 1 + 17 * t, np.uint8)
    rx, ry = int(W * 0.3), int(H * 0.3)
    m[ry:ry + H // 3, rx:rx + W // 3] = 0
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_arithmetic(hip.ARITH_CANONICAL)
    c.close()


def _frames(ctx, win, shifts):
    fr = []
    for t, f in enumerate(_rgb(shifts)):
        x = hip.Frame(ctx, W, H, win, MAX_LEVEL)
        x.set_rgb(f)
        if t > 0 and _mask(t - 1) is not None:
            x.set_mask(_mask(t - 1))
        fr.append(x)
    fr[0].set_keypoints(np.array(_keypoints()))
    return fr


def _analyzer_rows(ctx, opt, radius, affine, normalize, shifts):
    an = hip.Analyzer(ctx, W, H, hip.gftt_options(), opt, ring_frames=17, max_jobs=3)
    an.put_frame(1, _rgb(shifts)[0], will_detect=False)
    for t in range(3):
        an.set_mask(_mask(t))
        an.set_target_mask_margin(MARGIN if MASKED[t] else -1)
        an.put_frame(2 + t, _rgb(shifts)[1 + t], will_detect=False)
    an.set_keypoints(1, np.array(_keypoints()))
    an.set_search_radius(radius)
    an.set_affine_refinement(affine)
    an.set_normalize(normalize)
    an.set_min_correlation(MIN_CORRELATION)
    an.set_fb_threshold(FB)
    an.submit(1, [2 + t for t in range(3)])
    frame1, kps, detected, flows = an.collect()
    an.close()
    assert frame1 == 1 and not detected and kps.tobytes() == _keypoints().tobytes()
    return [flows[2 + t] for t in range(3)]


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("win", [10, 11])
@pytest.mark.parametrize("case", sorted(CASES))
def test_stage_call_and_analyzer_leave_the_same_rows(ctx, case, win, arith):
    radius, affine, normalize, shifts = CASES[case]
    ctx.set_arithmetic(ARITH[arith])
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    fr = _frames(ctx, win, shifts)
    # the job; the job without the mask and the correlation test; the job without any check
    full = hip.lk_track_search(ctx, fr[0], fr[1:], radius, affine, normalize, MIN_CORRELATION, FB, MARGIN, opt)
    loose = hip.lk_track_search(ctx, fr[0], fr[1:], radius, affine, normalize, 0.0, FB, -1, opt)
    bare = hip.lk_track_search(ctx, fr[0], fr[1:], radius, affine, normalize, 0.0, 0.0, -1, opt)
    for f in fr:
        f.close()
    rows = _analyzer_rows(ctx, opt, radius, affine, normalize, shifts)
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    xy, st, err = full[:3]
    assert xy.tobytes() == loose[0].tobytes() == bare[0].tobytes() and err.tobytes() == loose[2].tobytes() == bare[2].tobytes()
    if case == "constancy":     # both passes in front of the checks have changed rows
        assert (full[8] == search_ref.REPLACED).any() and (full[6] == aff_ref.ACCEPTED).any()
    kps, gray = _keypoints(), _gray(shifts)
    for t in range(3):
        # on the restatements: the filtered status, and that it keeps and loses rows
        masked = mask_ref.keep(xy[t], loose[1][t], _mask(t), MARGIN)
        want, _ = corr_ref.rows(gray[0], gray[1 + t], win, kps, xy[t], masked, MIN_CORRELATION)
        lost_to_mask = int(((loose[1][t] == 1) & (masked == 0)).sum())
        lost = int(((bare[1][t] == 1) & (want == 0)).sum())
        print(case, win, arith, "target", t, "rows of the bare job", int(bare[1][t].sum()), "lost to the mask", lost_to_mask,
              "lost to a check", lost, "kept", int(want.sum()))
        assert int(want.sum()) >= 1 and lost >= 1 and (lost_to_mask >= 1) == MASKED[t], (case, win, arith, t)
        assert np.array_equal(st[t], want), (case, win, arith, t, np.nonzero(st[t] != want)[0][:8].tolist())
        # the analyzer's rows are the stage call's status-1 rows, in keypoint order
        keep = np.nonzero(st[t] == 1)[0].astype(np.uint32)
        idx, axy, aerr = rows[t]
        assert idx.dtype == np.uint32 and idx.tobytes() == keep.tobytes(), (case, win, arith, t, "src_indices")
        assert axy.tobytes() == xy[t][keep].tobytes(), (case, win, arith, t, "tgt_xy")
        assert aerr.tobytes() == err[t][keep].tobytes(), (case, win, arith, t, "err")


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("win", [10, 11])
def test_filtered_fb_call_gives_the_status_1_rows_of_the_fb_call(ctx, win, arith):
    ctx.set_arithmetic(ARITH[arith])
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    fr = _frames(ctx, win, CASES["constancy"][3])
    xy, st, err, _, _ = hip.lk_track_fb(ctx, fr[0], fr[1:], FB, opt)
    forward = hip.lk_track(ctx, fr[0], fr[1:], opt)[1]
    rows = hip.lk_track_filtered_fb(ctx, fr[0], fr[1:], FB, opt)
    for f in fr:
        f.close()
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    for t in range(3):
        keep = np.nonzero(st[t] == 1)[0].astype(np.uint32)
        assert len(keep) >= 1 and int(((forward[t] == 1) & (st[t] == 0)).sum()) >= 1, (win, arith, t)
        idx, fxy, ferr = rows[t]
        assert idx.tobytes() == keep.tobytes() and fxy.tobytes() == xy[t][keep].tobytes() and ferr.tobytes() == err[t][keep].tobytes(), (win, arith, t)
