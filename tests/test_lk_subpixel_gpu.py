"""GPU: the forward LK kernels (kernels_lk3.hip: windows 4 .. 10; lk4_kernel.hpp: 3 and 11 .. 31) against the CPU oracle at
keypoints OFF THE INTEGER GRID and OUT OF THE FRAME, bit for bit, in both arithmetic orders -- the scenes of
tests/lk_subpixel_scene.py, whose conditions test_lk_subpixel_cpu.py asserts on the oracle alone.  Detected keypoints are integers:
every other forward test leaves the weights' rounding, w11 == -1, the padding and the bounds test of the template side unvisited.
The plain kernel is held to the same arrays by the subpixel_* cases of _lk_plain_check.py (test_lk_plain_gpu.py)."""
import numpy as np
import pytest

import lk_subpixel_scene as scene
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ARITH = {"canonical": hip.ARITH_CANONICAL, "lk_x86_order": hip.ARITH_LK_X86_ORDER}


@pytest.fixture(scope="module", params=sorted(ARITH))
def actx(request):
    ctx = hip.Context(0)
    ctx.set_arithmetic(ARITH[request.param])
    yield request.param, ctx
    ctx.close()


@pytest.mark.parametrize("win", scene.WINDOWS)
def test_stage_call_matches_the_oracle_off_the_grid(actx, win):
    arith, ctx = actx
    g1, targets, kps = scene.scene(win)
    scene.check_classes(win)
    exp = scene.expected(win, arith)
    fr = []
    for g in [g1] + list(targets):
        f = hip.Frame(ctx, scene.W, scene.H, win, scene.MAX_LEVEL)
        f.set_gray(g)
        fr.append(f)
    fr[0].set_keypoints(kps)
    assert np.array_equal(scene.bits(fr[0].keypoints()), scene.bits(kps))
    opt = hip.flow_options(window_size=win, max_level=scene.MAX_LEVEL)
    raw = hip.lk_track(ctx, fr[0], fr[1:], opt)
    why = scene.mismatch(win, raw, exp)
    assert why == "", "window %d, %s: %s" % (win, arith, why)
    # far keypoints: status 0 and err 0 on every target, whatever else holds
    e = scene.CLASSES["E"]
    assert not raw[1][:, e].any() and not scene.bits(raw[2][:, e]).any()
    # the filtered call == the raw arrays filtered on the host
    why = scene.filtered_mismatch(hip.lk_track_filtered(ctx, fr[0], fr[1:], opt), raw)
    assert why == "", "window %d, %s, filtered: %s" % (win, arith, why)
    for f in fr:
        f.close()


@pytest.mark.parametrize("win", [10, 21])
def test_analyzer_records_match_the_oracle_off_the_grid(win):
    """The product path -- binned visiting order, compaction, records -- with keypoints whose tile index has to be clamped
    (classes D and E), in the library's default arithmetic."""
    ctx = hip.Context(0)
    by_flag = {hip.ARITH_CANONICAL: "canonical", hip.ARITH_LK_X86_ORDER: "lk_x86_order", hip.ARITH_OPENCV_X86: "opencv_x86"}
    assert ctx.arithmetic in by_flag, ctx.arithmetic
    arith = by_flag[ctx.arithmetic]
    g1, targets, kps = scene.scene(win)
    exp = scene.expected(win, arith)
    an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), hip.flow_options(window_size=win, max_level=scene.MAX_LEVEL),
                      ring_frames=17, max_jobs=3)
    for i, g in enumerate([g1] + list(targets)):
        an.put_frame(1 + i, scene.rgb(g), will_detect=False)
    an.set_keypoints(1, kps)
    ids = list(range(2, 2 + len(targets)))
    an.submit(1, ids)
    frame1, got_kps, detected, flows = an.collect()
    assert frame1 == 1 and not detected and np.array_equal(scene.bits(got_kps), scene.bits(kps))
    assert sorted(flows) == ids
    for t, (exy, est, eerr) in enumerate(exp):
        idx, xy, err = flows[2 + t]
        keep = np.nonzero(est == 1)[0].astype(np.uint32)
        assert len(keep) and len(keep) < len(est)
        assert np.array_equal(idx, keep), ("window %d target %d: first differing row at %s" % (
            win, t, scene.class_of(int(sorted(set(idx.tolist()) ^ set(keep.tolist()))[0])) if set(idx.tolist()) ^ set(keep.tolist()) else "order"))
        bad = (scene.bits(xy) != scene.bits(exy[keep])).any(axis=1) | (scene.bits(err) != scene.bits(eerr[keep]))
        assert not bad.any(), "window %d target %d: the row of %s differs" % (win, t, scene.class_of(int(keep[np.nonzero(bad)[0][0]])))
    an.close()
    ctx.close()
