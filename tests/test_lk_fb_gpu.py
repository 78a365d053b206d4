"""GPU: the forward-backward check of the LK flow (include/polychase_hip.h: pc_lk_track_fb, pc_lk_track_filtered_fb,
pc_analyzer_set_fb_threshold; OpticalFlowOptions.forward_backward_threshold) against the CPU oracle composed with itself
(tests/fb_scene.py), bit for bit, in both arithmetic modes."""
import functools
import os
import sqlite3
import sys

import numpy as np
import pytest

import fb_scene
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "opencv_x86": (hip.ARITH_OPENCV_X86, oracle.EMU_OPENCV_X86)}

# name: (width, height, window, max_level, target kinds)
CASES = {
    "131x97_w10_l3": (131, 97, 10, 3, ("shift", "same", "border")),             # the pyramid ends before level 3
    "160x120_w15_l2": (160, 120, 15, 2, ("shift", "same", "unrelated", "border", "shift", "shift", "border", "shift")),
    "96x80_w5_l1": (96, 80, 5, 1, ("shift",)),
    "96x80_w16_l1": (96, 80, 16, 1, ("shift", "same")),                         # the launch's LDS sizing changes here (3 wavefronts per workgroup)
    "64x64_w3_l2": (64, 64, 3, 2, ("shift", "unrelated", "border")),
    "160x120_w31_l2": (160, 120, 31, 2, ("shift",)),
}


@functools.lru_cache(maxsize=None)
def _scene(case):
    w, h, win, ml, kinds = CASES[case]
    far = win > 10   # wide windows: finer texture and a larger shift (fb_scene.target)
    base = fb_scene.texture(w, h, 11 + win, 2 if far else 3)
    g1 = fb_scene.to_u8(base)
    targets = [fb_scene.target(base, k, 100 + 7 * i, far) for i, k in enumerate(kinds)]
    kps = oracle.gftt(g1)
    return g1, targets, kps


@functools.lru_cache(maxsize=None)
def _expected(case, arith, thr):
    """the composition on the CPU, once per (case, arithmetic, threshold); shared, never modified"""
    w, h, win, ml, kinds = CASES[case]
    g1, targets, kps = _scene(case)
    opt = oracle.flow_options(window_size=win, max_level=ml)
    with oracle.emulation(ARITH[arith][1]):
        p1 = oracle.Pyramid(g1, win, ml)
        out = [fb_scene.composed(p1, oracle.Pyramid(t, win, ml), kps, opt, thr) for t in targets]
    for c in out:
        for v in c.values():
            v.setflags(write=False)
    return out


def _frames(ctx, case, kps=None):
    w, h, win, ml, kinds = CASES[case]
    g1, targets, det = _scene(case)
    fr = []
    for g in [g1] + list(targets):
        f = hip.Frame(ctx, w, h, win, ml)
        f.set_gray(g)
        fr.append(f)
    fr[0].set_keypoints(det if kps is None else kps)
    return fr


@pytest.fixture(scope="module", params=sorted(ARITH))
def actx(request):
    ctx = hip.Context(0)
    ctx.set_arithmetic(ARITH[request.param][0])
    yield request.param, ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("thr", [0.5, 1.0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_stage_call_matches_the_composed_oracle(actx, case, thr):
    arith, ctx = actx
    w, h, win, ml, kinds = CASES[case]
    exp = _expected(case, arith, thr)
    for c, kind in zip(exp, kinds):
        fb_scene.check_fractions(c, kind)
    if "border" in kinds:   # some forward end points have left the frame, and they were tracked back from there
        q = np.concatenate([c["next_xy"][c["status_f"] == 1] for c, k in zip(exp, kinds) if k == "border"])
        assert ((q[:, 0] > w - 1) | (q[:, 1] > h - 1) | (q < 0).any(axis=1)).any()
    fr = _frames(ctx, case)
    xy, st, err, bxy, bst = hip.lk_track_fb(ctx, fr[0], fr[1:], thr, hip.flow_options(window_size=win, max_level=ml))
    for t, c in enumerate(exp):
        print(case, arith, thr, kinds[t], "forward", int((c["status_f"] == 1).sum()), "kept", int(c["status"].sum()),
              "status_b == 0:", int(((c["status_f"] == 1) & (c["back_status"] == 0)).sum()))
        assert np.array_equal(_bits(xy[t]), _bits(c["next_xy"])), (t, "next_xy")
        assert np.array_equal(_bits(err[t]), _bits(c["err"])), (t, "err")
        assert np.array_equal(bst[t], c["back_status"]), (t, "back_status")
        assert np.array_equal(_bits(bxy[t]), _bits(c["back_xy"])), (t, "back_xy")
        assert np.array_equal(st[t], c["status"]), (t, "status")
    for f in fr:
        f.close()


@pytest.mark.parametrize("thr", [0.5, 1.0])
@pytest.mark.parametrize("case", ["131x97_w10_l3", "160x120_w15_l2", "64x64_w3_l2"])
def test_filtered_call_gives_the_kept_rows_in_order(actx, case, thr):
    arith, ctx = actx
    w, h, win, ml, kinds = CASES[case]
    exp = _expected(case, arith, thr)
    fr = _frames(ctx, case)
    res = hip.lk_track_filtered_fb(ctx, fr[0], fr[1:], thr, hip.flow_options(window_size=win, max_level=ml))
    assert len(res) == len(kinds)
    for (idx, xy, err), c in zip(res, exp):
        keep = np.nonzero(c["status"] == 1)[0].astype(np.uint32)
        assert np.array_equal(idx, keep)           # ascending keypoint index; the row offsets are consistent with the counts
        assert np.array_equal(_bits(xy), _bits(c["next_xy"][keep])) and np.array_equal(_bits(err), _bits(c["err"][keep]))
    for f in fr:
        f.close()


@pytest.mark.parametrize("n", [0, 1, 5, 13])
def test_keypoint_counts_border_positions_and_a_target_without_survivors(actx, n):
    """supplied keypoints at fractional positions within a window of each border; a flat target: no forward survivor at all"""
    arith, ctx = actx
    w, h, win, ml = 96, 80, 7, 2
    base = fb_scene.texture(w, h, 5)
    g1 = fb_scene.to_u8(base)
    tg = [fb_scene.target(base, "shift", 3), np.full((h, w), 90, np.uint8), fb_scene.target(base, "border", 4)]
    pos = np.array([[1.3, 2.6], [w - 2.25, 3.5], [4.75, h - 1.5], [w - 6.5, h - 3.125], [0.0, 0.0], [w - 1.0, h - 1.0],
                    [40.5, 0.25], [0.75, 41.5], [w - 1.5, 30.25], [50.125, h - 2.75], [30.3, 30.7], [60.6, 50.2], [6.9, 6.1]], np.float32)
    kps = pos[:n]
    opt = oracle.flow_options(window_size=win, max_level=ml)
    with oracle.emulation(ARITH[arith][1]):
        p1 = oracle.Pyramid(g1, win, ml)
        exp = [fb_scene.composed(p1, oracle.Pyramid(t, win, ml), kps, opt, 1.0) for t in tg]
    assert not exp[1]["status_f"].any()
    fr = []
    for g in [g1] + tg:
        f = hip.Frame(ctx, w, h, win, ml)
        f.set_gray(g)
        fr.append(f)
    fr[0].set_keypoints(kps)
    xy, st, err, bxy, bst = hip.lk_track_fb(ctx, fr[0], fr[1:], 1.0, hip.flow_options(window_size=win, max_level=ml))
    assert xy.shape == (3, n, 2) and st.shape == (3, n)
    for t, c in enumerate(exp):
        assert np.array_equal(_bits(xy[t]), _bits(c["next_xy"])) and np.array_equal(_bits(err[t]), _bits(c["err"]))
        assert np.array_equal(bst[t], c["back_status"]) and np.array_equal(_bits(bxy[t]), _bits(c["back_xy"]))
        assert np.array_equal(st[t], c["status"])
    res = hip.lk_track_filtered_fb(ctx, fr[0], fr[1:], 1.0, hip.flow_options(window_size=win, max_level=ml))
    for (idx, _, _), c in zip(res, exp):
        assert np.array_equal(idx, np.nonzero(c["status"] == 1)[0].astype(np.uint32))
    for f in fr:
        f.close()


def test_threshold_zero_is_the_plain_call_and_bad_thresholds_raise(actx):
    arith, ctx = actx
    case = "131x97_w10_l3"
    w, h, win, ml, kinds = CASES[case]
    fr = _frames(ctx, case)
    opt = hip.flow_options(window_size=win, max_level=ml)
    xy0, st0, err0 = hip.lk_track(ctx, fr[0], fr[1:], opt)
    xy, st, err, bxy, bst = hip.lk_track_fb(ctx, fr[0], fr[1:], 0.0, opt)
    assert xy.tobytes() == xy0.tobytes() and st.tobytes() == st0.tobytes() and err.tobytes() == err0.tobytes()
    assert not bxy.any() and not bst.any()
    plain = hip.lk_track_filtered(ctx, fr[0], fr[1:], opt)
    filt = hip.lk_track_filtered_fb(ctx, fr[0], fr[1:], 0.0, opt)
    for a, b in zip(plain, filt):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(hip.PolychaseHipError):
            hip.lk_track_fb(ctx, fr[0], fr[1:], bad, opt)
        with pytest.raises(hip.PolychaseHipError):
            hip.lk_track_filtered_fb(ctx, fr[0], fr[1:], bad, opt)
    # the backward launch is timed under its own class, and only runs when the check is on
    ctx.enable_timing(["lk", "lk_fb"])
    ctx.reset_timing()
    hip.lk_track_fb(ctx, fr[0], fr[1:], 0.0, opt)
    assert ctx.timing()["lk"][0] == 1 and ctx.timing()["lk_fb"][0] == 0
    hip.lk_track_fb(ctx, fr[0], fr[1:], 1.0, opt)
    assert ctx.timing()["lk"][0] == 2 and ctx.timing()["lk_fb"][0] == 1
    ctx.enable_timing(False)
    for f in fr:
        f.close()


# ---- analyzer / product ----
@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


W, H, N = 160, 120, 12


@functools.lru_cache(maxsize=None)
def _clip():
    return fb_scene.clip(W, H, N)


@functools.lru_cache(maxsize=None)
def _clip_expected(thr):
    """oracle.analyze_clip's records (the product's default arithmetic = the oracle's default emulation) filtered by the
    composed check, as the database's blobs"""
    frames = _clip()
    kps, flows = oracle.analyze_clip(frames, first_frame=1, threads=4)
    opt = oracle.flow_options()
    pyr = {i + 1: oracle.Pyramid(oracle.rgb2gray(f)) for i, f in enumerate(frames)}
    k = {f: (len(v), v.tobytes()) for f, v in kps.items()}
    fl, fwd, kept = {}, 0, 0
    for (a, b), (idx, xy, err) in flows.items():
        c = fb_scene.composed(pyr[a], pyr[b], kps[a], opt, thr)
        assert np.array_equal(np.nonzero(c["status_f"] == 1)[0], idx) and np.array_equal(c["next_xy"][idx], xy)
        keep = np.nonzero(c["status"] == 1)[0].astype(np.uint32)
        fl[(a, b)] = (len(keep), keep.tobytes(), c["next_xy"][keep].tobytes(), c["err"][keep].tobytes())
        fwd += len(idx)
        kept += len(keep)
    assert kept >= 0.1 * fwd and fwd - kept >= 0.1 * fwd, (fwd, kept)
    return k, fl


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], r[2]) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): tuple(r[2:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _run(core, path, thr=None, shard=None):
    frames = _clip()
    fo = core.OpticalFlowOptions()
    if thr is not None:
        fo.forward_backward_threshold = thr
    vi = core.VideoInfo(W, H, 1, N)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, core.GFTTOptions(), fo)
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], None, path, shard[0], shard[1], flow_options=fo)


def test_database_holds_the_rows_the_composed_check_keeps(core, tmp_path):
    ek, ef = _clip_expected(1.0)
    path = str(tmp_path / "fb.db")
    _run(core, path, 1.0)
    k, f = _dump(path)
    assert k == ek            # the keypoints are not touched
    assert sorted(f) == sorted(ef)
    for key in sorted(ef):
        assert f[key] == ef[key], key


def test_threshold_zero_database_is_byte_identical_and_engines_do_not_inherit(core, tmp_path, monkeypatch):
    # One transaction per frame: with larger batches a transaction also ends whenever the writer's queue runs empty
    # (analysis_driver.cc: RecordWriter), so the NUMBER of commits -- SQLite's change counter, bytes 24..27 and 92..95 of the
    # file -- depends on timing, between two runs of the parent commit too.  With it fixed, whole files are compared.
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    a, b, c, d = (str(tmp_path / n) for n in ("plain.db", "zero.db", "one.db", "after.db"))
    _run(core, a)                 # attribute untouched
    _run(core, b, 0.0)
    assert open(a, "rb").read() == open(b, "rb").read()
    _run(core, c, 1.0)            # the parked engine of the runs above serves this one and the next
    _run(core, d, 0.0)
    assert open(d, "rb").read() == open(a, "rb").read()
    assert _dump(c)[1] == _clip_expected(1.0)[1] and _dump(c)[1] != _dump(a)[1]


def test_two_shards_give_the_records_of_one(core, tmp_path):
    one, s1, s2 = (str(tmp_path / n) for n in ("one.db", "s1.db", "s2.db"))
    _run(core, one, 1.0)
    _run(core, s1, 1.0, (1, 7))
    _run(core, s2, 1.0, (7, N + 1))
    k, f = _dump(one)
    k1, f1 = _dump(s1)
    k2, f2 = _dump(s2)
    assert sorted(k1) == list(range(1, 7)) and sorted(k2) == list(range(7, N + 1))
    assert {**k1, **k2} == k and {**f1, **f2} == f
    assert f == _clip_expected(1.0)[1]
