"""GPU: target-side masks through polychase_core (OpticalFlowOptions.target_mask_margin with detection_mask=).  Every pair's rows
must be the CPU oracle's rows for the masked keypoints (tests/masked_gftt_ref.py) filtered by the target frame's choked plane
(tests/target_mask_ref.py); the clip is tests/fb_scene.py's, the mask its fixed occluder rectangle, inverted."""
import functools
import os
import sqlite3
import sys
import time

import numpy as np
import pytest

import fb_scene
import masked_gftt_ref
import oracle
import target_mask_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 160, 120, 12
WIN, MAX_LEVEL = 10, 2
RX, RY, RW, RH = int(0.3 * W), int(0.3 * H), W // 3, H // 3      # fb_scene.occluded
SKIPS = (-8, -4, -2, -1, 1, 2, 4, 8)
MARGINS = (0, 3)


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@functools.lru_cache(maxsize=None)
def _clip():
    return fb_scene.clip(W, H, N)


@functools.lru_cache(maxsize=None)
def _plane():
    m = np.full((H, W), 255, np.uint8)
    m[RY:RY + RH, RX:RX + RW] = 0
    m.setflags(write=False)
    return m


def _polygon(core):
    """integer corners: by the half-open fill rule exactly _plane() when inverted"""
    return core.PolygonMask([np.array([(RX, RY), (RX + RW, RY), (RX + RW, RY + RH), (RX, RY + RH)], np.float32)], invert=True)


@functools.lru_cache(maxsize=None)
def _forward(unmasked=None):
    """the oracle's keypoints and forward rows of every pair, once; `unmasked`: a frame without a mask (detected without it)"""
    gray = {i + 1: oracle.rgb2gray(f) for i, f in enumerate(_clip())}
    gopt, fopt = oracle.gftt_options(), oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    kps = {f: masked_gftt_ref.gftt(g, gopt, None if f == unmasked else _plane())[0] for f, g in gray.items()}
    pyr = {f: oracle.Pyramid(g, WIN, MAX_LEVEL) for f, g in gray.items()}
    rows = {}
    for a in range(1, N + 1):
        for s in SKIPS:
            b = a + s
            if 1 <= b <= N:
                rows[(a, b)] = oracle.lk(pyr[a], pyr[b], kps[a], fopt)
    return kps, rows


@functools.lru_cache(maxsize=None)
def _expected(margin, unmasked=None):
    """-> (keypoints, flows) as the database's blobs, and (forward rows, rows the mask drops)"""
    kps, rows = _forward(unmasked)
    k = {f: (len(v), v.tobytes()) for f, v in kps.items()}
    fl, fwd, dropped = {}, 0, 0
    for (a, b), (q, sf, err) in rows.items():
        st = sf if margin < 0 else ref.keep(q, sf, None if b == unmasked else _plane(), margin)
        keep = np.nonzero(st == 1)[0].astype(np.uint32)
        fl[(a, b)] = (len(keep), keep.tobytes(), q[keep].tobytes(), err[keep].tobytes())
        fwd += int(sf.sum())
        dropped += int(sf.sum()) - len(keep)
    return (k, fl), (fwd, dropped)


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _options(core, margin=None, thr=None):
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    if margin is not None:
        fo.target_mask_margin = margin
    if thr is not None:
        fo.forward_backward_threshold = thr
    return fo


def _run(core, path, mask, margin=None, shard=None, callback=None, thr=None):
    frames = _clip()
    vi = core.VideoInfo(W, H, 1, N)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], callback, path, core.GFTTOptions(), _options(core, margin, thr),
                                            detection_mask=mask)
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], callback, path, shard[0], shard[1],
                                         flow_options=_options(core, margin, thr), detection_mask=mask)
    return _dump(path)


def _records(core, path, mask, margin, cuts):
    """generate_optical_flow_records shard by shard, the logs stored in order"""
    import torch
    frames = _clip()
    vi = core.VideoInfo(W, H, 1, N)
    for b, e in cuts:
        log = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
        used, st = core.generate_optical_flow_records(vi, lambda fid: frames[fid - 1], None, b, e, log.data_ptr(), log.numel(), core.GFTTOptions(),
                                                      _options(core, margin), detection_mask=mask)
        assert st.frames_processed == e - b
        core.write_optical_flow_records(path, log[:used].cpu().numpy(), used)
    return _dump(path)


def _assert_equal(got, want):
    assert got[0] == want[0], "keypoints"
    assert sorted(got[1]) == sorted(want[1])
    for key in sorted(want[1]):
        assert got[1][key] == want[1][key], key


def _check_expectation():
    """asserted on the ORACLE's result, before anything is compared with it"""
    for margin, least in ((0, 100), (3, 300)):
        fwd, dropped = _expected(margin)[1]
        print("margin", margin, "forward rows", fwd, "dropped by the mask", dropped)
        assert dropped >= least and fwd - dropped >= 0.9 * fwd, (margin, fwd, dropped)
    assert _expected(3)[1][1] > _expected(0)[1][1]


@pytest.mark.parametrize("margin", MARGINS)
def test_database_holds_the_oracles_rows_filtered_by_the_targets_choked_plane(core, tmp_path, margin):
    _check_expectation()
    _assert_equal(_run(core, str(tmp_path / "poly.db"), _polygon(core), margin), _expected(margin)[0])


@pytest.mark.parametrize("margin", MARGINS)
def test_records_of_one_shard_and_of_three_are_the_same_rows(core, tmp_path, margin):
    """the halo frames of a shard take the mask: rows that end in them are judged like any others"""
    _check_expectation()
    one = _records(core, str(tmp_path / "one.db"), _polygon(core), margin, [(1, N + 1)])
    _assert_equal(one, _expected(margin)[0])
    three = _records(core, str(tmp_path / "three.db"), _polygon(core), margin, [(1, 5), (5, 9), (9, N + 1)])
    assert three == one
    # ... and so do the shards of the database entry point
    k1, f1 = _run(core, str(tmp_path / "s1.db"), _polygon(core), margin, shard=(1, 7))
    k2, f2 = _run(core, str(tmp_path / "s2.db"), _polygon(core), margin, shard=(7, N + 1))
    assert sorted(k1) == list(range(1, 7)) and not set(k1) & set(k2)
    assert ({**k1, **k2}, {**f1, **f2}) == one


def test_the_same_mask_as_a_byte_plane(core, tmp_path):
    _assert_equal(_run(core, str(tmp_path / "bytes.db"), np.array(_plane()), 3), _expected(3)[0])


def _through_the_thread(core, path, mask, margin):
    frames = _clip()
    th = core.OpticalFlowThread(core.VideoInfo(W, H, 1, N), path, core.GFTTOptions(), _options(core, margin), detection_mask=mask)
    errors, done, t0 = [], False, time.time()
    while not done and time.time() - t0 < 120:
        msg = th.try_pop()
        if msg is None:
            time.sleep(0.0005)
        elif isinstance(msg, core.OpticalFlowRequest):
            th.provide_frame(msg.frame_id, frames[msg.frame_id - 1])
        elif isinstance(msg, core.CppException):
            errors.append(msg.what())
        elif msg is True:
            done = True
    th.join()
    assert done and errors == []
    return _dump(path)


def test_the_same_mask_as_a_dict_through_the_thread(core, tmp_path):
    table = {fid: _polygon(core) for fid in range(1, N + 1)}
    _assert_equal(_through_the_thread(core, str(tmp_path / "thread.db"), table, 3), _expected(3)[0])


def test_a_frame_missing_from_the_dict_keeps_every_row_tracked_into_it(core, tmp_path):
    missing = 7
    table = {fid: _polygon(core) for fid in range(1, N + 1) if fid != missing}
    want, (fwd, dropped) = _expected(3, missing)
    assert want != _expected(3)[0] and dropped > 0
    kps, rows = _forward(missing)
    for (a, b), (q, sf, err) in rows.items():
        if b == missing:
            assert want[1][(a, b)][0] == int(sf.sum()) > 0
    _assert_equal(_run(core, str(tmp_path / "dict.db"), table, 3), want)


def test_a_cancelled_run_resumes_to_the_identical_database(core, tmp_path):
    path = str(tmp_path / "resume.db")

    def cancel_at_6(progress, message):
        return not message.endswith("frame 6")

    k, f = _run(core, path, _polygon(core), 3, callback=cancel_at_6)
    assert sorted(k) == list(range(1, 6)), "frames 1..5 were finished"
    _assert_equal(_run(core, path, _polygon(core), 3), _expected(3)[0])


def test_margin_off_and_margin_without_a_mask_change_nothing(core, tmp_path, monkeypatch):
    # one transaction per frame, so that whole files can be compared (tests/test_lk_fb_gpu.py explains)
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    names = ("mask.db", "mask_off.db", "plain.db", "plain_margin.db", "mask_again.db")
    a, b, c, d, e = (str(tmp_path / n) for n in names)
    _run(core, a, _polygon(core))             # attribute untouched
    _run(core, b, _polygon(core), -1)
    assert open(a, "rb").read() == open(b, "rb").read()
    _assert_equal(_dump(a), _expected(-1)[0])
    _run(core, c, None)
    _run(core, d, None, 5)                    # a margin with nothing to choke
    assert open(c, "rb").read() == open(d, "rb").read() and _dump(c) != _dump(a)
    _run(core, e, _polygon(core), 3)          # the parked engine of the runs above serves these two: nothing is carried over
    _assert_equal(_dump(e), _expected(3)[0])
    _run(core, b + "2", _polygon(core), -1)
    assert open(b + "2", "rb").read() == open(a, "rb").read()


def test_with_the_forward_backward_check_the_status_is_the_and_of_both(core, tmp_path):
    """the mask test runs first; what it leaves goes through the composed check of tests/fb_scene.py"""
    kps, rows = _forward()
    fopt = oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    pyr = {i + 1: oracle.Pyramid(oracle.rgb2gray(f), WIN, MAX_LEVEL) for i, f in enumerate(_clip())}
    want = {}
    for (a, b), (q, sf, err) in rows.items():
        c = fb_scene.composed(pyr[a], pyr[b], kps[a], fopt, 1.0)
        keep = np.nonzero(ref.keep(q, c["status"], _plane(), 3) == 1)[0].astype(np.uint32)
        want[(a, b)] = (len(keep), keep.tobytes(), q[keep].tobytes(), err[keep].tobytes())
    got = _run(core, str(tmp_path / "fb.db"), _polygon(core), 3, thr=1.0)
    assert got[0] == _expected(3)[0][0]
    assert got[1] == want and want != _expected(3)[0][1]
