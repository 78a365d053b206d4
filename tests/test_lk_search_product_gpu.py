"""GPU: the search prepass through polychase_core (OpticalFlowOptions.search_radius).  The clip is tests/lk_search_scene.py's: 6
frames of 160 x 120 (R = G = B, so gray is the channel) panning by 12 px per frame, window 10, max_level 2, search_radius 64; the
detector keeps its 24 strongest corners per frame.  The rows of the default run ARE the forward records with status 1, so the
database of a run with the option must hold, pair by pair, what the numpy restatement of the rule (tests/lk_search_ref.py) makes of
them -- rows the forward launch had given up included."""
import functools
import os
import sqlite3
import sys

import numpy as np
import pytest

import lk_search_ref as ref
import lk_search_scene as scene
import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, STEP = scene.W, scene.H, 6, 12
WIN, MAX_LEVEL, R = 10, 2, 64
MAX_CORNERS = 24


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@functools.lru_cache(maxsize=None)
def _clip():
    return scene.clip(N, STEP)


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _options(core, search_radius=None, normalize=None):
    go = core.GFTTOptions()
    go.max_corners = MAX_CORNERS
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    if search_radius is not None:
        fo.search_radius = search_radius
    if normalize is not None:
        fo.normalize = normalize
    return go, fo


def _run(core, path, search_radius=None, normalize=None, asked=None):
    frames = _clip()

    def accessor(fid):
        if asked is not None:
            asked.append(fid)
        return frames[fid - 1]

    go, fo = _options(core, search_radius, normalize)
    core.generate_optical_flow_database(core.VideoInfo(W, H, 1, N), accessor, None, path, go, fo)
    return _dump(path)


def _good(kps, idx, xy, a, b):
    """rows within 0.5 px of the analytic flow of the pan"""
    end = kps[idx] + np.float32([-(b - a) * STEP, 0.0])
    return int((np.hypot(*(xy - end).T) <= 0.5).sum())


def test_database_holds_what_the_rule_makes_of_the_default_runs_rows(core, tmp_path):
    default = _run(core, str(tmp_path / "default.db"))
    got = _run(core, str(tmp_path / "search.db"), R)
    assert got[0] == default[0], "keypoints"
    with oracle.emulation(oracle.EMU_CANONICAL):
        planes = {i + 1: ref.Planes(oracle.Pyramid(np.ascontiguousarray(f[:, :, 0]), WIN, MAX_LEVEL)) for i, f in enumerate(_clip())}
    oopt = oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    want, replaced, rescued = {}, 0, 0
    good_off, good_on = 0, 0
    pairs = [(a, a + s) for a in range(1, N + 1) for s in (-8, -4, -2, -1, 1, 2, 4, 8) if 1 <= a + s <= N]
    for (a, b) in pairs:
        kps = np.frombuffer(default[0][a][1], np.float32).reshape(-1, 2)
        assert 12 <= len(kps) <= MAX_CORNERS
        q, st, e = np.zeros((len(kps), 2), np.float32), np.zeros(len(kps), np.uint8), np.zeros(len(kps), np.float32)
        if (a, b) in default[1]:
            _, idx, xy, err = default[1][(a, b)]
            idx = np.frombuffer(idx, np.uint32)
            q[idx], st[idx], e[idx] = np.frombuffer(xy, np.float32).reshape(-1, 2), 1, np.frombuffer(err, np.float32)
            if abs(b - a) == 4:
                good_off += _good(kps, idx, q[idx], a, b)
        r = ref.search(planes[a], [planes[b]], kps, [(q, st, e)], oopt, R)[0]
        sel = np.nonzero(r[1] == 1)[0].astype(np.uint32)
        if len(sel):
            want[(a, b)] = (len(sel), sel.tobytes(), r[0][sel].tobytes(), r[2][sel].tobytes())
        replaced += int((r[4] == ref.REPLACED).sum())
        rescued += int(((r[4] == ref.REPLACED) & (st == 0)).sum())
        if abs(b - a) == 4:
            good_on += _good(kps, sel, r[0][sel], a, b)
    # asserted on the REFERENCE's result, before anything is compared with it: the option replaces rows, rescues rows the forward
    # launch had given up, and on the pairs 4 frames (48 px) apart holds at least 3 x the rows within 0.5 px of the analytic flow
    print("reference: replaced", replaced, "of them rescued", rescued, "good rows on the +-4 pairs: off", good_off, "on", good_on)
    assert replaced >= 40 and rescued >= 1 and good_on >= 10 and good_on >= 3 * good_off
    assert sorted(got[1]) == sorted(want)
    for pair in sorted(want):
        assert got[1][pair] == want[pair], pair
    # ... and so does the database
    db_off = sum(_good(np.frombuffer(default[0][a][1], np.float32).reshape(-1, 2), np.frombuffer(v[1], np.uint32),
                       np.frombuffer(v[2], np.float32).reshape(-1, 2), a, b) for (a, b), v in default[1].items() if abs(b - a) == 4)
    db_on = sum(_good(np.frombuffer(got[0][a][1], np.float32).reshape(-1, 2), np.frombuffer(v[1], np.uint32),
                      np.frombuffer(v[2], np.float32).reshape(-1, 2), a, b) for (a, b), v in got[1].items() if abs(b - a) == 4)
    assert db_off == good_off and db_on == good_on and db_on >= 3 * db_off


def test_two_shards_give_the_one_shard_database(core, tmp_path):
    frames = _clip()
    one = _run(core, str(tmp_path / "one.db"), R)
    go, fo = _options(core, R)
    parts = []
    for k, (begin, end) in enumerate(((1, 4), (4, N + 1))):
        path = str(tmp_path / f"s{k}.db")
        core.generate_optical_flow_shard(core.VideoInfo(W, H, 1, N), lambda fid: frames[fid - 1], None, path, begin, end, detector_options=go,
                                         flow_options=fo)
        parts.append(_dump(path))
    (k1, f1), (k2, f2) = parts
    assert sorted(k1) == [1, 2, 3] and not set(k1) & set(k2) and f1 and f2
    assert ({**k1, **k2}, {**f1, **f2}) == one


def test_radius_0_gives_the_file_of_a_run_that_never_sets_the_attribute(core, tmp_path, monkeypatch):
    # one transaction per frame, so that whole files can be compared (tests/test_lk_fb_gpu.py explains)
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    a, b, c = (str(tmp_path / n) for n in ("untouched.db", "off.db", "on.db"))
    _run(core, a)
    _run(core, b, 0)
    assert open(a, "rb").read() == open(b, "rb").read()
    _run(core, c, R)
    assert open(c, "rb").read() != open(a, "rb").read() and _dump(c) != _dump(a)
    _run(core, b + "2", 0)      # the parked engine of the run above carries nothing over
    assert open(b + "2", "rb").read() == open(a, "rb").read()


def test_a_bad_radius_and_the_combination_with_normalize_are_value_errors_before_a_frame_is_asked_for(core, tmp_path):
    asked = []
    for radius in (-1, 257):
        with pytest.raises(ValueError, match="search_radius"):
            _run(core, str(tmp_path / "bad.db"), radius, asked=asked)
    with pytest.raises(ValueError, match="search_radius"):
        _run(core, str(tmp_path / "both.db"), R, True, asked=asked)
    assert not asked
    assert not os.path.exists(str(tmp_path / "bad.db")) and not os.path.exists(str(tmp_path / "both.db"))
