"""GPU: lens undistortion through polychase_core (OpticalFlowOptions.lens = LensModel | int32 (H, W, 2) array).  The clip is the
recipe scene of tests/test_lens_cpu.py cropped to 131 x 98 (the crop moves the model's principal point): 10 distorted frames, a
pan of (1.1, -0.7) per frame, window 10.  Equalities only:

  * the database of a run with lens = LensModel(...) holds, byte for byte, the rows of oracle.analyze_clip on the frames that
    tests/lens_ref.py undistorts; the equivalent map as an array gives the same file's rows;
  * under the pincushion model, whose corners leave the original frame, the default detection mask is in force: the rows are the
    oracle's for keypoints detected under pc_lens_map_valid eroded by window_size // 2 + 1 (tests/masked_gftt_ref.py), and the
    mask is seen to act;
  * OpticalFlowThread and two shards give the same database;
  * an all-valid lens allocates the map and the two planes and nothing else."""
import functools
import os
import sqlite3
import sys
import time

import numpy as np
import pytest

import lens_ref as ref
import masked_gftt_ref
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, WIN, MAX_LEVEL = 131, 98, 10, 10, 3
OX, OY = 94, 71
SKIPS = (-8, -4, -2, -1, 1, 2, 4, 8)
PAIRS = sum(1 for a in range(1, N + 1) for s in SKIPS if 1 <= a + s <= N)


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


def _recipe():
    return dict(ref.recipe_model(320, 240), cx=159.5 - OX, cy=119.5 - OY)


def _pincushion():
    return ref.pincushion(W, H)


@functools.lru_cache(maxsize=None)
def _clip(which):
    """the distorted frames as (H, W, 3) uint8 with R = G = B, the model, its map"""
    m = _recipe() if which == "recipe" else _pincushion()
    _, dist = ref.scene_frames(W, H, m, [(1.1 * k, -0.7 * k) for k in range(N)], seed=1)
    frames = [np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) for g in dist]
    assert all(np.array_equal(oracle.rgb2gray(f), g) for f, g in zip(frames, dist)), "equal channels: the gray plane is the channel"
    return frames, m, ref.build_map(m, W, H)


@functools.lru_cache(maxsize=None)
def _undistorted(which):
    frames, _, q = _clip(which)
    und = [ref.remap(f[:, :, 0], q) for f in frames]
    assert not any(np.array_equal(u, f[:, :, 0]) for u, f in zip(und, frames))
    return und


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _nonempty(d):
    return {a: v for a, v in d.items() if v[0] > 0}


def _options(core, lens):
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    fo.lens = lens
    return fo


def _run(core, path, which, lens, shard=None):
    frames = _clip(which)[0]
    vi = core.VideoInfo(W, H, 1, N)
    fo = _options(core, lens)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, core.GFTTOptions(), fo)
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], None, path, shard[0], shard[1], flow_options=fo)
    return _dump(path)


@functools.lru_cache(maxsize=None)
def _expected_recipe():
    und = [np.ascontiguousarray(np.repeat(u[:, :, None], 3, axis=2)) for u in _undistorted("recipe")]
    kps, flows = oracle.analyze_clip(und, first_frame=1, fopt=oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL), threads=4)
    k = {f: (len(v), v.tobytes()) for f, v in kps.items()}
    fl = {key: (len(v[0]), v[0].tobytes(), v[1].tobytes(), v[2].tobytes()) for key, v in flows.items()}
    return k, fl


@functools.lru_cache(maxsize=None)
def _default_mask():
    q = _clip("pincushion")[2]
    m = ref.valid(q, WIN // 2 + 1)
    assert np.array_equal(m, hip.lens_map_valid(q, WIN // 2 + 1))
    assert 0.01 < (m == 0).mean() < 0.6
    return m


@functools.lru_cache(maxsize=None)
def _expected_pincushion():
    """the oracle's keypoints under the eroded validity plane and its LK rows for them, as the database's blobs"""
    und = _undistorted("pincushion")
    gopt, fopt = oracle.gftt_options(), oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    kps = {i + 1: masked_gftt_ref.gftt(g, gopt, _default_mask())[0] for i, g in enumerate(und)}
    pyr = {i + 1: oracle.Pyramid(g, WIN, MAX_LEVEL) for i, g in enumerate(und)}
    k = {f: (len(v), v.tobytes()) for f, v in kps.items()}
    fl = {}
    for a in range(1, N + 1):
        for s in SKIPS:
            b = a + s
            if 1 <= b <= N:
                xy, st, err = oracle.lk(pyr[a], pyr[b], kps[a], fopt)
                keep = np.nonzero(st == 1)[0].astype(np.uint32)
                fl[(a, b)] = (len(keep), keep.tobytes(), xy[keep].tobytes(), err[keep].tobytes())
    return k, fl


def test_the_recipe_lens_is_all_valid_and_the_pincushion_is_not():
    assert (ref.valid(_clip("recipe")[2], WIN // 2 + 1) == 255).all()
    assert (_default_mask() == 0).any()


def test_database_under_a_lens_model_and_under_the_equivalent_array(core, tmp_path):
    _, m, q = _clip("recipe")
    lens = core.LensModel(**m)
    assert np.array_equal(lens.build_map(W, H), q)
    k, f = _run(core, str(tmp_path / "model.db"), "recipe", lens)
    ek, ef = _expected_recipe()
    assert min(v[0] for v in ek.values()) > 20 and len(_nonempty(ef)) == PAIRS
    assert _nonempty(k) == _nonempty(ek)
    assert _nonempty(f) == _nonempty(ef)
    assert _run(core, str(tmp_path / "array.db"), "recipe", q) == (k, f)
    # ... and it is the lens that does it: without one the rows are others, and the parked engine carries no map over
    plain = _run(core, str(tmp_path / "plain.db"), "recipe", None)
    assert _nonempty(plain[0]) != _nonempty(ek)
    frames = _clip("recipe")[0]
    pk, pf = oracle.analyze_clip(frames, first_frame=1, fopt=oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL), threads=4)
    assert _nonempty(plain[0]) == _nonempty({a: (len(v), v.tobytes()) for a, v in pk.items()})
    # the option reads back what was set
    fo = _options(core, lens)
    assert isinstance(fo.lens, core.LensModel) and fo.lens.k1 == m["k1"] and fo.lens.zoom == 1.0
    fo.lens = q
    assert np.array_equal(fo.lens, q)
    fo.lens = None
    assert fo.lens is None
    assert np.array_equal(core.lens_map_valid(q, 3), ref.valid(q, 3))


def test_the_default_mask_of_a_lens_that_leaves_the_frame(core, tmp_path):
    _, m, q = _clip("pincushion")
    k, f = _run(core, str(tmp_path / "pincushion.db"), "pincushion", core.LensModel(**m))
    ek, ef = _expected_pincushion()
    assert min(v[0] for v in ek.values()) > 10
    assert _nonempty(k) == _nonempty(ek)
    assert _nonempty(f) == _nonempty(ef)
    # the mask acts: the unmasked detector finds a keypoint where the mask is off
    mask = _default_mask()
    free = oracle.gftt(_undistorted("pincushion")[0])
    xy = np.rint(free).astype(int)
    assert (mask[xy[:, 1], xy[:, 0]] == 0).any()
    # a caller's mask is used as given, in undistorted coordinates
    mine = np.zeros((H, W), np.uint8)
    mine[20:80, 30:110] = 255
    frames = _clip("pincushion")[0]
    path = str(tmp_path / "mine.db")
    core.generate_optical_flow_database(core.VideoInfo(W, H, 1, N), lambda fid: frames[fid - 1], None, path, core.GFTTOptions(),
                                        _options(core, core.LensModel(**m)), detection_mask=mine)
    gopt = oracle.gftt_options()
    want = {i + 1: masked_gftt_ref.gftt(g, gopt, mine)[0] for i, g in enumerate(_undistorted("pincushion"))}
    assert _nonempty(_dump(path)[0]) == _nonempty({a: (len(v), v.tobytes()) for a, v in want.items()})


def test_the_thread_and_two_shards_give_the_same_database(core, tmp_path):
    frames, m, q = _clip("recipe")
    want = (_nonempty(_expected_recipe()[0]), _nonempty(_expected_recipe()[1]))
    path = str(tmp_path / "thread.db")
    th = core.OpticalFlowThread(core.VideoInfo(W, H, 1, N), path, core.GFTTOptions(), _options(core, core.LensModel(**m)))
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
    k, f = _dump(path)
    assert (_nonempty(k), _nonempty(f)) == want
    k1, f1 = _run(core, str(tmp_path / "s1.db"), "recipe", q, shard=(1, 6))
    k2, f2 = _run(core, str(tmp_path / "s2.db"), "recipe", q, shard=(6, N + 1))
    assert sorted(k1) == list(range(1, 6)) and not set(k1) & set(k2)
    assert (_nonempty({**k1, **k2}), _nonempty({**f1, **f2})) == want


def test_bad_lens_options_are_refused_before_any_frame_is_asked_for(core, tmp_path):
    asked = []
    vi = core.VideoInfo(W, H, 1, N)

    def accessor(fid):
        asked.append(fid)
        return None

    for lens in (core.LensModel(0.0, 300.0, 1.0, 1.0), core.LensModel(300.0, 300.0, float("nan"), 1.0),
                 core.LensModel(300.0, 300.0, 1.0, 1.0, zoom=-1.0), ref.identity_map(W + 1, H)):
        with pytest.raises(ValueError):
            core.generate_optical_flow_database(vi, accessor, None, str(tmp_path / "bad.db"), core.GFTTOptions(), _options(core, lens))
    fo = core.OpticalFlowOptions()
    for bad in (np.zeros((H, W, 2), np.float32), np.zeros((H, W), np.int32), np.zeros((H, W, 3), np.int32), "barrel"):
        with pytest.raises(ValueError):
            fo.lens = bad
    assert asked == []


def test_an_all_valid_lens_allocates_the_map_and_two_planes_only(core, tmp_path):
    core.release_cached_engine()
    idle = hip.live_resources()
    _run(core, str(tmp_path / "a.db"), "recipe", None)
    plain = hip.live_resources()                      # the parked engine of a run without a lens
    core.release_cached_engine()
    assert hip.live_resources()[0] == idle[0]
    _run(core, str(tmp_path / "b.db"), "recipe", core.LensModel(**_clip("recipe")[1]))
    with_lens = hip.live_resources()
    core.release_cached_engine()
    _run(core, str(tmp_path / "c.db"), "pincushion", core.LensModel(**_clip("pincushion")[1]))
    masked = hip.live_resources()
    core.release_cached_engine()
    print("device allocations: idle %d, plain run %d, all-valid lens %d, lens with a default mask %d" % (idle[0], plain[0], with_lens[0], masked[0]))
    assert with_lens[0] == plain[0] + 3, "the map and the two planes: no mask plane"
    assert with_lens[2:] == plain[2:], "no stream, no event"
    assert masked[0] > with_lens[0], "the default mask has planes: the count can tell"
    assert hip.live_resources()[0] == idle[0]
