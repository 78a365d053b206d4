"""GPU: the detection mask (pc_frame_set_mask / pc_analyzer_set_mask / detection_mask=) against the CPU reference
tests/masked_gftt_ref.py -- candidate count, keypoints in value and order, and a response map that does not depend on the mask,
bit for bit, in both arithmetic modes.

Sizes: 67x45 (4x4 cells of 17x12, smaller than a tile: per-pixel atomics), 333x211 (w % 4 != 0: scalar loads, partial tiles),
320x200 (float4 / dword paths), 640x360 (cells of 160x90: tiles inside one cell and across two or four)."""
import functools
import os
import sqlite3
import sys

import numpy as np
import pytest

import masked_gftt_ref as ref
import oracle
from polychase_amd import hip, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "opencv_x86": (hip.ARITH_OPENCV_X86, oracle.EMU_OPENCV_X86)}
SIZES = [(67, 45), (333, 211), (320, 200), (640, 360)]
OPTION_SETS = dict(ref.OPTION_SETS, dist100=dict(min_distance=100.0))     # + the large-radius suppression kernel
MASKS = {
    "disc": ref.mask_column_and_disc,
    "speckle": ref.mask_speckle,
    "ring": ref.mask_ring,
}


@functools.lru_cache(maxsize=None)
def _image(size):
    g = ref.test_image(*size)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _mask(size, name):
    m = MASKS[name](*size)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _expected(arith, size, optname, maskname):
    """the reference, once per case; shared, never modified"""
    with oracle.emulation(ARITH[arith][1]):
        kps, eig, ncand = ref.gftt(_image(size), oracle.gftt_options(**OPTION_SETS[optname]), _mask(size, maskname) if maskname else None)
    kps.setflags(write=False)
    eig.setflags(write=False)
    return kps, eig, ncand


@pytest.fixture(scope="module", params=sorted(ARITH))
def actx(request):
    ctx = hip.Context(0)
    ctx.set_arithmetic(ARITH[request.param][0])
    yield request.param, ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _detect(ctx, size, optname, mask):
    w, h = size
    f = hip.Frame(ctx, w, h)
    f.set_gray(_image(size))
    f.set_mask(mask)
    f.detect(hip.gftt_options(**OPTION_SETS[optname]))
    out = f.keypoints(), f.min_eig(), f.num_candidates
    f.close()
    return out


@pytest.mark.parametrize("optname", sorted(OPTION_SETS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_masked_detection_matches_the_reference(actx, size, optname):
    arith, ctx = actx
    m = _mask(size, "disc")
    ekps, eeig, encand = _expected(arith, size, optname, "disc")
    opt = oracle.gftt_options(**OPTION_SETS[optname])
    if optname != "dist100" or size != (67, 45):     # (one corner survives a 100 px radius on the smallest frame either way)
        with oracle.emulation(ARITH[arith][1]):
            assert not np.array_equal(ekps, ref.post_filtered(_image(size), opt, m)), "the case must tell a post-filter apart"
    kps, eig, ncand = _detect(ctx, size, optname, m)
    assert np.array_equal(_bits(eig), _bits(eeig)), "the response map does not depend on the mask"
    assert ncand == encand
    assert np.array_equal(kps, ekps), "keypoints must match in value AND order"


@pytest.mark.parametrize("maskname", ["speckle", "ring"])
@pytest.mark.parametrize("optname", ["default", "harris"])       # the fused kernel / the general kernels
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_speckle_and_ring_masks(actx, size, optname, maskname):
    arith, ctx = actx
    ekps, eeig, encand = _expected(arith, size, optname, maskname)
    kps, eig, ncand = _detect(ctx, size, optname, _mask(size, maskname))
    assert np.array_equal(_bits(eig), _bits(eeig))
    assert ncand == encand and np.array_equal(kps, ekps)
    if maskname == "ring":
        assert ncand == 0 and len(kps) == 0      # every cell maximum comes from border pixels, no interior pixel is on


@pytest.mark.parametrize("optname", ["default", "harris", "nodist"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_all_on_is_no_mask_and_all_off_is_nothing(actx, size, optname):
    arith, ctx = actx
    w, h = size
    kps0, eig0, n0 = _detect(ctx, size, optname, None)
    ekps, eeig, encand = _expected(arith, size, optname, None)
    assert n0 == encand and np.array_equal(kps0, ekps) and np.array_equal(_bits(eig0), _bits(eeig))
    kps1, eig1, n1 = _detect(ctx, size, optname, np.full((h, w), 255, np.uint8))
    assert n1 == n0 and kps1.tobytes() == kps0.tobytes() and eig1.tobytes() == eig0.tobytes()
    kps2, eig2, n2 = _detect(ctx, size, optname, np.zeros((h, w), np.uint8))
    assert n2 == 0 and len(kps2) == 0 and eig2.tobytes() == eig0.tobytes()


@pytest.mark.parametrize("size", [(333, 211), (320, 200)], ids=lambda s: "%dx%d" % s)
def test_row_pitch_above_width_and_mask_replacement(actx, size):
    arith, ctx = actx
    w, h = size
    wide = np.full((h, w + 13), 255, np.uint8)      # the bytes beyond the width say "on": reading them would show
    wide[:, :w] = _mask(size, "disc")
    f = hip.Frame(ctx, w, h)
    f.set_gray(_image(size))
    f.set_mask(wide[:, :w])
    f.detect()
    assert f.num_candidates == _expected(arith, size, "default", "disc")[2]
    assert np.array_equal(f.keypoints(), _expected(arith, size, "default", "disc")[0])
    f.set_mask(_mask(size, "speckle"))               # replaced ...
    f.detect()
    assert np.array_equal(f.keypoints(), _expected(arith, size, "default", "speckle")[0])
    f.set_mask(None)                                 # ... and cleared
    f.detect()
    assert np.array_equal(f.keypoints(), _expected(arith, size, "default", None)[0])
    with pytest.raises(hip.PolychaseHipError):
        hip._check(hip.load().pc_frame_set_mask(ctx._h, f._h, wide.ctypes.data, w - 1, 0))    # row_pitch < width
    f.close()


def test_masked_frame_that_overflows_a_value_bucket_is_redone_with_its_mask():
    """the input of tests/test_fused_chain_gpu.py (a value bucket beyond its slots -> slow-path redo) plus the disc mask"""
    w, h = 320, 240
    g = np.zeros((h, w), np.uint8)
    g[4:h - 4:4, 4:w - 4:4] = 200
    m = ref.mask_column_and_disc(w, h)
    ekps, eeig, encand = ref.gftt(g, oracle.gftt_options(), m)
    assert encand > 4 * 512 and np.unique(eeig[eeig > 0.01 * eeig.max()]).size < 16, "the frame must overflow a value bucket"
    ctx = hip.Context(0)
    f = hip.Frame(ctx, w, h)
    f.set_gray(g)
    f.set_mask(m)
    for _ in range(2):
        f.detect()
        assert f.num_candidates == encand
        assert np.array_equal(f.keypoints(), ekps)
    f.close()
    ctx.close()


# ---- analyzer / database ----
@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


W, H, N = 320, 240, 12
SKIPS = (-8, -4, -2, -1, 1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def _clip():
    c = synth.NoiseClip(W, H, N)
    return [c.frame(i) for i in range(N)]


def _moving_mask(fid):
    """a rectangle that moves with the frame; frame 4 has no mask, frame 9 an empty one"""
    if fid == 4:
        return None
    m = np.zeros((H, W), np.uint8)
    if fid != 9:
        m[20 + 5 * fid:150 + 5 * fid, 15 * fid:120 + 15 * fid] = (1, 128, 255)[fid % 3]
    return m


def _static_mask():
    m = np.zeros((H, W), np.uint8)
    m[30:200, 100:300] = 7
    return m


@functools.lru_cache(maxsize=None)
def _clip_expected(kind):
    """{frame: (rows, blob)}, {(from, to): (rows, idx, xy, err blobs)}: the reference's keypoints per frame under that frame's
    mask, oracle.lk from those keypoints for every pair (the product's default arithmetic = the oracle's default emulation)"""
    frames = _clip()
    gray = {i + 1: oracle.rgb2gray(f) for i, f in enumerate(frames)}
    pyr = {i: oracle.Pyramid(g) for i, g in gray.items()}
    static = _static_mask()
    k, fl = {}, {}
    for a in range(1, N + 1):
        mask = {"moving": _moving_mask(a), "static": static, "none": None}[kind]
        kps = ref.gftt(gray[a], oracle.gftt_options(), mask)[0]
        if mask is not None:
            assert np.all(mask[kps[:, 1].astype(int), kps[:, 0].astype(int)] != 0)
        k[a] = (len(kps), kps.tobytes())
        for s in SKIPS:
            b = a + s
            if not 1 <= b <= N:
                continue
            xy, st, err = oracle.lk(pyr[a], pyr[b], kps)
            idx = np.nonzero(st == 1)[0].astype(np.uint32)
            fl[(a, b)] = (len(idx), idx.tobytes(), xy[idx].tobytes(), err[idx].tobytes())
    return k, fl


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], r[2]) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): tuple(r[2:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _nonempty(d):
    """rows with nothing in them compare equal to rows that are absent (a frame without keypoints has no flow)"""
    return {key: (v[0],) + tuple(bytes(b) for b in v[1:]) for key, v in d.items() if v[0] > 0}


def _run(core, path, mask, thr=None, shard=None):
    frames = _clip()
    fo = core.OpticalFlowOptions()
    if thr is not None:
        fo.forward_backward_threshold = thr
    vi = core.VideoInfo(W, H, 1, N)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, core.GFTTOptions(), fo, detection_mask=mask)
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], None, path, shard[0], shard[1], flow_options=fo,
                                         detection_mask=mask)


def _check_db(path, kind):
    ek, ef = _clip_expected(kind)
    k, f = _dump(path)
    assert _nonempty(k) == _nonempty(ek)
    assert _nonempty(f) == _nonempty(ef)
    return k, f


def test_database_with_a_mask_per_frame(core, tmp_path):
    asked = []

    def mask(fid):
        asked.append(fid)
        return _moving_mask(fid)

    path = str(tmp_path / "moving.db")
    _run(core, path, mask)
    assert asked == list(range(1, N + 1)), "asked once per detected frame, in order"
    k, f = _check_db(path, "moving")
    assert k.get(9, (0, b""))[0] == 0 and k[4][0] == _clip_expected("none")[0][4][0]
    # forward-backward check on top: runs, keeps the keypoints, and keeps a subset of the rows
    path_fb = str(tmp_path / "moving_fb.db")
    _run(core, path_fb, _moving_mask, thr=1.0)
    kf, ff = _dump(path_fb)
    assert _nonempty(kf) == _nonempty(k)
    for key, v in _nonempty(ff).items():
        idx, full = np.frombuffer(v[1], np.uint32), np.frombuffer(_nonempty(f)[key][1], np.uint32)
        assert np.all(np.isin(idx, full)), key


def test_database_with_one_static_mask_then_none(core, tmp_path):
    _run(core, str(tmp_path / "static.db"), _static_mask())
    _check_db(str(tmp_path / "static.db"), "static")
    # the parked engine of the masked run serves this one: it must have carried nothing over
    _run(core, str(tmp_path / "plain.db"), None)
    k, f = _check_db(str(tmp_path / "plain.db"), "none")
    ok, of = oracle.analyze_clip(_clip(), first_frame=1, threads=4)       # today's output
    assert {a: v[1] for a, v in k.items()} == {a: v.tobytes() for a, v in ok.items()}


def test_a_resumed_run_keeps_the_stored_keypoints_whatever_the_mask(core, tmp_path):
    path = str(tmp_path / "resume.db")
    _run(core, path, _moving_mask, shard=(1, 7))
    k1, f1 = _dump(path)
    assert sorted(k1) == list(range(1, 7))
    asked = []

    def other(fid):
        asked.append(fid)
        return _static_mask()

    _run(core, path, other)
    assert asked == list(range(7, N + 1)), "frames whose keypoints row exists are not asked about"
    k2, f2 = _dump(path)
    assert {a: k2[a] for a in k1} == k1 and {p: f2[p] for p in f1} == f1
    ek = _clip_expected("static")[0]
    assert {a: (k2[a][0], bytes(k2[a][1])) for a in range(7, N + 1)} == {a: ek[a] for a in range(7, N + 1)}


def test_two_shards_with_a_mask_per_frame_give_the_records_of_one(core, tmp_path):
    s1, s2 = str(tmp_path / "s1.db"), str(tmp_path / "s2.db")
    _run(core, s1, _moving_mask, shard=(1, 7))
    _run(core, s2, _moving_mask, shard=(7, N + 1))
    k1, f1 = _dump(s1)
    k2, f2 = _dump(s2)
    assert sorted(k1) == list(range(1, 7)) and not set(k1) & set(k2)
    ek, ef = _clip_expected("moving")
    assert _nonempty({**k1, **k2}) == _nonempty(ek) and _nonempty({**f1, **f2}) == _nonempty(ef)


def test_analyzer_keeps_the_mask_a_detection_was_enqueued_with():
    """the ring holds ~20 detections in flight: every frame is put under its own mask before any job is collected"""
    frames = _clip()
    ek = _clip_expected("moving")[0]
    ctx = hip.Context(0)
    an = hip.Analyzer(ctx, W, H)
    for fid in range(1, N + 1):
        an.set_mask(_moving_mask(fid))
        an.put_frame(fid, frames[fid - 1], will_detect=True)
    an.set_mask(np.zeros((H, W), np.uint8))          # must not reach the detections already enqueued
    got = {}
    for fid in range(1, N + 1):
        an.submit(fid, [])
        r = an.collect()
        got[r[0]] = (len(r[1]), r[1].tobytes())
    an.reset()
    an.put_frame(1, frames[0], will_detect=True)     # reset cleared the mask
    an.submit(1, [])
    assert an.collect()[1].tobytes() == _clip_expected("none")[0][1][1]
    an.close()
    ctx.close()
    assert _nonempty(got) == _nonempty(ek)
