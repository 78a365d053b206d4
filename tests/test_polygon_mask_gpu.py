"""GPU: polygon detection masks, stage level.  The plane the rasteriser kernel writes (Frame.set_mask_polygons, Frame.mask)
against the integer reference tests/polygon_mask_ref.py, byte for byte; detection under a polygon mask against detection under
the reference plane and against tests/masked_gftt_ref.py, bit for bit; the analyzer with a polygon per frame.

Sizes: 67x45 (one tile column, w % 4 = 3: byte stores at every row end, rows that start off a dword), 333x211 (w % 4 = 1, a last
band of 3 rows), 320x200 (dword stores only), 640x360.  None of them is wider than one 1024-pixel tile: 1100x45 adds the second
tile column, where edges wholly left of the tile are dropped."""
import functools

import numpy as np
import pytest

import masked_gftt_ref as gref
import oracle
import polygon_mask_ref as ref
from polychase_amd import hip, synth

pytestmark = pytest.mark.gpu

SIZES = [(67, 45), (333, 211), (320, 200), (640, 360)]
ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "opencv_x86": (hip.ARITH_OPENCV_X86, oracle.EMU_OPENCV_X86)}
OPTION_SETS = {"default": {}, "harris": dict(use_harris=1), "dist100": dict(min_distance=100.0)}


@functools.lru_cache(maxsize=None)
def _plane(name, size):
    """the reference plane, once per case; shared, never modified"""
    m = ref.plane(ref.SHAPES[name](*size), *size)
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("size", SIZES + [(1100, 45)], ids=lambda s: "%dx%d" % s)
def test_the_plane_is_the_reference_plane_byte_for_byte(ctx, size):
    w, h = size
    f = hip.Frame(ctx, w, h)
    for name in sorted(ref.SHAPES):
        polys = ref.SHAPES[name](w, h)
        e = _plane(name, size)
        f.set_mask_polygons(polys)
        got = f.mask()
        assert np.array_equal(got, e), (name, int((got != e).sum()), np.argwhere(got != e)[:4].tolist())
        f.set_mask_polygons(polys, invert=True)
        got = f.mask()
        assert np.array_equal(got, 255 - e), (name, "invert", int((got != 255 - e).sum()))
    f.close()


@functools.lru_cache(maxsize=None)
def _image(size):
    g = gref.test_image(*size)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _expected(arith, size, optname, shape):
    with oracle.emulation(ARITH[arith][1]):
        kps = gref.gftt(_image(size), oracle.gftt_options(**OPTION_SETS[optname]), _plane(shape, size) if shape else None)[0]
    kps.setflags(write=False)
    return kps


@pytest.fixture(scope="module", params=sorted(ARITH))
def actx(request):
    c = hip.Context(0)
    c.set_arithmetic(ARITH[request.param][0])
    yield request.param, c
    c.close()


@pytest.mark.parametrize("optname", sorted(OPTION_SETS))
@pytest.mark.parametrize("size", [(333, 211), (320, 200)], ids=lambda s: "%dx%d" % s)
def test_detection_under_polygons_is_detection_under_their_plane(actx, size, optname):
    arith, c = actx
    w, h = size
    opt = hip.gftt_options(**OPTION_SETS[optname])
    f = hip.Frame(c, w, h)
    f.set_gray(_image(size))
    f.set_mask_polygons(ref.star(w, h))
    f.detect(opt)
    kp, ncp = f.keypoints(), f.num_candidates
    f.set_mask(_plane("star", size))
    f.detect(opt)
    kb, ncb = f.keypoints(), f.num_candidates
    f.close()
    e = _expected(arith, size, optname, "star")
    assert len(e) > 0
    assert ncp == ncb and kp.tobytes() == kb.tobytes(), "bit-equal, in order, to the byte mask's keypoints"
    assert np.array_equal(kp, e), "and to the reference's"


def test_replacing_polygons_by_bytes_polygons_and_none(actx):
    arith, c = actx
    size = w, h = (333, 211)
    f = hip.Frame(c, w, h)
    f.set_gray(_image(size))
    with pytest.raises(hip.PolychaseHipError):
        f.mask()                                              # no mask on: PC_E_STATE
    f.set_mask_polygons(ref.star(w, h))
    f.detect()
    assert np.array_equal(f.keypoints(), _expected(arith, size, "default", "star"))
    disc = gref.mask_column_and_disc(w, h)
    f.set_mask(disc)                                          # replaced by bytes ...
    assert np.array_equal(f.mask(), disc)
    f.detect()
    with oracle.emulation(ARITH[arith][1]):
        assert np.array_equal(f.keypoints(), gref.gftt(_image(size), oracle.gftt_options(), disc)[0])
    f.set_mask_polygons(ref.bow_tie(w, h))                    # ... by other polygons ...
    assert np.array_equal(f.mask(), _plane("bow_tie", size))
    f.detect()
    assert np.array_equal(f.keypoints(), _expected(arith, size, "default", "bow_tie"))
    f.set_mask_polygons([])                                   # ... by none of them: nothing is found
    f.detect()
    assert f.num_candidates == 0 and len(f.keypoints()) == 0
    f.set_mask_polygons([], invert=True)                      # everything on: the unmasked keypoints
    f.detect()
    assert np.array_equal(f.keypoints(), _expected(arith, size, "default", None))
    f.set_mask_polygons(ref.star(w, h))
    f.set_mask(None)                                          # ... and cleared
    with pytest.raises(hip.PolychaseHipError):
        f.mask()
    f.detect()
    assert np.array_equal(f.keypoints(), _expected(arith, size, "default", None))
    f.close()


def test_refused_polygons_leave_the_previous_mask_in_force(ctx):
    size = w, h = (320, 200)
    L = hip.load()
    f = hip.Frame(ctx, w, h)
    an = hip.Analyzer(ctx, w, h)
    f.set_mask_polygons(ref.star(w, h))
    bad = {
        "33 polygons": [ref.rectangle(w, h)[0]] * 33,
        "a count of 2": [ref.rectangle(w, h)[0][:2]],
        "4097 vertices": [np.concatenate([ref.circle4096(w, h)[0], [[1, 1]]]).astype(np.float32)],
        "nan": [np.array([(1, 1), (np.nan, 2), (4, 8)], np.float32)],
        "out of range": [np.array([(1, 1), (40000, 2), (4, 8)], np.float32)],
    }
    for name, polys in bad.items():
        xy, counts = hip._polygon_arrays(polys)
        assert L.pc_frame_set_mask_polygons(ctx._h, f._h, xy.ctypes.data, counts.ctypes.data, len(counts), 0) == -1, name
        assert L.pc_analyzer_set_mask_polygons(an._h, xy.ctypes.data, counts.ctypes.data, len(counts), 0) == -1, name
        with pytest.raises(hip.PolychaseHipError):
            f.set_mask_polygons(polys)
    xy, counts = hip._polygon_arrays(ref.star(w, h))
    assert L.pc_frame_set_mask_polygons(ctx._h, f._h, xy.ctypes.data, counts.ctypes.data, -1, 0) == -1
    assert L.pc_frame_set_mask_polygons(ctx._h, f._h, None, None, 1, 0) == -1
    assert np.array_equal(f.mask(), _plane("star", size))
    an.close()
    f.close()


# ---- analyzer ----
W, H, N = 320, 200, 12


@functools.lru_cache(maxsize=None)
def _clip():
    c = synth.NoiseClip(W, H, N)
    return [c.frame(i) for i in range(N)]


def _under_plane(fid, polys, invert=False):
    """the reference's keypoints of clip frame `fid` under the reference plane of `polys` (None: no mask)"""
    mask = None if polys is None else ref.plane(polys, W, H, invert)
    return gref.gftt(oracle.rgb2gray(_clip()[fid - 1]), oracle.gftt_options(), mask)[0]


def test_analyzer_keeps_the_polygons_a_detection_was_enqueued_with():
    """a dozen frames, each under its own polygon, put without waiting: the vertex ring has four buffers, so each is written
    three times while launches that read it may still be queued"""
    frames = _clip()
    c = hip.Context(0)
    an = hip.Analyzer(c, W, H)
    shapes = {}
    for fid in range(1, N + 1):
        polys = ref.moving(fid, W, H)
        invert = fid % 5 == 0
        shapes[fid] = (polys, invert)
        if polys is None:
            an.set_mask(None)
        else:
            an.set_mask_polygons(polys, invert=invert)
        an.put_frame(fid, frames[fid - 1], will_detect=True)
    an.set_mask_polygons([])                           # must not reach the detections already enqueued
    got = {}
    for fid in range(1, N + 1):
        an.submit(fid, [])
        r = an.collect()
        got[r[0]] = r[1].copy()
    for fid in range(1, N + 1):
        polys, invert = shapes[fid]
        e = _under_plane(fid, polys, invert)
        assert np.array_equal(got[fid], e), fid
        assert polys == [] or len(e) > 0, fid
    # a byte mask replaces polygons, polygons replace a byte mask, reset clears them
    plane = ref.plane(ref.star(W, H), W, H)
    an.set_mask_polygons(ref.bow_tie(W, H))
    an.set_mask(plane)
    an.put_frame(13, frames[0], will_detect=True)
    an.set_mask_polygons(ref.star(W, H))
    an.put_frame(14, frames[0], will_detect=True)
    for fid in (13, 14):
        an.submit(fid, [])
        assert np.array_equal(an.collect()[1], _under_plane(1, ref.star(W, H))), fid
    an.reset()
    an.put_frame(1, frames[0], will_detect=True)
    an.submit(1, [])
    assert np.array_equal(an.collect()[1], _under_plane(1, None))
    an.close()
    c.close()
