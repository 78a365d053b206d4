"""GPU: the frame-preparation kernels at the shapes where their code paths part, bit for bit against the CPU oracle.

Response map (min_eig_fused_kernel): a lane walks a band of ME_R = 10 rows, a wavefront two bands of 32 column pairs.  Heights
1 .. 33 and 2 ME_R +- 1 by widths 1 .. 129 give bands that end inside the image, the one-row-early emit at h - 1, odd widths
(scalar stores), partial and second tiles; grids of 1 x 1, 1 x 2 and 4 x 4 cells put a tile inside one cell (one atomic per
wavefront), across two cells that are at least a tile large (four registers; 129 px wide frames) and over cells smaller than a
tile (per-pixel atomics); with and without a detection mask; the four Sobel arithmetic modes.

Pyramid (level_kernel): 11 x 11 (the smallest level a 10-px window allows), 12 x 13, 63 x 65, 130 x 67, to four levels, from u8
gray, RGB8 and float RGB sources: the image, uint16 and Scharr planes of every level with their whole padding.

NMS (nms_kernel stages a 64 x 64 block in two parts of 32 rows): a frame whose corners sit in one block (every other part
leaves after staging), a frame mirrored about every 16th row boundary (equal responses, bit for bit, on both sides of tile,
part and block boundaries; a left-right mirror does not tie: the Sobel row filter rounds in tap order), a frame without a
candidate; with the default options and with min_distance 0, where the keypoints ARE the sorted
candidate list.  The library has no download of the state bytes or of the key list; what it delivers of them is compared: the
candidate count (the non-zero state bytes), every candidate in sorted order (min_distance 0), the accepted ones in order.

Suppression: the 255 / 256 / 257-candidate workgroup edges and the frame that overflows a value bucket, as
tests/test_gftt_edges_gpu.py and tests/test_fused_chain_gpu.py build them -- completion and equality only."""
import functools

import numpy as np
import pytest

import _gftt_edges_check as chk
import _ingest_check as ingest
import ingest_layouts as il
import masked_gftt_ref as ref
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ME_R = 10                                        # kernels_gftt.hip
HEIGHTS = [1, 2, 15, 16, 17, 31, 32, 33, 2 * ME_R - 1, 2 * ME_R + 1]
WIDTHS = [1, 2, 63, 64, 65, 129]
GRIDS = [(1, 1), (1, 2), (4, 4)]                 # rows, cols
# PC_ARITH_SOBEL_FMA = 2, PC_ARITH_SOBEL_ROW_FMA = 4: the library's flags and the oracle's emulation flags are the same numbers
SOBEL_MODES = {"canonical": 0, "sobel_fma": hip.ARITH_SOBEL_FMA, "row_fma": hip.ARITH_SOBEL_ROW_FMA,
               "sobel_row_fma": hip.ARITH_SOBEL_FMA | hip.ARITH_SOBEL_ROW_FMA}
assert (oracle.EMU_SOBEL_FMA, oracle.EMU_SOBEL_ROW_FMA) == (hip.ARITH_SOBEL_FMA, hip.ARITH_SOBEL_ROW_FMA)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_arithmetic(hip.ARITH_OPENCV_X86)
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _noise(w, h, seed=0):
    g = np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w), dtype=np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _speckle(w, h):
    m = (np.random.default_rng(7 * w + h).integers(0, 4, (h, w)) != 0).astype(np.uint8) * 255
    m.setflags(write=False)
    return m


def _detect(ctx, gray, mask, **options):
    h, w = gray.shape
    f = hip.Frame(ctx, w, h, 5, 0)
    try:
        f.set_gray(np.ascontiguousarray(gray))
        f.set_mask(mask)
        f.detect(hip.gftt_options(**options))
        return f.keypoints(), f.min_eig(), f.num_candidates
    finally:
        f.close()


def _reference(gray, mask, **options):
    kps, eig, ncand = ref.gftt(gray, oracle.gftt_options(**options), mask)
    return kps, eig, ncand


# ---------------------------------------------------------------------------------------------------------------------------
# response map
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("mode", sorted(SOBEL_MODES))
def test_response_map_and_cell_maxima_at_band_and_tile_edges(ctx, mode, masked):
    flags = SOBEL_MODES[mode]
    ctx.set_arithmetic(flags)
    bad = []
    with oracle.emulation(flags):
        for h in HEIGHTS:
            for w in WIDTHS:
                gray = _noise(w, h)
                mask = _speckle(w, h) if masked else None
                for rows, cols in GRIDS:
                    opt = dict(grid_rows=rows, grid_cols=cols)
                    ekps, eeig, encand = _reference(gray, mask, **opt)
                    kps, eig, ncand = _detect(ctx, gray, mask, **opt)
                    if not np.array_equal(_bits(eig), _bits(eeig)):
                        ys, xs = np.nonzero(_bits(eig) != _bits(eeig))
                        bad.append("%dx%d grid %dx%d: response differs at %d pixels, first x=%d y=%d" % (w, h, rows, cols, len(xs), xs[0], ys[0]))
                    elif ncand != encand or not np.array_equal(kps, ekps):
                        # the per-cell maxima set the thresholds: a wrong one shows in the candidates
                        bad.append("%dx%d grid %dx%d: %d candidates / %d keypoints, expected %d / %d (or their order differs)" % (
                            w, h, rows, cols, ncand, len(kps), encand, len(ekps)))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_cell_maxima_in_four_registers_across_both_axes(ctx, masked):
    """129 x 41 under a 2 x 2 grid: cells of 65 x 21, one pixel larger than a wavefront's tile (64 x 20) in both axes -- tiles
    inside one cell, across two and across four"""
    ctx.set_arithmetic(hip.ARITH_OPENCV_X86)
    gray, mask = _noise(129, 41), (_speckle(129, 41) if masked else None)
    with oracle.emulation(oracle.EMU_OPENCV_X86):
        ekps, eeig, encand = _reference(gray, mask, grid_rows=2, grid_cols=2)
    kps, eig, ncand = _detect(ctx, gray, mask, grid_rows=2, grid_cols=2)
    assert np.array_equal(_bits(eig), _bits(eeig))
    assert ncand == encand and np.array_equal(kps, ekps)


# ---------------------------------------------------------------------------------------------------------------------------
# pyramid
# ---------------------------------------------------------------------------------------------------------------------------
def _source(kind, w, h):
    rng = np.random.default_rng(w * 131 + h)
    if kind == "gray8":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "rgb8":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return rng.random((h, w, 3), dtype=np.float32)


@pytest.mark.parametrize("kind", ["gray8", "rgb8", "rgbf32"])
@pytest.mark.parametrize("size", [(11, 11), (12, 13), (63, 65), (130, 67)], ids=lambda s: "%dx%d" % s)
def test_pyramid_planes_with_their_padding(ctx, size, kind):
    w, h = size
    img = _source(kind, w, h)
    e = il.expected(img, 10, 3)
    f = hip.Frame(ctx, w, h, 10, 3)
    try:
        if kind == "gray8":
            f.set_gray(img)
        else:
            f.set_rgb(img)
        why = ingest.planes_mismatch(f, e)
    finally:
        f.close()
    assert not why, why


# ---------------------------------------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------------------------------------
NMS_W, NMS_H = 256, 192                          # 4 x 3 blocks of 64 x 64; 4 x 4 cells of 64 x 48


def _one_block_frame():
    g = np.full((NMS_H, NMS_W), 128, np.uint8)
    g[70:122, 70:122] = _noise(52, 52)           # inside block (1, 1): x, y in 64 .. 127
    return g


def _mirrored_frame():
    q = _noise(NMS_W, 16, seed=3)
    pair = np.concatenate([q, q[::-1]], axis=0)              # mirrored about y = 15.5, and, tiled, about every multiple of 16 less
    return np.ascontiguousarray(np.tile(pair, (6, 1)))       # a half: tile, part and block boundaries alike


def _flat_frame():
    return np.full((NMS_H, NMS_W), 77, np.uint8)


NMS_FRAMES = {"one_block": _one_block_frame, "mirrored": _mirrored_frame, "flat": _flat_frame}


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("name", sorted(NMS_FRAMES))
def test_nms_candidates_sorted_list_and_keypoints(ctx, name, masked):
    ctx.set_arithmetic(hip.ARITH_OPENCV_X86)
    gray = NMS_FRAMES[name]()
    mask = _speckle(NMS_W, NMS_H) if masked else None
    with oracle.emulation(oracle.EMU_OPENCV_X86):
        opt = oracle.gftt_options()
        eig = ref.response(gray, opt)
        vals, idx = ref.candidates(eig, opt, mask)
        ekps, _, encand = ref.gftt(gray, opt, mask)
        ekps0, _, encand0 = ref.gftt(gray, oracle.gftt_options(min_distance=0.0), mask)
    assert encand == encand0 == len(idx)
    if name == "flat":
        assert encand == 0
    else:
        assert encand > 0
    if name == "one_block":
        ys, xs = idx // NMS_W, idx % NMS_W
        assert xs.min() >= 64 and xs.max() < 128 and ys.min() >= 64 and ys.max() < 128, "every candidate in block (1, 1)"
    if name == "mirrored" and not masked:
        t = np.where(eig > 0, eig, 0)
        for y in (15, 31, 63):                               # a tile boundary inside a part, a part boundary, a block boundary
            assert (t[y] == t[y + 1]).all() and t[y].max() > 0, "equal responses on both sides of row %d | %d" % (y, y + 1)
            assert np.isin(idx // NMS_W, (y, y + 1)).any(), "candidates on the boundary rows"
    sorted_xy = np.stack([idx % NMS_W, idx // NMS_W], axis=1).astype(np.float32)
    assert np.array_equal(ekps0, sorted_xy), "min_distance 0: the reference's keypoints are its sorted candidates"
    # the sorted candidate list
    kps0, geig, ncand0 = _detect(ctx, gray, mask, min_distance=0.0)
    assert np.array_equal(_bits(geig), _bits(eig))
    assert ncand0 == encand and np.array_equal(kps0, sorted_xy), "candidates must match in value AND order"
    # the accepted ones
    kps, _, ncand = _detect(ctx, gray, mask)
    assert ncand == encand and np.array_equal(kps, ekps), "keypoints must match in value AND order"


def test_nms_with_a_negative_threshold_takes_the_float_stencil(ctx):
    """Harris responses: a cell of a flat region with one edge has a negative maximum, hence a negative threshold, and the
    stencil compares floats, not their bit patterns"""
    ctx.set_arithmetic(hip.ARITH_OPENCV_X86)
    g = _one_block_frame()
    g[:48, :64] = 10
    g[:48, 20:22] = 250                          # cell (0, 0): an edge and nothing else -- Harris is negative along it, 0 elsewhere
    g[150:, 200:] = _noise(56, 42, seed=5)
    with oracle.emulation(oracle.EMU_OPENCV_X86):
        opt = oracle.gftt_options(use_harris=1)
        eig = ref.response(g, opt)
        ekps, _, encand = ref.gftt(g, opt, None)
    assert eig.min() < 0 and encand > 0
    kps, geig, ncand = _detect(ctx, g, None, use_harris=1)
    assert np.array_equal(_bits(geig), _bits(eig))
    assert ncand == encand and np.array_equal(kps, ekps)


# ---------------------------------------------------------------------------------------------------------------------------
# suppression
# ---------------------------------------------------------------------------------------------------------------------------
SUPPRESSION_CASES = [c for c in chk.S.cases() if c[0] in ("count_255", "count_256", "count_257", "bucket_513")]


@pytest.mark.parametrize("name,run", SUPPRESSION_CASES, ids=["%s-%s" % c for c in SUPPRESSION_CASES])
def test_suppression_at_workgroup_edges_and_on_an_overflowing_frame(ctx, name, run):
    ctx.set_arithmetic(hip.ARITH_OPENCV_X86)
    assert chk.mode_of_process() == "default"
    why = chk.run_case(ctx, name, run, "default")
    assert not why, why


def test_dense_dot_frame_that_overflows_a_value_bucket(ctx):
    """the frame of tests/test_fused_chain_gpu.py: redone on the slow path, the oracle's keypoints"""
    ctx.set_arithmetic(hip.ARITH_OPENCV_X86)
    w, h = 320, 240
    g = np.zeros((h, w), np.uint8)
    g[4:h - 4:4, 4:w - 4:4] = 200
    with oracle.emulation(oracle.EMU_OPENCV_X86):
        xy, _, ncand = oracle.gftt(g, want_eig=True)
    assert ncand > 4 * 512
    f = hip.Frame(ctx, w, h)
    try:
        f.set_gray(g)
        for _ in range(2):
            f.detect()
            assert f.num_candidates == ncand
            assert np.array_equal(f.keypoints(), xy), "keypoints must match in value AND order"
    finally:
        f.close()
