"""CPU: polygon detection masks.  The fill rule's reference (tests/polygon_mask_ref.py) has the properties the header
promises; the new C entry points refuse null handles and invalid polygons before they touch a device; PolygonMask and
detection_mask= refuse bad input before any frame is asked for; the rasteriser kernel fits the helper budget of
tests/test_kernel_resources_cpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import polygon_mask_ref as ref
from polychase_amd import build, hip
from test_kernel_resources_cpu import HELPER_LDS_BUDGET, HELPER_VGPR_BUDGET, _code_objects, _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 67, 45


# ---- the rule ----
def test_an_integer_rectangle_is_half_open():
    m = ref.plane(ref.rectangle(W, H), W, H)
    e = np.zeros((H, W), np.uint8)
    e[5:15, 10:20] = 255
    assert np.array_equal(m, e) and int((m > 0).sum()) == 100


def test_polygons_that_share_an_edge_partition_the_pixels():
    # a slanted shared edge with fractional ends; the merged outline is the union
    a = [(8.3, 4.6), (31.55, 9.2), (27.1, 38.4)]
    b = [(31.55, 9.2), (59.7, 30.3), (27.1, 38.4)]
    merged = [(8.3, 4.6), (31.55, 9.2), (59.7, 30.3), (27.1, 38.4)]
    ia, ib, im = ref.inside(a, W, H), ref.inside(b, W, H), ref.inside(merged, W, H)
    assert ia.any() and ib.any()
    assert not (ia & ib).any(), "no pixel twice"
    assert np.array_equal(ia | ib, im)
    assert np.array_equal(ref.plane([a, b], W, H), ref.plane([merged], W, H))
    # pixel centres exactly on a shared vertical edge go to one side
    l, r = [(10, 5), (20, 5), (20, 15), (10, 15)], [(20, 5), (33, 5), (33, 15), (20, 15)]
    assert not (ref.inside(l, W, H) & ref.inside(r, W, H)).any()
    assert int((ref.plane([l, r], W, H) > 0).sum()) == 230


@pytest.mark.parametrize("name", sorted(ref.SHAPES))
def test_orientation_does_not_matter(name):
    polys = ref.SHAPES[name](W, H)
    assert np.array_equal(ref.plane(polys, W, H), ref.plane([p[::-1] for p in polys], W, H))


def test_the_rule_agrees_with_a_float64_crossing_test_on_random_polygons():
    rng = np.random.default_rng(2024)
    some = 0
    for _ in range(200):
        k = int(rng.integers(3, 12))
        p = np.stack([rng.uniform(-10, W + 10, k), rng.uniform(-10, H + 10, k)], axis=1).astype(np.float32)
        got = ref.inside(p, W, H)
        some += int(got.any())
        assert np.array_equal(got, ref.inside_float64(p, W, H))
    assert some > 150


@pytest.mark.parametrize("name", sorted(ref.NOTHING))
def test_sub_pixel_outside_and_degenerate_shapes_turn_nothing_on(name):
    assert not ref.plane(ref.NOTHING[name](W, H), W, H).any()
    assert ref.plane(ref.NOTHING[name](W, H), W, H, invert=True).all()


def test_horizontal_and_zero_length_edges_never_cross():
    with_them = ref.closing_and_horizontal(W, H)
    without = [with_them[0][:-1]]
    assert np.array_equal(ref.plane(with_them, W, H), ref.plane(without, W, H))
    e = np.zeros((H, W), np.uint8)
    e[7:21, 5:30] = 255             # y in [7, 20.5): rows 7..20
    assert np.array_equal(ref.plane(with_them, W, H), e)


def test_a_frame_covering_shape_turns_everything_on():
    assert ref.plane(ref.frame_covering(W, H), W, H).all()
    assert not ref.plane(ref.frame_covering(W, H), W, H, invert=True).any()


def test_rint_ties_go_to_even():
    v = ref.snap([(0.03125, 0.09375), (1, 1), (2, 0)])
    assert tuple(v[0]) == (0, 2)
    m = ref.plane(ref.ties(W, H), W, H)
    e = np.zeros((H, W), np.uint8)
    e[3:20, 10:41] = 255            # 160.5 -> 160: column 10 in; 48.5 -> 48: row 3 in; 320.5 -> 320: row 20 out; 641.5 -> 642: column 40 in
    assert np.array_equal(m, e)


def test_bad_coordinates_are_errors_in_the_reference_too():
    for bad in (np.nan, np.inf, -np.inf, 32768.5, -40000.0):
        with pytest.raises(ValueError):
            ref.snap([(0, 0), (bad, 1), (2, 2)])
    ref.snap([(32768, -32768), (0, 0), (1, 5)])


# ---- the C ABI ----
def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "polychase_hip.h")).read()
    for name, value in (("PC_MASK_MAX_POLYGONS", 32), ("PC_MASK_MAX_VERTICES", 4096), ("PC_MASK_SUBPIXEL", 16)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), text), name
    assert (hip.MASK_MAX_POLYGONS, hip.MASK_MAX_VERTICES, hip.MASK_SUBPIXEL) == (32, 4096, 16)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in ("pc_frame_set_mask_polygons", "pc_analyzer_set_mask_polygons", "pc_frame_download_mask"):
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in hip.SYMBOLS and hasattr(lib, s), s


def _args(polys):
    xy, counts = hip._polygon_arrays(polys)
    return xy, counts, xy.ctypes.data, counts.ctypes.data, len(counts)


def test_entry_points_refuse_null_handles():
    """needs no device and none must be absent: the calls return an error before they touch one"""
    L = hip.load()
    xy, counts, pxy, pc, n = _args(ref.rectangle(W, H))
    assert L.pc_frame_set_mask_polygons(None, None, pxy, pc, n, 0) != 0
    assert L.pc_frame_set_mask_polygons(None, None, None, None, 0, 0) != 0
    assert L.pc_analyzer_set_mask_polygons(None, pxy, pc, n, 0) != 0
    assert L.pc_analyzer_set_mask_polygons(None, None, None, 0, 1) != 0
    out = np.zeros(16, np.uint8)
    assert L.pc_frame_download_mask(None, None, out.ctypes.data) != 0


def _tri(n=3):
    return np.array([(1, 1), (9, 2), (4, 8)] + [(4, 8)] * (n - 3), np.float32)


# case -> (polygons, n_polygons passed or None = their number, what pc_last_error must say)
INVALID_POLYGONS = {
    "33_polygons": ([_tri()] * 33, None, r"33 polygons"),
    "minus_one_polygons": ([_tri()], -1, r"-1 polygons"),
    "a_count_of_2": ([_tri(), _tri()[:2]], None, r"polygon 1 has 2 vertices"),
    "a_count_of_0": ([_tri(), _tri()[:0]], None, r"polygon 1 has 0 vertices"),
    "4097_vertices": ([_tri(4000), _tri(97)], None, r"more than 4096 vertices"),
    "nan": ([np.array([(1, 1), (np.nan, 2), (4, 8)], np.float32)], None, r"vertex 1: coordinate"),
    "inf": ([np.array([(1, 1), (9, 2), (4, -np.inf)], np.float32)], None, r"vertex 2: coordinate"),
    "out_of_range": ([np.array([(1, 1), (32768.5, 2), (4, 8)], np.float32)], None, r"vertex 1: coordinate"),
    "null_arrays": (None, 1, r"null argument"),
}


def _last_error():
    L = hip.load()
    L.pc_last_error.restype = ctypes.c_char_p
    return L.pc_last_error().decode()


@pytest.mark.parametrize("case", sorted(INVALID_POLYGONS))
def test_invalid_polygons_are_refused_for_what_they_are(case):
    """the polygons are checked before the handles, so the refusal of each invalid argument shows without a device: the
    message names the polygons' fault, not the null handle.  With real handles the same cases return PC_E_INVALID and leave the
    previous mask in force (tests/test_polygon_mask_gpu.py)."""
    L = hip.load()
    polys, n_override, message = INVALID_POLYGONS[case]
    if polys is None:
        pxy = pc = None
        n = n_override
    else:
        xy, counts, pxy, pc, n = _args(polys)
        n = n if n_override is None else n_override
    PC_E_INVALID = -1
    assert L.pc_frame_set_mask_polygons(None, None, pxy, pc, n, 0) == PC_E_INVALID
    assert re.search(message, _last_error()), _last_error()
    assert L.pc_analyzer_set_mask_polygons(None, pxy, pc, n, 1) == PC_E_INVALID
    assert re.search(message, _last_error()), _last_error()
    # valid polygons and a null handle: refused for the handle
    xy, counts, pxy, pc, n = _args([_tri()] * 32)
    assert L.pc_frame_set_mask_polygons(None, None, pxy, pc, n, 0) == PC_E_INVALID and "null" in _last_error()
    assert L.pc_analyzer_set_mask_polygons(None, pxy, pc, n, 0) == PC_E_INVALID and "null" in _last_error()


def test_the_reference_refuses_the_same_polygons():
    for case in ("a_count_of_2", "a_count_of_0", "nan", "inf", "out_of_range"):
        with pytest.raises(ValueError):
            [ref.snap(p) for p in INVALID_POLYGONS[case][0]]
    for case in ("33_polygons", "4097_vertices"):
        with pytest.raises(ValueError):
            ref.plane(INVALID_POLYGONS[case][0], W, H)


# ---- polychase_core ----
@pytest.fixture(scope="module")
def core():
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


def test_polygon_mask_holds_float32_copies_and_the_flag(core):
    src = [np.array([(1, 2), (30, 4), (9, 20.5)], np.float64), [(5, 5), (9, 5), (9, 9), (5, 9)]]
    m = core.PolygonMask(src, invert=True)
    assert m.invert is True and core.PolygonMask(src).invert is False
    assert len(m.polygons) == 2
    for got, want in zip(m.polygons, src):
        assert got.dtype == np.float32 and np.array_equal(got, np.asarray(want, np.float32))
        assert not got.flags.writeable
    src[0][0, 0] = 99
    assert m.polygons[0][0, 0] == 1, "copied at construction"
    with pytest.raises(AttributeError):
        m.invert = False
    with pytest.raises(AttributeError):
        m.polygons = ()
    assert len(core.PolygonMask([]).polygons) == 0


BAD_POLYGON_MASKS = {
    "wrong_shape_k3": [np.ones((4, 3), np.float32)],
    "wrong_shape_flat": [np.ones(8, np.float32)],
    "two_vertices": [np.array([(1, 1), (5, 5)], np.float32)],
    "33_polygons": [_tri()] * 33,
    "4097_vertices": [_tri(4000), _tri(97)],
    "nan": [np.array([(1, 1), (np.nan, 2), (4, 8)], np.float32)],
    "inf": [np.array([(1, 1), (9, np.inf), (4, 8)], np.float32)],
    "out_of_range": [np.array([(1, 1), (-32769, 2), (4, 8)], np.float32)],
    "not_numbers": [np.array([("a", "b"), ("c", "d"), ("e", "f")])],
    "not_a_sequence": 7,
    "none": None,
}


@pytest.mark.parametrize("bad", sorted(BAD_POLYGON_MASKS))
def test_polygon_mask_construction_errors(core, bad):
    with pytest.raises(ValueError):
        core.PolygonMask(BAD_POLYGON_MASKS[bad])
    with pytest.raises(ValueError):
        core.PolygonMask(BAD_POLYGON_MASKS[bad], invert=True)


def test_the_limits_themselves_are_accepted(core):
    core.PolygonMask([_tri()] * 32)
    core.PolygonMask([_tri(4096)])
    core.PolygonMask([np.array([(32768, -32768), (0, 0), (1, 5)], np.float32)])


def _bad_detection_masks(core):
    good = core.PolygonMask(ref.rectangle(32, 24))
    return {
        "dict_with_an_array": {1: good, 2: np.ones((24, 32), np.uint8)},
        "dict_with_a_list": {1: ref.rectangle(32, 24)},
        "dict_with_a_string_key": {"1": good},
        "list_of_polygons": ref.rectangle(32, 24),              # not wrapped in a PolygonMask
    }


@pytest.mark.parametrize("bad", ["dict_with_an_array", "dict_with_a_list", "dict_with_a_string_key", "list_of_polygons"])
def test_a_bad_polygon_mask_is_refused_by_all_five_entry_points_before_any_frame_is_asked_for(core, bad, tmp_path):
    vi = core.VideoInfo(32, 24, 1, 4)
    asked = []

    def accessor(fid):
        asked.append(fid)
        return np.zeros((24, 32, 3), np.uint8)

    mask = _bad_detection_masks(core)[bad]
    with pytest.raises(ValueError):
        core.generate_optical_flow_database(vi, accessor, None, str(tmp_path / "a.db"), detection_mask=mask)
    with pytest.raises(ValueError):
        core.generate_optical_flow_shard(vi, accessor, None, str(tmp_path / "b.db"), 1, 3, detection_mask=mask)
    with pytest.raises(ValueError):
        core.generate_optical_flow_records(vi, accessor, None, 1, 3, 0, 0, detection_mask=mask)
    with pytest.raises(ValueError):
        core.generate_optical_flow_database_multi_gpu(vi, accessor, None, str(tmp_path / "c.db"), 1, 0, detection_mask=mask)
    with pytest.raises(ValueError):
        core.OpticalFlowThread(vi, str(tmp_path / "d.db"), detection_mask=mask)
    assert asked == [], "no frame may be asked for"


def test_the_thread_still_refuses_a_callable_that_returns_polygons(core, tmp_path):
    good = core.PolygonMask(ref.rectangle(32, 24))
    with pytest.raises(ValueError):
        core.OpticalFlowThread(core.VideoInfo(32, 24, 1, 4), str(tmp_path / "t.db"), detection_mask=lambda fid: good)


def test_wrapper_checks_polygon_shapes():
    with pytest.raises(ValueError):
        hip._polygon_arrays([np.ones((4, 3), np.float32)])
    xy, counts = hip._polygon_arrays(ref.quads32(W, H))
    assert xy.shape == (128, 2) and xy.dtype == np.float32 and xy.flags.c_contiguous and counts.tolist() == [4] * 32
    xy, counts = hip._polygon_arrays([])
    assert xy.shape == (0, 2) and len(counts) == 0


# ---- the kernel's resources ----
@pytest.fixture(scope="module")
def kernels():
    path = build.hip_library_path()
    if not os.path.exists(path):
        build.build_hip()
    return {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}


def test_the_rasteriser_fits_beside_three_lk_wavefronts(kernels):
    found = [(n, k) for n, k in kernels.items() if "polygon_mask_kernel" in n]
    assert len(found) == 1, [n for n, _ in found]
    name, k = found[0]
    print(name, "VGPRs", k[".vgpr_count"], "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
    assert (k[".vgpr_count"] + 7) // 8 * 8 <= HELPER_VGPR_BUDGET == 104, f"{name}: {k['.vgpr_count']} VGPRs"
    assert k.get(".agpr_count", 0) == 0, name
    assert k[".group_segment_fixed_size"] <= HELPER_LDS_BUDGET == 18 * 1024, f"{name}: {k['.group_segment_fixed_size']} B of LDS"
    assert k.get(".private_segment_fixed_size", 0) == 0, f"{name}: spills to scratch"
