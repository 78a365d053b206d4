"""CPU: target-side masks.  The reference (tests/target_mask_ref.py) has the properties the header promises; the new C entry
points refuse null handles and bad margins before they touch a device; OpticalFlowOptions.target_mask_margin outside -1..31 is
refused by every entry point before any frame is asked for; the two new kernels fit the helper budget of
tests/test_kernel_resources_cpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import target_mask_ref as ref
from polychase_amd import build, hip
from test_kernel_resources_cpu import HELPER_LDS_BUDGET, HELPER_VGPR_BUDGET, _code_objects, _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 53, 41


# ---- the choked plane ----
def test_margin_zero_is_the_on_off_image():
    m = np.random.default_rng(1).integers(0, 4, (H, W)).astype(np.uint8) * 85      # 0, 85, 170, 255
    assert np.array_equal(ref.choke(m, 0), (m != 0).astype(np.uint8) * 255)


@pytest.mark.parametrize("r", [1, 2, 7, 31])
def test_an_off_rectangle_grows_by_the_margin_and_is_clipped_at_the_frame(r):
    m = np.full((H, W), 255, np.uint8)
    m[10:14, 20:29] = 0
    e = np.full((H, W), 255, np.uint8)
    e[max(10 - r, 0):min(14 + r, H), max(20 - r, 0):min(29 + r, W)] = 0
    assert np.array_equal(ref.choke(m, r), e)
    assert (ref.choke(m, r) == 0).sum() > (m == 0).sum()


@pytest.mark.parametrize("shape", [(1, 1), (5, 67), (H, W)])
def test_an_all_on_plane_stays_all_on_so_the_border_is_ignored(shape):
    for r in (0, 1, 5, 31):
        assert ref.choke(np.full(shape, 255, np.uint8), r).all()


def test_choking_twice_adds_the_margins():
    rng = np.random.default_rng(2)
    for off in (0.5, 0.02):
        m = (rng.random((H, W)) >= off).astype(np.uint8) * 255
        for a, b in ((1, 1), (2, 3), (4, 1), (7, 24)):
            assert np.array_equal(ref.choke(ref.choke(m, a), b), ref.choke(m, a + b)), (off, a, b)
    assert ref.choke(m, 3).any() and not ref.choke(m, 3).all()


def test_non_zero_bytes_other_than_255_count_as_on():
    rng = np.random.default_rng(3)
    on = rng.random((H, W)) >= 0.05
    a = np.where(on, 255, 0).astype(np.uint8)
    b = np.where(on, rng.integers(1, 255, (H, W)), 0).astype(np.uint8)
    assert (b[on] != 255).any() and (b[on] != 0).all()
    for r in (0, 1, 4):
        assert np.array_equal(ref.choke(a, r), ref.choke(b, r))
        assert set(np.unique(ref.choke(b, r))) <= {0, 255}


def test_margins_outside_the_range_are_errors_in_the_reference_too():
    for bad in (-1, 32):
        with pytest.raises(ValueError):
            ref.choke(np.ones((4, 4), np.uint8), bad)


# ---- the end point's pixel ----
def test_the_end_point_rule_on_hand_made_coordinates():
    w, h = 20, 12
    xs = np.array([9.5, -0.5, -3.2, w + 4, np.nan, 9.49, 18.5, 18.49, np.inf, -np.inf, 0.0], np.float32)
    want = [10, 0, 0, w - 1, 0, 9, w - 1, 18, w - 1, 0, 0]
    ix, iy = ref.pixel(np.stack([xs, xs], axis=1), w, h)
    assert ix.tolist() == want
    assert iy.tolist() == [min(v, h - 1) for v in want]
    # float32 throughout: 8388609 + 0.5 is not representable and rounds to even before the floor
    ix, _ = ref.pixel(np.array([[8388609.0, 0.0]], np.float32), 2 ** 24, 4)
    assert ix.tolist() == [8388610]


def test_keep_judges_rows_by_the_choked_plane_and_only_rows_that_are_alive():
    m = np.full((12, 20), 255, np.uint8)
    m[4:8, 6:10] = 0
    xy = np.array([[7.2, 5.1], [5.4, 5.0], [5.6, 5.0], [4.6, 5.0], [7.0, 5.0], [30.0, -9.0]], np.float32)
    st = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    assert ref.keep(xy, st, m, 0).tolist() == [0, 1, 0, 1, 0, 1]
    assert ref.keep(xy, st, m, 1).tolist() == [0, 0, 0, 0, 0, 1]
    assert ref.keep(xy, st, None, 5).tolist() == st.tolist()


# ---- the C ABI ----
NEW_SYMBOLS = ("pc_frame_download_choked_mask", "pc_lk_track_masked", "pc_analyzer_set_target_mask_margin")


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "polychase_hip.h")).read()
    assert re.search(r"#define PC_TARGET_MASK_MAX_MARGIN\s+31\b", text)
    assert hip.TARGET_MASK_MAX_MARGIN == ref.MAX_MARGIN == 31
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in hip.SYMBOLS and hasattr(lib, s), s
    for name in ("lk_track_masked",):
        assert callable(getattr(hip, name))
    assert callable(hip.Frame.choked_mask) and callable(hip.Analyzer.set_target_mask_margin)


def _last_error():
    L = hip.load()
    L.pc_last_error.restype = ctypes.c_char_p
    return L.pc_last_error().decode()


def test_entry_points_refuse_null_handles():
    """needs no device: the calls return an error before they touch one"""
    L = hip.load()
    PC_E_INVALID = -1
    out = np.zeros(16, np.uint8)
    assert L.pc_frame_download_choked_mask(None, None, 0, out.ctypes.data) == PC_E_INVALID and "null" in _last_error()
    assert L.pc_analyzer_set_target_mask_margin(None, 0) == PC_E_INVALID and "null" in _last_error()
    assert L.pc_analyzer_set_target_mask_margin(None, -1) == PC_E_INVALID and "null" in _last_error()
    opt = hip.flow_options()
    for margin in (-1, 0, 31):
        assert L.pc_lk_track_masked(None, None, None, 1, ctypes.byref(opt), 0.0, margin, None, None, None) == PC_E_INVALID
        assert "null" in _last_error()


@pytest.mark.parametrize("margin", [-2, 32, -(2 ** 31), 2 ** 31 - 1])
def test_bad_margins_are_refused_for_what_they_are(margin):
    """the margin is checked before the handles, so its refusal shows without a device: the message names the margin"""
    L = hip.load()
    PC_E_INVALID = -1
    out = np.zeros(16, np.uint8)
    opt = hip.flow_options()
    assert L.pc_frame_download_choked_mask(None, None, margin, out.ctypes.data) == PC_E_INVALID
    assert re.search(r"margin %d\b" % margin, _last_error()), _last_error()
    assert L.pc_analyzer_set_target_mask_margin(None, margin) == PC_E_INVALID
    assert re.search(r"margin %d\b" % margin, _last_error()), _last_error()
    assert L.pc_lk_track_masked(None, None, None, 1, ctypes.byref(opt), 0.0, margin, None, None, None) == PC_E_INVALID
    assert re.search(r"margin %d\b" % margin, _last_error()), _last_error()


def test_the_plane_download_has_no_off_value():
    """-1 means "off" to the analyzer and to pc_lk_track_masked; a plane of margin -1 does not exist"""
    L = hip.load()
    out = np.zeros(16, np.uint8)
    assert L.pc_frame_download_choked_mask(None, None, -1, out.ctypes.data) == -1
    assert re.search(r"margin -1\b", _last_error()), _last_error()


# ---- polychase_core ----
@pytest.fixture(scope="module")
def core():
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


def test_the_option_exists_and_is_off_by_default(core):
    fo = core.OpticalFlowOptions()
    assert fo.target_mask_margin == -1
    fo.target_mask_margin = 31
    assert fo.target_mask_margin == 31
    with pytest.raises(TypeError):
        fo.target_mask_margin = 1.5


@pytest.mark.parametrize("margin", [-2, 32])
def test_a_bad_margin_is_refused_by_all_five_entry_points_and_the_thread_before_any_frame_is_asked_for(core, margin, tmp_path):
    vi = core.VideoInfo(32, 24, 1, 4)
    asked = []

    def accessor(fid):
        asked.append(fid)
        return np.zeros((24, 32, 3), np.uint8)

    fo = core.OpticalFlowOptions()
    fo.target_mask_margin = margin
    go = core.GFTTOptions()
    for mask in (None, np.ones((24, 32), np.uint8)):   # refused with and without a mask to apply it to
        with pytest.raises(ValueError, match="target_mask_margin"):
            core.generate_optical_flow_database(vi, accessor, None, str(tmp_path / "a.db"), go, fo, detection_mask=mask)
        with pytest.raises(ValueError, match="target_mask_margin"):
            core.generate_optical_flow_shard(vi, accessor, None, str(tmp_path / "b.db"), 1, 3, flow_options=fo, detection_mask=mask)
        with pytest.raises(ValueError, match="target_mask_margin"):
            core.generate_optical_flow_records(vi, accessor, None, 1, 3, 0, 0, go, fo, detection_mask=mask)
        with pytest.raises(ValueError, match="target_mask_margin"):
            core.generate_optical_flow_database_multi_gpu(vi, accessor, None, str(tmp_path / "c.db"), 1, 0, flow_options=fo,
                                                          detection_mask=mask)
        with pytest.raises(ValueError, match="target_mask_margin"):
            core.OpticalFlowThread(vi, str(tmp_path / "d.db"), go, fo, detection_mask=mask)
    assert asked == [], "no frame may be asked for"
    assert not any(os.path.exists(str(tmp_path / n)) for n in ("a.db", "b.db", "c.db", "d.db")), "and no database is opened"


# ---- the kernels' resources ----
@pytest.fixture(scope="module")
def kernels():
    path = build.hip_library_path()
    if not os.path.exists(path):
        build.build_hip()
    return {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}


@pytest.mark.parametrize("kernel", ["mask_choke_kernel", "lk_target_mask_kernel"])
def test_the_new_kernels_fit_beside_three_lk_wavefronts(kernels, kernel):
    found = [(n, k) for n, k in kernels.items() if kernel in n]
    assert len(found) == 1, [n for n, _ in found]
    name, k = found[0]
    print(name, "VGPRs", k[".vgpr_count"], "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
    assert (k[".vgpr_count"] + 7) // 8 * 8 <= HELPER_VGPR_BUDGET == 104, f"{name}: {k['.vgpr_count']} VGPRs"
    assert k.get(".agpr_count", 0) == 0, name
    assert k[".group_segment_fixed_size"] <= HELPER_LDS_BUDGET == 18 * 1024, f"{name}: {k['.group_segment_fixed_size']} B of LDS"
    assert k.get(".private_segment_fixed_size", 0) == 0, f"{name}: spills to scratch"
