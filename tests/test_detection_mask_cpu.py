"""CPU: the detection mask's reference (tests/masked_gftt_ref.py) is the oracle's detector when nothing is masked; the new
surface exists and refuses bad arguments before it touches a device; the masked kernel variants exist in the built library
and fit the helper budget of tests/test_kernel_resources_cpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import masked_gftt_ref as ref
import oracle
from polychase_amd import build, hip
from test_kernel_resources_cpu import HELPER_LDS_BUDGET, HELPER_VGPR_BUDGET, _code_objects, _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(333, 211), (320, 200), (67, 45)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(ref.OPTION_SETS))
def test_reference_without_a_mask_is_the_oracle(size, name):
    """the reference's own check: mask=None and an all-255 mask reproduce oracle.gftt in keypoints, order and candidate count"""
    w, h = size
    g = ref.test_image(w, h)
    opt = oracle.gftt_options(**ref.OPTION_SETS[name])
    xy, _, ncand = oracle.gftt(g, opt, want_eig=True)
    assert len(xy) > 0
    for mask in (None, np.full((h, w), 255, np.uint8)):
        kps, _, n = ref.gftt(g, opt, mask)
        assert n == ncand
        assert np.array_equal(kps, xy), "keypoints must match in value AND order"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_mask_is_not_a_filter_on_the_unmasked_keypoints(size):
    w, h = size
    g = ref.test_image(w, h)
    opt = oracle.gftt_options()
    m = ref.mask_column_and_disc(w, h)
    kps = ref.gftt(g, opt, m)[0]
    assert len(kps) > 0 and np.all(m[kps[:, 1].astype(int), kps[:, 0].astype(int)] != 0)
    assert not np.array_equal(kps, ref.post_filtered(g, opt, m))


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polychase_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in ("pc_frame_set_mask", "pc_analyzer_set_mask"):
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in hip.SYMBOLS and hasattr(lib, s), s


def test_entry_points_refuse_null_handles():
    """needs no device and none must be absent: the calls return an error before they touch one"""
    L = hip.load()
    m = np.zeros((4, 4), np.uint8)
    assert L.pc_frame_set_mask(None, None, m.ctypes.data, 4, 0) != 0
    assert L.pc_frame_set_mask(None, None, None, 0, 0) != 0
    assert L.pc_analyzer_set_mask(None, m.ctypes.data, 4, 0) != 0
    assert L.pc_analyzer_set_mask(None, None, 0, 0) != 0


@pytest.fixture(scope="module")
def core():
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


BAD_MASKS = {
    "float32": np.ones((24, 32), np.float32),
    "bool": np.ones((24, 32), bool),
    "transposed": np.ones((32, 24), np.uint8),
    "three_channels": np.ones((24, 32, 3), np.uint8),
    "too_small": np.ones((23, 32), np.uint8),
    "not_an_array": "mask",
}


@pytest.mark.parametrize("bad", sorted(BAD_MASKS))
def test_a_mask_of_wrong_dtype_or_shape_raises_before_any_gpu_work(core, bad, tmp_path):
    vi = core.VideoInfo(32, 24, 1, 4)
    asked = []

    def accessor(fid):
        asked.append(fid)
        return np.zeros((24, 32, 3), np.uint8)

    mask = BAD_MASKS[bad]
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


def test_the_thread_takes_a_static_mask_only(core, tmp_path):
    with pytest.raises(ValueError):
        core.OpticalFlowThread(core.VideoInfo(32, 24, 1, 4), str(tmp_path / "t.db"), detection_mask=lambda fid: None)


def test_wrapper_checks_dtype_and_shape():
    with pytest.raises(ValueError):
        hip._mask_ptr(np.ones((24, 32), np.float32), 32, 24)
    with pytest.raises(ValueError):
        hip._mask_ptr(np.ones((32, 24), np.uint8), 32, 24)
    wide = np.ones((24, 45), np.uint8)
    keep, p, dev, pitch = hip._mask_ptr(wide[:, :32], 32, 24)      # a view of a wider array: passed with its pitch
    assert (p, dev, pitch) == (wide.ctypes.data, 0, 45)


@pytest.fixture(scope="module")
def kernels():
    path = build.hip_library_path()
    if not os.path.exists(path):
        build.build_hip()
    return {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}


# substring of the mangled name -> number of instantiations; ELb1 / ILb1: MASKED = true
MASKED_HELPERS = {"min_eig_fused_kernelILi0ELb1": 1, "min_eig_fused_kernelILi1ELb1": 1, "min_eig_fused_kernelILi2ELb1": 1,
                  "min_eig_fused_kernelILi3ELb1": 1, "nms_kernelILb1": 1, "box_response_kernelILb1": 1}


@pytest.mark.parametrize("helper", sorted(MASKED_HELPERS))
def test_masked_kernels_exist_and_fit_beside_three_lk_wavefronts(kernels, helper):
    found = [(n, k) for n, k in kernels.items() if helper in n]
    assert len(found) == MASKED_HELPERS[helper], f"{helper}: {[n for n, _ in found]}"
    name, k = found[0]
    assert (k[".vgpr_count"] + 7) // 8 * 8 <= HELPER_VGPR_BUDGET, f"{name}: {k['.vgpr_count']} VGPRs"
    assert k.get(".agpr_count", 0) == 0, name
    assert k[".group_segment_fixed_size"] <= HELPER_LDS_BUDGET, f"{name}: {k['.group_segment_fixed_size']} B of LDS"
    assert k.get(".private_segment_fixed_size", 0) == 0, f"{name}: spills to scratch"
    # the unmasked twin is still there, as its own instantiation
    twin = helper.replace("ELb1", "ELb0").replace("ILb1", "ILb0")
    assert sum(twin in n for n in kernels) == 1, twin
