"""CPU: the surface of the forward-backward check exists where its users look for it (include/polychase_hip.h,
polychase_amd/hip.py, polychase_core.OpticalFlowOptions), and there is no CPU fallback behind it."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import fb_scene
import oracle
from polychase_amd import build, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pc_lk_track_fb", "pc_lk_track_filtered_fb", "pc_analyzer_set_fb_threshold"]


def test_options_attribute_exists_with_default_zero():
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core as core
    fo = core.OpticalFlowOptions()
    assert fo.forward_backward_threshold == 0.0
    fo.forward_backward_threshold = 1.5
    assert fo.forward_backward_threshold == 1.5
    # the reference's five attributes and defaults stay
    d = core.OpticalFlowOptions()
    assert (d.window_size, d.max_level, d.term_max_iters, d.term_epsilon, d.min_eigen_threshold) == (10, 3, 30, 0.01, 1e-4)


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polychase_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in hip.SYMBOLS and hasattr(lib, s), s
    assert "lk_fb" in hip.KERNEL_CLASSES and re.search(r"#define PC_K_LK_FB %d\b" % hip.KERNEL_CLASSES.index("lk_fb"), text)
    assert re.search(r"#define PC_K_COUNT %d\b" % len(hip.KERNEL_CLASSES), text)
    # pc_flow_options keeps the layout the ctypes mirror and the reference-side binding rely on
    assert [f[0] for f in hip.FlowOptions._fields_] == ["window_size", "max_level", "term_max_iters", "term_epsilon", "min_eigen_threshold"]


def test_no_cpu_fallback_behind_the_fb_calls():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hip.PolychaseHipError):
        ctx = hip.Context(0)
        hip.lk_track_fb(ctx, None, [], 1.0)


def test_entry_points_refuse_a_null_context():
    """needs no device and none must be absent: the calls return an error before they touch one"""
    L = hip.load()
    assert L.pc_lk_track_fb(None, None, None, 1, None, 1.0, None, None, None, None, None) != 0
    assert L.pc_lk_track_filtered_fb(None, None, None, 1, None, 1.0, None, None, None, None) != 0
    assert L.pc_analyzer_set_fb_threshold(None, 1.0) != 0


def test_composition_rule_on_the_oracle():
    """the expected values of the GPU tests: NaN and the threshold itself decide as the header says"""
    base = fb_scene.texture(96, 80, 16)
    g1, g2 = fb_scene.to_u8(base), fb_scene.target(base, "shift", 100)
    kps = oracle.gftt(g1)
    p1, p2 = oracle.Pyramid(g1, 5, 1), oracle.Pyramid(g2, 5, 1)
    c = fb_scene.composed(p1, p2, kps, oracle.flow_options(window_size=5, max_level=1), 1.0)
    fb_scene.check_fractions(c, "shift")
    ok = c["status_f"] == 1
    assert not c["status"][~ok].any() and not c["back_status"][~ok].any() and not c["back_xy"][~ok].any()
    d = c["back_xy"][ok] - kps[ok]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    assert d2.dtype == np.float32 and np.array_equal(c["status"][ok] == 1, (c["back_status"][ok] == 1) & (d2 <= np.float32(1.0)))
    assert fb_scene.thr2_of(0.1) == np.float32(0.1 * 0.1) and not (np.float32("nan") <= fb_scene.thr2_of(1.0))
