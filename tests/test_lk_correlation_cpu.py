"""CPU: minimum correlation of the LK flow rows.  The numpy restatement of the rule (tests/lk_correlation_ref.py) reproduces the
oracle's patch error bit for bit, so its two windows ARE the windows LK compared; it has the properties the header promises; the
scenes of the GPU tests exercise both outcomes; the surface exists where its users look for it, refuses what no run accepts
before a frame is asked for, and has no CPU fallback behind it; the new kernel fits the helper budget of
tests/test_kernel_resources_cpu.py."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

import lk_correlation_ref as ref
import lk_correlation_scene as scene
import oracle
from polychase_amd import build, hip
from test_kernel_resources_cpu import HELPER_LDS_BUDGET, HELPER_VGPR_BUDGET, _code_objects, _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("same", "shift", "gain", "unrelated")


@functools.lru_cache(maxsize=None)
def _forward(win, kind):
    """the oracle's forward rows in its default arithmetic and options, once per (window, target)"""
    opt = oracle.flow_options(window_size=win)
    g1, gt, kps = scene.frame1(), scene.target(kind, win), scene.detected()
    q, sf, err = oracle.lk(oracle.Pyramid(g1, win, opt.max_level), oracle.Pyramid(gt, win, opt.max_level), kps, opt)
    return gt, q, sf, err


# ---- the restatement is tied to the oracle ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("win", scene.WINDOWS)
def test_the_two_windows_give_the_oracles_patch_error_bit_for_bit(win, kind):
    g1, kps = scene.frame1(), scene.detected()
    gt, q, sf, err = _forward(win, kind)
    rows = np.nonzero(sf == 1)[0]
    assert len(rows) >= 3, (win, kind, len(rows))
    for i in rows:
        I, J = ref.window_values(g1, win, kps[i, 0], kps[i, 1]), ref.window_values(gt, win, q[i, 0], q[i, 1])
        assert I is not None and J is not None, (win, kind, i, "a status-1 row has passed the bounds test for both windows")
        assert I.shape == J.shape == (win, win) and I.min() >= 0 and J.min() >= 0 and I.max() <= 8160 and J.max() <= 8160
        e = np.float32(np.float32(np.abs(J - I).sum()) / np.float32(32 * win * win))
        assert e.view(np.uint32) == err[i].view(np.uint32), (win, kind, i, e, err[i])


# ---- properties ----
def _texture_window(win, seed=3):
    return np.random.default_rng(seed).integers(0, 8161, (win, win)).astype(np.int64)


@pytest.mark.parametrize("win", scene.WINDOWS)
def test_identical_windows_are_kept_at_threshold_one_with_score_one(win):
    I = _texture_window(win)
    c = ref.sums(I, I)
    assert c[0] == c[1] == c[2] > 0
    assert ref.keep(*c, 1.0) and ref.score(*c) == np.float32(1.0)
    # ... and so are real ones: every row of the 'same' target
    g1, kps = scene.frame1(), scene.detected()
    gt, q, sf, err = _forward(win, "same")
    k, sc = ref.rows(g1, gt, win, kps, q, sf, 1.0)
    assert sf.all() and k.all() and (sc == np.float32(1.0)).all()


@pytest.mark.parametrize("win", scene.WINDOWS)
def test_gain_and_bias_do_not_matter_inversion_and_flatness_do(win):
    I = _texture_window(win)
    J = np.rint(0.6 * I + 40 * 32).astype(np.int64)          # x 0.6 + 40 grey levels, in the windows' x 32 scale
    assert ref.keep(*ref.sums(I, J), 0.99) and ref.score(*ref.sums(I, J)) > np.float32(0.99)
    inv = 8160 - I
    c = ref.sums(I, inv)
    assert c[0] < 0 and not ref.keep(*c, 0.01) and ref.score(*c) == np.float32(-1.0)
    for flat in (np.zeros_like(I), np.full_like(I, 4000)):
        for c in (ref.sums(I, flat), ref.sums(flat, I), ref.sums(flat, flat)):
            assert c[0] == 0 and (c[1] == 0 or c[2] == 0)
            assert not ref.keep(*c, 0.01) and not ref.keep(*c, 1.0) and ref.score(*c) == np.float32(0.0)


def test_the_decision_is_monotone_in_the_threshold_and_agrees_with_the_score_away_from_it():
    g1, kps = scene.frame1(), scene.detected()
    gt, q, sf, err = _forward(10, "shift")
    prev = None
    for thr in (0.25, 0.5, 0.75, 0.9, 0.99, 1.0):
        k, sc = ref.rows(g1, gt, 10, kps, q, sf, thr)
        assert not k[sf == 0].any() and not sc[sf == 0].any()
        away = (sf == 1) & (np.abs(sc - np.float32(thr)) > 1e-6)
        assert np.array_equal(k[away] == 1, sc[away] > thr), thr
        assert prev is None or not (k & ~prev).any(), thr
        prev = k
    k0, sc0 = ref.rows(g1, gt, 10, kps, q, sf, 0.0)
    assert np.array_equal(k0, sf) and np.array_equal(sc0, sc)


def test_windows_that_fail_the_bounds_test_have_no_values():
    g, win = scene.frame1(), 10
    half = (win - 1) * 0.5
    assert ref.window_values(g, win, -win + half, 5.0) is not None           # ipx == -win
    assert ref.window_values(g, win, -win + half - 0.01, 5.0) is None
    assert ref.window_values(g, win, scene.W - 1 + half + 0.5, 5.0) is not None      # ipx == w - 1
    assert ref.window_values(g, win, scene.W + half, 5.0) is None
    assert ref.window_values(g, win, 5.0, scene.H + half) is None and ref.window_values(g, win, 5.0, np.float32("nan")) is None
    # at an integer position the window is the pixels x 32
    v = ref.window_values(g, 3, 10.0, 20.0)
    assert np.array_equal(v, g[19:22, 9:12].astype(np.int64) * 32)


# ---- the scenes exercise both outcomes ----
TABLE = {(3, "shift"): (92, 74), (10, "shift"): (159, 122), (10, "gain"): (140, 99), (21, "shift"): (167, 37), (31, "shift"): (167, 27)}


@pytest.mark.parametrize("win,kind", sorted(TABLE))
def test_the_scenes_drop_some_rows_and_keep_some_at_075(win, kind):
    g1, kps = scene.frame1(), scene.detected()
    gt, q, sf, err = _forward(win, kind)
    k, sc = ref.rows(g1, gt, win, kps, q, sf, 0.75)
    fwd, kept = int(sf.sum()), int(k.sum())
    print("window", win, kind, "forward", fwd, "kept", kept, "mean err", float(err[sf == 1].mean()))
    scene.check_fractions(fwd, kept, (win, kind))
    assert (fwd, kept) == TABLE[(win, kind)]          # the figures the rule was proposed with, in the oracle's default arithmetic


@pytest.mark.parametrize("win", [10, 21, 31])
def test_an_unrelated_target_keeps_nothing_from_window_10_on(win):
    g1, kps = scene.frame1(), scene.detected()
    gt, q, sf, err = _forward(win, "unrelated")
    k, sc = ref.rows(g1, gt, win, kps, q, sf, 0.75)
    assert sf.sum() >= 10 and not k.any()


def test_the_patch_error_doubles_under_gain_and_the_share_kept_barely_moves():
    g1, kps = scene.frame1(), scene.detected()
    shares, errs = [], []
    for kind in ("shift", "gain"):
        gt, q, sf, err = _forward(10, kind)
        k, _ = ref.rows(g1, gt, 10, kps, q, sf, 0.75)
        shares.append(k.sum() / sf.sum())
        errs.append(float(err[sf == 1].mean()))
    assert errs[1] > 1.7 * errs[0] and abs(shares[1] - shares[0]) < 0.1, (errs, shares)


# ---- the surface ----
NEW_SYMBOLS = ("pc_lk_track_correlated", "pc_analyzer_set_min_correlation")


@pytest.fixture(scope="module")
def core():
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


def test_the_option_exists_and_is_off_by_default(core):
    fo = core.OpticalFlowOptions()
    assert fo.min_correlation == 0.0
    fo.min_correlation = 0.75
    assert fo.min_correlation == 0.75
    d = core.OpticalFlowOptions()
    assert (d.window_size, d.max_level, d.term_max_iters, d.term_epsilon, d.min_eigen_threshold) == (10, 3, 30, 0.01, 1e-4)
    assert d.forward_backward_threshold == 0.0 and d.target_mask_margin == -1


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polychase_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in hip.SYMBOLS and hasattr(lib, s), s
    assert callable(hip.lk_track_correlated) and callable(hip.Analyzer.set_min_correlation)
    assert hip.KERNEL_CLASSES[-1] == "lk_corr" and re.search(r"#define PC_K_LK_CORR %d\b" % hip.KERNEL_CLASSES.index("lk_corr"), text)
    assert re.search(r"#define PC_K_COUNT %d\b" % len(hip.KERNEL_CLASSES), text)
    assert [f[0] for f in hip.FlowOptions._fields_] == ["window_size", "max_level", "term_max_iters", "term_epsilon", "min_eigen_threshold"]


def test_entry_points_refuse_a_null_context_and_bad_values():
    """needs no device: the calls return an error before they touch one"""
    L = hip.load()
    L.pc_last_error.restype = ctypes.c_char_p
    opt = hip.flow_options()
    for v in (0.0, 0.75, 1.0):
        assert L.pc_lk_track_correlated(None, None, None, 1, ctypes.byref(opt), v, 0.0, -1, None, None, None, None) == -1
        assert "null" in L.pc_last_error().decode()
        assert L.pc_analyzer_set_min_correlation(None, v) == -1 and "null" in L.pc_last_error().decode()
    for v in (-0.1, 1.5, float("nan"), float("inf")):
        assert L.pc_lk_track_correlated(None, None, None, 1, ctypes.byref(opt), v, 0.0, -1, None, None, None, None) == -1
        assert "min_correlation" in L.pc_last_error().decode()
        assert L.pc_analyzer_set_min_correlation(None, v) == -1 and "min_correlation" in L.pc_last_error().decode()


def test_no_cpu_fallback_behind_the_call():
    import torch
    if torch.cuda.is_available():
        return      # with a device the GPU tests say what the call does
    with pytest.raises(hip.PolychaseHipError):
        ctx = hip.Context(0)
        hip.lk_track_correlated(ctx, None, [], 0.75)


@pytest.mark.parametrize("value", [-0.1, 1.5, float("nan")])
def test_a_bad_value_is_refused_by_every_entry_point_and_the_thread_before_any_frame_is_asked_for(core, value, tmp_path):
    vi = core.VideoInfo(32, 24, 1, 4)
    asked = []

    def accessor(fid):
        asked.append(fid)
        return np.zeros((24, 32, 3), np.uint8)

    fo = core.OpticalFlowOptions()
    fo.min_correlation = value
    go = core.GFTTOptions()
    with pytest.raises(ValueError, match="min_correlation"):
        core.generate_optical_flow_database(vi, accessor, None, str(tmp_path / "a.db"), go, fo)
    with pytest.raises(ValueError, match="min_correlation"):
        core.generate_optical_flow_shard(vi, accessor, None, str(tmp_path / "b.db"), 1, 3, flow_options=fo)
    with pytest.raises(ValueError, match="min_correlation"):
        core.generate_optical_flow_records(vi, accessor, None, 1, 3, 0, 0, go, fo)
    with pytest.raises(ValueError, match="min_correlation"):
        core.generate_optical_flow_database_multi_gpu(vi, accessor, None, str(tmp_path / "c.db"), 1, 0, flow_options=fo)
    with pytest.raises(ValueError, match="min_correlation"):
        core.OpticalFlowThread(vi, str(tmp_path / "d.db"), go, fo)
    assert asked == [], "no frame may be asked for"
    assert not any(os.path.exists(str(tmp_path / n)) for n in ("a.db", "b.db", "c.db", "d.db")), "and no database is opened"


# ---- the kernel's resources ----
@pytest.fixture(scope="module")
def kernels():
    path = build.hip_library_path()
    if not os.path.exists(path):
        build.build_hip()
    return {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}


def test_the_correlation_kernel_fits_beside_three_lk_wavefronts(kernels):
    found = [(n, k) for n, k in kernels.items() if "lk_corr_kernel" in n]
    assert len(found) == 1, [n for n, _ in found]        # the window is a runtime value, the arithmetic mode plays no part
    name, k = found[0]
    print(name, "VGPRs", k[".vgpr_count"], "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
    assert (k[".vgpr_count"] + 7) // 8 * 8 <= HELPER_VGPR_BUDGET == 104, f"{name}: {k['.vgpr_count']} VGPRs"
    assert k.get(".agpr_count", 0) == 0, name
    assert k[".group_segment_fixed_size"] <= HELPER_LDS_BUDGET == 18 * 1024, f"{name}: {k['.group_segment_fixed_size']} B of LDS"
    assert k.get(".private_segment_fixed_size", 0) == 0, f"{name}: spills to scratch"
    assert not k.get(".uses_dynamic_stack", False), name
