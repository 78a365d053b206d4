"""CPU: affine refinement of the LK flow rows.  The numpy restatement of the rule (tests/lk_affine_ref.py; include/polychase_hip.h:
pc_lk_track_affine) on the oracle's forward rows under canonical emulation: what the header promises of it, the scenes of the GPU
tests exercise both outcomes, refined end points lie closer to the analytic flow of a rolling or zooming target, and the new kernel
is in the built library without scratch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import lk_affine_ref as ref
import lk_affine_scene as scene
from polychase_amd import build, hip
from test_kernel_resources_cpu import _code_objects, _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (3, 10, 21, 31)
IDENTITY = np.array([1.0, 0.0, 0.0, 1.0], np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


# ---- 1. a target identical to frame 1 ----
@pytest.mark.parametrize("win", WINDOWS)
def test_an_identical_target_keeps_every_row_bit_identical_under_the_identity(win):
    """e = 0 everywhere: every forward row whose template has a factor is accepted.  The header's rule gives a keypoint whose H
    is singular no factor ('no refinement unless s > 0'): the reflected border makes it so for a keypoint in a corner of the frame,
    (0, 0) and (95, 79) at window 3, and for one 3.5 px left of the frame at window 10.  Those rows are 'run and left unchanged';
    there may be at most two of them."""
    kps, forward, refined = scene.reference(win)
    t = scene.MIX7.index("same")
    (xy0, st0, err0), (xy, st, err, m, state) = forward[t], refined[t]
    fwd = st0 == 1
    assert fwd.sum() >= 100 and np.array_equal(st, st0)
    factor = np.array([fwd[i] and ref.Template(ref.Planes(_pyramid(win)), kps[i, 0], kps[i, 1]).L is not None for i in range(len(kps))])
    print(win, "forward rows", int(fwd.sum()), "without a factor", int((fwd & ~factor).sum()), kps[fwd & ~factor].tolist())
    assert (fwd & ~factor).sum() <= 2
    assert (state[factor] == ref.ACCEPTED).all() and (state[fwd & ~factor] == ref.UNCHANGED).all() and (state[~fwd] == ref.NOT_RUN).all()
    assert np.array_equal(_bits(xy), _bits(xy0)) and np.array_equal(_bits(err), _bits(err0))
    assert (_bits(m[fwd]) == _bits(IDENTITY)).all() and not m[~fwd].any()


def _pyramid(win):
    import oracle
    with oracle.emulation(oracle.EMU_CANONICAL):
        return oracle.Pyramid(np.array(scene.frame1()), win, scene.MAX_LEVEL)


# ---- 2. both outcomes occur ----
@pytest.mark.parametrize("win", WINDOWS)
def test_the_mix_of_seven_targets_shows_both_outcomes(win):
    kps, forward, refined = scene.reference(win)
    state = np.stack([r[4] for r in refined])
    st = np.stack([f[1] for f in forward])
    fwd, acc, unch = int((st == 1).sum()), int((state == ref.ACCEPTED).sum()), int((state == ref.UNCHANGED).sum())
    print("window", win, "forward", fwd, "accepted", acc, "unchanged", unch, "per target",
          list(zip(scene.MIX7, (state == ref.ACCEPTED).sum(axis=1).tolist(), (st == 1).sum(axis=1).tolist())))
    assert np.array_equal(state != ref.NOT_RUN, st == 1) and acc + unch == fwd
    assert fwd >= 10 and acc >= 0.1 * fwd and unch >= 0.1 * fwd


# ---- 3. closer to the analytic flow ----
@pytest.mark.parametrize("kind", sorted(scene.SIMILARITIES))
@pytest.mark.parametrize("win", [10, 21])
def test_refined_rows_lie_closer_to_the_analytic_flow_of_a_rolling_or_zooming_target(win, kind):
    kps, forward, refined = scene.reference(win)
    t = scene.MIX7.index(kind)
    sel = (refined[t][4] == ref.ACCEPTED) & scene.interior(kps, win)
    want = scene.flow(kind, kps)

    def median_epe(xy):
        d = xy[sel].astype(np.float64) - want[sel]
        return float(np.median(np.hypot(d[:, 0], d[:, 1])))

    before, after = median_epe(forward[t][0]), median_epe(refined[t][0])
    print("window", win, kind, "interior accepted rows", int(sel.sum()), "median end-point error %.4f -> %.4f px" % (before, after))
    assert sel.sum() >= 20
    assert after < 0.5 * before


# ---- 4. never a worse match, and nothing else moves ----
@pytest.mark.parametrize("win", WINDOWS)
def test_accepted_rows_match_their_patch_no_worse_and_every_other_row_is_the_oracles(win):
    kps, forward, refined = scene.reference(win)
    moved = 0
    for kind, (xy0, st0, err0), (xy, st, err, m, state) in zip(scene.MIX7, forward, refined):
        acc = state == ref.ACCEPTED
        assert np.array_equal(st, st0), kind
        assert (err[acc] <= err0[acc]).all(), kind
        assert np.array_equal(_bits(xy[~acc]), _bits(xy0[~acc])) and np.array_equal(_bits(err[~acc]), _bits(err0[~acc])), kind
        d = xy[acc] - xy0[acc]
        half = np.float32(win - 1) * np.float32(0.5)
        assert (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= half * half).all(), kind
        assert (np.abs(m[acc] - IDENTITY) <= 0.5).all(), kind
        moved += int((_bits(xy[acc]) != _bits(xy0[acc])).any(axis=1).sum())
    assert moved >= 10, "the refinement moves end points"


# ---- 5. the kernel ----
def test_the_affine_kernel_is_in_the_library_and_uses_no_scratch_and_no_agprs():
    path = build.hip_library_path()
    kernels = {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}
    found = [k for n, k in kernels.items() if "lk_affine_kernel" + "E" in n]          # (the mangled name: <length><name>E<parameters>)
    assert len(found) == 1, [n for n in kernels if "lk_affine" in n]                     # one instance: runtime window, no arithmetic mode
    k = found[0]
    print("lk_affine_kernel VGPRs", k[".vgpr_count"], "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
    assert k[".private_segment_fixed_size"] == 0, k[".private_segment_fixed_size"]
    assert k.get(".agpr_count", 0) == 0
    assert not k.get(".uses_dynamic_stack", False)


# ---- 6. the surface ----
NEW_SYMBOLS = ("pc_lk_track_affine", "pc_analyzer_set_affine_refinement")


@pytest.fixture(scope="module")
def core():
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


def test_new_symbols_are_declared_bound_and_exported_and_no_timing_class_is_added():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polychase_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in hip.SYMBOLS and hasattr(lib, s), s
    assert callable(hip.lk_track_affine) and callable(hip.Analyzer.set_affine_refinement)
    assert hip.KERNEL_CLASSES[-1] == "lk_corr" and re.search(r"#define PC_K_COUNT %d\b" % len(hip.KERNEL_CLASSES), text)


def test_the_option_exists_is_off_by_default_and_excludes_normalize_before_any_frame_is_asked_for(core, tmp_path):
    fo = core.OpticalFlowOptions()
    assert fo.affine_refinement is False and fo.normalize is False
    fo.affine_refinement = True
    assert fo.affine_refinement is True
    fo.normalize = True
    vi = core.VideoInfo(32, 24, 1, 4)
    asked = []

    def accessor(fid):
        asked.append(fid)
        return np.zeros((24, 32, 3), np.uint8)

    go = core.GFTTOptions()
    with pytest.raises(ValueError, match="affine_refinement"):
        core.generate_optical_flow_database(vi, accessor, None, str(tmp_path / "a.db"), go, fo)
    with pytest.raises(ValueError, match="affine_refinement"):
        core.generate_optical_flow_shard(vi, accessor, None, str(tmp_path / "b.db"), 1, 3, flow_options=fo)
    with pytest.raises(ValueError, match="affine_refinement"):
        core.generate_optical_flow_database_multi_gpu(vi, accessor, None, str(tmp_path / "c.db"), 1, 0, flow_options=fo)
    with pytest.raises(ValueError, match="affine_refinement"):
        core.OpticalFlowThread(vi, str(tmp_path / "d.db"), go, fo)
    assert asked == [] and not any(os.path.exists(str(tmp_path / n)) for n in ("a.db", "b.db", "c.db", "d.db"))


def test_entry_points_refuse_bad_values_before_the_handles():
    """needs no device: the calls return an error before they touch one"""
    L = hip.load()
    L.pc_last_error.restype = ctypes.c_char_p
    opt = hip.flow_options()

    def track(affine, normalize):
        return L.pc_lk_track_affine(None, None, None, 1, ctypes.byref(opt), affine, normalize, 0.0, 0.0, -1, None, None, None, None, None, None, None)

    for affine in (0, 1):
        assert track(affine, 0) == -1 and "null" in L.pc_last_error().decode()
        assert L.pc_analyzer_set_affine_refinement(None, affine) == -1 and "null" in L.pc_last_error().decode()
    for affine in (2, -1):
        assert track(affine, 0) == -1 and "affine" in L.pc_last_error().decode()
        assert L.pc_analyzer_set_affine_refinement(None, affine) == -1 and "affine" in L.pc_last_error().decode()
    assert track(1, 1) == -1 and "normalize" in L.pc_last_error().decode()
    assert track(0, 1) == -1 and "null" in L.pc_last_error().decode()
