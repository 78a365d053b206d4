"""CPU: the numpy restatement of the brightness-normalised LK rule (tests/lk_normalized_ref.py; include/polychase_hip.h:
pc_lk_track_normalized) against the oracle, and the two new kernels' resources read from the built library."""
import functools

import numpy as np
import pytest

import fb_scene
import lk_correlation_scene as cscene
import lk_normalized_ref as ref
import lk_subpixel_scene as sscene
import oracle
from test_kernel_resources_cpu import _code_objects, _kernel_metadata
from polychase_amd import build

MAX_LEVEL = 2
WINDOWS = (5, 10, 21)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same_bits(got, want):
    return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _pyr(gray, win):
    return oracle.Pyramid(np.array(gray), win, MAX_LEVEL)


# ---- 1. with its two replacements switched off the restatement IS the oracle ----
def _switched_off_cases(win):
    """(name, frame1, target, keypoints): sub-pixel, border and out-of-frame keypoints on shifted, unchanged and gain-changed targets"""
    g1, kps = cscene.frame1(), cscene.keypoints(win)
    for kind in ("shift", "gain", "border"):
        yield "correlation/" + kind, g1, cscene.target(kind, win), kps
    s1, stargets, skps = sscene.scene(win)
    yield "subpixel/" + sscene.target_kinds(win)[0], s1, stargets[0], skps


@pytest.mark.parametrize("win", WINDOWS)
def test_switched_off_the_restatement_reproduces_the_oracle_bit_for_bit(win):
    opt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    with oracle.emulation(oracle.EMU_CANONICAL):
        for name, g1, gt, kps in _switched_off_cases(win):
            p1, pt = _pyr(g1, win), _pyr(gt, win)
            want = oracle.lk(p1, pt, kps, opt)
            got = ref.track(ref.Planes(p1), ref.Planes(pt), kps, opt, normalize=False)
            print(win, name, "keypoints", len(kps), "status 1:", int(want[1].sum()))
            assert 0 < want[1].sum() < len(kps), (win, name, "the scene must show both outcomes")
            assert np.array_equal(got[1], want[1]), (win, name, "status", np.nonzero(got[1] != want[1])[0][:8])
            assert np.array_equal(_bits(got[0]), _bits(want[0])), (win, name, "next_xy", np.nonzero((_bits(got[0]) != _bits(want[0])).any(axis=1))[0][:8])
            assert np.array_equal(_bits(got[2]), _bits(want[2])), (win, name, "err", np.nonzero(_bits(got[2]) != _bits(want[2]))[0][:8])


# ---- 2. a bias on either frame changes nothing, exactly ----
BIAS = 17


@functools.lru_cache(maxsize=None)
def _bias_frames(win):
    """frame 1 and a shifted target squeezed into 20 .. 224, so that adding BIAS clips nothing"""
    f1 = cscene.gain(cscene.frame1(), 0.8, 20.0)
    ft = cscene.gain(cscene.target("shift", win), 0.8, 20.0)
    assert f1.min() >= 20 and ft.min() >= 20 and int(f1.max()) + BIAS <= 255 and int(ft.max()) + BIAS <= 255
    return f1, ft


@pytest.mark.parametrize("win", (5, 10))
def test_an_integer_bias_on_either_frame_leaves_the_normalised_rows_bit_identical(win):
    f1, ft = _bias_frames(win)
    kps = cscene.keypoints(win)
    opt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    with oracle.emulation(oracle.EMU_CANONICAL):
        p1, pt = _pyr(f1, win), _pyr(ft, win)
        p1b, ptb = _pyr(f1 + np.uint8(BIAS), win), _pyr(ft + np.uint8(BIAS), win)
        # the oracle itself is NOT invariant: asserted first
        plain = oracle.lk(p1, pt, kps, opt)
        for what, a, b in (("searched", p1, ptb), ("template", p1b, pt)):
            moved = oracle.lk(a, b, kps, opt)
            differ = int(((_bits(moved[0]) != _bits(plain[0])).any(axis=1) | (moved[1] != plain[1])).sum())
            print(win, "plain LK, bias on the", what, "frame:", differ, "of", len(kps), "rows differ")
            assert differ >= 1, (win, what)
    P1, PT, P1B, PTB = (ref.Planes(p) for p in (p1, pt, p1b, ptb))
    base = ref.track(P1, PT, kps, opt)
    assert base[1].sum() >= 10
    for what, a, b in (("searched", P1, PTB), ("template", P1B, PT), ("both", P1B, PTB)):
        got = ref.track(a, b, kps, opt)
        assert np.array_equal(got[1], base[1]) and np.array_equal(_bits(got[0]), _bits(base[0])), (win, what)


# ---- 3. under a gain and bias change the normalised rows lie closer to the known flow ----
SHIFT = (2.3, -1.7)


def test_under_gain_and_bias_the_normalised_rows_are_closer_to_the_known_translation():
    win = 10
    base = fb_scene.texture(cscene.W, cscene.H, cscene.BASE_SEED)
    g1 = fb_scene.to_u8(base)
    gt = cscene.gain(fb_scene.to_u8(fb_scene.shifted(base, *SHIFT)), 0.7, 30.0)
    kps = np.array(cscene.detected())
    inner = ((kps[:, 0] > win + 4) & (kps[:, 0] < cscene.W - win - 4) & (kps[:, 1] > win + 4) & (kps[:, 1] < cscene.H - win - 4))
    kps = kps[inner]
    opt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    with oracle.emulation(oracle.EMU_CANONICAL):
        p1, pt = _pyr(g1, win), _pyr(gt, win)
        plain = oracle.lk(p1, pt, kps, opt)
    norm = ref.track(ref.Planes(p1), ref.Planes(pt), kps, opt)

    def median_epe(xy, st):
        d = xy[st == 1] - kps[st == 1] - np.array(SHIFT, np.float32)
        return float(np.median(np.hypot(d[:, 0], d[:, 1])))

    assert len(kps) >= 20 and 2 * int(norm[1].sum()) >= len(kps) and 2 * int(plain[1].sum()) >= len(kps), (len(kps), int(norm[1].sum()), int(plain[1].sum()))
    m_norm, m_plain = median_epe(norm[0], norm[1]), median_epe(plain[0], plain[1])
    print("median end-point error: normalised %.4f px (%d rows), plain %.4f px (%d rows), %d keypoints"
          % (m_norm, int(norm[1].sum()), m_plain, int(plain[1].sum()), len(kps)))
    assert m_norm < m_plain


# ---- 4. the two kernels exist and use no scratch ----
def test_the_normalised_kernels_are_in_the_library_and_use_no_scratch():
    path = build.hip_library_path()
    kernels = {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}
    for name in ("lk_norm_kernel", "lk_norm_fb_kernel"):
        found = [k for n, k in kernels.items() if name + "E" in n]          # (the mangled name: <length><name>E<parameters>)
        assert len(found) == 1, (name, [n for n in kernels if name in n])
        assert found[0][".private_segment_fixed_size"] == 0, (name, found[0][".private_segment_fixed_size"])
        assert found[0].get(".agpr_count", 0) == 0, name


# ---- 5. the kernels built from the shared pair helpers (csrc/hip/lk_pair.hpp, lk_fb.hpp) keep their registers ----
# (mangled-name fragment, VGPRs of the build before the helpers were shared: profiles/lk_pair_helpers.json)
PAIR_HELPER_INSTANCES = [
    ("12lk_fb_kernelILb0E", 56), ("12lk_fb_kernelILb1E", 78),
    ("18lk_wmask_fb_kernelILb0E", 62), ("18lk_wmask_fb_kernelILb1E", 78),
    ("15lk_wmask_kernelILb0E", 123), ("15lk_wmask_kernelILb1E", 129),
    ("15lk_plain_kernelILb0E", 125), ("15lk_plain_kernelILb1E", 156),
    ("17lk_norm_fb_kernelE", 71), ("19lk_search_fb_kernelE", 61), ("16lk_search_kernelE", 136),
]


@pytest.mark.parametrize("fragment,parent_vgprs", PAIR_HELPER_INSTANCES)
def test_a_kernel_of_the_pair_family_exists_once_and_keeps_its_registers(fragment, parent_vgprs):
    path = build.hip_library_path()
    kernels = {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}
    found = [k for n, k in kernels.items() if fragment in n]
    assert len(found) == 1, (fragment, [n for n in kernels if fragment in n])
    k = found[0]
    print("%s: %d VGPRs (before: %d)" % (k[".name"], k[".vgpr_count"], parent_vgprs))
    assert k.get(".private_segment_fixed_size", 0) == 0, (fragment, k.get(".private_segment_fixed_size"))
    assert k.get(".agpr_count", 0) == 0, (fragment, k.get(".agpr_count"))
    assert k[".vgpr_count"] <= parent_vgprs, (fragment, k[".vgpr_count"], parent_vgprs)
