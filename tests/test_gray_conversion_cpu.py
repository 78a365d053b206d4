"""CPU: the gray conversion (include/polychase_hip.h: pc_gray_conversion; OpticalFlowOptions.channel_weights / float_transfer).  The
rule restated in numpy (tests/gray_conversion_ref.py) against what the header states of it, the host-side table builder entry for
entry, the options' validation at every entry point before a frame is asked for, the setter's validation at the C ABI without a
device, and the new kernel instances in the built library, without scratch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import gray_conversion_ref as ref
import oracle
from polychase_amd import build, hip
from test_kernel_resources_cpu import _code_objects, _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = [("srgb", 2.2, 0.0), ("srgb", 2.2, 4.0), ("gamma", 2.2, 0.0)]


@pytest.fixture(scope="module")
def core():
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


# ---- 1. weights ----
# the header's cases, then what they leave open: a tie between G and B that takes the residual, a tie without one, a zero channel
QUANTISED = [((0.299, 0.587, 0.114), (9798, 19234, 3736)), ((9798, 19235, 3735), (9798, 19235, 3735)), ((1, 1, 1), (10922, 10923, 10923)),
             ((3, 3, 1), (14044, 14043, 4681)), ((0.2126, 0.7152, 0.0722), (6966, 23436, 2366)),
             ((1, 3, 3), (4681, 14044, 14043)), ((0, 1, 1), (0, 16384, 16384)), ((0, 0, 5), (0, 0, 32768)), ((2, 1, 1), (16384, 8192, 8192))]


@pytest.mark.parametrize("weights,want", QUANTISED)
def test_the_librarys_quantiser_gives_what_the_header_states(core, weights, want):
    """pc_gray_quantize_weights is the one host quantiser: the driver calls it for OpticalFlowOptions.channel_weights, polychase_core and
    the ctypes binding expose it"""
    assert ref.quantize(weights) == want and sum(want) == 32768
    assert hip.quantize_channel_weights(weights) == want
    assert tuple(core.quantize_channel_weights(weights)) == want


def test_the_librarys_quantiser_equals_the_numpy_rule_on_random_weights(core):
    rng = np.random.default_rng(15)
    cases = [tuple(rng.uniform(0, 1, 3)) for _ in range(300)] + [tuple(rng.integers(0, 6, 3).astype(float)) for _ in range(300)]
    cases = [c for c in cases if sum(c) > 0]
    residuals = 0
    for w in cases:
        want = ref.quantize(w)
        s = sum(w)
        residuals += sum(int(np.floor(c / s * 32768.0 + 0.5)) for c in w) != 32768
        assert hip.quantize_channel_weights(w) == want and tuple(core.quantize_channel_weights(w)) == want, w
    assert residuals >= 100 and sum(len(set(c)) < 3 for c in cases) >= 100     # the residual and the tie-break are exercised
    for bad in ((1.0, -0.5, 0.5), (0.0, 0.0, 0.0), (float("nan"), 1.0, 1.0), (float("inf"), 1.0, 1.0)):
        with pytest.raises(ValueError):
            core.quantize_channel_weights(bad)


def test_the_default_weights_give_the_oracles_gray_and_a_unit_weight_gives_its_channel():
    rgb = np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    rgb[0, :3] = [[255, 255, 255], [0, 0, 0], [255, 0, 255]]
    c = hip.GrayConversion()
    hip.load().pc_gray_default_conversion(ctypes.byref(c))
    default = (c.weight_r, c.weight_g, c.weight_b)
    assert default == ref.DEFAULT_WEIGHTS == hip.DEFAULT_GRAY_WEIGHTS
    assert np.array_equal(ref.weighted_gray(rgb, default), oracle.rgb2gray(rgb))
    for k, w in enumerate([(1, 0, 0), (0, 2.5, 0), (0, 0, 1e-3)]):
        assert np.array_equal(ref.weighted_gray(rgb, hip.quantize_channel_weights(w)), rgb[:, :, k])


# ---- 2. the table ----
@pytest.mark.parametrize("kind,gamma,exposure", TABLES)
def test_the_builder_equals_the_numpy_rule_entry_for_entry(kind, gamma, exposure):
    u = ref.unrounded(kind, gamma, exposure)
    gap = float(np.abs(u - np.round(u)).min())
    print(kind, gamma, exposure, "nearest 255 f + 0.5 comes to an integer: %.3g" % gap)
    assert gap > 1e-6, "an entry could round either way: equality of two libms would be luck"
    want = ref.table(kind, gamma, exposure)
    got = hip.float_transfer_table(kind, gamma, exposure)
    assert got.dtype == np.uint8 and got.shape == (ref.ENTRIES,) and hip.TRANSFER_ENTRIES == ref.ENTRIES
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert want[0] == 0 and want[-1] == 255


def test_the_srgb_table_is_monotone_in_steps_of_one_and_the_256_codes_round_trip(core):
    t = ref.table("srgb")
    d = np.diff(t[1:].astype(np.int32))
    assert d.min() == 0 and d.max() == 1
    codes = np.arange(256)
    lin = ref.srgb_eotf(codes / 255.0).astype(np.float32)
    assert np.array_equal(t[ref.transfer_index(lin)], codes.astype(np.uint8))
    # ... and 4 stops down under exposure +4: the planes of the darkened plate are the original's
    t4 = ref.table("srgb", exposure=4.0)
    assert np.array_equal(t4[ref.transfer_index((ref.srgb_eotf(codes / 255.0) / 16.0).astype(np.float32))], codes.astype(np.uint8))
    assert np.array_equal(np.asarray(core.float_transfer_table("srgb")), t)
    assert np.array_equal(np.asarray(core.float_transfer_table("srgb", exposure=4.0)), t4)
    assert np.array_equal(np.asarray(core.float_transfer_table("gamma", gamma=2.2)), ref.table("gamma", 2.2))
    for bad in (dict(kind="linear"), dict(kind="gamma", gamma=0.5), dict(kind="gamma", gamma=float("nan")), dict(kind="srgb", exposure=17.0),
                dict(kind="srgb", exposure=float("inf"))):
        with pytest.raises(ValueError):
            core.float_transfer_table(**bad)


def test_the_index_rule_on_special_values():
    f = np.float32
    lo, hi = f(2.0 ** -16), f(16.0)
    idx = lambda v: int(ref.transfer_index(np.array([v], np.float32))[0])   # noqa: E731
    for v in (f(np.nan), f(-np.inf), f(0.0), f(-0.0), f(1e-40), f(-1e-40), f(-0.25), np.nextafter(lo, f(0))):
        assert idx(v) == 0, v
    assert idx(lo) == 1 and idx(np.nextafter(lo, f(1))) == 1
    assert idx(np.nextafter(hi, f(0))) == 20480 and idx(hi) == 20480 and idx(np.nextafter(hi, f(32))) == 20480
    assert idx(f(np.inf)) == 20480 and idx(f(3.4e38)) == 20480
    assert idx(f(1.0)) == 1 + 16 * 1024 and idx(np.nextafter(f(1.0), f(0))) == 16 * 1024
    # the low 13 bits do not take part; the 14th does
    pat = lambda b: np.array([b], np.uint32).view(np.float32)[0]   # noqa: E731
    assert idx(pat(0x3E000000)) == idx(pat(0x3E001FFF)) == idx(pat(0x3E002000)) - 1
    # entry i covers [x_i, x_i + 2^e / 1024)
    for i in (1, 2, 1024, 1025, 17000, 20480):
        e, m = -16 + (i - 1) // 1024, (i - 1) % 1024
        x = f(2.0 ** e * (1 + m / 1024))
        assert idx(x) == i and idx(np.nextafter(x, f(0))) == i - 1, i
    # the function the kernels compile (common.hpp: transfer_index, an unsigned range test and a shift on the pattern), run on the
    # host through pc_float_transfer_index: the specials, then every pattern whose low 13 bits are all zero or all one -- every
    # exponent, sign and index bit there is
    s = ref.specials()
    assert np.isnan(s).sum() >= 3 and np.isinf(s).sum() == 2 and (s.view(np.uint32) & 0x1FFF == 0x1FFF).sum() >= 3
    assert np.array_equal(hip.transfer_index(s), ref.transfer_index(s))
    top = np.arange(1 << 19, dtype=np.uint32) << np.uint32(13)
    for low in (0, 0x1FFF, 0x1000):
        v = (top | np.uint32(low)).view(np.float32)
        got, want = hip.transfer_index(v), ref.transfer_index(v)
        assert np.array_equal(got, want), (low, np.nonzero(got != want)[0][:4])
    assert set(np.unique(hip.transfer_index(top.view(np.float32))).tolist()) == set(range(ref.ENTRIES))


# ---- 3. the options ----
BAD_OPTIONS = [("channel_weights", (1.0, -0.5, 0.5)), ("channel_weights", (0.0, 0.0, 0.0)), ("channel_weights", (float("nan"), 1.0, 1.0)),
               ("channel_weights", (float("inf"), 1.0, 1.0)), ("float_transfer", "linear"), ("float_transfer", ""),
               ("float_transfer_gamma", 0.5), ("float_transfer_gamma", 4.5), ("float_transfer_gamma", float("nan")),
               ("float_exposure", 16.5), ("float_exposure", -17.0), ("float_exposure", float("nan")), ("float_exposure", float("inf"))]


def test_the_options_exist_with_their_defaults(core):
    fo = core.OpticalFlowOptions()
    assert fo.channel_weights is None and fo.float_transfer == "none" and fo.float_transfer_gamma == 2.2 and fo.float_exposure == 0.0
    fo.channel_weights = (0.0, 0.0, 1.0)
    assert list(fo.channel_weights) == [0.0, 0.0, 1.0]
    fo.channel_weights = None
    assert fo.channel_weights is None
    fo.float_transfer, fo.float_transfer_gamma, fo.float_exposure = "gamma", 2.4, -1.5
    assert (fo.float_transfer, fo.float_transfer_gamma, fo.float_exposure) == ("gamma", 2.4, -1.5)


@pytest.mark.parametrize("name,value", BAD_OPTIONS)
def test_every_bad_value_is_refused_at_every_entry_point_before_a_frame_is_asked_for(core, tmp_path, name, value):
    fo = core.OpticalFlowOptions()
    setattr(fo, name, value)
    vi = core.VideoInfo(32, 24, 1, 4)
    asked = []

    def accessor(fid):
        asked.append(fid)
        return np.zeros((24, 32, 3), np.uint8)

    go = core.GFTTOptions()
    with pytest.raises(ValueError, match=name):
        core.generate_optical_flow_database(vi, accessor, None, str(tmp_path / "a.db"), go, fo)
    with pytest.raises(ValueError, match=name):
        core.generate_optical_flow_shard(vi, accessor, None, str(tmp_path / "b.db"), 1, 3, flow_options=fo)
    with pytest.raises(ValueError, match=name):
        core.generate_optical_flow_records(vi, accessor, None, 1, 3, 0, 0, flow_options=fo)
    with pytest.raises(ValueError, match=name):
        core.generate_optical_flow_database_multi_gpu(vi, accessor, None, str(tmp_path / "c.db"), 1, 0, flow_options=fo)
    with pytest.raises(ValueError, match=name):
        core.OpticalFlowThread(vi, str(tmp_path / "d.db"), go, fo)
    assert asked == [] and not any(os.path.exists(str(tmp_path / n)) for n in ("a.db", "b.db", "c.db", "d.db"))


# ---- 4. the C ABI ----
NEW_SYMBOLS = ("pc_gray_default_conversion", "pc_context_set_gray_conversion", "pc_context_get_gray_conversion", "pc_float_transfer_table",
               "pc_gray_quantize_weights", "pc_float_transfer_index")


def test_new_symbols_are_declared_bound_and_exported_and_no_timing_class_is_added():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polychase_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in hip.SYMBOLS and hasattr(lib, s), s
    assert re.search(r"#define PC_TRANSFER_ENTRIES %d\b" % ref.ENTRIES, text)
    assert callable(hip.Context.set_gray_conversion) and callable(hip.Context.gray_conversion)
    assert hip.KERNEL_CLASSES[-1] == "lk_corr" and re.search(r"#define PC_K_COUNT %d\b" % len(hip.KERNEL_CLASSES), text)


def test_the_setter_and_the_builder_refuse_bad_values_without_a_device():
    """needs no device: the calls return an error before they touch one"""
    L = hip.load()
    c = hip.GrayConversion()
    L.pc_gray_default_conversion(ctypes.byref(c))
    assert (c.weight_r, c.weight_g, c.weight_b, c.float_table) == (9798, 19235, 3735, None)

    def set_(r, g, b):
        c.weight_r, c.weight_g, c.weight_b = r, g, b
        return L.pc_context_set_gray_conversion(None, ctypes.byref(c)), L.pc_last_error().decode()

    for w in ((32769, 0, -1), (-1, 32768, 1), (40000, -7232, 0), (9798, 19235, 3736), (0, 0, 0), (32768, 32768, 32768), (2 ** 31 - 1, 2 ** 31 - 1, 2)):
        rc, why = set_(*w)
        assert rc == -1 and "weight" in why, (w, why)
    for w in ((9798, 19235, 3735), (32768, 0, 0), (0, 0, 32768)):
        rc, why = set_(*w)
        assert rc == -1 and "null" in why, (w, why)
    assert L.pc_context_set_gray_conversion(None, None) == -1 and "null" in L.pc_last_error().decode()
    out = np.zeros(ref.ENTRIES, np.uint8)
    for kind, gamma, exposure, word in ((0, 2.2, 0.0, "kind"), (3, 2.2, 0.0, "kind"), (2, 0.99, 0.0, "gamma"), (2, 4.01, 0.0, "gamma"),
                                        (2, float("nan"), 0.0, "gamma"), (1, float("inf"), 0.0, "gamma"), (1, 2.2, 16.01, "exposure"),
                                        (1, 2.2, -16.01, "exposure"), (1, 2.2, float("nan"), "exposure"), (2, 2.2, float("inf"), "exposure")):
        assert L.pc_float_transfer_table(kind, gamma, exposure, out.ctypes.data) == -1 and word in L.pc_last_error().decode(), (kind, gamma, exposure)
    assert not out.any()
    assert L.pc_float_transfer_table(1, 2.2, 0.0, None) == -1 and "null" in L.pc_last_error().decode()
    assert L.pc_float_transfer_table(2, 1.0, -16.0, out.ctypes.data) == 0 and L.pc_float_transfer_table(2, 4.0, 16.0, out.ctypes.data) == 0
    with pytest.raises(ValueError):
        hip.float_transfer_table("linear")
    for bad in ((1, 2), (1, -1, 1), (0, 0, 0), (float("nan"), 1, 1), (float("inf"), 1, 1)):
        with pytest.raises(ValueError):
            hip.quantize_channel_weights(bad)


# ---- 5. the kernels ----
def test_the_new_kernel_instances_are_in_the_library_and_use_no_scratch():
    path = build.hip_library_path()
    kernels = {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}
    # (mangled names: <length><name>I<template arguments>E...; level_kernel<4 | 5 | 6> are SRC_RGB8_W, SRC_RGBF32_W, SRC_RGBF32_T)
    wanted = ["level_kernelILi4EE", "level_kernelILi5EE", "level_kernelILi6EE", "rgb2gray_weighted_kernel" + "E",
              "rgbf32_to_gray_converted_kernelILb0EE", "rgbf32_to_gray_converted_kernelILb1EE"]
    for frag in wanted:
        found = [k for n, k in kernels.items() if frag in n]
        assert len(found) == 1, (frag, [n for n in kernels if "level_kernel" in n or "gray" in n])
        k = found[0]
        print(frag, "VGPRs", k[".vgpr_count"], "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0, (frag, k[".private_segment_fixed_size"])
        assert k.get(".agpr_count", 0) == 0
        assert not k.get(".uses_dynamic_stack", False)
    # the instances of the default conversion are still there, one each
    for frag in ("level_kernelILi0EE", "level_kernelILi1EE", "level_kernelILi2EE", "level_kernelILi3EE"):
        assert len([n for n in kernels if frag in n]) == 1, frag
