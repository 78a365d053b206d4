"""CPU: the channel rules of the 16-bit and RGBA frame types (include/polychase_hip.h: pc_frame_set_pixels) -- the restatement of
tests/ingest16_ref.py against plain arithmetic over all 65536 values of a 16-bit channel, and polychase_core.frame_channel_bytes
(the host's use of the rule header the kernels include) against the restatement.  Everything is exact."""
import ctypes

import numpy as np
import pytest

import ingest16_ref as ref
import ingest_layouts as il
from polychase_amd import build, hip

ALL16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)


@pytest.fixture(scope="module")
def core():
    import os
    import sys
    build.build_all()
    import torch  # noqa: F401  (one HIP runtime per process: load torch's first, see polychase_amd/hip.py)
    sys.path.insert(0, os.path.dirname(build.core_module_path()))
    import polychase_core
    return polychase_core


def test_uint16_rule_is_the_nearest_integer_to_v_over_257():
    b = ref.u16_to_u8(ALL16).astype(np.int64)
    v = np.arange(65536, dtype=np.int64)
    assert np.array_equal(b, (2 * v + 257) // 514)            # round(v / 257); 257 is odd, so no v lies half-way
    assert np.all((2 * v) % 514 != 257)                       # a tie would need 2 v = 257 (2 k + 1)
    assert np.array_equal(b, np.floor(v / 257.0 + 0.5).astype(np.int64))
    assert np.array_equal(b[257 * np.arange(256)], np.arange(256))
    assert np.all(np.diff(b) >= 0) and b.min() == 0 and b.max() == 255
    assert int(np.count_nonzero(b != (v >> 8))) == 16256      # the top-byte rule is another rule


def test_half_widening_matches_numpy_on_every_pattern():
    got = ref.f16_bits_to_f32(ALL16)
    want = ALL16.view(np.float16).astype(np.float32)
    nan = np.isnan(want)
    assert int(nan.sum()) == 2 * 1023 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    sub = ((ALL16 >> 10) & 31 == 0) & (ALL16 & 0x3ff != 0)
    assert int(sub.sum()) == 2046 and np.all(got[sub] != 0)   # no subnormal half is flushed


def _every_pattern_frame(dtype, channels, seed):
    """256 x 256: channel c holds every 16-bit pattern once, in an order of its own; alpha is noise"""
    rng = np.random.default_rng(seed)
    planes = [ALL16, ALL16[::-1], rng.permutation(ALL16)]
    if channels == 4:
        planes.append(rng.integers(0, 65536, 65536).astype(np.uint16))
    return np.ascontiguousarray(np.stack(planes, axis=1).reshape(256, 256, channels)).view(dtype)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("dtype", [np.uint16, np.float16])
def test_frame_channel_bytes_on_every_pattern(core, dtype, channels):
    img = _every_pattern_frame(dtype, channels, 5)
    got = core.frame_channel_bytes(img)
    assert got.dtype == np.uint8 and got.shape == (256, 256, 3)
    assert np.array_equal(got, ref.channel_bytes(img))
    if dtype == np.float16:     # ... which for halves is the float32 frame's
        assert np.array_equal(got, core.frame_channel_bytes(img.astype(np.float32)))
        assert np.array_equal(got, il.float_to_u8(img[:, :, :3].astype(np.float32)))


def test_frame_channel_bytes_of_the_byte_and_float_types(core):
    rng = np.random.default_rng(6)
    u8 = rng.integers(0, 256, (9, 7, 4), dtype=np.uint8)
    assert np.array_equal(core.frame_channel_bytes(u8), u8[:, :, :3])
    assert np.array_equal(core.frame_channel_bytes(u8[:, :, :3]), u8[:, :, :3])      # a view that is not contiguous
    f = rng.uniform(-0.5, 1.5, (9, 7, 3)).astype(np.float32)
    f[0, 0] = (np.nan, np.inf, -np.inf)
    assert np.array_equal(core.frame_channel_bytes(f), il.float_to_u8(f))
    x = (u8[:, :, :3].astype(np.uint16) * 257)
    assert np.array_equal(core.frame_channel_bytes(x), u8[:, :, :3])


@pytest.mark.parametrize("bad", [np.zeros((4, 4, 3), np.int16), np.zeros((4, 4, 3), np.float64), np.zeros((4, 4, 2), np.uint16),
                                 np.zeros((4, 4), np.uint16), np.zeros((4, 4, 5), np.float16)],
                         ids=["int16", "float64", "two_channels", "no_channel_axis", "five_channels"])
def test_frame_channel_bytes_refuses_other_frames(core, bad):
    with pytest.raises(ValueError, match="uint16"):     # the message lists the accepted types
        core.frame_channel_bytes(bad)


def test_the_new_symbols_are_bound_and_exported():
    new = ("pc_frame_set_pixels", "pc_analyzer_put_frame_pixels")
    assert set(new) <= set(hip.SYMBOLS)
    lib = ctypes.CDLL(build.hip_library_path())
    for s in new:
        assert hasattr(lib, s), s
    assert callable(hip.Frame.set_pixels) and callable(hip.Analyzer.put_frame_pixels)
    assert (hip.PIXEL_U8, hip.PIXEL_U16, hip.PIXEL_F16, hip.PIXEL_F32) == (0, 1, 2, 3)


def test_the_binding_refuses_other_frames_before_the_library_sees_them():
    for bad in (np.zeros((4, 4, 3), np.int16), np.zeros((4, 4, 3), np.float64), np.zeros((4, 4, 2), np.uint16), np.zeros((4, 4), np.uint16)):
        with pytest.raises(ValueError):
            hip._pixels_args(bad, 4, 4)
    assert hip._pixels_args(np.zeros((4, 4, 4), np.float16), 4, 4)[1:] == (32, hip.PIXEL_F16, 4, 0)
