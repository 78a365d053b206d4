"""The channel rules of the 16-bit and RGBA frame types (pc_frame_set_pixels; csrc/hip/pixel_rules.hpp), restated in numpy, and
what a frame put as such pixels must hold.  TEST INFRASTRUCTURE ONLY; nothing here needs a GPU.

  u16_to_u8(v)             uint16 channel -> byte: (v * 255 + 32895) >> 16 in 32-bit unsigned arithmetic
  f16_bits_to_f32(bits)    IEEE binary16 patterns -> the float32 of the same value, by integer operations (no astype)
  channel_bytes(img, table)    (H, W, 3) bytes of a frame of any accepted type; float channels through `table` when given
  planes_expected(img, weights, table, win, max_level)   gray and the planes of every level, from the CPU oracle
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import gray_conversion_ref as gref
import ingest_layouts as il
import oracle

PIXEL_U8, PIXEL_U16, PIXEL_F16, PIXEL_F32 = 0, 1, 2, 3     # pc_pixel_type of include/polychase_hip.h
PIXEL_TYPE = {np.dtype(np.uint8): PIXEL_U8, np.dtype(np.uint16): PIXEL_U16, np.dtype(np.float16): PIXEL_F16, np.dtype(np.float32): PIXEL_F32}


def u16_to_u8(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v)
    assert v.dtype == np.uint16
    return ((v.astype(np.uint32) * np.uint32(255) + np.uint32(32895)) >> np.uint32(16)).astype(np.uint8)


def f16_bits_to_f32(bits: np.ndarray) -> np.ndarray:
    """uint16 patterns -> float32 values.  Normal numbers: the exponent rebased by 112, the mantissa shifted by 13; subnormals
    m * 2^-24: the leading one of m becomes the hidden bit; exponent 31: inf / NaN with the payload shifted; zeros keep their
    sign."""
    h = np.asarray(bits)
    assert h.dtype == np.uint16
    h = h.astype(np.uint32)
    sign = (h & 0x8000) << 16
    e = (h >> 10) & 31
    m = h & 0x3ff
    # position of the leading one of m (0 .. 9) by comparisons; m == 0 is not used
    top = np.zeros_like(m)
    for k in range(1, 10):
        top = np.where(m >= (1 << k), k, top)
    s = (10 - top).astype(np.uint32)                                  # shift that puts the leading one at bit 10
    sub = sign | ((113 - s) << 23) | (((m << s) & 0x3ff) << 13)
    out = np.where(e == 0, np.where(m == 0, sign, sub), np.where(e == 31, sign | 0x7f800000 | (m << 13), sign | ((e + 112) << 23) | (m << 13)))
    return out.astype(np.uint32).view(np.float32)


def channel_bytes(img: np.ndarray, table: np.ndarray | None = None) -> np.ndarray:
    """(H, W, 3) uint8: every colour channel by the rule of the frame's type; alpha dropped.  `table` (the float transfer table)
    applies to float16 / float32 frames only."""
    assert img.ndim == 3 and img.shape[2] in (3, 4), img.shape
    c = np.ascontiguousarray(img[:, :, :3])
    if c.dtype == np.uint8:
        return c
    if c.dtype == np.uint16:
        return u16_to_u8(c)
    x = f16_bits_to_f32(c.view(np.uint16)) if c.dtype == np.float16 else c
    assert x.dtype == np.float32
    if table is not None:
        return np.asarray(table, np.uint8)[gref.transfer_index(x)]
    return il.float_to_u8(x)


def gray_expected(img: np.ndarray, weights=None, table=None) -> np.ndarray:
    q = np.asarray(gref.DEFAULT_WEIGHTS if weights is None else weights, np.int64)
    assert q.sum() == 32768
    b = channel_bytes(img, table).astype(np.int64)
    return ((b[:, :, 0] * q[0] + b[:, :, 1] * q[1] + b[:, :, 2] * q[2] + (1 << 14)) >> 15).astype(np.uint8)


def planes_of_gray(gray: np.ndarray, win: int, max_level: int) -> SimpleNamespace:
    """the namespace of ingest_layouts.expected, from a gray plane"""
    gray = np.ascontiguousarray(gray)
    pyr = oracle.Pyramid(gray, win, max_level)
    e = SimpleNamespace(gray=gray, num_levels=pyr.num_levels, sizes=[], level=[], deriv=[], level16=[])
    for l in range(pyr.num_levels):
        u8 = pyr.image(l)
        e.sizes.append(pyr.level_size(l))
        e.level.append(u8)
        e.deriv.append(pyr.deriv(l))
        e.level16.append(u8.astype(np.uint16) << 7)
    for a in [e.gray] + e.level + e.deriv + e.level16:
        a.setflags(write=False)
    return e


def planes_expected(img: np.ndarray, weights, table, win: int, max_level: int) -> SimpleNamespace:
    return planes_of_gray(gray_expected(img, weights, table), win, max_level)
