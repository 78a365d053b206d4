"""The gray conversion of include/polychase_hip.h (pc_gray_conversion) restated in numpy.  TEST INFRASTRUCTURE ONLY; nothing here
needs a GPU or the library.

  quantize(weights)                  user weights (r, g, b) -> the three 15-bit integers, sum 32768
  weighted_gray(rgb_u8, q)           Y = (wr R + wg G + wb B + 2^14) >> 15 in unsigned 32-bit
  transfer_index(x)                  float32 values -> table entries, from the bit patterns alone
  table(kind, gamma, exposure)       the built-in tables in float64
  float_to_channels(x, table)        float channels -> u8 through a table (None: the `(x * 255).astype(uint8)` rule)
  gray(img, q, table)                the gray plane of a u8 RGB or float RGB(A) frame under a conversion
  srgb_eotf(c)                       sRGB-encoded [0, 1] -> linear, float64
"""
from __future__ import annotations

import numpy as np

import ingest_layouts as il

ENTRIES = 20481                       # PC_TRANSFER_ENTRIES: black + 20 octaves x 1024
DEFAULT_WEIGHTS = (9798, 19235, 3735)


def quantize(weights) -> tuple:
    w = np.asarray(weights, dtype=np.float64)
    assert w.shape == (3,) and np.isfinite(w).all() and (w >= 0).all() and w.sum() > 0, weights
    s = w[0] + w[1] + w[2]
    q = [int(np.floor((c / s) * 32768.0 + 0.5)) for c in w]
    q[int(np.argmax(w))] += 32768 - sum(q)       # argmax returns the first of equal maxima: ties in the order R, G, B
    return tuple(q)


def weighted_gray(rgb: np.ndarray, q) -> np.ndarray:
    assert rgb.dtype == np.uint8 and rgb.shape[-1] == 3
    assert all(0 <= int(v) <= 32768 for v in q) and sum(int(v) for v in q) == 32768, q
    c = rgb.astype(np.uint32)
    y = (c[..., 0] * np.uint32(q[0]) + c[..., 1] * np.uint32(q[1]) + c[..., 2] * np.uint32(q[2]) + np.uint32(1 << 14)) >> np.uint32(15)
    assert y.max(initial=0) <= 255
    return y.astype(np.uint8)


def transfer_index(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32).astype(np.int64)
    with np.errstate(invalid="ignore"):
        live = x >= np.float32(2.0 ** -16)       # false for NaN, negatives, zeros, denormals and tiny values
    idx = np.minimum((bits >> 13) - (111 << 10) + 1, ENTRIES - 1)
    return np.where(live, idx, 0).astype(np.int64)


def entry_midpoints(exposure: float = 0.0) -> np.ndarray:
    """y of the entries 1 .. ENTRIES - 1: the interval's midpoint times 2^exposure, float64"""
    i = np.arange(1, ENTRIES, dtype=np.int64)
    scale = np.ldexp(1.0, (-16 + (i - 1) // 1024).astype(np.int32))
    m = ((i - 1) % 1024).astype(np.float64)
    return (scale * (1.0 + m / 1024.0) + scale / 2048.0) * np.exp2(np.float64(exposure))


def curve(kind: str, y: np.ndarray, gamma: float = 2.2) -> np.ndarray:
    if kind == "srgb":
        return np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(y, 1.0 / 2.4) - 0.055)
    assert kind == "gamma", kind
    return np.power(y, 1.0 / np.float64(gamma))


def unrounded(kind: str, gamma: float = 2.2, exposure: float = 0.0) -> np.ndarray:
    """255 min(f(y), 1) + 0.5 of the entries 1 .. ENTRIES - 1: what floor() is applied to"""
    return 255.0 * np.minimum(curve(kind, entry_midpoints(exposure), gamma), 1.0) + 0.5


def table(kind: str, gamma: float = 2.2, exposure: float = 0.0) -> np.ndarray:
    out = np.zeros(ENTRIES, np.uint8)
    out[1:] = np.floor(unrounded(kind, gamma, exposure)).astype(np.uint8)
    return out


def float_to_channels(x: np.ndarray, tab) -> np.ndarray:
    if tab is None:
        return il.float_to_u8(x)
    tab = np.asarray(tab)
    assert tab.dtype == np.uint8 and tab.shape == (ENTRIES,)
    return tab[transfer_index(x)]


def gray(img: np.ndarray, q=DEFAULT_WEIGHTS, tab=None) -> np.ndarray:
    if img.dtype == np.float32:
        assert img.ndim == 3 and img.shape[2] in (3, 4), img.shape
        return weighted_gray(float_to_channels(np.ascontiguousarray(img[:, :, :3]), tab), q)    # alpha is dropped
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    return weighted_gray(img, q)


def srgb_eotf(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c, dtype=np.float64)
    return np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4))


def specials() -> np.ndarray:
    """float32 values at which a wrong index shows: NaN, +-inf, +-0, denormals, 2^-16 and 16 each +- 1 ulp, patterns whose low 13
    bits are 0 and 0x1FFF, a negative, values beyond the table's top"""
    f = np.float32
    lo, hi = f(2.0 ** -16), f(16.0)
    vals = [f(np.nan), f(np.inf), f(-np.inf), f(0.0), f(-0.0), f(1e-40), f(-1e-40), np.nextafter(f(0), f(1)),
            np.nextafter(lo, f(0)), lo, np.nextafter(lo, f(1)), np.nextafter(hi, f(0)), hi, np.nextafter(hi, f(32)),
            f(-0.25), f(1e10), f(3.4e38), f(0.18), f(1.0)]
    pats = np.array([0x3E000000, 0x3E001FFF, 0x3E002000, 0x3F7FFFFF, 0x3F7FE000, 0x3F7FDFFF, 0x37801FFF, 0x37802000,
                     0x417FFFFF, 0x7FC00001, 0xFFC00000, 0x7F800001], np.uint32).view(np.float32)
    return np.concatenate([np.array(vals, np.float32), pats])
