"""Source layouts of a frame as the C ABI accepts them (pc_frame_set_rgb / _gray / _rgb_f32: base pointer, row_pitch, placement,
pixel type), and what the frame's planes must then hold.  TEST INFRASTRUCTURE ONLY; nothing here needs a GPU except the three
GPU-read placements of lay_out.

  lay_out(img, offset, pitch, where)   the image in a buffer of exactly offset + pitch * (h - 1) + row_bytes bytes whose every
                                       other byte is seeded noise ("poison"): a kernel that reads the pitch gap or the bytes in
                                       front of the base computes something else
  float_to_u8(x)                       the documented float -> u8 rule of pc_frame_set_rgb_f32, in explicit integers
  expected(img, win, max_level)        gray and, per level, the padded u8 plane, the derivative plane and the uint16 plane,
                                       all from the CPU oracle
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

import oracle

PINNED_HOST = 2   # PC_FRAME_PINNED_HOST of include/polychase_hip.h
PLACEMENTS = ("pageable", "device", "pinned_read", "pinned_dma")


def row_bytes(img: np.ndarray) -> int:
    return int(img.shape[1]) * (1 if img.ndim == 2 else int(img.shape[2])) * img.dtype.itemsize


def buffer_size(img: np.ndarray, offset: int, pitch: int) -> int:
    """rows 0 .. h-2 with their pitch, the last row without: the header promises callers need not provide a full last pitch"""
    return offset + pitch * (int(img.shape[0]) - 1) + row_bytes(img)


def fill(img: np.ndarray, offset: int, pitch: int, seed: int) -> np.ndarray:
    """the bytes of the buffer: seeded poison everywhere, the image's rows at offset + y * pitch"""
    assert img.dtype in (np.uint8, np.float32) and img.ndim in (2, 3), (img.dtype, img.shape)
    rb = row_bytes(img)
    assert offset >= 0 and pitch >= rb, (offset, pitch, rb)
    if img.dtype == np.float32:
        assert offset % 4 == 0 and pitch % 4 == 0, "float frames need a 4-byte aligned pointer and pitch"
    h = int(img.shape[0])
    buf = np.random.default_rng(seed).integers(0, 256, buffer_size(img, offset, pitch), dtype=np.uint8)
    rows = np.ascontiguousarray(img).view(np.uint8).reshape(h, rb)
    for y in range(h):
        buf[offset + y * pitch: offset + y * pitch + rb] = rows[y]
    return buf


def pixels_of(buf: np.ndarray, img_like: np.ndarray, offset: int, pitch: int) -> np.ndarray:
    """the strided view of the buffer that holds the pixels, shaped and typed like the image"""
    h, rb = int(img_like.shape[0]), row_bytes(img_like)
    rows = np.lib.stride_tricks.as_strided(buf[offset:], shape=(h, rb), strides=(pitch, 1), writeable=False)
    return np.ascontiguousarray(rows).view(img_like.dtype).reshape(img_like.shape)


class Layout:
    """Keeps the buffer of a lay_out() alive.  release() frees page-locked memory: call it only after a synchronising call on
    the frame (any download is one); for the other placements it just drops the reference."""

    def __init__(self, buffer, pinned_ptr=None):
        self.buffer, self._pinned = buffer, pinned_ptr

    def release(self):
        self.buffer = None
        if self._pinned:
            from polychase_amd import hip
            hip.load().pc_host_buffer_free(self._pinned)
            self._pinned = None


def lay_out(img: np.ndarray, offset: int, pitch: int, where: str, seed: int = 0):
    """-> (keepalive, address, pitch, on_device) for pc_frame_set_rgb / _gray / _rgb_f32"""
    assert where in PLACEMENTS, where
    host = fill(img, offset, pitch, seed)
    if where == "pageable":
        assert host.ctypes.data % 4 == 0
        return Layout(host), host.ctypes.data + offset, pitch, 0
    if where == "device":
        import torch
        t = torch.from_numpy(host).cuda()
        torch.cuda.current_stream(t.device).synchronize()   # the library reads it on a stream of its own
        assert t.is_contiguous() and t.numel() == len(host) and t.data_ptr() % 4 == 0
        return Layout(t), t.data_ptr() + offset, pitch, 1
    from polychase_amd import hip
    p = C.c_void_p()
    hip._check(hip.load().pc_host_buffer_alloc(len(host), C.byref(p)))
    assert p.value and p.value % 4 == 0
    view = np.frombuffer((C.c_uint8 * len(host)).from_address(p.value), dtype=np.uint8)
    view[:] = host
    return Layout(view, p), p.value + offset, pitch, (1 if where == "pinned_read" else PINNED_HOST)


def float_to_u8(x: np.ndarray) -> np.ndarray:
    """pc_frame_set_rgb_f32's conversion: s = x * float32(255); s in [-2^31, 2^31) truncates toward zero, everything else (NaN
    too) is -2^31; the low byte of that.  Integers only after the one float32 product: no C cast whose result out of range
    would be the host's business."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = x * np.float32(255)
    assert s.dtype == np.float32
    with np.errstate(invalid="ignore"):
        in_range = (s >= np.float32(-2.0 ** 31)) & (s < np.float32(2.0 ** 31))
    t = np.trunc(np.where(in_range, s, np.float32(0)).astype(np.float64)).astype(np.int64)
    i = np.where(in_range, t, np.int64(-2 ** 31))
    return (i & 0xff).astype(np.uint8)


def gray_of(img: np.ndarray) -> np.ndarray:
    if img.dtype == np.float32:
        assert img.ndim == 3 and img.shape[2] in (3, 4), img.shape
        return oracle.rgb2gray(float_to_u8(img[:, :, :3]))   # alpha is dropped, whatever it holds
    assert img.dtype == np.uint8
    return oracle.rgb2gray(img) if img.ndim == 3 else np.ascontiguousarray(img)


def expected(img: np.ndarray, win: int, max_level: int) -> SimpleNamespace:
    """gray, num_levels, sizes[l] = (w, h), level[l], deriv[l], level16[l] (the last three padded by win); read-only arrays"""
    gray = gray_of(img)
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
