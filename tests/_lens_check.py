#!/usr/bin/env python3
"""Case list and runner of tests/test_lens_gpu.py: frames put under a lens map (pc_context_set_lens_map) against the numpy rule
(tests/lens_ref.py) fed to the CPU oracle, bit for bit: the gray plane and, for every level, the padded u8 plane, the derivative
plane and the uint16 plane, i.e. oracle.Pyramid(lens_ref.remap(gray_of(source), q)) through _ingest_check.planes_mismatch.

The test file runs the cases in its own process (gray kernel -> remap -> fused level kernel; at 23 x 19 under a 25-px window the
unfused chain) and, through main() below, once more in ONE child process under POLYCHASE_PYRAMID_VARIANT=1 -- a switch the library
reads once per process.  One line per case: "PASS <name>" or "FAIL <name> <what differs first>".

A case is one (size, map) and walks every source on one context: u8 RGB aligned and at an odd offset and pitch, float32 x 3 and
x 4, gray; three more at one size each put a page-locked frame through the copy engine and a frame under channel weights and
under the sRGB table, so that the conversion is seen to come before the blend."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _ingest_check as check  # noqa: E402
import gray_conversion_ref as gref  # noqa: E402
import ingest_layouts as il  # noqa: E402
import lens_ref as ref  # noqa: E402
from polychase_amd import hip  # noqa: E402

MAX_LEVEL = 3
# a four-pixel store group that is short, exact, one over, an odd multi-tile width; (23, 19, 25): level 0 on the unfused chain
SIZES = [(63, 15, 10), (64, 16, 10), (65, 17, 10), (131, 34, 10), (23, 19, 25)]
MAPS = ("identity", "random", "pincushion", "invalid", "clamped")
# (name, pixel type, placement, offset, pitch beyond the row)
SOURCES = [("rgb_aligned", "rgb", "device", 0, None), ("rgb_odd", "rgb", "device", 1, 7), ("f32x3", "f32x3", "device", 0, 0),
           ("f32x4", "f32x4", "device", 4, 20), ("gray", "gray", "pageable", 3, 5)]
WEIGHTS = (3277, 0, 29491)          # mostly blue: far from the default's gray
EXTRA = [("pinned", (65, 17, 10), "pincushion"), ("weights", (131, 34, 10), "random"), ("srgb", (63, 15, 10), "pincushion")]


@functools.lru_cache(maxsize=None)
def lens_map(name, w, h):
    rng = np.random.default_rng([w, h, MAPS.index(name)])
    if name == "identity":
        q = ref.identity_map(w, h)
    elif name == "pincushion":
        q = ref.build_map(ref.pincushion(w, h), w, h)
    else:
        # uniformly random positions from 3 px outside the frame to 2 px beyond its far edge
        q = np.empty((h, w, 2), np.int32)
        q[..., 0] = rng.integers(-3 * 256, (w + 2) * 256 + 1, (h, w))
        q[..., 1] = rng.integers(-3 * 256, (h + 2) * 256 + 1, (h, w))
        # every value of wx and of wy occurs
        flat = q.reshape(-1, 2)
        ax, ay = rng.permutation(len(flat))[:256], rng.permutation(len(flat))[:256]
        flat[ax, 0] = (flat[ax, 0] & ~255) | np.arange(256)
        flat[ay, 1] = (flat[ay, 1] & ~255) | np.arange(256)
        if name == "invalid":
            q[h // 3: h // 3 + 5, 2: min(w, 2 + 9)] = ref.INVALID           # a block ...
            for k in rng.permutation(w * h)[:12]:                              # ... and scattered single entries
                q[k // w, k % w] = ref.INVALID
            q[0, w - 1] = ref.INVALID
            q[h - 1, 0, 0] = ref.INVALID                                       # one component alone invalidates the entry
            q[h - 1, 1, 1] = ref.INVALID
        if name == "clamped":
            for k, (sx, sy) in enumerate([(1, 1), (1, -1), (-1, 1), (-1, -1), (1, 0), (0, -1)]):
                y, x = (k * 5) % h, (k * 11 + 3) % w
                q[y, x] = (sx * ref.CLAMP if sx else q[y, x, 0], sy * ref.CLAMP if sy else q[y, x, 1])
    q = np.ascontiguousarray(q)
    q.setflags(write=False)
    return q


def cases():
    return [(size, name) for size in SIZES for name in MAPS]


def case_name(case):
    (w, h, win), name = case
    return "%s-%dx%d_w%d" % (name, w, h, win)


def extra_name(extra):
    what, (w, h, win), name = extra
    return "%s-%s-%dx%d_w%d" % (what, name, w, h, win)


def case_names():
    return [case_name(c) for c in cases()] + [extra_name(e) for e in EXTRA]


@functools.lru_cache(maxsize=None)
def expected(kind, w, h, win, which, name, conv=None):
    """conv: None = the default gray conversion, "weights", "srgb" """
    img = check.image(kind, w, h, which)
    if conv == "weights":
        gray = gref.gray(img, WEIGHTS, None)
    elif conv == "srgb":
        gray = gref.gray(img, gref.DEFAULT_WEIGHTS, gref.table("srgb"))
    else:
        gray = il.gray_of(img)
    return il.expected(ref.remap(gray, lens_map(name, w, h)), win, MAX_LEVEL)


def _put_and_compare(ctx, frame, kind, where, offset, pitch, which, seed, e):
    img = check.image(kind, frame.w, frame.h, which)
    keep, rc = check.put(ctx, frame, kind, img, offset, pitch, where, seed)
    try:
        return ("set call returned %d: %s" % (rc, hip.load().pc_last_error().decode())) if rc else check.planes_mismatch(frame, e)
    finally:
        if rc:
            ctx.synchronize()
        keep.release()


def _pitch(kind, w, beyond):
    rb = check.row_bytes_of(kind, w)
    return rb + (-rb) % 4 if beyond is None else rb + beyond


def run_case(ctx, case):
    (w, h, win), name = case
    ctx.set_lens_map(lens_map(name, w, h))
    try:
        assert ctx.lens_map_size() == (w, h)
        for k, (src, kind, where, offset, beyond) in enumerate(SOURCES):
            frame = hip.Frame(ctx, w, h, win, MAX_LEVEL)
            try:
                for which in (0, 1):          # twice on one handle: nothing of the first image may stay
                    why = _put_and_compare(ctx, frame, kind, where, offset, _pitch(kind, w, beyond), which, 3000 + k,
                                           expected(kind, w, h, win, which, name))
                    if why:
                        return "%s image %d: %s" % (src, which, why)
            finally:
                frame.close()
    finally:
        ctx.set_lens_map(None)
    return ""


def run_extra(ctx, extra):
    what, (w, h, win), name = extra
    ctx.set_lens_map(lens_map(name, w, h))
    if what == "weights":
        ctx.set_gray_conversion(WEIGHTS, None)
    if what == "srgb":
        ctx.set_gray_conversion(None, gref.table("srgb"))
    try:
        kind = {"pinned": "rgb", "weights": "rgb", "srgb": "f32x4"}[what]
        conv = None if what == "pinned" else what
        e = expected(kind, w, h, win, 0, name, conv)
        if conv and np.array_equal(e.gray, expected(kind, w, h, win, 0, name).gray):
            return "the conversion does not show in the expected planes"
        frame = hip.Frame(ctx, w, h, win, MAX_LEVEL)
        try:
            return _put_and_compare(ctx, frame, kind, "pinned_dma" if what == "pinned" else "device", 0, _pitch(kind, w, None if kind == "rgb" else 0),
                                    0, 3100, e)
        finally:
            frame.close()
    finally:
        ctx.set_gray_conversion()
        ctx.set_lens_map(None)


def run_all(ctx, report):
    for case in cases():
        report(case_name(case), run_case(ctx, case))
    for extra in EXTRA:
        report(extra_name(extra), run_extra(ctx, extra))


def main():
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT") == "1", "this helper is about the kernels behind POLYCHASE_PYRAMID_VARIANT=1"
    ctx = hip.Context(0)
    run_all(ctx, lambda name, why: print(("FAIL %s %s" % (name, why)) if why else ("PASS %s" % name), flush=True))
    ctx.close()


if __name__ == "__main__":
    main()
