"""GPU: the gray conversion at the C ABI (pc_context_set_gray_conversion) -- channel weights and the float transfer table through
pc_frame_set_rgb / _rgb_f32 against the numpy rule (tests/gray_conversion_ref.py) fed to the CPU oracle.  Everything is bit-exact;
nothing is a tolerance.

  * tests/_gray_conversion_check.py has the case list and what a case compares (gray; per level the padded u8 plane, the derivative
    plane and the uint16 plane).  The cases run here on the fused level kernel (at 23 x 19 under a 25-px window on the unfused
    level-0 kernels) and once more in ONE child process under POLYCHASE_PYRAMID_VARIANT=1 on the unfused kernels;
  * one PC_FRAME_PINNED_HOST case; (1, 0, 0) is the R channel; the default set explicitly is a context that never called the
    setter, in bytes and in launches per timing class; a refused setter changes nothing; NULL restores the default; gray sources
    are untouched."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _gray_conversion_check as gc
import _ingest_check as check
import gray_conversion_ref as ref
import ingest_layouts as il
from polychase_amd import hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


# ---- plane parity, fused kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.cases(), ids=gc.case_name)
def test_planes_under_a_conversion_match_the_oracle(ctx, case):
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT", "0") == "0", "this process must run the fused level kernel"
    assert gc.run_case(ctx, case) == ""
    assert ctx.gray_conversion() == (ref.DEFAULT_WEIGHTS, None)


def test_the_case_list_covers_what_it_claims():
    assert {(w, h, win) for w, h, win in gc.SIZES} == {(63, 15, 10), (64, 16, 10), (65, 17, 10), (67, 35, 10), (131, 34, 10), (23, 19, 25)}
    conv = gc.conversions()
    assert [conv[n][0] for n in ("r", "b", "mix")] == [(32768, 0, 0), (0, 0, 32768), ref.quantize((0.2, 0.3, 0.5))]
    assert conv["srgb"][0] == ref.DEFAULT_WEIGHTS and np.array_equal(conv["srgb"][1], ref.table("srgb"))
    q, tab = conv["random_table_mix"]
    assert q != ref.DEFAULT_WEIGHTS and len(set(tab.tolist())) == 256 and (np.diff(tab.astype(int)) != 0).mean() > 0.9
    sp = set(ref.specials().view(np.uint32).tolist())
    for w, h, win in gc.SIZES:
        lay = gc.layouts_of("rgb", w)
        assert any(o % 4 and p % 4 for o, p in lay) and any(o % 4 == 0 and p % 4 == 0 for o, p in lay)
        for kind in ("f32x3", "f32x4"):
            for which in (0, 1):
                img = gc.image(kind, w, h, which)
                assert sp <= set(img[:, :, :3].view(np.uint32).ravel().tolist())
                assert kind == "f32x3" or np.isnan(img[:, :, 3]).all()
                idx = ref.transfer_index(np.ascontiguousarray(img[:, :, :3]))
                assert idx.min() == 0 and idx.max() == ref.ENTRIES - 1 and len(np.unique(idx >> 10)) >= 20
        for name in conv:        # the two images of a size differ, and a conversion differs from the default's planes
            a, b = gc.expected("f32x3", w, h, win, 0, name), gc.expected("f32x3", w, h, win, 1, name)
            assert not np.array_equal(a.gray, b.gray)
            assert not np.array_equal(a.gray, il.gray_of(gc.image("f32x3", w, h, 0)))
        for name in ("r", "b", "mix"):
            assert not np.array_equal(gc.expected("rgb", w, h, win, 0, name).gray, il.gray_of(gc.image("rgb", w, h, 0)))


# ---- the same cases on the unfused kernels --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unfused_lines():
    env = dict(os.environ)
    env["POLYCHASE_PYRAMID_VARIANT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_gray_conversion_check.py")], env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, f"the helper failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", gc.case_names())
def test_unfused_kernels_match_the_oracle(unfused_lines, name):
    mine = [l for l in unfused_lines if l.split()[1:2] == [name]]
    assert mine == [f"PASS {name}"], mine


# ---- one transfer by the copy engine --------------------------------------------------------------------------------
def test_a_pinned_host_frame_fetched_by_the_copy_engine(ctx):
    assert gc.run_case(ctx, ((67, 35, 10), "random_table_mix"), placements=("pinned_dma",)) == ""


# ---- the other promises of the header -------------------------------------------------------------------------------
W, H, WIN = 67, 35, 10


def _put(ctx, frame, kind, which=0):
    img = gc.image(kind, W, H, which)
    keep, rc = check.put(ctx, frame, kind, img, 0, check.row_bytes_of(kind, W), "pageable", seed=5)
    assert rc == 0, hip.load().pc_last_error().decode()
    keep.release()
    return img


def test_unit_red_weight_gives_the_red_channel(ctx):
    frame = hip.Frame(ctx, W, H, WIN, gc.MAX_LEVEL)
    ctx.set_gray_conversion((32768, 0, 0))
    try:
        rgb = _put(ctx, frame, "rgb")
        assert np.array_equal(frame.gray(), rgb[:, :, 0])
        f = _put(ctx, frame, "f32x4")
        assert np.array_equal(frame.gray(), il.float_to_u8(f[:, :, 0]))
    finally:
        ctx.set_gray_conversion()
        frame.close()


@pytest.mark.parametrize("size", [(131, 34, 10), (23, 19, 25)], ids=["fused", "unfused_level0"])
def test_index_revealing_tables_show_the_index_of_every_channel_value(ctx, size):
    """a table that holds the low byte of its own index, then one that holds the high byte, under a unit weight per channel: the
    two gray planes together ARE the kernel's index of every value of that channel, specials included"""
    w, h, win = size
    entries = np.arange(ref.ENTRIES)
    img = gc.image("f32x4", w, h, 0)
    want = ref.transfer_index(np.ascontiguousarray(img[:, :, :3]))
    assert want.min() == 0 and want.max() == ref.ENTRIES - 1 and len(np.unique(want)) >= 500      # (the small image holds 1311 values)
    frame = hip.Frame(ctx, w, h, win, gc.MAX_LEVEL)
    try:
        for c in range(3):
            unit = tuple(32768 if k == c else 0 for k in range(3))
            planes = []
            for tab in ((entries & 0xff).astype(np.uint8), (entries >> 8).astype(np.uint8)):
                ctx.set_gray_conversion(unit, tab)
                keep, rc = check.put(ctx, frame, "f32x4", img, 0, check.row_bytes_of("f32x4", w), "device", seed=7)
                assert rc == 0, hip.load().pc_last_error().decode()
                planes.append(frame.gray().astype(np.int64))
                keep.release()
            got = planes[0] | (planes[1] << 8)
            assert np.array_equal(got, want[:, :, c]), (c, np.argwhere(got != want[:, :, c])[:4])
    finally:
        ctx.set_gray_conversion()
        frame.close()


def test_the_default_set_explicitly_is_a_context_that_never_called_the_setter():
    planes, counts = [], []
    for explicit in (False, True):
        c = hip.Context(0)
        if explicit:
            conv = hip.GrayConversion()
            hip.load().pc_gray_default_conversion(ctypes.byref(conv))
            assert hip.load().pc_context_set_gray_conversion(c._h, ctypes.byref(conv)) == 0
            c.set_gray_conversion(ref.DEFAULT_WEIGHTS, None)
        c.enable_timing(True)
        c.reset_timing()
        got = []
        for kind, size in (("rgb", (W, H, WIN)), ("f32x3", (W, H, WIN)), ("f32x4", (W, H, WIN)), ("gray", (W, H, WIN)), ("rgb", (23, 19, 25)),
                           ("f32x4", (23, 19, 25))):
            w, h, win = size
            frame = hip.Frame(c, w, h, win, gc.MAX_LEVEL)
            keep, rc = check.put(c, frame, kind, check.image(kind, w, h, 0), 0, check.row_bytes_of(kind, w), "pageable", seed=5)
            assert rc == 0
            assert check.planes_mismatch(frame, check.expected(kind, w, h, win, 0)) == ""
            got.append([frame.gray()] + [p for l in range(frame.num_levels) for p in (frame.level(l), frame.deriv(l), frame.level16(l))])
            keep.release()
            frame.close()
        planes.append(got)
        counts.append({k: v[0] for k, v in c.timing().items()})
        c.close()
    print(counts)
    assert counts[0] == counts[1] and counts[0]["pyramid"] > 0 and counts[0]["gray"] > 0
    for a, b in zip(planes[0], planes[1]):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_refused_setter_changes_nothing_and_null_restores_the_default(ctx):
    L = hip.load()
    q, tab = gc.conversions()["random_table_mix"]
    frame = hip.Frame(ctx, W, H, WIN, gc.MAX_LEVEL)
    try:
        ctx.set_gray_conversion(q, tab)
        got_q, got_tab = ctx.gray_conversion()
        assert got_q == q and np.array_equal(got_tab, tab)
        for bad in ((32768, 1, 0), (-1, 32768, 1), (9798, 19235, 3736), (40000, 0, -7232)):
            conv = hip.GrayConversion(bad[0], bad[1], bad[2], None)
            assert L.pc_context_set_gray_conversion(ctx._h, ctypes.byref(conv)) == check.PC_E_INVALID, bad
            with pytest.raises(hip.PolychaseHipError, match="weight"):
                ctx.set_gray_conversion(bad, ref.table("srgb"))
        got_q, got_tab = ctx.gray_conversion()
        assert got_q == q and np.array_equal(got_tab, tab)
        for kind in ("rgb", "f32x4"):
            _put(ctx, frame, kind)
            assert check.planes_mismatch(frame, gc.expected(kind, W, H, WIN, 0, "random_table_mix")) == "", kind
        # gray sources are untouched by a conversion
        keep, rc = check.put(ctx, frame, "gray", check.image("gray", W, H, 1), 0, W, "pageable", seed=6)
        assert rc == 0 and check.planes_mismatch(frame, check.expected("gray", W, H, WIN, 1)) == ""
        keep.release()
        # the table without the weights, then the weights without the table
        ctx.set_gray_conversion(None, tab)
        assert ctx.gray_conversion()[0] == ref.DEFAULT_WEIGHTS
        img = _put(ctx, frame, "f32x3")
        assert np.array_equal(frame.gray(), ref.gray(img, ref.DEFAULT_WEIGHTS, tab))
        rgb = _put(ctx, frame, "rgb")
        assert np.array_equal(frame.gray(), il.gray_of(rgb)), "a float table does nothing for u8 frames"
        ctx.set_gray_conversion(q, None)
        assert ctx.gray_conversion() == (q, None)
        img = _put(ctx, frame, "f32x3")
        assert np.array_equal(frame.gray(), ref.gray(img, q, None))
        ctx.set_gray_conversion(q, tab)
        assert L.pc_context_set_gray_conversion(ctx._h, None) == 0
        assert ctx.gray_conversion() == (ref.DEFAULT_WEIGHTS, None)
        for kind in ("rgb", "f32x4"):
            img = _put(ctx, frame, kind, 1)
            assert np.array_equal(frame.gray(), il.gray_of(img)), kind
    finally:
        ctx.set_gray_conversion()
        frame.close()
