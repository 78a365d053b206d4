"""No GPU: the numpy restatement of the mesh render (tests/mesh_render_ref.py) on the scene whose planes are known in closed form,
the erosion and the polarity, and the share of pixels of the soup scenes that float32 cannot decide -- the condition under which
tests/test_mesh_render_gpu.py compares the GPU with float64."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_ref as mr  # noqa: E402

W, H = mr.EXACT_W, mr.EXACT_H


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_scene_is_the_rectangle(dtype):
    verts, tris, cam = mr.exact_scene()
    prim, depth, mask, r = mr.render(dtype, verts, tris, cam, W, H)
    assert np.array_equal(mask, mr.rect_plane(W, H, *mr.EXACT_RECT))
    assert (prim == 0).sum() == 300 and (prim == 1).sum() == 300 and (prim == -1).sum() == W * H - 600
    assert np.all(depth[mask == 255] == 4) and np.all(depth[mask == 0] == 0)
    # nothing sits near an outline or the diagonal: both precisions decide every pixel with room to spare
    assert r.m_bary.min() > 8e-3


def test_exact_scene_masked_triangle_is_a_miss_but_keeps_its_id():
    verts, tris, cam = mr.exact_scene()
    free = mr.render(np.float32, verts, tris, cam, W, H)
    prim, depth, mask, _ = mr.render(np.float32, verts, tris, cam, W, H, masked=[False, True], check_mask=True)
    assert np.array_equal(prim, free[0]) and np.array_equal(depth, free[1])
    assert np.array_equal(mask == 255, free[0] == 0)


def test_erosion_and_polarity_on_the_exact_scene():
    verts, tris, cam = mr.exact_scene()
    _, _, m3, _ = mr.render(np.float32, verts, tris, cam, W, H, margin=3)
    assert np.array_equal(m3, mr.rect_plane(W, H, 14, 37, 9, 22))
    _, _, i3, _ = mr.render(np.float32, verts, tris, cam, W, H, invert=True, margin=3)
    assert np.array_equal(i3, mr.rect_plane(W, H, 8, 43, 3, 28, inside=0, outside=255))
    # the frame border stays on: outside counts as on
    assert np.all(i3[0] == 255) and np.all(i3[-1] == 255) and np.all(i3[:, 0] == 255) and np.all(i3[:, -1] == 255)


def test_erode_rule():
    rng = np.random.default_rng(5)
    plane = (rng.uniform(size=(23, 37)) < 0.97).astype(np.uint8) * 7          # any non-zero byte is on
    assert np.array_equal(mr.erode(plane, 0), np.where(plane != 0, 255, 0))
    for margin in (1, 2, 5):
        want = np.empty(plane.shape, np.uint8)
        for y in range(plane.shape[0]):
            for x in range(plane.shape[1]):
                win = plane[max(0, y - margin):y + margin + 1, max(0, x - margin):x + margin + 1]
                want[y, x] = 255 if np.all(win != 0) else 0
        assert np.array_equal(mr.erode(plane, margin), want)
    full = np.full((9, 5), 255, np.uint8)
    assert np.all(mr.erode(full, mr.MAX_MARGIN) == 255)                        # a margin beyond the frame: still on
    # erosion never switches a pixel on, and a larger margin never keeps more
    assert np.all(mr.erode(plane, 3)[plane == 0] == 0) and np.all(mr.erode(plane, 5) <= mr.erode(plane, 3))


def test_an_uninverted_mask_only_keeps_pixels_that_hit():
    """the consequence the detection relies on: on => the pixel's own ray hits an unmasked triangle"""
    verts, tris = mr.soup_mesh()
    masked = np.arange(len(tris)) % 7 == 0
    w, h, _ = mr.SOUP_SCENES["67x45"]
    cam = mr.soup_camera("67x45")
    for margin in (0, 2):
        prim, _, mask, r = mr.render(np.float32, verts, tris, cam, w, h, masked=masked, check_mask=True, margin=margin)
        on = mask == 255
        assert on.any() or margin > 0
        assert np.all(prim[on] >= 0) and not masked[prim[on]].any()


@pytest.mark.parametrize("name", list(mr.SOUP_SCENES))
def test_soup_scenes_have_few_ambiguous_pixels(name):
    w, h, cam, prim, hit, amb = mr.soup_reference(name)
    print(f"{name}: {int(amb.sum())} of {amb.size} pixels ambiguous, {int(hit.sum())} hit, {len(np.unique(prim[hit]))} triangles seen")
    assert amb.mean() <= 0.005
    assert hit.mean() > 0.2 and len(np.unique(prim[hit])) > 30                 # the scene is not empty
