#!/usr/bin/env python3
"""The bodies of tests/test_resource_lifecycle_gpu.py, each run in a process of its own (`python _resource_lifecycle_cases.py
<case>`): there hip.live_resources() -- device allocations, pinned allocations, streams, events owned by objects of the library
-- is absolute: no handle of another test, no object Python has yet to collect.  A case prints ONE line of JSON with the counts
it took and the return codes it saw; the test asserts on that line.

Frames are 160 x 120 under a 10-px window with max_level 2, a few hundred keypoints set with pc_frame_set_keypoints; the mesh is
a cube of 12 triangles."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from polychase_amd import hip  # noqa: E402
from test_tracker_abi_gpu import (RayCamera, RefineCamera, RefineDesc, TrackSource, _block, _p, _refine_desc,  # noqa: E402
                                  _refine_problem)

VP = C.c_void_p
W, H, WIN, MAX_LEVEL = 160, 120, 10, 2
RECTANGLE = [np.array([(20, 15), (140, 15), (140, 105), (20, 105)], np.float32)]


def _images(n):
    """n views of one smooth random texture, each a few pixels further along x"""
    rng = np.random.default_rng(11)
    coarse = rng.integers(0, 256, ((H + 16) // 4, (W + 64) // 4, 3)).astype(np.float32)
    big = np.kron(coarse, np.ones((4, 4, 1), np.float32))
    big = (big + np.roll(big, 2, 0) + np.roll(big, 2, 1) + np.roll(big, (2, 2), (0, 1))) / 4
    return [np.ascontiguousarray(big[4:4 + H, 3 * k:3 * k + W].astype(np.uint8)) for k in range(n)]


def _keypoints(n, seed=5):
    return np.random.default_rng(seed).uniform([25, 20], [135, 100], (n, 2)).astype(np.float32)


def _frame(ctx, image, n_kps=300):
    f = hip.Frame(ctx, W, H, WIN, MAX_LEVEL)
    f.set_rgb(image)
    f.set_keypoints(_keypoints(n_kps))
    return f


def _cube():
    verts = np.array([[x, y, z] for z in (-4, 4) for y in (-4, 4) for x in (-4, 4)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    return verts, tris


def _ray_camera():
    """OpenCV convention, in front of the cube's face z = -4"""
    cam = RayCamera()
    cam.dir_matrix[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    cam.origin[:] = [0, 0, -9]
    cam.fx = cam.fy = 150.0
    cam.cx, cam.cy, cam.unproject_sign = W / 2, H / 2, 1.0
    return cam


def _tracker_abi():
    L = hip.load()
    L.pc_mesh_create.argtypes = [VP, VP, C.c_int, VP, C.c_int, C.POINTER(VP)]
    L.pc_raycast_pixels.argtypes = [VP, VP, C.POINTER(RayCamera), VP, C.c_int, C.c_int, VP, VP, VP, VP]
    L.pc_corr_set_create.argtypes = [VP, C.POINTER(VP)]
    L.pc_corr_set_reserve.argtypes = [VP, VP, C.c_int, C.c_int, C.c_int]
    L.pc_track_frame_upload.argtypes = [VP, VP, VP, C.c_size_t, C.POINTER(TrackSource), C.c_int]
    L.pc_corr_set_append.argtypes = [VP, VP, VP, C.POINTER(RayCamera), VP, C.c_longlong, VP, C.c_int, VP, VP, C.c_int, C.c_int]
    L.pc_pnp_problem_create.argtypes = [VP, VP, VP, VP, C.c_int, C.POINTER(VP)]
    L.pc_pnp_problem_from_set.argtypes = [VP, VP, C.POINTER(VP)]
    L.pc_refine_problem_create.argtypes = [VP, VP, C.POINTER(RefineDesc), C.POINTER(VP)]
    L.pc_refine_total_cost.argtypes = [VP, VP, C.POINTER(RefineCamera), C.c_int, C.c_float, C.POINTER(C.c_double)]
    for name in ("pc_mesh_destroy", "pc_corr_set_destroy", "pc_pnp_problem_destroy", "pc_refine_problem_destroy"):
        getattr(L, name).argtypes = [VP]
        getattr(L, name).restype = None
    return L


def _ok(rc):
    assert rc == 0, hip.load().pc_last_error()


def lifecycle():
    """everything the C ABI can own, alive at once, then destroyed in reverse order of creation"""
    L = _tracker_abi()
    images = _images(4)
    before = hip.live_resources()
    ctx = hip.Context(0)
    ctx.enable_timing(True)
    f0, f1 = _frame(ctx, images[0]), _frame(ctx, images[1])
    fm = _frame(ctx, images[2])
    fm.set_mask_polygons(RECTANGLE)
    fm.choked_mask(2)
    fm.window_weights(0)
    f0.detect(hip.gftt_options())
    f0.set_keypoints(_keypoints(300))
    opt = hip.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    hip.lk_track_search(ctx, f0, [f1, fm], 8, fb_threshold=1.0, opt=opt)
    hip.lk_track_window_masked(ctx, fm, [f0, f1], 1, fb_threshold=1.0, opt=opt)
    hip.lk_track_correlated(ctx, f0, [f1], 0.5, opt=opt, corr=True)
    hip.lk_track_filtered_fb(ctx, f0, [f1], 1.0, opt=opt)
    ctx.timing()

    an = hip.Analyzer(ctx, W, H, hip.gftt_options(), opt, ring_frames=3, max_jobs=2)
    an.set_mask(np.full((H, W), 255, np.uint8))
    an.put_frame(1, images[0])
    an.put_frame(2, images[1])
    an.set_mask_polygons(RECTANGLE)
    an.put_frame(3, images[2])
    an.put_frame(4, images[3])
    an.submit(3, [4])
    an.collect()

    verts, tris = _cube()
    mesh, cset, own, from_set, refine = VP(), VP(), VP(), VP(), VP()
    _ok(L.pc_mesh_create(ctx._h, _p(verts), len(verts), _p(tris), len(tris), C.byref(mesh)))
    cam = _ray_camera()
    kps = _keypoints(200)
    hit, pos = np.zeros(len(kps), np.uint8), np.zeros((len(kps), 3), np.float32)
    prim, uvt = np.zeros(len(kps), np.uint32), np.zeros((len(kps), 3), np.float32)
    _ok(L.pc_raycast_pixels(ctx._h, mesh, C.byref(cam), _p(kps), len(kps), 0, _p(hit), _p(pos), _p(prim), _p(uvt)))
    assert hit.all()
    _ok(L.pc_corr_set_create(ctx._h, C.byref(cset)))
    _ok(L.pc_corr_set_reserve(ctx._h, cset, len(kps), len(kps), 1))
    idx = np.arange(len(kps), dtype=np.uint32)
    blob, offs = _block([(idx, kps)])
    src = (TrackSource * 1)()
    src[0].cam, src[0].keypoints_key, src[0].keypoints_xy, src[0].n_keypoints, src[0].n_matches = cam, 7, _p(kps), len(kps), len(idx)
    src[0].idx_offset, src[0].tgt_offset = offs[0]
    _ok(L.pc_track_frame_upload(ctx._h, cset, _p(blob), blob.nbytes, src, 1))
    X = np.ascontiguousarray(pos)
    _ok(L.pc_pnp_problem_create(ctx._h, _p(X), _p(kps), None, len(kps), C.byref(own)))
    model = np.eye(4, dtype=np.float32)
    _ok(L.pc_corr_set_append(ctx._h, cset, mesh, C.byref(cam), _p(model), 7, _p(kps), len(kps), _p(idx), _p(kps), len(idx), 0))
    _ok(L.pc_pnp_problem_from_set(ctx._h, cset, C.byref(from_set)))
    arrays, cams = _refine_problem(np.random.default_rng(3), n_frames=3, n_kp=40)
    desc = _refine_desc(arrays, True)
    _ok(L.pc_refine_problem_create(ctx._h, mesh, C.byref(desc), C.byref(refine)))
    cost = C.c_double()
    _ok(L.pc_refine_total_cost(ctx._h, refine, cams, 2, 1.0, C.byref(cost)))
    alive = hip.live_resources()

    L.pc_refine_problem_destroy(refine)
    L.pc_pnp_problem_destroy(from_set)
    L.pc_pnp_problem_destroy(own)
    L.pc_corr_set_destroy(cset)
    L.pc_mesh_destroy(mesh)
    an.close()
    for f in (fm, f1, f0):
        f.close()
    ctx.close()
    return {"before": before, "alive": alive, "after": hip.live_resources()}


def growth():
    """a scratch buffer that grows is replaced: more keypoints, the same number of allocations"""
    images = _images(2)
    ctx = hip.Context(0)
    f0, f1 = _frame(ctx, images[0], 100), _frame(ctx, images[1], 100)
    opt = hip.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    device = []
    for n in (100, 5000, 100):
        f0.set_keypoints(_keypoints(n, seed=n))
        hip.lk_track(ctx, f0, [f1], opt)
        device.append(hip.live_resources()[0])
    frame = []
    for n in (100, 50000):
        f1.set_keypoints(_keypoints(n, seed=n))
        frame.append(hip.live_resources()[0])
    f1.close()
    f0.close()
    ctx.close()
    return {"lk_track": device, "set_keypoints": frame, "after": hip.live_resources()}


def bad_arith():
    """POLYCHASE_ARITH=bogus in this process's environment: pc_context_create refuses and keeps no stream it had made"""
    h = VP()
    rc = hip.load().pc_context_create(0, C.byref(h))
    return {"rc": rc, "handle": bool(h.value), "message": hip.load().pc_last_error().decode(), "after": hip.live_resources()}


def refusals():
    """creators that refuse their arguments return today's code and hold nothing afterwards: [name, rc, counts before, after]"""
    L = _tracker_abi()
    ctx = hip.Context(0)
    verts, tris = _cube()
    mesh, cset = VP(), VP()
    _ok(L.pc_mesh_create(ctx._h, _p(verts), len(verts), _p(tris), len(tris), C.byref(mesh)))
    _ok(L.pc_corr_set_create(ctx._h, C.byref(cset)))
    gftt, flow = hip.gftt_options(), hip.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    bad_tris = tris.copy()
    bad_tris[5, 1] = len(verts)
    arrays, _cams = _refine_problem(np.random.default_rng(3), n_frames=3, n_kp=40)
    arrays["res_src_kp"] = arrays["res_src_kp"].copy()
    arrays["res_src_kp"][arrays["edge_offset"][1] + 5] = 40          # the frames have keypoints 0 .. 39
    desc = _refine_desc(arrays, True)
    out = VP()
    calls = {
        "frame window 2": lambda: L.pc_frame_create(ctx._h, W, H, 2, MAX_LEVEL, C.byref(out)),
        "analyzer ring 0": lambda: L.pc_analyzer_create(ctx._h, W, H, C.byref(gftt), C.byref(flow), 0, 2, C.byref(out)),
        "mesh index": lambda: L.pc_mesh_create(ctx._h, _p(verts), len(verts), _p(bad_tris), len(bad_tris), C.byref(out)),
        "refine keypoint": lambda: L.pc_refine_problem_create(ctx._h, mesh, C.byref(desc), C.byref(out)),
        "pnp from empty set": lambda: L.pc_pnp_problem_from_set(ctx._h, cset, C.byref(out)),
    }
    rows = []
    for name, call in calls.items():
        before = hip.live_resources()
        rc = call()
        rows.append([name, rc, bool(out.value), L.pc_last_error().decode(), before, hip.live_resources()])
    L.pc_corr_set_destroy(cset)
    L.pc_mesh_destroy(mesh)
    ctx.close()
    return {"rows": rows, "after": hip.live_resources()}


if __name__ == "__main__":
    print(json.dumps({"lifecycle": lifecycle, "growth": growth, "bad_arith": bad_arith, "refusals": refusals}[sys.argv[1]]()))
