#!/usr/bin/env python3
"""End-to-end rates of GenerateOpticalFlowDatabase through the polychase_core module (what the Blender
addon experiences), next to bench.py's HBM-resident number.  Not the headline metric.

  python tools/e2e_bench.py [--config c2|c3] [--frames 60] [--mask-fraction F [--mask-polygon] [--mask-outline N]
                             [--target-mask-margin R]] [--min-correlation V] [--normalize] [--affine]
                             [--search-radius N] [--mask-windows] [--pan PX] [--lens-k1 K]
  python tools/e2e_bench.py --mask-mesh [--config c2] [--frames 120]

--mask-mesh: what a mesh mask (polychase_core.MeshMask, DESIGN.md section 4 "Mesh render") costs and saves.  The benchmark's C5 mesh
(the two-triangle plane) under a pose per frame that covers a quarter of the frame.  "product": frames/s of
generate_optical_flow_database on device frames without a database -- no mask, the MeshMask, and the same planes as host byte
masks from a callable (what polychase_core takes from a caller) -- median of three alternating runs each, and keypoints / flow
rows per frame of a SQLite run with and without the mask.  "pipelined": the driver's loop over the C ABI
(polychase_amd.pipeline.ClipAnalyzer) with, per frame put, either the caller's equivalent DEVICE byte mask or pc_mesh_render on a
second context into a device plane followed by the same pc_analyzer_set_mask(on_device = 1) -- the difference is the render plus
its synchronisation, per step.  Written into profiles/mesh_render.json under "product_<config>".

--lens-k1 K: OpticalFlowOptions.lens = LensModel(fx = fy = width, centred principal point, k1 = K) of every run, and the same map on
the context of the per-class pass (the gray kernel and the remap are timed under class "gray").
Modes: frames as torch CUDA tensors / host numpy arrays (PCIe upload included), with and without the
SQLite insert.  --mask-fraction F: every run takes detection_mask = a centred rectangle of the frame's aspect covering F of
its area (1.0: an all-on mask, the masked kernels with nothing masked out); the SQLite modes then also report the mean number
of keypoints per frame.  --mask-polygon: the same rectangle as a 4-vertex PolygonMask with integer corners -- by the fill rule
(include/polychase_hip.h: pc_frame_set_mask_polygons) the identical mask, so the keypoint counts must match the byte-mask run --
rasterised on the GPU instead of uploaded.  --mask-outline N: instead of the rectangle an N-vertex ellipse of that area, as
polygons with --mask-polygon and otherwise as the plane the rasteriser gives for it.  "mask_fill_ms_per_call": wall-clock of
Frame.set_mask_polygons (vertex copy, rasteriser launch, wait), mean of 200 calls: an upper bound of the launch, which belongs
to no timed kernel class.  "gpu_ms_per_step": per-class GPU time, launches and keypoints of a step (pc_context_get_timing: HIP
events around every launch) from a pass of this tool's own context and analyzer over the same frames under the same mask --
the driver's context cannot be read from here, and events around every launch slow the step, so the rates above come from
untimed runs.  --target-mask-margin R (with --mask-fraction): OpticalFlowOptions.target_mask_margin of every run, and of the
per-class pass -- rows that end where the mask, choked by R pixels, is off are dropped (-1, the default: off); the SQLite modes
then also report the mean number of flow rows per frame.  --min-correlation V: OpticalFlowOptions.min_correlation of every run, and
of the per-class pass (class "lk_corr") -- rows whose reference and matched windows correlate below V are dropped (0, the default:
off); the SQLite modes then report the mean number of flow rows per frame too.  --normalize: OpticalFlowOptions.normalize of every
run, and of the per-class pass (the normalised launch is timed under class "lk").  --affine: OpticalFlowOptions.affine_refinement of
every run, and of the per-class pass (the refinement launch is timed under class "lk" too: two launches per step).  --search-radius N: OpticalFlowOptions.search_radius of
every run, and of the per-class pass (the search launch is timed under class "lk" as well).  --mask-windows (with --mask-fraction):
OpticalFlowOptions.mask_windows of every run, and of the per-class pass (the masked launch is timed under class "lk" too, the weight
planes of a frame under no class).  --pan PX: instead of the benchmark clip,
frame t is frame 0 rolled by t * PX pixels in x -- a pan the plain search loses on the long skips."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_class_ms(w, h, ml, frames, mask, steps=40, polygons=None, target_margin=-1, min_correlation=0.0, normalize=False, affine=False, search_radius=0,
                 mask_windows=False, lens_map=None):
    """one pipelined pass (polychase_amd.pipeline.ClipAnalyzer) with every kernel class timed: 20 untimed steps, then `steps`"""
    from polychase_amd import hip
    from polychase_amd.pipeline import ClipAnalyzer

    ctx = hip.Context(0)
    if lens_map is not None:
        ctx.set_lens_map(lens_map)
    an = ClipAnalyzer(ctx, w, h, 1, len(frames), lambda f: frames[f - 1], hip.gftt_options(), hip.flow_options(max_level=ml))
    if polygons is not None:
        an.an.set_mask_polygons(polygons)
    else:
        an.an.set_mask(mask)
    an.an.set_target_mask_margin(target_margin)
    an.an.set_min_correlation(min_correlation)
    an.an.set_normalize(normalize)
    an.an.set_affine_refinement(affine)
    an.an.set_search_radius(search_radius)
    an.an.set_mask_windows(mask_windows)
    steps = min(steps, len(frames) - 9 - 29)
    an.run(range(9, 29), None)
    ctx.synchronize()
    ctx.enable_timing(True)
    ctx.reset_timing()
    kps = []
    an.run(range(29, 29 + steps), lambda f1, k, det, flows: kps.append(len(k)), copy=False)
    t = ctx.timing()
    ctx.enable_timing(False)
    an.close()
    ctx.close()
    return {"steps": steps, "mean_keypoints_per_frame": sum(kps) / len(kps),
            "ms": {k: round(v[1] / steps, 4) for k, v in t.items()}, "launches": {k: v[0] for k, v in t.items()}}


def mask_mesh(a):
    import ctypes as C
    import statistics

    import numpy as np
    import torch
    from polychase_amd import hip, synth
    from polychase_amd.pipeline import ClipAnalyzer
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core as core

    w, h, ml = {"c2": (1920, 1080, 3), "c3": (3840, 2160, 4)}[a.config]
    n = a.frames
    clip = synth.NoiseClip(w, h, max(n, 30), device="cuda")
    dev = [clip.frame_torch(t) for t in range(n)]
    torch.cuda.synchronize()
    # the C5 plane (tests/c5_endtoend.py), 6 units in front of a camera that drifts a little: half the frame wide and high
    verts = np.array([[-2, -1.125, 0], [2, -1.125, 0], [2, 1.125, 0], [-2, 1.125, 0]], np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    f = 0.75 * w
    origin = lambda fid: np.array([0.004 * fid, -0.002 * fid, -6.0], np.float32)   # noqa: E731
    intr = core.CameraIntrinsics(fx=f, fy=f, cx=w / 2, cy=h / 2, aspect_ratio=1.0, width=w, height=h, convention=core.CameraConvention.OpenCV)

    def pose(fid):
        view = np.eye(4, dtype=np.float32)
        view[:3, 3] = -origin(fid)
        return core.SceneTransformations(np.eye(4, dtype=np.float32), view, intr)

    mesh = core.AcceleratedMesh(verts, tris)
    poses = {fid: pose(fid) for fid in range(1, n + 1)}
    host_planes = {}
    for fid in range(1, n + 1):
        ids, _ = core.render_mesh(mesh, poses[fid], w, h)
        host_planes[fid] = np.where(ids >= 0, 255, 0).astype(np.uint8)
    out = {"config": a.config, "frames": n, "mesh": "c5_plane", "mask_fraction": float(np.mean([p.mean() / 255.0 for p in host_planes.values()]))}
    fo = core.OpticalFlowOptions()
    fo.max_level = ml
    vi = core.VideoInfo(w, h, 1, n)
    variants = {"no_mask": lambda: None, "mesh_mask": lambda: core.MeshMask(mesh, poses), "host_byte_mask": lambda: (lambda fid: host_planes[fid])}

    def product(mask, db=""):
        t0 = time.perf_counter()
        st = core.generate_optical_flow_database(vi, lambda fid: dev[fid - 1], None, db, core.GFTTOptions(), fo, detection_mask=mask)
        dt = time.perf_counter() - t0
        return n / (dt - st.seconds_setup)

    for make in variants.values():   # warm-up: engine, planes, allocations
        core.generate_optical_flow_database(core.VideoInfo(w, h, 1, 12), lambda fid: dev[fid - 1], None, "", core.GFTTOptions(), fo, detection_mask=make())
    fps = {k: [] for k in variants}
    for _ in range(3):
        for k, make in variants.items():
            fps[k].append(product(make()))
    out["product"] = {k: {"fps_median": statistics.median(v), "fps_runs": [round(x, 1) for x in v]} for k, v in fps.items()}
    import sqlite3
    with tempfile.TemporaryDirectory() as td:
        for k in ("no_mask", "mesh_mask"):
            db = os.path.join(td, k + ".db")
            product(variants[k](), db)
            con = sqlite3.connect(db)
            out["product"][k]["mean_keypoints_per_frame"] = con.execute("select avg(rows) from keypoints").fetchone()[0]
            out["product"][k]["mean_flow_rows_per_frame"] = con.execute("select sum(rows) from optical_flow").fetchone()[0] / n
            con.close()
    core.release_cached_engine()

    # the driver's loop over the C ABI: a caller's device byte mask per frame against the render per frame
    L = hip.load()
    VP = C.c_void_p

    class RayCamera(C.Structure):
        _fields_ = [("dir_matrix", C.c_float * 9), ("origin", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                    ("cx", C.c_float), ("cy", C.c_float), ("unproject_sign", C.c_float)]

    L.pc_mesh_create.argtypes = [VP, VP, C.c_int, VP, C.c_int, C.POINTER(VP)]
    L.pc_mesh_destroy.argtypes = [VP]
    L.pc_mesh_render.argtypes = [VP, VP, C.POINTER(RayCamera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP, VP, VP]
    mesh_ctx = hip.Context(0)
    m = VP()
    assert L.pc_mesh_create(mesh_ctx._h, verts.ctypes.data_as(VP), 4, tris.ctypes.data_as(VP), 2, C.byref(m)) == 0

    def camera(fid):
        cam = RayCamera()
        cam.dir_matrix[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        cam.origin[:] = [float(v) for v in origin(fid)]
        cam.fx = cam.fy = f
        cam.cx, cam.cy, cam.unproject_sign = w / 2, h / 2, 1.0
        return cam

    planes = {fid: torch.empty((h, w), dtype=torch.uint8, device="cuda:0") for fid in range(1, n + 1)}   # one per frame: none is reused
    torch.cuda.synchronize()

    def render(fid):
        cam = camera(fid)
        assert L.pc_mesh_render(mesh_ctx._h, m, C.byref(cam), w, h, 1, 0, 0, 1, None, None, VP(planes[fid].data_ptr())) == 0, L.pc_last_error()

    for fid in planes:
        render(fid)
    assert all(np.array_equal(planes[fid].cpu().numpy(), host_planes[fid]) for fid in (1, n))
    render_s = [0.0]

    def loop(per_frame):
        ctx = hip.Context(0)
        state = {}

        def source(fid):
            per_frame(state["an"], fid)
            return dev[fid - 1]

        an = ClipAnalyzer(ctx, w, h, 1, n, source, hip.gftt_options(), hip.flow_options(max_level=ml))
        state["an"] = an.an
        an.run(range(1, 21), None, copy=False)
        ctx.synchronize()
        render_s[0] = 0.0
        t0 = time.perf_counter()
        an.run(range(21, n - 9), None, copy=False)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        an.close()
        ctx.close()
        return 1e3 * dt / (n - 9 - 21)

    def with_device_mask(an, fid):
        an.set_mask(planes[fid])

    def with_render(an, fid):
        t0 = time.perf_counter()
        render(fid)
        render_s[0] += time.perf_counter() - t0
        an.set_mask(planes[fid])

    ms = {"device_byte_mask": [], "render_per_frame": []}
    render_ms = []
    for _ in range(3):
        ms["device_byte_mask"].append(loop(with_device_mask))
        ms["render_per_frame"].append(loop(with_render))
        render_ms.append(1e3 * render_s[0] / (n - 9 - 21))
    a_ms, b_ms = statistics.median(ms["device_byte_mask"]), statistics.median(ms["render_per_frame"])
    out["pipelined"] = {"ms_per_step": {k: {"median": statistics.median(v), "runs": [round(x, 4) for x in v]} for k, v in ms.items()},
                        "render_call_ms_per_step": statistics.median(render_ms), "difference_ms": b_ms - a_ms,
                        "difference_share_of_step": (b_ms - a_ms) / a_ms}
    L.pc_mesh_destroy(m)
    mesh_ctx.close()
    prof = os.path.join(ROOT, "profiles", "mesh_render.json")
    doc = json.load(open(prof)) if os.path.exists(prof) else {}
    doc["product_" + a.config] = out
    json.dump(doc, open(prof, "w"), indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--mask-mesh", action="store_true")
    ap.add_argument("--mask-fraction", type=float, default=None)
    ap.add_argument("--mask-polygon", action="store_true")
    ap.add_argument("--mask-outline", type=int, default=0)
    ap.add_argument("--target-mask-margin", type=int, default=-1)
    ap.add_argument("--min-correlation", type=float, default=0.0)
    ap.add_argument("--normalize", action="store_true")
    ap.add_argument("--affine", action="store_true")
    ap.add_argument("--search-radius", type=int, default=0)
    ap.add_argument("--mask-windows", action="store_true")
    ap.add_argument("--pan", type=int, default=0)
    ap.add_argument("--lens-k1", type=float, default=None, metavar="K")
    a = ap.parse_args()
    if a.mask_mesh:
        return mask_mesh(a)
    import torch
    from polychase_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core as core

    w, h, ml = {"c2": (1920, 1080, 3), "c3": (3840, 2160, 4)}[a.config]
    clip = synth.NoiseClip(w, h, max(a.frames, 30), device="cuda")
    dev = [clip.frame_torch(t) for t in range(a.frames)]
    if a.pan:
        dev = [torch.roll(dev[0], t * a.pan, 1).contiguous() for t in range(a.frames)]
    torch.cuda.synchronize()
    host = [f.cpu().numpy() for f in dev]
    fo = core.OpticalFlowOptions()
    fo.max_level = ml
    fo.target_mask_margin = a.target_mask_margin
    fo.min_correlation = a.min_correlation
    fo.normalize = a.normalize
    fo.affine_refinement = a.affine
    fo.search_radius = a.search_radius
    fo.mask_windows = a.mask_windows
    lens_map = None
    if a.lens_k1 is not None:
        fo.lens = core.LensModel(float(w), float(w), (w - 1) / 2.0, (h - 1) / 2.0, k1=a.lens_k1)
        lens_map = fo.lens.build_map(w, h)
    if a.mask_windows and a.mask_fraction is None:
        ap.error("--mask-windows needs a mask (--mask-fraction, optionally --mask-polygon / --mask-outline)")
    vi = core.VideoInfo(w, h, 1, a.frames)
    out = {}
    mask = None
    if a.mask_fraction is not None:
        import numpy as np
        assert 0.0 < a.mask_fraction <= 1.0
        mw, mh = int(round(w * a.mask_fraction ** 0.5)), int(round(h * a.mask_fraction ** 0.5))
        from polychase_amd import hip
        x0, y0 = (w - mw) // 2, (h - mh) // 2
        polygons = [np.array([(x0, y0), (x0 + mw, y0), (x0 + mw, y0 + mh), (x0, y0 + mh)], np.float32)]
        if a.mask_outline:
            ang = 2 * np.pi * np.arange(a.mask_outline) / a.mask_outline
            r = (a.mask_fraction / np.pi) ** 0.5       # an ellipse of the frame's aspect: pi (r w)(r h) = F w h
            polygons = [np.stack([w / 2 + r * w * np.cos(ang), h / 2 + r * h * np.sin(ang)], axis=1).astype(np.float32)]
        ctx = hip.Context(0)
        fr = hip.Frame(ctx, w, h)
        fr.set_mask_polygons(polygons)
        mask = fr.mask()
        t0 = time.perf_counter()
        for _ in range(200):
            fr.set_mask_polygons(polygons)
        out["mask_fill_ms_per_call"] = 1e3 * (time.perf_counter() - t0) / 200
        fr.close()
        ctx.close()
        if not a.mask_outline:
            rect = np.zeros((h, w), np.uint8)
            rect[y0:y0 + mh, x0:x0 + mw] = 255
            assert np.array_equal(mask, rect), "the rasterised rectangle is the byte mask"
        out["mask_fraction"] = float(mask.mean() / 255.0)
        out["mask_vertices"] = int(len(polygons[0]))
        out["mask_polygon"] = bool(a.mask_polygon)
        out["target_mask_margin"] = a.target_mask_margin
        if a.mask_polygon:
            mask = core.PolygonMask(polygons)
    polygons = polygons if a.mask_polygon and a.mask_fraction is not None else None
    if a.min_correlation:
        out["min_correlation"] = a.min_correlation
    if a.normalize:
        out["normalize"] = True
    if a.affine:
        out["affine_refinement"] = True
    if a.search_radius:
        out["search_radius"] = a.search_radius
    if a.mask_windows:
        out["mask_windows"] = True
    if a.pan:
        out["pan_px_per_frame"] = a.pan
    if a.lens_k1 is not None:
        out["lens_k1"] = a.lens_k1
    if a.frames >= 39:
        out["gpu_ms_per_step"] = per_class_ms(w, h, ml, dev, mask, polygons=polygons,
                                              target_margin=a.target_mask_margin if a.mask_fraction is not None else -1,
                                              min_correlation=a.min_correlation, normalize=a.normalize, affine=a.affine,
                                              search_radius=a.search_radius, mask_windows=a.mask_windows, lens_map=lens_map)
    else:
        out["gpu_ms_per_step"] = {"skipped": "the per-class pass needs --frames 39 or more (20 untimed steps, then at least one)"}
    with tempfile.TemporaryDirectory() as td:
        for name, frames, db in [("device_frames_no_db", dev, ""), ("host_frames_no_db", host, ""),
                                 ("host_frames_sqlite", host, os.path.join(td, "a.db")),
                                 ("device_frames_sqlite", dev, os.path.join(td, "b.db"))]:
            core.generate_optical_flow_database(core.VideoInfo(w, h, 1, 12), lambda f: frames[f - 1], None, "", core.GFTTOptions(), fo, detection_mask=mask)
            c0 = core._async_write_counters()
            t0 = time.perf_counter()
            st = core.generate_optical_flow_database(vi, lambda f: frames[f - 1], None, db, core.GFTTOptions(), fo, detection_mask=mask)
            dt = time.perf_counter() - t0
            c1 = core._async_write_counters()
            out[name] = {"fps": a.frames / dt, "fps_without_setup": a.frames / (dt - st.seconds_setup), "seconds_db": st.seconds_db,
                         "db_bytes": os.path.getsize(db) if db else 0,
                         # the driver thread's stage clock, ms per frame
                         "driver_ms_per_frame": {k: round(1e3 * getattr(st, "seconds_" + k) / a.frames, 4)
                                                 for k in ("accessor", "put", "submit", "collect", "writer_wait")},
                         "setup_ms": round(1e3 * st.seconds_setup, 1),
                         # page writes of the database file: handed to the worker threads / carried out by SQLite's own thread
                         "db_page_writes": {k: c1[k] - c0[k] for k in c1}}
            if db:
                import sqlite3
                con = sqlite3.connect(db)
                out[name]["mean_keypoints_per_frame"] = con.execute("select avg(rows) from keypoints").fetchone()[0]
                out[name]["mean_flow_rows_per_frame"] = con.execute("select sum(rows) from optical_flow").fetchone()[0] / a.frames
                con.close()
    print(json.dumps({"config": a.config, "frames": a.frames, **out}))


if __name__ == "__main__":
    main()
