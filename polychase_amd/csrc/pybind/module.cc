// module.cc -- the `polychase_core` extension module with the reference's Python surface
// (cpp/polychase_pybind.cc:29-348), backed by the MI355X path.  Blender's addon imports it with
// `from polychase_core import *` (blender_addon/core.py:16-22) and is meant to run unchanged.
#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cmath>
#include <deque>
#include <map>

#include "../../../include/polychase_hip.h"
#include "../host/debug_images.h"
#include "../host/async_write_vfs.h"
#include "../host/flow_database.h"
#include "../host/analysis.h"
#include "../host/frame_pool.h"
#include "../host/pixel_convert.h"
#include "../host/analysis_thread.h"
#include "../host/multi_gpu.h"
#include "../host/stage_clock.h"
#include <chrono>
#include <thread>

#include "../host/numa_pin.h"
#include "../host/track_sequence.h"
#include "../host/gpu_context.h"
#include "../host/ray_casting.h"
#include "np_helpers.h"

#ifdef PC_WITH_TRACKER
void BindTracker(py::module_& m);  // tracker_bindings.cc
#endif

namespace {

using U8Array = py::array_t<uint8_t, py::array::c_style>;

constexpr const char* kAcceptedFrames = "uint8 (H, W, 3|4), uint16 (H, W, 3|4), float16 (H, W, 3|4) or float32 (H, W, 3|4)";

// dtype of a numpy frame -> pc_pixel_type, -1 for a dtype the library does not take (kind and size: 'e' is a kind 'f' of 2 bytes)
int PixelTypeOfDtype(const py::dtype& dt) {
    const char kind = dt.kind();
    const py::ssize_t size = dt.itemsize();
    if (kind == 'u' && size == 1) return PC_PIXEL_U8;
    if (kind == 'u' && size == 2) return PC_PIXEL_U16;
    if (kind == 'f' && size == 2) return PC_PIXEL_F16;
    if (kind == 'f' && size == 4) return PC_PIXEL_F32;
    return -1;
}

// a numpy frame of an accepted type, C-contiguous (copied if it is not) -> its pixel type; ValueError for anything else
py::array AcceptedFrameArray(const py::object& obj, int* pixel_type) {
    py::array arr = py::array::ensure(obj);
    if (!arr) throw py::value_error(std::string("frame must be ") + kAcceptedFrames);
    if (arr.dtype().kind() == 'b') arr = py::array_t<uint8_t>::ensure(arr);   // a bool array has always passed as bytes
    *pixel_type = PixelTypeOfDtype(arr.dtype());
    if (*pixel_type < 0 || arr.ndim() != 3 || (arr.shape(2) != 3 && arr.shape(2) != 4))
        throw py::value_error(std::string("frame must be ") + kAcceptedFrames + ", got " + py::str(arr.dtype()).cast<std::string>() + " " +
                              py::str(py::tuple(arr.attr("shape"))).cast<std::string>());
    if (!(arr.flags() & py::array::c_style) || !arr.dtype().attr("isnative").cast<bool>())
        arr = py::module_::import("numpy").attr("ascontiguousarray")(arr, arr.dtype().attr("newbyteorder")("="));
    return arr;
}

// Python frame (numpy, or a torch CUDA tensor; the types of kAcceptedFrames) -> FrameView.
// Host arrays are deep-copied under the GIL; device tensors are referenced (the caller keeps the
// py::object alive, see GenerateOpticalFlowDatabasePy).
std::optional<FrameView> FrameFromPython(const py::object& obj, std::deque<py::object>& keep_alive) {
    if (obj.is_none()) return std::nullopt;
    if (py::hasattr(obj, "is_cuda") && obj.attr("is_cuda").cast<bool>()) {
        py::object t = obj;
        if (!t.attr("is_contiguous")().cast<bool>()) t = t.attr("contiguous")();
        // the analysis runs on its own HIP stream: wait for whatever produced the tensor
        py::module_::import("torch").attr("cuda").attr("current_stream")(t.attr("device")).attr("synchronize")();
        const auto shape = t.attr("shape").cast<std::vector<py::ssize_t>>();
        if (shape.size() != 3) throw py::value_error(std::string("frame must be ") + kAcceptedFrames);
        const std::string dtype = py::str(t.attr("dtype")).cast<std::string>();
        FrameView v;
        if (dtype == "torch.uint8") v.pixel_type = PC_PIXEL_U8;
        else if (dtype == "torch.uint16") v.pixel_type = PC_PIXEL_U16;
        else if (dtype == "torch.float16") v.pixel_type = PC_PIXEL_F16;
        else if (dtype == "torch.float32") v.pixel_type = PC_PIXEL_F32;
        else throw py::value_error(std::string("frame must be ") + kAcceptedFrames + ", got " + dtype);
        v.elem_size = static_cast<int>(PixelTypeBytes(v.pixel_type));
        v.data = reinterpret_cast<const uint8_t*>(t.attr("data_ptr")().cast<uintptr_t>());
        v.rows = static_cast<int>(shape[0]);
        v.cols = static_cast<int>(shape[1]);
        v.channels = static_cast<int>(shape[2]);
        v.row_pitch = static_cast<size_t>(shape[1] * shape[2]) * v.elem_size;
        v.on_device = true;
        keep_alive.push_back(t);
        while (keep_alive.size() > 40) keep_alive.pop_front();
        return v;
    }
    // host pixels of every type are converted on the GPU (no numpy pass on the host: `(x * 255).astype(uint8)` of float frames,
    // the widening of halves, the narrowing of 16-bit plates, the `[..., :3]` of RGBA bytes)
    int pixel_type = -1;
    const py::array a = AcceptedFrameArray(obj, &pixel_type);
    const size_t bytes = static_cast<size_t>(a.size()) * PixelTypeBytes(pixel_type);
    std::shared_ptr<void> buf = AcquirePinnedFrameBuffer(bytes);
    {
        py::gil_scoped_release nogil;   // `a` keeps the array alive
        CopyFrameBytes(buf.get(), a.data(), bytes);
    }
    FrameView v;
    v.on_device = true;   // pinned host memory (frame_pool.h)
    v.pinned_host = true;
    v.data = static_cast<const uint8_t*>(buf.get());
    v.rows = static_cast<int>(a.shape(0));
    v.cols = static_cast<int>(a.shape(1));
    v.channels = static_cast<int>(a.shape(2));
    v.pixel_type = pixel_type;
    v.elem_size = static_cast<int>(PixelTypeBytes(pixel_type));
    v.row_pitch = static_cast<size_t>(a.shape(1) * a.shape(2)) * v.elem_size;
    v.owner = buf;
    return v;
}

// polychase_core.frame_channel_bytes: the (H, W, 3) bytes the default conversion makes of a frame's channels, on the host
py::array_t<uint8_t> FrameChannelBytesPy(const py::object& frame) {
    int pixel_type = -1;
    const py::array a = AcceptedFrameArray(frame, &pixel_type);
    py::array_t<uint8_t> out({a.shape(0), a.shape(1), static_cast<py::ssize_t>(3)});
    FrameChannelBytes(static_cast<const uint8_t*>(a.data()), static_cast<int>(a.shape(0)), static_cast<int>(a.shape(1)),
                      static_cast<int>(a.shape(2)), pixel_type, static_cast<size_t>(a.shape(1) * a.shape(2)) * PixelTypeBytes(pixel_type),
                      out.mutable_data());
    return out;
}

using I32Array = py::array_t<int32_t, py::array::c_style>;

// int32 (H, W, 2) -> an owned copy; ValueError for any other dtype or shape (no silent conversion: a float array is not a map)
std::shared_ptr<const LensMapData> LensMapFromPython(const py::object& obj) {
    if (!py::isinstance<py::array>(obj)) throw py::value_error("lens must be None, a LensModel or an int32 array of shape (H, W, 2)");
    const py::array arr = py::reinterpret_borrow<py::array>(obj);
    if (!arr.dtype().is(py::dtype::of<int32_t>())) throw py::value_error("a lens map must have dtype int32");
    if (arr.ndim() != 3 || arr.shape(2) != 2 || arr.shape(0) < 1 || arr.shape(1) < 1) throw py::value_error("a lens map must have shape (H, W, 2)");
    const I32Array a = I32Array::ensure(arr);
    auto m = std::make_shared<LensMapData>();
    m->height = static_cast<int>(a.shape(0));
    m->width = static_cast<int>(a.shape(1));
    m->q.assign(a.data(), a.data() + a.size());
    return m;
}

py::array_t<int32_t> LensMapToPython(const LensMapData& m) {
    py::array_t<int32_t> out({static_cast<py::ssize_t>(m.height), static_cast<py::ssize_t>(m.width), static_cast<py::ssize_t>(2)});
    std::copy(m.q.begin(), m.q.end(), out.mutable_data());
    return out;
}

pc_lens_model ToAbi(const LensModel& m) { return pc_lens_model{m.fx, m.fy, m.cx, m.cy, m.k1, m.k2, m.k3, m.p1, m.p2, m.zoom}; }

// Python detection mask (numpy H x W uint8) -> MaskView owning a packed copy.  ValueError for any other dtype or shape: the
// reference CHECKs CV_8UC1 and the image's size (gftt.cc:22-27); no silent conversion.
MaskView MaskFromPython(const py::object& obj, const VideoInfo& video_info) {
    if (!py::isinstance<py::array>(obj)) throw py::value_error("detection_mask must be a uint8 array of shape (H, W), a callable or None");
    const py::array arr = py::reinterpret_borrow<py::array>(obj);
    if (!arr.dtype().is(py::dtype::of<uint8_t>())) throw py::value_error("detection_mask must have dtype uint8");
    if (arr.ndim() != 2 || arr.shape(0) != static_cast<py::ssize_t>(video_info.height) || arr.shape(1) != static_cast<py::ssize_t>(video_info.width))
        throw py::value_error("detection_mask must have shape (" + std::to_string(video_info.height) + ", " + std::to_string(video_info.width) + ")");
    const U8Array a = U8Array::ensure(arr);   // C order (a strided view is packed here)
    auto copy = std::make_shared<std::vector<uint8_t>>(a.data(), a.data() + a.size());
    MaskView v;
    v.data = copy->data();
    v.rows = static_cast<int>(video_info.height);
    v.cols = static_cast<int>(video_info.width);
    v.row_pitch = static_cast<size_t>(video_info.width);
    v.owner = copy;
    return v;
}

// polychase_core.PolygonMask(polygons, invert=False): a detection mask as closed polygons (csrc/host/analysis.h PolygonMaskData;
// the fill rule: include/polychase_hip.h pc_frame_set_mask_polygons).  Everything the engine would refuse is a ValueError here,
// at construction, before any GPU work.
struct PolygonMaskPy {
    std::shared_ptr<const PolygonMaskData> data;
    py::tuple polygons;   // the float32 (K, 2) copies, read-only
};

PolygonMaskPy MakePolygonMask(const py::object& polygons, bool invert) {
    if (polygons.is_none() || py::isinstance<py::str>(polygons) || !py::isinstance<py::sequence>(polygons))
        throw py::value_error("PolygonMask takes a sequence of polygons, each an array of shape (K, 2)");
    auto data = std::make_shared<PolygonMaskData>();
    data->invert = invert;
    py::list kept;
    for (const py::handle& item : py::reinterpret_borrow<py::sequence>(polygons)) {
        py::array raw;
        try {
            raw = py::array::ensure(item);
        } catch (const py::error_already_set&) {
            raw = py::array();
        }
        if (!raw || raw.ndim() != 2 || raw.shape(1) != 2) throw py::value_error("a polygon must be an array of shape (K, 2)");
        const char kind = raw.dtype().kind();
        if (kind != 'f' && kind != 'i' && kind != 'u') throw py::value_error("a polygon must hold numbers");
        // a copy of our own, converted to float32 in C order
        F32Array p = F32Array::ensure(py::module_::import("numpy").attr("array")(raw, py::arg("dtype") = "float32", py::arg("order") = "C"));
        if (!p) throw py::value_error("a polygon must be convertible to float32");
        if (p.shape(0) < 3) throw py::value_error("a polygon needs at least 3 vertices, got " + std::to_string(p.shape(0)));
        if (data->counts.size() >= static_cast<size_t>(PC_MASK_MAX_POLYGONS))
            throw py::value_error("more than " + std::to_string(PC_MASK_MAX_POLYGONS) + " polygons");
        if (data->xy.size() / 2 + static_cast<size_t>(p.shape(0)) > static_cast<size_t>(PC_MASK_MAX_VERTICES))
            throw py::value_error("more than " + std::to_string(PC_MASK_MAX_VERTICES) + " vertices");
        const float* v = p.data();
        for (py::ssize_t i = 0; i < p.size(); i++)
            if (!(std::fabs(v[i]) <= 32768.0f)) throw py::value_error("a polygon's coordinates must be finite and within +-32768");
        data->xy.insert(data->xy.end(), v, v + p.size());
        data->counts.push_back(static_cast<int32_t>(p.shape(0)));
        p.attr("setflags")(py::arg("write") = false);
        kept.append(p);
    }
    return PolygonMaskPy{std::move(data), py::tuple(kept)};
}

// polychase_core.MeshMask(accel_mesh, scene_transforms, check_mask=True, invert=False, margin=0): a detection mask as the
// silhouette of a mesh under the poses a user has (csrc/host/analysis.h MeshMaskData; the rule: include/polychase_hip.h
// pc_mesh_render).  scene_transforms: one SceneTransformations (every frame), or a dict {frame_id: SceneTransformations} (a frame
// without an entry is detected without a mask).  The cameras are made at construction, so a singular view * model is an error
// here; the object keeps the AcceleratedMesh alive.  With check_mask the mesh's masked_triangles are sent when a frame's mask is
// rendered, on the run's thread (OpticalFlowThread: without the GIL): they must not be edited through inner_mut() while a run
// uses the mesh -- the rule TrackerThread already has for its mesh.
struct MeshMaskPy {
    std::shared_ptr<const AcceleratedMesh> mesh;
    std::optional<pc_ray_camera> one;
    std::map<int32_t, pc_ray_camera> by_frame;
    bool check_mask = true, invert = false;
    int margin = 0;
    int device = 0;

    std::optional<MaskView> View(std::optional<int32_t> frame_id) const {
        const pc_ray_camera* cam = one ? &*one : nullptr;
        if (!cam && frame_id) {
            const auto it = by_frame.find(*frame_id);
            if (it != by_frame.end()) cam = &it->second;
        }
        if (!cam) return std::nullopt;
        auto data = std::make_shared<MeshMaskData>();
        data->owner = mesh;
        data->gpu = mesh->Gpu();
        data->ctx = SharedGpuContext();
        data->device = device;
        data->cam = *cam;
        data->check_mask = check_mask;
        data->invert = invert;
        data->margin = margin;
        const AcceleratedMesh* m = mesh.get();   // kept alive by `owner`
        data->sync_mask = [m] { m->SyncMask(); };
        MaskView v;
        v.mesh = std::move(data);
        return v;
    }
};

MeshMaskPy MakeMeshMask(std::shared_ptr<const AcceleratedMesh> mesh, const py::object& scene_transforms, bool check_mask, bool invert, int margin) {
    if (!mesh) throw py::value_error("MeshMask needs an AcceleratedMesh");
    if (margin < 0 || margin > PC_TARGET_MASK_MAX_MARGIN)
        throw py::value_error("MeshMask: margin must be in 0.." + std::to_string(PC_TARGET_MASK_MAX_MARGIN) + ", got " + std::to_string(margin));
    MeshMaskPy out;
    out.mesh = std::move(mesh);
    out.check_mask = check_mask;
    out.invert = invert;
    out.margin = margin;
    out.device = SharedGpuDevice();   // the mesh was created on the shared context
    auto camera_of = [](const py::handle& h) {
        if (!py::isinstance<SceneTransformations>(h)) throw py::value_error("MeshMask: scene_transforms is a SceneTransformations or a dict {frame_id: SceneTransformations}");
        pc_ray_camera cam;
        try {
            MakeRayCamera(h.cast<const SceneTransformations&>(), &cam);
        } catch (const std::runtime_error& e) {
            throw py::value_error(std::string("MeshMask: ") + e.what());
        }
        return cam;
    };
    if (py::isinstance<py::dict>(scene_transforms)) {
        for (const auto& kv : py::reinterpret_borrow<py::dict>(scene_transforms)) {
            if (!py::isinstance<py::int_>(kv.first)) throw py::value_error("MeshMask: the keys of a dict are frame ids");
            out.by_frame[kv.first.cast<int32_t>()] = camera_of(kv.second);
        }
    } else {
        out.one = camera_of(scene_transforms);
    }
    return out;
}

// array | PolygonMask | MeshMask -> MaskView (a MeshMask of per-frame poses without one for `frame_id`: nothing)
std::optional<MaskView> AnyMaskFromPython(const py::object& obj, const VideoInfo& video_info, std::optional<int32_t> frame_id) {
    if (py::isinstance<PolygonMaskPy>(obj)) {
        MaskView v;
        v.polygons = obj.cast<const PolygonMaskPy&>().data;
        return v;
    }
    if (py::isinstance<MeshMaskPy>(obj)) return obj.cast<const MeshMaskPy&>().View(frame_id);
    return MaskFromPython(obj, video_info);
}

// detection_mask=None | array | PolygonMask | MeshMask | callable(frame_id) -> array | PolygonMask | MeshMask | None | dict
// {frame_id: PolygonMask | MeshMask | None} (copied here; a missing key = no mask for that frame; an array as a value is refused:
// a clip of planes does not belong in a dictionary).  `obj` must outlive the run (the callable is called with the GIL from the
// driver's thread).
// allow_callable = false: OpticalFlowThread, whose protocol has no mask request -- its per-frame masks come as a dict, or as a
// MeshMask of per-frame poses.
DetectionMask DetectionMaskFromPython(const py::object& obj, const VideoInfo& video_info, bool allow_callable = true) {
    DetectionMask m;
    if (obj.is_none()) return m;
    if (py::isinstance<py::dict>(obj)) {
        auto table = std::make_shared<std::map<int32_t, MaskView>>();
        for (const auto& kv : py::reinterpret_borrow<py::dict>(obj)) {
            if (!py::isinstance<py::int_>(kv.first)) throw py::value_error("detection_mask: the keys of a dict are frame ids");
            if (kv.second.is_none()) continue;
            const int32_t frame_id = kv.first.cast<int32_t>();
            if (py::isinstance<MeshMaskPy>(kv.second)) {
                const MeshMaskPy& mm = kv.second.cast<const MeshMaskPy&>();
                if (std::optional<MaskView> v = mm.View(frame_id)) (*table)[frame_id] = *v;
                m.mesh_device = mm.device;
                continue;
            }
            if (!py::isinstance<PolygonMaskPy>(kv.second)) throw py::value_error("detection_mask: the values of a dict are PolygonMask, MeshMask or None");
            MaskView v;
            v.polygons = kv.second.cast<const PolygonMaskPy&>().data;
            (*table)[frame_id] = v;
        }
        m.per_frame = [table](int32_t frame_id) -> std::optional<MaskView> {
            const auto it = table->find(frame_id);
            if (it == table->end()) return std::nullopt;
            return it->second;
        };
        return m;
    }
    if (py::isinstance<MeshMaskPy>(obj)) {
        const MeshMaskPy mm = obj.cast<const MeshMaskPy&>();   // a copy of our own: the cameras and a reference to the mesh
        if (mm.one) {
            m.fixed = mm.View(std::nullopt);
        } else {
            m.mesh_device = mm.device;
            m.per_frame = [mm](int32_t frame_id) { return mm.View(frame_id); };
        }
        return m;
    }
    if (!py::isinstance<PolygonMaskPy>(obj) && PyCallable_Check(obj.ptr())) {
        if (!allow_callable) throw py::value_error("detection_mask must be a uint8 array of shape (H, W), a PolygonMask, a MeshMask, a dict of them or None");
        m.per_frame = [&obj, video_info](int32_t frame_id) -> std::optional<MaskView> {
            py::gil_scoped_acquire gil;
            const py::object r = obj(frame_id);
            if (r.is_none()) return std::nullopt;
            return AnyMaskFromPython(r, video_info, frame_id);
        };
        return m;
    }
    m.fixed = AnyMaskFromPython(obj, video_info, std::nullopt);
    return m;
}

OpticalFlowRunStats GenerateOpticalFlowDatabasePy(const VideoInfo& video_info, py::object frame_accessor,
                                                  py::object callback, const std::string& database_path,
                                                  const GFTTOptions& detector_options,
                                                  const OpticalFlowOptions& flow_options, bool write_images,
                                                  py::object detection_mask) {
    const DetectionMask mask = DetectionMaskFromPython(detection_mask, video_info);
    std::deque<py::object> keep_alive;
    FrameAccessorFunction accessor;
    if (!frame_accessor.is_none())
        accessor = [&](int32_t frame_id) -> std::optional<FrameView> {
            py::gil_scoped_acquire gil;
            return FrameFromPython(frame_accessor(frame_id), keep_alive);
        };
    OpticalFlowProgressCallback cb;
    if (!callback.is_none())
        cb = [&](float progress, const std::string& msg) -> bool {
            py::gil_scoped_acquire gil;
            return callback(progress, msg).cast<bool>();
        };
    OpticalFlowRunStats stats;
    {
        py::gil_scoped_release release;  // polychase_pybind.cc:332
        GenerateOpticalFlowDatabase(video_info, accessor, cb, database_path, detector_options, flow_options,
                                    write_images, &stats, mask);
    }
    keep_alive.clear();
    return stats;
}

// one shard of a multi-process analysis: records into a device log (a torch uint8 CUDA tensor's memory)
py::tuple GenerateOpticalFlowRecordsPy(const VideoInfo& video_info, py::object frame_accessor, py::object callback,
                                       int32_t shard_begin, int32_t shard_end, uintptr_t device_log, size_t capacity_bytes,
                                       const GFTTOptions& detector_options, const OpticalFlowOptions& flow_options,
                                       py::object detection_mask) {
    const DetectionMask mask = DetectionMaskFromPython(detection_mask, video_info);
    std::deque<py::object> keep_alive;
    FrameAccessorFunction accessor;
    if (!frame_accessor.is_none())
        accessor = [&](int32_t frame_id) -> std::optional<FrameView> {
            py::gil_scoped_acquire gil;
            return FrameFromPython(frame_accessor(frame_id), keep_alive);
        };
    OpticalFlowProgressCallback cb;
    if (!callback.is_none())
        cb = [&](float progress, const std::string& msg) -> bool {
            py::gil_scoped_acquire gil;
            return callback(progress, msg).cast<bool>();
        };
    OpticalFlowRunStats stats;
    size_t used = 0;
    {
        py::gil_scoped_release release;
        used = GenerateOpticalFlowRecords(video_info, accessor, cb, shard_begin, shard_end, reinterpret_cast<void*>(device_log),
                                          capacity_bytes, detector_options, flow_options, &stats, mask);
    }
    keep_alive.clear();
    return py::make_tuple(used, stats);
}

// one shard with everything the multi-rank driver needs: records into the database (the rank that owns the file) and / or
// into a device log that is handed over piece by piece (on_piece(piece, offset_bytes, bytes, first_frame1, n_frames),
// called with the GIL on the driver's thread; the part of the log may be reused when it returns)
py::dict GenerateOpticalFlowShardPy(const VideoInfo& video_info, py::object frame_accessor, py::object callback,
                                    const std::string& database_path, int32_t shard_begin, int32_t shard_end, uintptr_t device_log,
                                    size_t capacity_bytes, int log_buffers, int piece_frames, py::object on_piece, bool host_records,
                                    const GFTTOptions& detector_options, const OpticalFlowOptions& flow_options,
                                    py::object detection_mask) {
    const DetectionMask mask = DetectionMaskFromPython(detection_mask, video_info);
    std::deque<py::object> keep_alive;
    FrameAccessorFunction accessor;
    if (!frame_accessor.is_none())
        accessor = [&](int32_t frame_id) -> std::optional<FrameView> {
            py::gil_scoped_acquire gil;
            return FrameFromPython(frame_accessor(frame_id), keep_alive);
        };
    OpticalFlowProgressCallback cb;
    if (!callback.is_none())
        cb = [&](float progress, const std::string& msg) -> bool {
            py::gil_scoped_acquire gil;
            return callback(progress, msg).cast<bool>();
        };
    OpticalFlowShard shard;
    shard.begin = shard_begin;
    shard.end = shard_end;
    shard.device_log = reinterpret_cast<void*>(device_log);
    shard.capacity_bytes = capacity_bytes;
    shard.log_buffers = log_buffers;
    shard.piece_frames = piece_frames;
    shard.host_records = host_records;
    if (!on_piece.is_none())
        shard.on_piece = [&](int piece, size_t offset, size_t bytes, int32_t first_frame1, int n_frames) {
            py::gil_scoped_acquire gil;
            on_piece(piece, offset, bytes, first_frame1, n_frames);
        };
    OpticalFlowRunStats stats;
    {
        py::gil_scoped_release release;
        GenerateOpticalFlowShard(video_info, accessor, cb, database_path, shard, detector_options, flow_options, &stats, mask);
    }
    keep_alive.clear();
    py::dict out;
    out["used_bytes"] = shard.used_bytes;
    out["pieces"] = shard.pieces;
    out["cancelled"] = shard.cancelled;
    out["stats"] = stats;
    return out;
}

// GenerateOpticalFlowDatabaseMultiGpu (csrc/host/multi_gpu.h): this rank's part of the multi-GPU analysis, RCCL + TCP control
// channel underneath, no torch.  Not in the reference (its analysis is one process).
py::dict GenerateOpticalFlowDatabaseMultiGpuPy(const VideoInfo& video_info, py::object frame_accessor, py::object callback,
                                               const std::string& database_path, int world_size, int rank, const std::string& master_addr,
                                               int master_port, int device, int piece_frames, const std::string& transport,
                                               size_t keypoints_per_frame, const GFTTOptions& detector_options,
                                               const OpticalFlowOptions& flow_options, py::object detection_mask) {
    const DetectionMask mask = DetectionMaskFromPython(detection_mask, video_info);
    std::deque<py::object> keep_alive;
    FrameAccessorFunction accessor;
    if (!frame_accessor.is_none())
        accessor = [&](int32_t frame_id) -> std::optional<FrameView> {
            py::gil_scoped_acquire gil;
            return FrameFromPython(frame_accessor(frame_id), keep_alive);
        };
    OpticalFlowProgressCallback cb;
    if (!callback.is_none())
        cb = [&](float progress, const std::string& msg) -> bool {
            py::gil_scoped_acquire gil;
            return callback(progress, msg).cast<bool>();
        };
    MultiGpuConfig cfg;
    cfg.world_size = world_size;
    cfg.rank = rank;
    cfg.master_addr = master_addr;
    cfg.master_port = master_port;
    cfg.device = device;
    cfg.piece_frames = piece_frames;
    cfg.transport = transport;
    cfg.keypoints_per_frame = keypoints_per_frame;
    MultiGpuResult r;
    {
        py::gil_scoped_release release;
        r = GenerateOpticalFlowDatabaseMultiGpu(video_info, accessor, cb, database_path, cfg, detector_options, flow_options, mask);
    }
    keep_alive.clear();
    py::dict out;
    out["shard"] = py::make_tuple(r.shard_begin, r.shard_end);
    out["pieces"] = r.pieces;
    out["bytes_moved"] = r.bytes_moved;
    out["cancelled"] = r.cancelled;
    out["seconds_analysis"] = r.seconds_analysis;
    out["seconds_total"] = r.seconds_total;
    out["seconds_blocked"] = r.seconds_blocked;
    out["stats"] = r.stats;
    return out;
}

OpticalFlowRunStats WriteOpticalFlowRecordsPy(const std::string& database_path, const U8Array& log, size_t bytes) {
    if (bytes > static_cast<size_t>(log.size())) throw py::value_error("bytes exceeds the buffer");
    OpticalFlowRunStats stats;
    {
        py::gil_scoped_release release;
        WriteOpticalFlowRecords(database_path, log.data(), bytes, &stats);
    }
    return stats;
}

}  // namespace

PYBIND11_MODULE(polychase_core, m) {
    m.doc() = "polychase_core on MI355X: drop-in for the reference's pybind11 module (video-analysis path)";
    // a hardware queue per stream of the engine: must be in the environment before the process first touches HIP -- importing
    // the module is the earliest moment the add-on gives us (include/polychase_hip.h: pc_runtime_init)
    {
        int was_up = 0, queues = 0;
        pc_runtime_init(&was_up, &queues);
        m.attr("_runtime_was_up_at_import") = was_up != 0;   // not in the reference (diagnostics)
        m.attr("_gpu_max_hw_queues") = queues;
    }

    m.def("_async_write_counters", [] {   // not in the reference (tests, diagnostics): totals of csrc/host/async_write_vfs.h
        const AsyncWriteVfsCounters c = AsyncWriteVfsTotals();
        py::dict d;
        d["deferred_writes"] = c.deferred_writes;
        d["deferred_bytes"] = c.deferred_bytes;
        d["direct_writes"] = c.direct_writes;
        d["drains"] = c.drains;
        d["drains_that_waited"] = c.drains_that_waited;
        d["waits_for_a_slab"] = c.waits_for_a_slab;
        return d;
    });
    py::class_<Database>(m, "Database")
        .def(py::init<const std::string&>(), py::arg("path"))
        // not in the reference (tests): the connection mode of the analysis' writer, csrc/host/async_write_vfs.h
        .def_static("_open_bulk_writer", [](const std::string& path) { return std::make_unique<Database>(path, true); }, py::arg("path"))
        .def("open", [](Database& db, const std::string& path) { db.Open(path); }, py::arg("path"))
        .def("close", &Database::Close)
        .def("_set_journal_mode", &Database::SetJournalMode, py::arg("mode"))   // not in the reference (tests)
        .def("_begin", &Database::Begin)                                          // ... explicit transactions (tests)
        .def("_commit", &Database::Commit)
        .def("_rollback", &Database::Rollback)
        .def("read_keypoints", [](const Database& db, int32_t id) { return VecToNumpy<2>(db.ReadKeypoints(id)); },
             py::arg("image_id"))
        .def("write_keypoints",
             [](Database& db, int32_t id, const F32Array& kps) { db.WriteKeypoints(id, NumpyToVec<2>(kps)); },
             py::arg("image_id"), py::arg("keypoints"))
        .def("read_image_pair_flow",
             py::overload_cast<int32_t, int32_t>(&Database::ReadImagePairFlow, py::const_), py::arg("image_id_from"),
             py::arg("image_id_to"))
        .def("write_image_pair_flow",
             [](Database& db, int32_t from, int32_t to, const U32Array& idx, const F32Array& tgt, const F32Array& err) {
                 db.WriteImagePairFlow(from, to, NumpyToVec1<uint32_t>(idx), NumpyToVec<2>(tgt), NumpyToVec1<float>(err));
             },
             py::arg("image_id_from"), py::arg("image_id_to"), py::arg("src_kps_indices"), py::arg("tgt_kps"),
             py::arg("flow_errors"))
        .def("write_image_pair_flow", py::overload_cast<const ImagePairFlow&>(&Database::WriteImagePairFlow),
             py::arg("image_pair_flow"))
        .def("find_optical_flows_from_image",
             py::overload_cast<int32_t>(&Database::FindOpticalFlowsFromImage, py::const_), py::arg("image_id_from"))
        .def("find_optical_flows_to_image", py::overload_cast<int32_t>(&Database::FindOpticalFlowsToImage, py::const_),
             py::arg("image_id_to"))
        .def("keypoints_exist", &Database::KeypointsExist, py::arg("image_id"))
        .def("image_pair_flow_exists", &Database::ImagePairFlowExists, py::arg("image_id_from"),
             py::arg("image_id_to"))
        .def("get_min_image_id_with_keypoints", &Database::GetMinImageIdWithKeypoints)
        .def("get_max_image_id_with_keypoints", &Database::GetMaxImageIdWithKeypoints);

    py::class_<ImagePairFlow>(m, "ImagePairFlow")
        .def(py::init<>())
        .def_readwrite("image_id_from", &ImagePairFlow::image_id_from)
        .def_readwrite("image_id_to", &ImagePairFlow::image_id_to)
        .def_property(
            "src_kps_indices", [](const ImagePairFlow& f) { return Vec1ToNumpy(f.src_kps_indices); },
            [](ImagePairFlow& f, const U32Array& a) { f.src_kps_indices = NumpyToVec1<uint32_t>(a); })
        .def_property(
            "tgt_kps", [](const ImagePairFlow& f) { return VecToNumpy<2>(f.tgt_kps); },
            [](ImagePairFlow& f, const F32Array& a) { f.tgt_kps = NumpyToVec<2>(a); })
        .def_property(
            "flow_errors", [](const ImagePairFlow& f) { return Vec1ToNumpy(f.flow_errors); },
            [](ImagePairFlow& f, const F32Array& a) { f.flow_errors = NumpyToVec1<float>(a); });

    py::class_<VideoInfo>(m, "VideoInfo")
        .def(py::init([](uint32_t width, uint32_t height, uint32_t first_frame, uint32_t num_frames) {
                 return VideoInfo{width, height, static_cast<int32_t>(first_frame), num_frames};
             }),
             py::arg("width"), py::arg("height"), py::arg("first_frame"), py::arg("num_frames"))
        .def_readwrite("width", &VideoInfo::width)
        .def_readwrite("height", &VideoInfo::height)
        .def_readwrite("first_frame", &VideoInfo::first_frame)
        .def_readwrite("num_frames", &VideoInfo::num_frames);

    // grid_rows / grid_cols are not exposed by the reference either (polychase_pybind.cc:128-136)
    py::class_<GFTTOptions>(m, "GFTTOptions")
        .def(py::init<>())
        .def_readwrite("quality_level", &GFTTOptions::quality_level)
        .def_readwrite("min_distance", &GFTTOptions::min_distance)
        .def_readwrite("block_size", &GFTTOptions::block_size)
        .def_readwrite("gradient_size", &GFTTOptions::gradient_size)
        .def_readwrite("max_corners", &GFTTOptions::max_corners)
        .def_readwrite("use_harris", &GFTTOptions::use_harris)
        .def_readwrite("harris_k", &GFTTOptions::harris_k);

    // not in the reference: lens undistortion at ingest (include/polychase_hip.h: pc_lens_model, pc_context_set_lens_map)
    py::class_<LensModel>(m, "LensModel")
        .def(py::init([](double fx, double fy, double cx, double cy, double k1, double k2, double k3, double p1, double p2, double zoom) {
                 return LensModel{fx, fy, cx, cy, k1, k2, k3, p1, p2, zoom};
             }),
             py::arg("fx"), py::arg("fy"), py::arg("cx"), py::arg("cy"), py::arg("k1") = 0.0, py::arg("k2") = 0.0, py::arg("k3") = 0.0,
             py::arg("p1") = 0.0, py::arg("p2") = 0.0, py::arg("zoom") = 1.0)
        .def_readwrite("fx", &LensModel::fx)
        .def_readwrite("fy", &LensModel::fy)
        .def_readwrite("cx", &LensModel::cx)
        .def_readwrite("cy", &LensModel::cy)
        .def_readwrite("k1", &LensModel::k1)
        .def_readwrite("k2", &LensModel::k2)
        .def_readwrite("k3", &LensModel::k3)
        .def_readwrite("p1", &LensModel::p1)
        .def_readwrite("p2", &LensModel::p2)
        .def_readwrite("zoom", &LensModel::zoom)
        // the lens map int32 (H, W, 2) the run builds from this model for a clip of that size (pc_lens_build_map)
        .def("build_map", [](const LensModel& lm, int width, int height) {
            const pc_lens_model abi = ToAbi(lm);
            LensMapData d;
            d.width = width;
            d.height = height;
            if (width >= 1 && height >= 1 && static_cast<long long>(width) * height <= (1ll << 30)) d.q.resize(static_cast<size_t>(width) * height * 2);
            if (pc_lens_build_map(&abi, width, height, d.q.data()) != PC_OK) throw std::invalid_argument(pc_last_error());
            return LensMapToPython(d);
        }, py::arg("width"), py::arg("height"));
    // float32 STmap (H, W, 2) in [0, 1] -> lens map (pc_lens_map_from_stmap); flip_v: t = 0 is the bottom row (the usual STmap)
    m.def("lens_map_from_stmap", [](const py::array& st, bool flip_v) {
        if (!st.dtype().is(py::dtype::of<float>()) || st.ndim() != 3 || st.shape(2) != 2 || st.shape(0) < 1 || st.shape(1) < 1)
            throw py::value_error("an STmap must be a float32 array of shape (H, W, 2)");
        const F32Array a = F32Array::ensure(st);
        LensMapData d;
        d.height = static_cast<int>(a.shape(0));
        d.width = static_cast<int>(a.shape(1));
        d.q.resize(static_cast<size_t>(a.size()));
        if (pc_lens_map_from_stmap(a.data(), d.width, d.height, flip_v ? 1 : 0, d.q.data()) != PC_OK) throw std::invalid_argument(pc_last_error());
        return LensMapToPython(d);
    }, py::arg("st"), py::arg("flip_v") = true);
    // the validity plane uint8 (H, W), 255 / 0, of a lens map, eroded by `erode` pixels (pc_lens_map_valid)
    m.def("lens_map_valid", [](const py::object& q, int erode) {
        const std::shared_ptr<const LensMapData> d = LensMapFromPython(q);
        py::array_t<uint8_t> out({static_cast<py::ssize_t>(d->height), static_cast<py::ssize_t>(d->width)});
        if (pc_lens_map_valid(d->q.data(), d->width, d->height, erode, out.mutable_data(), nullptr) != PC_OK) throw std::invalid_argument(pc_last_error());
        return out;
    }, py::arg("q"), py::arg("erode") = 0);

    py::class_<OpticalFlowOptions>(m, "OpticalFlowOptions")
        .def(py::init<>())
        .def_readwrite("window_size", &OpticalFlowOptions::window_size)
        .def_readwrite("max_level", &OpticalFlowOptions::max_level)
        .def_readwrite("term_max_iters", &OpticalFlowOptions::term_max_iters)
        .def_readwrite("term_epsilon", &OpticalFlowOptions::term_epsilon)
        .def_readwrite("min_eigen_threshold", &OpticalFlowOptions::min_eigen_threshold)
        .def_readwrite("forward_backward_threshold", &OpticalFlowOptions::forward_backward_threshold)   // not in the reference; 0 = off
        .def_readwrite("target_mask_margin", &OpticalFlowOptions::target_mask_margin)   // not in the reference; -1 = off, 0..31
        .def_readwrite("min_correlation", &OpticalFlowOptions::min_correlation)   // not in the reference; 0 = off, 0..1
        .def_readwrite("normalize", &OpticalFlowOptions::normalize)   // not in the reference; brightness-normalised LK, off by default
        .def_readwrite("affine_refinement", &OpticalFlowOptions::affine_refinement)   // not in the reference; off by default, not with normalize
        .def_readwrite("search_radius", &OpticalFlowOptions::search_radius)   // not in the reference; 0 = off, 1..256, not with normalize
        .def_readwrite("mask_windows", &OpticalFlowOptions::mask_windows)   // not in the reference; off by default, needs a detection_mask
        // not in the reference: the gray conversion (include/polychase_hip.h: pc_gray_conversion)
        .def_readwrite("channel_weights", &OpticalFlowOptions::channel_weights)           // None or three floats (r, g, b)
        .def_readwrite("float_transfer", &OpticalFlowOptions::float_transfer)             // "none", "srgb" or "gamma"
        .def_readwrite("float_transfer_gamma", &OpticalFlowOptions::float_transfer_gamma)
        .def_readwrite("float_exposure", &OpticalFlowOptions::float_exposure)             // stops
        // not in the reference: lens undistortion at ingest -- None, a LensModel, or a lens map int32 (H, W, 2) of the clip's size
        .def_property(
            "lens",
            [](const OpticalFlowOptions& o) -> py::object {
                if (o.lens_model) return py::cast(*o.lens_model);
                if (o.lens_map) return LensMapToPython(*o.lens_map);
                return py::none();
            },
            [](OpticalFlowOptions& o, const py::object& v) {
                if (v.is_none()) {
                    o.lens_model.reset();
                    o.lens_map.reset();
                } else if (py::isinstance<LensModel>(v)) {
                    o.lens_model = v.cast<LensModel>();
                    o.lens_map.reset();
                } else {
                    o.lens_map = LensMapFromPython(v);
                    o.lens_model.reset();
                }
            });

    py::class_<OpticalFlowProgress>(m, "OpticalFlowProgress")
        .def_readonly("progress", &OpticalFlowProgress::progress)
        .def_readonly("progress_message", &OpticalFlowProgress::progress_message);

    py::class_<OpticalFlowRequest>(m, "OpticalFlowRequest").def_readonly("frame_id", &OpticalFlowRequest::frame_id);

    py::class_<CppException>(m, "CppException").def("what", [](const CppException& e) { return e.message; });

    py::class_<OpticalFlowRunStats>(m, "OpticalFlowRunStats")
        .def_readonly("frames_processed", &OpticalFlowRunStats::frames_processed)
        .def_readonly("keypoint_rows_written", &OpticalFlowRunStats::keypoint_rows_written)
        .def_readonly("flow_rows_written", &OpticalFlowRunStats::flow_rows_written)
        .def_readonly("seconds_total", &OpticalFlowRunStats::seconds_total)
        .def_readonly("seconds_db", &OpticalFlowRunStats::seconds_db)
        .def_readonly("seconds_setup", &OpticalFlowRunStats::seconds_setup)
        .def_readonly("engine_reused", &OpticalFlowRunStats::engine_reused)
        .def_readonly("seconds_accessor", &OpticalFlowRunStats::seconds_accessor)
        .def_readonly("seconds_put", &OpticalFlowRunStats::seconds_put)
        .def_readonly("seconds_submit", &OpticalFlowRunStats::seconds_submit)
        .def_readonly("seconds_collect", &OpticalFlowRunStats::seconds_collect)
        .def_readonly("seconds_writer_wait", &OpticalFlowRunStats::seconds_writer_wait);

    py::class_<PolygonMaskPy>(m, "PolygonMask")   // not in the reference
        .def(py::init(&MakePolygonMask), py::arg("polygons"), py::arg("invert") = false)
        .def_property_readonly("polygons", [](const PolygonMaskPy& p) { return p.polygons; })
        .def_property_readonly("invert", [](const PolygonMaskPy& p) { return p.data->invert; });

    py::class_<MeshMaskPy>(m, "MeshMask")   // not in the reference
        .def(py::init(&MakeMeshMask), py::arg("accel_mesh"), py::arg("scene_transforms"), py::arg("check_mask") = true,
             py::arg("invert") = false, py::arg("margin") = 0)
        .def_property_readonly("accel_mesh", [](const MeshMaskPy& p) { return std::const_pointer_cast<AcceleratedMesh>(p.mesh); })
        .def_property_readonly("frame_ids", [](const MeshMaskPy& p) {
            py::list ids;
            for (const auto& kv : p.by_frame) ids.append(kv.first);
            return ids;
        })
        .def_property_readonly("check_mask", [](const MeshMaskPy& p) { return p.check_mask; })
        .def_property_readonly("invert", [](const MeshMaskPy& p) { return p.invert; })
        .def_property_readonly("margin", [](const MeshMaskPy& p) { return p.margin; });

    py::class_<OpticalFlowThread>(m, "OpticalFlowThread")
        .def(py::init([](VideoInfo video_info, std::string database_path, GFTTOptions detector_options, OpticalFlowOptions flow_options,
                         bool write_images, py::object detection_mask) {
                 DetectionMask mask = DetectionMaskFromPython(detection_mask, video_info, /*allow_callable=*/false);
                 return std::make_unique<OpticalFlowThread>(video_info, std::move(database_path), detector_options, flow_options, write_images,
                                                            std::move(mask));
             }),
             py::arg("video_info"), py::arg("database_path"), py::arg("detector_options") = GFTTOptions{},
             py::arg("OpticalFlowOptions") = OpticalFlowOptions{},  // sic: polychase_pybind.cc:186
             py::arg("write_images") = false, py::arg("detection_mask") = py::none())   // detection_mask: not in the reference
        .def("request_stop", &OpticalFlowThread::RequestStop)
        .def("join", &OpticalFlowThread::Join, py::call_guard<py::gil_scoped_release>())
        .def("try_pop", &OpticalFlowThread::TryPop)
        .def("empty", &OpticalFlowThread::Empty)
        .def("provide_frame", [](OpticalFlowThread& t, int32_t frame_id, const py::array& frame) {
            int pixel_type = -1;
            const py::array a = AcceptedFrameArray(frame, &pixel_type);   // ValueError for any other dtype or shape
            const int elem = static_cast<int>(PixelTypeBytes(pixel_type));
            t.ProvideFrame(frame_id, static_cast<const uint8_t*>(a.data()), static_cast<int>(a.shape(0)), static_cast<int>(a.shape(1)),
                           static_cast<int>(a.shape(2)), static_cast<size_t>(a.shape(1) * a.shape(2)) * elem, elem, pixel_type);
        });

    // not in the reference: the two halves of a multi-GPU analysis (polychase_amd/analyze.py launches them, one
    // process per GPU, and all-gathers the record logs over RCCL in between)
    m.def("generate_optical_flow_records", &GenerateOpticalFlowRecordsPy, py::arg("video_info"), py::arg("frame_accessor_function"),
          py::arg("callback"), py::arg("shard_begin"), py::arg("shard_end"), py::arg("device_log"), py::arg("capacity_bytes"),
          py::arg("detector_options") = GFTTOptions{}, py::arg("flow_options") = OpticalFlowOptions{},
          py::arg("detection_mask") = py::none());
    // not in the reference's module: its SaveImageForDebugging (cpp/opticalflow.cc:80-96) by itself, for the tests
    m.def("_save_image_for_debugging", [](const U8Array& rgb, int32_t frame_id, const std::string& dir, const F32Array& kps) {
        if (rgb.ndim() != 3 || rgb.shape(2) != 3) throw py::value_error("rgb must be (H, W, 3) uint8");
        std::vector<uint8_t> img(rgb.data(), rgb.data() + rgb.size());
        SaveImageForDebugging(img.data(), static_cast<int>(rgb.shape(1)), static_cast<int>(rgb.shape(0)), frame_id, dir, kps.data(),
                              static_cast<int>(kps.size() / 2));
    });
    // not in the reference: what the default conversion makes of the channels of a frame of any accepted type, on the host by the
    // rules the GPU applies (csrc/hip/pixel_rules.hpp) -- like float_transfer_table, the CPU-testable face of a device rule
    m.def("frame_channel_bytes", &FrameChannelBytesPy, py::arg("frame"));
    m.def("_engine_cache_timer_running", &EngineCacheTimerRunning);   // testing aid
    // measurement aid (not in the reference): the stage totals of the last finished call of that kind -- "TrackCameraTrajectory",
    // "RefineTrajectory" -- as {label: (milliseconds or count, calls)} (csrc/host/stage_clock.h)
    m.def("_stage_report", [](const std::string& title) {
        py::dict d;
        for (const auto& kv : StageClock::Last(title)) d[py::str(kv.first)] = py::make_tuple(kv.second.first, kv.second.second);
        return d;
    });
    // measurement aid (not in the reference): where the library's host threads were put (csrc/host/numa_pin.h), as a JSON string
    m.def("_thread_placement", [] { return numa::Placement(); });
    // not in the reference: gives back what the calls keep for the next one -- the parked analysis engine, the tracker's parked
    // correspondence set and its pool of page-locked blocks
    m.def("release_cached_engine", [] {
        ReleaseCachedEngine();
        ReleaseTrackerCaches();
    });
    // not in the reference: the built-in float transfer table of OpticalFlowOptions.float_transfer (include/polychase_hip.h:
    // pc_float_transfer_table), uint8 [PC_TRANSFER_ENTRIES]; computed on the host
    m.def("float_transfer_table", [](const std::string& kind, double gamma, double exposure) {
        if (kind != "srgb" && kind != "gamma") throw std::invalid_argument("float transfer kind must be \"srgb\" or \"gamma\", got \"" + kind + "\"");
        py::array_t<uint8_t> out(PC_TRANSFER_ENTRIES);
        if (pc_float_transfer_table(kind == "srgb" ? PC_TRANSFER_SRGB : PC_TRANSFER_GAMMA, gamma, exposure, out.mutable_data()) != PC_OK)
            throw std::invalid_argument(pc_last_error());
        return out;
    }, py::arg("kind"), py::arg("gamma") = 2.2, py::arg("exposure") = 0.0);
    // not in the reference: what OpticalFlowOptions.channel_weights becomes -- the three 15-bit integers of pc_gray_conversion
    // (include/polychase_hip.h: pc_gray_quantize_weights, the quantiser the driver calls)
    m.def("quantize_channel_weights", [](const std::array<double, 3>& weights) {
        pc_gray_conversion c;
        pc_gray_default_conversion(&c);
        if (pc_gray_quantize_weights(weights.data(), &c) != PC_OK) throw std::invalid_argument(pc_last_error());
        return py::make_tuple(c.weight_r, c.weight_g, c.weight_b);
    }, py::arg("weights"));
    m.def("generate_optical_flow_shard", &GenerateOpticalFlowShardPy, py::arg("video_info"), py::arg("frame_accessor_function"),
          py::arg("callback"), py::arg("database_path"), py::arg("shard_begin"), py::arg("shard_end"), py::arg("device_log") = 0,
          py::arg("capacity_bytes") = 0, py::arg("log_buffers") = 1, py::arg("piece_frames") = 0, py::arg("on_piece") = py::none(),
          py::arg("host_records") = true, py::arg("detector_options") = GFTTOptions{}, py::arg("flow_options") = OpticalFlowOptions{},
          py::arg("detection_mask") = py::none());
    m.def("generate_optical_flow_database_multi_gpu", &GenerateOpticalFlowDatabaseMultiGpuPy, py::arg("video_info"),
          py::arg("frame_accessor_function"), py::arg("callback"), py::arg("database_path"), py::arg("world_size"), py::arg("rank"),
          py::arg("master_addr") = "127.0.0.1", py::arg("master_port") = 29611, py::arg("device") = -1, py::arg("piece_frames") = 16,
          py::arg("transport") = "rccl", py::arg("keypoints_per_frame") = 0, py::arg("detector_options") = GFTTOptions{},
          py::arg("flow_options") = OpticalFlowOptions{}, py::arg("detection_mask") = py::none());
    // Testing aid (not in the reference): GenerateOpticalFlowDatabaseMultiGpu's protocol -- credits, headers, ordered pieces, failure
    // propagation, the cancelled flag -- with the rank's shard given as ready-made record logs instead of an analysis
    // (MultiGpuConfig::synthetic_shard, transport "tcp"): runs on a box without a GPU (tests/test_distributed_cpu.py).
    // pieces: [(bytes-like log, first_frame1, n_frames)]; delay_ms: sleep before every piece; fail_after: raise after that many.
    m.def("_multi_gpu_protocol_selftest",
          [](int world_size, int rank, int master_port, const std::string& database_path, py::list pieces, int delay_ms, int fail_after) {
              struct Piece {
                  std::string bytes;
                  int32_t first;
                  int frames;
              };
              std::vector<Piece> ps;
              for (const py::handle& h : pieces) {
                  const py::tuple t = h.cast<py::tuple>();
                  ps.push_back(Piece{t[0].cast<py::bytes>(), t[1].cast<int32_t>(), t[2].cast<int>()});
              }
              MultiGpuConfig cfg;
              cfg.world_size = world_size;
              cfg.rank = rank;
              cfg.master_port = master_port;
              cfg.transport = "tcp";
              cfg.connect_timeout_s = 60.0;
              cfg.synthetic_shard = [&](int, const std::function<void(const void*, size_t, int32_t, int)>& emit) {
                  int sent = 0;
                  for (const Piece& p : ps) {
                      if (fail_after >= 0 && sent == fail_after) throw std::runtime_error("synthetic shard failed on purpose");
                      if (delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(delay_ms));
                      emit(p.bytes.data(), p.bytes.size(), p.first, p.frames);
                      sent++;
                  }
                  if (fail_after >= 0 && sent == fail_after) throw std::runtime_error("synthetic shard failed on purpose");
              };
              MultiGpuResult r;
              {
                  py::gil_scoped_release release;
                  r = GenerateOpticalFlowDatabaseMultiGpu(VideoInfo{}, nullptr, nullptr, database_path, cfg);
              }
              py::dict out;
              out["pieces"] = r.pieces;
              out["bytes_moved"] = r.bytes_moved;
              out["cancelled"] = r.cancelled;
              out["keypoint_rows_written"] = r.stats.keypoint_rows_written;
              out["flow_rows_written"] = r.stats.flow_rows_written;
              return out;
          },
          py::arg("world_size"), py::arg("rank"), py::arg("master_port"), py::arg("database_path"), py::arg("pieces"),
          py::arg("delay_ms") = 0, py::arg("fail_after") = -1);
    py::class_<OpticalFlowRecordWriter>(m, "OpticalFlowRecordWriter")
        .def(py::init<const std::string&>(), py::arg("database_path"))
        .def("write",
             [](OpticalFlowRecordWriter& w, const U8Array& log, size_t bytes) {
                 if (bytes > static_cast<size_t>(log.size())) throw py::value_error("bytes exceeds the buffer");
                 OpticalFlowRunStats stats;
                 {
                     py::gil_scoped_release release;
                     w.Write(log.data(), bytes, &stats);
                 }
                 return stats;
             },
             py::arg("log"), py::arg("bytes"))
        .def("close", &OpticalFlowRecordWriter::Close);
    m.def("write_optical_flow_records", &WriteOpticalFlowRecordsPy, py::arg("database_path"), py::arg("log"), py::arg("bytes"));
    m.def("generate_optical_flow_database", &GenerateOpticalFlowDatabasePy, py::arg("video_info"),
          py::arg("frame_accessor_function"), py::arg("callback"), py::arg("database_path"),
          py::arg("detector_options") = GFTTOptions{}, py::arg("flow_options") = OpticalFlowOptions{},
          py::arg("write_images") = false, py::arg("detection_mask") = py::none());   // detection_mask: not in the reference

#ifdef PC_WITH_TRACKER
    BindTracker(m);
#endif
}
