// analysis.h -- "Analyze Video" on the MI355X path: option structs, frame hand-off type and the
// entry point GenerateOpticalFlowDatabase.
//
// The structs carry the reference's field names and defaults because polychase_core exposes them
// one to one (cpp/polychase_pybind.cc:119-145): GFTTOptions <- cpp/feature_detection/gftt.h:5-21,
// OpticalFlowOptions and VideoInfo <- cpp/opticalflow.h:20-33.  cv::Mat is replaced by FrameView.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/polychase_hip.h"

// ---- options -----------------------------------------------------------------------------------

// Shi-Tomasi detector with per-grid-cell quality threshold.  On the HIP path block_size and
// gradient_size must be 3 and use_harris false (what the addon always uses).
struct GFTTOptions {
    double quality_level = 0.01;  // keep responses above quality_level * (max response of the grid cell)
    double min_distance = 5.0;    // greedy suppression radius, pixels
    int block_size = 3;
    int gradient_size = 3;
    int max_corners = 0;          // 0: unlimited
    bool use_harris = false;
    double harris_k = 0.04;
    int grid_rows = 4;            // not exposed to Python by the reference either
    int grid_cols = 4;
};

// Polynomial lens model of the ORIGINAL frames (include/polychase_hip.h: pc_lens_model has the formula; not in the reference).
// The undistorted camera -- the one the tracker and the refiner must be given -- has fx * zoom, fy * zoom, cx, cy.
struct LensModel {
    double fx = 1.0, fy = 1.0, cx = 0.0, cy = 0.0;
    double k1 = 0.0, k2 = 0.0, k3 = 0.0, p1 = 0.0, p2 = 0.0;
    double zoom = 1.0;
};
// A ready-made lens map: int32 q[height][width][2], source positions in 1 / 256 px (pc_lens_build_map, pc_lens_map_from_stmap)
struct LensMapData {
    int width = 0, height = 0;
    std::vector<int32_t> q;
};

// Pyramidal Lucas-Kanade.  max_level counts pyramid levels ABOVE level 0 (OpenCV semantics).
struct OpticalFlowOptions {
    int window_size = 10;
    int max_level = 3;
    int term_max_iters = 30;
    double term_epsilon = 0.01;
    double min_eigen_threshold = 1e-4;
    // not in the reference: forward-backward check (include/polychase_hip.h: pc_lk_track_fb), pixels at level 0; 0 = off
    double forward_backward_threshold = 0.0;
    // not in the reference: target-side masks (include/polychase_hip.h: pc_lk_track_masked).  -1 = off; 0..31: a flow row is
    // dropped when its end point lies where the detection mask of its TARGET frame, choked by this many pixels, is off.  Does
    // nothing without a detection_mask.
    int target_mask_margin = -1;
    // not in the reference: minimum correlation (include/polychase_hip.h: pc_lk_track_correlated).  0 = off; 0 < v <= 1: a flow
    // row is dropped when the normalised cross-correlation of the two windows LK compared lies below v (Blender's tracker
    // calls it correlation_min, default 0.75 there)
    double min_correlation = 0.0;
    // not in the reference: brightness normalisation (include/polychase_hip.h: pc_lk_track_normalized).  true: every LK pass of the
    // analysis tracks g (J - mean J) against (I - mean I), so a gain or bias change between two frames no longer displaces the
    // end points (Blender's tracker calls it "normalize")
    bool normalize = false;
    // not in the reference: affine refinement (include/polychase_hip.h: pc_lk_track_affine).  true: the end point of every forward
    // row is refined at level 0 under a 6-parameter warp of the window, so that it survives the roll and zoom between frames up
    // to 8 apart (Blender's tracker calls it the affine motion model).  Not together with normalize.
    bool affine_refinement = false;
    // not in the reference: search prepass (include/polychase_hip.h: pc_lk_track_search).  0: off; 1..256: per (keypoint, target)
    // pair an integer displacement within that many pixels is found by block matching, LK runs once more from it, and the row
    // with the smaller patch error stays -- flow rows that survive fast pans and the long skips (Blender's tracker calls the
    // search its prepass).  Not together with normalize.
    int search_radius = 0;
    // not in the reference: masked windows (include/polychase_hip.h: pc_lk_track_window_masked).  true: the template pixels of an
    // LK window that lie outside the detection mask of the window's frame carry no weight (Blender's use_mask), so keypoints near
    // the outline of a matted object follow the object and not the layer behind it.  Like target_mask_margin it makes every frame
    // take its mask, and it does nothing without a detection_mask.  Not together with normalize, affine_refinement, search_radius
    // or min_correlation, which do not weight their windows.
    bool mask_windows = false;
    // not in the reference: gray conversion (include/polychase_hip.h: pc_gray_conversion).  channel_weights: nothing = the
    // reference's RGB2GRAY; (r, g, b), finite, >= 0, not all zero = the weights of the three channels in the gray plane that is
    // detected and tracked (Blender's tracker has R / G / B switches), for u8 and float frames.  float_transfer: "none" = float
    // frames through the addon's `(x * 255).astype(uint8)`; "srgb" / "gamma" = scene-linear float frames through the sRGB curve or
    // pow(y, 1 / float_transfer_gamma), 1 <= gamma <= 4, after float_exposure stops (|v| <= 16) of gain; nothing for u8 frames.
    std::optional<std::array<double, 3>> channel_weights;
    std::string float_transfer = "none";
    double float_transfer_gamma = 2.2;
    double float_exposure = 0.0;
    // not in the reference: lens undistortion at ingest (include/polychase_hip.h: pc_context_set_lens_map).  Either a polynomial
    // model, from which the run builds the map at the clip's size, or a ready-made map of the clip's size (an STmap of an
    // anamorphic or fisheye lens); nothing = frames are taken as pinhole.  Every frame is resampled into the undistorted camera as
    // it is put, AFTER its gray conversion: keypoints, flow rows and a caller's detection_mask are all in undistorted pixel
    // coordinates, and the database must not be resumed under another lens.  Without a detection_mask of the caller the run masks
    // the detection where the map leaves the original frame (pc_lens_map_valid eroded by window_size / 2 + 1), when any pixel does.
    std::optional<LensModel> lens_model;
    std::shared_ptr<const LensMapData> lens_map;
};
// std::invalid_argument for what no run accepts; every entry point calls it before it asks for a frame
inline void CheckOpticalFlowOptions(const OpticalFlowOptions& o) {
    if (o.target_mask_margin < -1 || o.target_mask_margin > 31)
        throw std::invalid_argument("target_mask_margin must be -1 (off) or 0..31, got " + std::to_string(o.target_mask_margin));
    if (!(o.min_correlation >= 0.0 && o.min_correlation <= 1.0))   // a NaN fails
        throw std::invalid_argument("min_correlation must be in [0, 1] (0 = off), got " + std::to_string(o.min_correlation));
    if (o.search_radius < 0 || o.search_radius > 256)
        throw std::invalid_argument("search_radius must be 0 (off) or 1..256, got " + std::to_string(o.search_radius));
    if (o.search_radius > 0 && o.normalize)
        throw std::invalid_argument("search_radius assumes brightness constancy: it cannot be combined with normalize");
    if (o.mask_windows && (o.normalize || o.affine_refinement || o.search_radius > 0 || o.min_correlation > 0.0))
        throw std::invalid_argument("mask_windows cannot be combined with normalize, affine_refinement, search_radius or min_correlation: they do not weight their windows");
    if (o.affine_refinement && o.normalize)
        throw std::invalid_argument("affine_refinement assumes brightness constancy: it cannot be combined with normalize");
    if (o.channel_weights) {
        const auto& w = *o.channel_weights;
        for (double c : w)
            if (!(std::isfinite(c) && c >= 0.0))
                throw std::invalid_argument("channel_weights must be finite and >= 0, got " + std::to_string(c));
        const double s = w[0] + w[1] + w[2];
        if (!(s > 0.0 && std::isfinite(s))) throw std::invalid_argument("channel_weights must have a positive, finite sum");
    }
    if (o.lens_model && o.lens_map) throw std::invalid_argument("lens: a model or a map, not both");
    if (o.lens_model) {
        const LensModel& m = *o.lens_model;
        for (double v : {m.fx, m.fy, m.cx, m.cy, m.k1, m.k2, m.k3, m.p1, m.p2, m.zoom})
            if (!std::isfinite(v)) throw std::invalid_argument("lens model values must be finite, got " + std::to_string(v));
        if (!(m.fx > 0.0 && m.fy > 0.0 && m.zoom > 0.0)) throw std::invalid_argument("lens model: fx, fy and zoom must be > 0");
    }
    if (o.lens_map) {
        const LensMapData& m = *o.lens_map;
        if (m.width < 1 || m.height < 1 || m.q.size() != static_cast<size_t>(m.width) * static_cast<size_t>(m.height) * 2)
            throw std::invalid_argument("lens map must be int32 of shape (H, W, 2)");
    }
    if (o.float_transfer != "none" && o.float_transfer != "srgb" && o.float_transfer != "gamma")
        throw std::invalid_argument("float_transfer must be \"none\", \"srgb\" or \"gamma\", got \"" + o.float_transfer + "\"");
    if (!(o.float_transfer_gamma >= 1.0 && o.float_transfer_gamma <= 4.0))   // a NaN fails
        throw std::invalid_argument("float_transfer_gamma must be in [1, 4], got " + std::to_string(o.float_transfer_gamma));
    if (!(std::fabs(o.float_exposure) <= 16.0))
        throw std::invalid_argument("float_exposure must be in [-16, 16] stops, got " + std::to_string(o.float_exposure));
}

// The clip: frames first_frame .. first_frame + num_frames - 1, all width x height.
struct VideoInfo {
    uint32_t width;
    uint32_t height;
    int32_t first_frame;
    uint32_t num_frames;
};

// ---- frame hand-off ----------------------------------------------------------------------------

// One RGB frame, rows x cols x 3 uint8.  `data` is host memory, or HIP device memory of the GPU in
// use when on_device is set (zero-copy ingestion); `owner` keeps it alive while the frame is read.
struct FrameView {
    const uint8_t* data = nullptr;
    int rows = 0;
    int cols = 0;
    int channels = 0;
    int elem_size = 1;     // 1: uint8 (channels == 3); 4: float32 as Blender hands frames out (channels 3 or 4),
                           // converted on the GPU like the addon's `(image * 255).astype(np.uint8)`
    int pixel_type = -1;   // pc_pixel_type; -1: what elem_size says (uint8 or float32).  uint16 and float16 frames (elem_size 2,
                           // channels 3 or 4) and uint8 frames with 4 channels are converted on the GPU by the rules of
                           // pc_frame_set_pixels
    int PixelType() const { return pixel_type >= 0 ? pixel_type : (elem_size == 4 ? 3 : 0); }
    size_t row_pitch = 0;  // bytes between rows
    bool on_device = false;
    bool pinned_host = false;   // with on_device: `data` is page-locked host memory (frame_pool.h) -> PC_FRAME_PINNED_HOST
    std::shared_ptr<void> owner;
};

// ---- detection mask (not in the reference's Python surface; its detector has it: cpp/feature_detection/gftt.cc:14-86) ------
// rows x cols uint8, non-zero = keypoints may be detected here; the semantics are the reference's `mask` argument
// (include/polychase_hip.h: pc_frame_set_mask), not a filter on the unmasked keypoints.  `data` is host memory (consumed when
// the mask is handed to the engine) or HIP device memory of the GPU in use (on_device; `owner` keeps it alive while it is read).
// Or outlines instead of bytes (`polygons` set; the other fields unused): closed polygons in pixel coordinates, rasterised on the
// GPU by the exact fill rule of include/polychase_hip.h: pc_frame_set_mask_polygons -- a few hundred bytes per frame instead of a
// plane, so a mask that moves with every frame keeps pace.  Holes are not expressible.
struct PolygonMaskData {
    std::vector<float> xy;          // x, y of every vertex, polygon after polygon
    std::vector<int32_t> counts;    // vertices per polygon
    bool invert = false;
};
// Or a mesh under a pose (`mesh` set; the other fields unused): the silhouette pc_mesh_render draws for `cam` at the clip's size,
// on the mesh's own context, into a device plane of the run -- so the frame's mask is on where a keypoint's ray (RayCast, the
// tracker) would hit the mesh (invert: where it would not), `margin` pixels inside.  No plane crosses the bus.  The mesh lives on
// the GPU of its context: a run on another device refuses the mask (std::invalid_argument) before any GPU work.
struct MeshMaskData {
    std::shared_ptr<const void> owner;     // keeps the mesh behind `gpu` alive
    const pc_mesh* gpu = nullptr;
    pc_context* ctx = nullptr;             // the context the mesh was created in
    int device = 0;                        // ... and its HIP device
    pc_ray_camera cam{};
    bool check_mask = true;
    bool invert = false;
    int margin = 0;                        // 0..PC_TARGET_MASK_MAX_MARGIN
    std::function<void()> sync_mask;       // sends the mesh's current masked_triangles (check_mask), or empty
                                           // (called on the run's thread: the bits must not be edited while a run uses the mesh)
};
struct MaskView {
    std::shared_ptr<const PolygonMaskData> polygons;
    std::shared_ptr<const MeshMaskData> mesh;
    const uint8_t* data = nullptr;
    int rows = 0;
    int cols = 0;
    size_t row_pitch = 0;  // bytes between rows
    bool on_device = false;
    std::shared_ptr<void> owner;
};
// Either one mask for every frame the run detects (`fixed`), or a function asked once per such frame (`per_frame`; nothing =
// that frame is detected without a mask); empty = no mask.  Asked only for frames that WILL be detected: not for the halo
// frames of a shard, and not for frames whose `keypoints` row exists -- a resumed run keeps the stored keypoints whatever mask
// is passed.  With OpticalFlowOptions::target_mask_margin >= 0 the mask also judges the rows that END in a frame, so per_frame
// is then asked once for EVERY frame the run puts, in order -- halo frames and frames with stored keypoints included (their
// detection, if any, still runs without it) -- and nothing = rows into that frame are all kept.  A resumed run keeps the flow
// rows already stored, whatever margin they were made under.  The mask is not stored in the database.  A mask of another size
// than the clip: std::invalid_argument.
struct DetectionMask {
    std::optional<MaskView> fixed;
    std::function<std::optional<MaskView>(int32_t frame_id)> per_frame;
    int mesh_device = -1;   // >= 0: per_frame may answer with meshes of this device (a run on another refuses before any GPU work)
    bool empty() const { return !fixed && !per_frame; }
};

// Returns the frame with the given id, or nothing if it cannot be supplied.
using FrameAccessorFunction = std::function<std::optional<FrameView>(int32_t frame_id)>;
// (progress in [0,1], message); returning false cancels the run.
using OpticalFlowProgressCallback = std::function<bool(float progress, const std::string& progress_message)>;

// What one run did (not in the reference; used by bench / tests).
struct OpticalFlowRunStats {
    int frames_processed = 0;
    int keypoint_rows_written = 0;
    int flow_rows_written = 0;
    double seconds_total = 0;
    double seconds_db = 0;
    // where the driver's thread spent the call (the stage clock of tools/e2e_bench.py)
    double seconds_setup = 0;        // database open, context + analyzer creation (before the first frame is asked for)
    double seconds_accessor = 0;     // inside frame_accessor (Python: the GIL, the copy into a pinned buffer)
    double seconds_put = 0;          // pc_analyzer_put_frame* (enqueue of the frame's preparation)
    double seconds_submit = 0;       // pc_analyzer_submit (keypoint count of frame1 + enqueue of its job)
    double seconds_collect = 0;      // pc_analyzer_collect (waiting for the GPU)
    double seconds_writer_wait = 0;  // RecordWriter::Enqueue / Flush (waiting for SQLite)
    double seconds_callback = 0;     // progress callback + database look-ups of the loop
    bool engine_reused = false;      // the call took the process's parked engine (context + analyzer) instead of creating one
};

// ---- entry point -------------------------------------------------------------------------------

// Detects keypoints in every frame and tracks them into the frames at distance 1, 2, 4 and 8 on
// both sides, storing `keypoints` and `optical_flow` rows in the SQLite file at database_path
// (created if missing; existing rows are kept and not recomputed, so an interrupted run resumes).
// An empty database_path produces the records without storing them.  write_images: the reference's debug dump
// (opticalflow.cc:80-96): <directory of the database>/frames/%06d.png and keypoints_%06d.png of every frame1.
void GenerateOpticalFlowDatabase(const VideoInfo& video_info, FrameAccessorFunction frame_accessor,
                                 OpticalFlowProgressCallback callback, const std::string& database_path,
                                 const GFTTOptions& detector_options = {}, const OpticalFlowOptions& flow_options = {},
                                 bool write_images = false, OpticalFlowRunStats* stats = nullptr,
                                 const DetectionMask& detection_mask = {});

// Frees the idle engine a finished run has parked for the next one (GPU memory of ~20 resident frames; analysis_driver.cc:
// EngineCache).  POLYCHASE_ENGINE_CACHE=0 disables the parking altogether.
void ReleaseCachedEngine();
// testing aid: true while the idle timer of a parked engine exists (a thread that lives only as long as an engine is parked)
bool EngineCacheTimerRunning();

// ---- multi-GPU analysis (one process per GPU, frame1 ranges sharded, RCCL only for the stitch) ----------

// One shard of the clip: the frame1 loop of GenerateOpticalFlowDatabase (cpp/opticalflow.cc:237-316) for
// frame1 in [begin, end) only.  Frames up to 8 outside the shard are requested from the accessor as tracking targets
// (gray + pyramid, no detection); pairs are clipped to the clip of `video_info`, so the records do not depend on how
// the clip is cut.  Where the records go:
//   * database_path non-empty: into the SQLite file, exactly like GenerateOpticalFlowDatabase (the rank that owns the
//     file runs its own shard this way: the inserts overlap the analysis);
//   * device_log non-null: every frame1's record (keypoints + the status == 1 rows of its pairs) is appended on the
//     GPU to `device_log` (HIP device memory of the GPU in use, 16-byte aligned) in the analyzer's log format
//     (include/polychase_hip.h, pc_analyzer_set_device_log) -- the bytes the ranks exchange over RCCL.
// The log buffer is used as `log_buffers` equal parts that are filled in turn, one PIECE each: a piece ends after
// `piece_frames` frame1s (0: never) or when the next record does not fit the part.  on_piece is called on the
// driver's thread when all records of a piece are complete in device memory; the part may be overwritten as soon as
// the call returns (with two parts the analysis of the next piece runs meanwhile).  Memory is therefore bounded by the
// buffer, whatever the length of the clip.
struct OpticalFlowShard {
    int32_t begin = 0, end = 0;
    void* device_log = nullptr;
    size_t capacity_bytes = 0;
    int log_buffers = 1;
    int piece_frames = 0;
    std::function<void(int piece, size_t offset_bytes, size_t bytes, int32_t first_frame1, int n_frames)> on_piece;
    bool host_records = true;   // false (and no database): the records are not downloaded to host memory as well
    int device = -1;            // HIP device of the run; -1: $POLYCHASE_DEVICE, else 0
    // results
    size_t used_bytes = 0;      // bytes of the last piece (a run with one piece: of the run)
    int pieces = 0;
    bool cancelled = false;     // the progress callback returned false: the records end early
};
void GenerateOpticalFlowShard(const VideoInfo& video_info, FrameAccessorFunction frame_accessor, OpticalFlowProgressCallback callback,
                              const std::string& database_path, OpticalFlowShard& shard, const GFTTOptions& detector_options = {},
                              const OpticalFlowOptions& flow_options = {}, OpticalFlowRunStats* stats = nullptr,
                              const DetectionMask& detection_mask = {});
// The same with ONE piece in a buffer of capacity_bytes and nothing stored.  Returns the bytes used; throws
// ("device log full") when the log is too small.
size_t GenerateOpticalFlowRecords(const VideoInfo& video_info, FrameAccessorFunction frame_accessor,
                                  OpticalFlowProgressCallback callback, int32_t shard_begin, int32_t shard_end,
                                  void* device_log, size_t capacity_bytes, const GFTTOptions& detector_options = {},
                                  const OpticalFlowOptions& flow_options = {}, OpticalFlowRunStats* stats = nullptr,
                                  const DetectionMask& detection_mask = {});

// Stores a record log (host copy, e.g. one rank's part of the all-gather) in the database: per record one transaction
// with the `keypoints` row and its `optical_flow` rows, rows that exist are kept (opticalflow.cc:168-178, :286) --
// the statements of the single-process run in the same order, so logs written in frame order give the same file.
// A `keypoints` row that exists must hold the record's keypoints (else: std::runtime_error, nothing of the record stored).
void WriteOpticalFlowRecords(const std::string& database_path, const uint8_t* log, size_t bytes,
                             OpticalFlowRunStats* stats = nullptr);
// The same for a sequence of logs (the pieces rank 0 receives): one connection, rows loaded under a rollback journal
// like GenerateOpticalFlowDatabase's own inserts, the file back in WAL mode when the writer is closed or destroyed.
class OpticalFlowRecordWriter {
   public:
    explicit OpticalFlowRecordWriter(const std::string& database_path);
    ~OpticalFlowRecordWriter();
    void Write(const uint8_t* log, size_t bytes, OpticalFlowRunStats* stats = nullptr);
    void Close();

   private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};
