// api_internal.hpp -- helpers shared by the C-ABI translation units (api.hip, api_analyzer.hip, api_tracker.hip).
#pragma once

#include <chrono>
#include <ratio>

#include "internal.hpp"

namespace pc_api {

// HIP-event timing of one kernel class on one stream (pc_context_enable_timing)
struct ScopedTimer {
    pc_context* c;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s = nullptr;
    ScopedTimer(pc_context* ctx, int k, hipStream_t on = nullptr) : c(ctx), cls(k), s(on ? on : ctx->work) {
        if (!(c->timing_mask & (1u << k))) return;
        auto get = [&]() {
            hipEvent_t e = nullptr;
            if (!c->event_pool.empty()) {
                e = c->event_pool.back();
                c->event_pool.pop_back();
            } else {
                (void)hipEventCreate(&e);
            }
            return e;
        };
        a = get();
        b = get();
        (void)hipEventRecord(a, s);
    }
    ~ScopedTimer() {
        if (!a) return;
        (void)hipEventRecord(b, s);
        c->ranges.push_back({cls, a, b});
    }
};

// image / detection helpers enqueue on prep_stream while one of these is alive
struct PrepScope {
    pc_context* c;
    explicit PrepScope(pc_context* ctx) : c(ctx) {
        c->work = c->prep_stream;
        c->prep_dirty = true;
    }
    ~PrepScope() { c->work = c->stream; }
};

// POLYCHASE_TRACE_ALLOC: report host-side sections of a call that take more than 2 ms
struct SlowSection {
    const char* name;
    std::chrono::steady_clock::time_point t0;
    explicit SlowSection(const char* n) : name(n), t0(std::chrono::steady_clock::now()) {}
    ~SlowSection() {
        if (!pc::trace_allocations()) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > 2.0) fprintf(stderr, "[polychase_hip] slow host section %s: %.2f ms\n", name, ms);
    }
};

int collect_timing(pc_context* c);
int ensure_kp_capacity(pc_frame* f, int n);
int validate_gftt(const pc_gftt_options* opt, int w, int h, pc::GfttGrid* g);
// GoodFeaturesToTrack (internal.hpp DetectScratch): everything enqueued on the current work stream / the count on the host
int detect_reserve(pc_context* ctx, int w, int h, DetectScratch& d, const pc_gftt_options* opt = nullptr);   // opt: also the fused chain's buffers
int detect_enqueue(pc_context* ctx, pc_frame* f, const pc::GfttGrid& grid, const pc_gftt_options& opt, DetectScratch& d,
                   DevBuf<uint32_t>& hist, bool full_launch = false);
// *redone (may be null): the frame took the slow path, its keypoints were written again just now
int detect_finish(pc_context* ctx, pc_frame* f, const pc::GfttGrid& grid, const pc_gftt_options& opt, DetectScratch& d,
                  DevBuf<uint32_t>& hist, bool* redone = nullptr);
// orders `stream` behind everything queued on the side streams so far
int join_prep(pc_context* ctx);
int order_keypoints_spatially(pc_context* ctx, pc_frame* f, DevBuf<uint32_t>& hist);
int check_lk_args(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                  const pc_flow_options* opt);
// LK launch into output set `set` on job lane `set` (0: the context's main stream); normalize (check_normalize: 0 or 1): the
// brightness-normalised kernels (include/polychase_hip.h: pc_lk_track_normalized) instead, here and in run_lk_fb
int check_normalize(int normalize);
int run_lk(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets, const pc_flow_options* opt,
           int set = 0, int normalize = 0);
// forward-backward check on the records run_lk has just left in set `set`, on the same lane (fb_threshold > 0);
// back_xy / back_status: device arrays [n_targets][n] or null
int check_fb_threshold(double fb_threshold);
// search: run_lk_search has run on the set; the rows it replaced are tracked back by a launch of their own (timed under PC_K_LK_FB too)
int run_lk_fb(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets, const pc_flow_options* opt,
              double fb_threshold, int set = 0, float2* back_xy = nullptr, uint8_t* back_status = nullptr, int normalize = 0,
              bool search = false);
// search prepass (include/polychase_hip.h: pc_lk_track_search) on the records run_lk has just left in set `set`, on the same lane,
// before run_lk_affine and everything after it.  check_search_radius: 0 .. 256, and > 0 not together with normalize.  The
// displacements and states stay in pc_context::lk_search_d / lk_search_state of the set, [target][n], for run_lk_fb
int check_search_radius(int search_radius, int normalize);
int run_lk_search(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets, const pc_flow_options* opt,
                  int search_radius, int set = 0);
// affine refinement (include/polychase_hip.h: pc_lk_track_affine) of the records run_lk has just left in set `set`, on the same
// lane, before run_lk_target_mask, run_lk_corr and run_lk_fb, which then judge the refined end points.  check_affine: 0 or 1, and
// not together with normalize; affine_m / affine_state: device arrays [target][n], zeroed by the caller, or null
int check_affine(int affine, int normalize);
int run_lk_affine(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets, const pc_flow_options* opt,
                  int set = 0, float4* affine_m = nullptr, uint8_t* affine_state = nullptr);
// minimum correlation (include/polychase_hip.h: pc_lk_track_correlated) on the records run_lk has just left in set `set`, on the
// same lane, between run_lk_target_mask and run_lk_fb.  check_min_correlation: 0 <= v <= 1; run_lk_corr drops the rows below
// min_correlation (0: none) and, with `corr` (device, [target][n]), writes the scores
int check_min_correlation(double min_correlation);
int run_lk_corr(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets, double min_correlation, int set = 0,
                float* corr = nullptr);
// target-side masks (include/polychase_hip.h: pc_lk_track_masked).  check_target_margin: -1 (only with allow_off) .. 31;
// ensure_choked_plane allocates pc_frame::d_choked (once); run_lk_target_mask drops, on the lane of set `set`, the records
// run_lk has just left there that end where the plane of their target is off (plane[t] null: target t keeps its rows; all null:
// nothing is enqueued)
int check_target_margin(int margin, bool allow_off);
int ensure_choked_plane(pc_frame* f);
int run_lk_target_mask(pc_context* ctx, const pc_frame* frame1, const uint8_t* const* plane, int n_targets, int set = 0);
// gray (+ pyramid) of a frame from u8 gray / u8 RGB / float32 RGB(A) pixels, host or device, on the work stream
// `clear` (may be null): clear_words words zeroed in front of the frame's kernels (by the level-0 kernel where there is one)
int set_image(pc_context* ctx, pc_frame* f, const uint8_t* src, size_t row_pitch, int on_device, int channels, int elem_size = 1,
              uint32_t* clear = nullptr, int clear_words = 0);
int detect_counter_words(const DetectScratch& d);   // words of DetectScratch::counters a detection expects zeroed
// detection mask of a frame: ensure_mask_plane allocates pc_frame::d_mask (w * h bytes, once); upload_mask copies `mask`
// (host or device memory, rows row_pitch apart) into it on stream `s`, stream-ordered, and switches the mask on
int ensure_mask_plane(pc_frame* f);
int upload_mask(pc_frame* f, const uint8_t* mask, size_t row_pitch, int on_device, hipStream_t s);
// polygon mask (pc_frame_set_mask_polygons): check_polygons refuses what the header lists and returns the vertex count;
// snap_polygons writes the checked polygons in the layout of pc::launch_polygon_mask (kernels.hpp) and returns the words used;
// fill_mask_polygons rasterises that layout, now in device memory, into the frame's plane on stream `s` and switches the mask on
int check_polygons(const float* xy, const int32_t* counts, int n_polygons, int* n_vertices);
size_t snap_polygons(const float* xy, const int32_t* counts, int n_polygons, int32_t* out);
int fill_mask_polygons(pc_frame* f, const int32_t* d_poly, int n_vertices, int n_polygons, int invert, hipStream_t s);

}  // namespace pc_api
