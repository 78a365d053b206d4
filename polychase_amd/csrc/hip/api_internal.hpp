// api_internal.hpp -- helpers shared by the C-ABI translation units (api.hip, api_lk.hip, api_analyzer.hip, api_tracker.hip).
#pragma once

#include <chrono>
#include <ratio>

#include "internal.hpp"

namespace pc_api {

// HIP-event timing of one kernel class on one stream (pc_context_enable_timing)
struct ScopedTimer {
    pc_context* c;
    int cls;
    Event a, b;
    hipStream_t s = nullptr;
    ScopedTimer(pc_context* ctx, int k, hipStream_t on = nullptr) : c(ctx), cls(k), s(on ? on : ctx->work) {
        if (!(c->timing_mask & (1u << k))) return;
        auto get = [&]() {
            Event e;
            if (!c->event_pool.empty()) {
                e = std::move(c->event_pool.back());
                c->event_pool.pop_back();
            } else {
                (void)e.create();
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
        c->ranges.push_back({cls, std::move(a), std::move(b)});
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
// --- the LK stage (api_lk.hip) ---
// argument checks of the stage calls and of the analyzer's setters, each refusing with the message the C ABI documents:
// normalize and affine 0 or 1, search_radius 0 .. 256, affine and search not together with normalize, 0 <= min_correlation <= 1,
// fb_threshold finite and >= 0, margin -1 (only with allow_off) .. 31
int check_lk_args(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                  const pc_flow_options* opt);
int check_normalize(int normalize);
int check_fb_threshold(double fb_threshold);
int check_search_radius(int search_radius, int normalize);
int check_affine(int affine, int normalize);
int check_min_correlation(double min_correlation);
int check_target_margin(int margin, bool allow_off);
// mask_windows 0 or 1, and 1 not together with normalize, affine, a search radius or a minimum correlation
int check_mask_windows(int mask_windows, int normalize, int affine, int search_radius, double min_correlation);
// What follows the forward launch of an LK job (include/polychase_hip.h: pc_lk_track_search and the entry points before it).
// Value-initialised: the forward launch only.  The side arrays are device memory, [target][n], null where nobody asks.
struct LkPasses {
    int search_radius;          // > 0: the search prepass
    int affine;                 // 1: the affine refinement
    int normalize;              // 1: the brightness-normalised forward and backward kernels
    double min_correlation;     // > 0: rows that correlate below it are dropped
    double fb_threshold;        // > 0: the forward-backward check
    const uint8_t* plane[PC_MAX_TARGETS];   // target-side mask of target t (choked by the caller), null: it keeps its rows
    float4* affine_m;           // the refinement's matrices and states
    uint8_t* affine_state;
    float* corr;                // the correlation scores: the pass then runs whatever min_correlation
    float2* back_xy;            // the backward end points and status
    uint8_t* back_status;
    // 1: the masked windows.  weights_f1 / weights_tgt[t]: that frame has weight planes (pc_frame::wt, ready in stream order when
    // the job starts) -- frame1's weight the forward windows, a target's those of its backward pass; touched: which keypoints the
    // forward weights touched, [n] (zeroed by the job), or null
    int mask_windows;
    bool weights_f1;
    bool weights_tgt[PC_MAX_TARGETS];
    uint8_t* touched;
};
// Enqueues a whole job on `lane` (one of pc_context::lanes; the stage calls: lanes[0]): the forward launch and the passes, in the
// one order they have.  Afterwards the lane's rec / slot_of hold the records and the inverse visiting order, and with a search
// radius its search_d / search_state the displacements and states.  gate_value: what the forward launch stores into the
// context's gate (LkGate::wait_and_next), 0: not gated.  The arguments have passed the checks above
int run_lk_job(pc_context* ctx, LkLane& lane, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
               const pc_flow_options* opt, const LkPasses& passes, uint32_t gate_value = 0);
// Compacts the records run_lk_job left on `lane` (status filter; kernels.hpp launch_compact) into the four arrays, on the lane's stream
int compact_lane(pc_context* ctx, LkLane& lane, int n, int n_targets, long long* row_offset, uint32_t* src_indices, float2* tgt_xy, float* err);
// target-side masks: ensure_choked_plane allocates pc_frame::d_choked (once)
int ensure_choked_plane(pc_frame* f);
// masked windows: the weight planes (pc_frame::wt) of the mask in the frame's plane, allocated the first time
// (alloc_window_weights, which also sets the padding, on stream `s`) and made on stream `s` unless they are those of that mask
// (make_window_weights; an analyzer's frame holds its mask as a target whether or not its detection reads it).
// ensure_window_weights: the same for a frame of the stage calls, PC_E_STATE when it has no mask on
int alloc_window_weights(pc_frame* f, hipStream_t s);
int make_window_weights(pc_frame* f, hipStream_t s);
int ensure_window_weights(pc_frame* f, hipStream_t s);
// gray (+ pyramid) of a frame from pixels of `pixel_type` (pc_pixel_type) with `channels` channels, host or device, on the work
// stream; the legal pairs are those of pc_frame_set_pixels, which check_pixels tests together with the alignment of pointer
// and pitch (PC_OK, or PC_E_INVALID with the error set; nothing is enqueued)
// `clear` (may be null): clear_words words zeroed in front of the frame's kernels (by the level-0 kernel where there is one)
int check_pixels(const void* src, size_t row_pitch, int pixel_type, int channels);
int set_image(pc_context* ctx, pc_frame* f, const uint8_t* src, size_t row_pitch, int on_device, int channels, int pixel_type = PC_PIXEL_U8,
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
