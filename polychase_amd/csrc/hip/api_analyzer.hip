// api_analyzer.hip -- pc_analyzer: the pipelined per-clip engine behind GenerateOpticalFlowDatabase
// (reference cpp/opticalflow.cc:209-321).  See include/polychase_hip.h for the contract and DESIGN.md section 3
// for the stream / event structure.
#include "api_internal.hpp"

using namespace pc_api;

// =============================================================================================
// analyzer: pipelined per-clip engine (see include/polychase_hip.h)
// =============================================================================================

namespace {

constexpr int kSpareSlots = PC_ANALYZER_SPARE_SLOTS;

enum DetState { DET_NONE = 0, DET_ENQUEUED = 2, DET_DONE = 3 };   // detection enqueued / keypoint count on the host

struct Slot {
    pc_frame* frame = nullptr;
    int32_t frame_id = 0;
    bool valid = false;
    DetState det = DET_NONE;
    bool supplied = false;  // keypoints came from the caller (database), not from detection
    // not owned (pc_analyzer::lk_done), per job lane: `lk_done` of the latest job whose LK reads this slot
    hipEvent_t last_read[2] = {nullptr, nullptr};
    Event img_ready;   // gray + pyramid of the resident frame are complete (prep stream)
    Event kps_ready;   // keypoints + visiting order are complete (prep stream)
    DetectScratch scratch;
};

struct Job {
    int32_t frame1 = 0;
    int n_kps = 0;
    bool detected = false;
    int n_targets = 0;
    int32_t targets[PC_MAX_TARGETS];
    Event done;               // records of this job are in pinned memory (the job's lane)
    PinBuf<uint8_t> h_pack;   // the job's records, a copy of its lane's pack
    pc::RecordLayout layout;  // ... of both
    bool host_records = true;       // the whole pack was downloaded (else its row offsets only)
};

// the resident slots a job reads
struct JobSlots {
    Slot* frame1 = nullptr;
    int n_targets = 0;
    Slot* target[PC_MAX_TARGETS];
    const pc_frame* target_frame[PC_MAX_TARGETS];   // the same as run_lk_job takes them
};

// Issue priority of the helper kernels this analyzer enqueues (common.hpp: helper_priority), from what it observes.
// The preparation stream is a FIFO: pyramid of frame f+9, then its detection.  When that chain falls behind the LK
// launches -- the pyramid of the SECOND newest frame is not complete when a job is collected, i.e. less than one frame of
// slack is left before a launch has to wait for it -- the helpers get the high priority; when no lag has been seen for
// kCalm collects in a row (and it takes kLagsToRaise lags among 16 collects to raise it) they go back to filling the slots LK leaves (the better mode whenever they keep up).
// POLYCHASE_HELPER_PRIO=0 / 1 pins the priority, "auto" (default) is this controller.
struct HelperPriorityControl {
    static constexpr int kCalm = 48;        // collects without a lag before the priority is dropped again
    static constexpr int kLagsToRaise = 3;  // ... of the last 16 collects (one late pyramid at a clip's start is no trend)
    int mode = -1;          // -1 auto, 0 / 1 pinned
    int hi = 0;
    int calm = 0;
    uint32_t window = 0;    // the last 16 observations, newest in bit 0
    uint64_t lag_seen = 0, switched_on = 0;
    void init() {
        const char* v = getenv("POLYCHASE_HELPER_PRIO");
        mode = (v && (v[0] == '0' || v[0] == '1') && v[1] == 0) ? v[0] - '0' : -1;
        hi = mode == 1 ? 1 : 0;
    }
    void observe(bool lagging) {
        if (mode >= 0) return;
        window = ((window << 1) | (lagging ? 1u : 0u)) & 0xffffu;
        if (lagging) {
            lag_seen++;
            calm = 0;
            if (!hi && __builtin_popcount(window) >= kLagsToRaise) {
                hi = 1;
                switched_on++;
            }
        } else if (hi && ++calm >= kCalm) {
            hi = 0;
            calm = 0;
            window = 0;
        }
    }
};
struct HelperPriorityScope {   // the enqueues of one analyzer call carry its priority; stage-level calls on this thread stay at 0
    explicit HelperPriorityScope(int hi) { pc::set_helper_prio(hi); }
    ~HelperPriorityScope() { pc::set_helper_prio(0); }
};

}  // namespace

struct pc_analyzer {
    pc_context* ctx = nullptr;
    int w = 0, h = 0;
    pc_gftt_options gopt;
    pc_flow_options fopt;
    pc::GfttGrid grid;
    std::vector<Slot> slots;
    std::vector<Job> jobs;
    size_t job_head = 0, job_count = 0;  // ring of in-flight jobs
    uint64_t submitted = 0;              // jobs submitted so far
    // POLYCHASE_LK_LANES=1 when the analyzer was created: every job on lane 0, i.e. no two LK launches in flight -- a launch's
    // start-to-end time is then its own duration (the recipe of tools/collect_profiles.sh under rocprofv3 and of bench.py's
    // roofline time base); the product runs two lanes
    bool one_lane = false;
    // "the LK launch of a job finished", per lane, handed out round-robin.  Slots remember the event of the last job
    // that read them; an event that has been re-recorded since marks a LATER launch of the same lane, which the
    // lane's stream order puts behind the remembered one -- waiting for it is still correct.
    static constexpr int kLaneEvents = 16;
    Event lk_done[2][kLaneEvents];
    // The lane (index into pc_context::lanes, Slot::last_read and lk_done) of the job submitted next -- job k runs on lane
    // k & 1 -- and, in *done, the lane's lk_done event that is this job's turn
    int next_lane(hipEvent_t* done) const {
        const int lane = one_lane ? 0 : (int)(submitted & 1);
        *done = lk_done[lane][(one_lane ? submitted : submitted >> 1) % kLaneEvents];
        return lane;
    }
    // a gated launch of THIS analyzer is ahead: the next one waits for its "all dispatched" signal (the context's LkGate)
    bool gate_armed = false;
    HelperPriorityControl prio;
    int32_t put_newest = 0, put_previous = 0;   // frame ids of the two most recent put_frame calls
    int puts = 0;
    bool host_records = true;            // download every job's records to pinned host memory
    double fb_threshold = 0.0;           // forward-backward check of the jobs submitted from now on (0: off)
    double min_correlation = 0.0;        // minimum correlation of the jobs submitted from now on (0: off)
    int normalize = 0;                   // brightness-normalised LK for the jobs submitted from now on (0: off)
    int search_radius = 0;               // search prepass of the jobs submitted from now on (0: off); submit refuses > 0 beside normalize
    int affine = 0;                      // affine refinement of the jobs submitted from now on (0: off); submit refuses 1 beside normalize
    // Target-side masks (pc_analyzer_set_target_mask_margin): -1 off, else the margin of the frames put from now on.  While it is
    // >= 0 and a mask is in force every frame put takes the mask -- pc_frame::target_margin is the frame's role as a target,
    // beside mask_on, which stays the detection's -- and with a margin > 0 its choked plane too.
    int target_margin = -1;
    // Masked windows (pc_analyzer_set_mask_windows) of the frames put and the jobs submitted from now on.  While it is on and a
    // mask is in force every frame put takes the mask and gets its weight planes: pc_frame::window_weights, beside mask_on.
    int mask_windows = 0;
    // Detection mask of the frames put from now on with will_detect (pc_analyzer_set_mask).  The mask a detection reads is the
    // plane of its own slot's frame, filled on the preparation stream when the frame is put: a detection already enqueued keeps
    // the mask it was enqueued with.  A host mask is copied at once into one of kMaskGens pinned buffers, used in turn, so that
    // the per-frame copies into the slots never wait for the host; mask_copied[g]: the latest copy out of buffer g is complete.
    static constexpr int kMaskGens = 4;
    int mask_kind = 0;                   // 0 none, 1 host (mask_host[mask_gen]), 2 device (mask_dev, mask_dev_pitch), 3 polygons (poly_dev[poly_gen])
    int mask_gen = 0;
    Event mask_copied[kMaskGens];
    PinBuf<uint8_t> mask_host[kMaskGens];
    const uint8_t* mask_dev = nullptr;   // not owned: the caller's memory
    size_t mask_dev_pitch = 0;
    // Polygon masks (pc_analyzer_set_mask_polygons): the snapped vertices are written into one of kMaskGens pinned buffers, used
    // in turn, and copied on the preparation stream into that buffer's device twin, which the frames' rasteriser launches read
    // on the same stream.  poly_read[g]: the latest copy out of poly_host[g] and the latest launch that read poly_dev[g] are
    // complete -- the host waits for it before it writes poly_host[g] again, kMaskGens masks later.
    int poly_gen = 0, poly_vertices = 0, poly_polygons = 0, poly_invert = 0;
    Event poly_read[kMaskGens];
    PinBuf<int32_t> poly_host[kMaskGens];
    DevBuf<int32_t> poly_dev[kMaskGens];
    uint8_t* d_log = nullptr;            // not owned (the caller's memory): optional device-resident record log
    size_t log_cap = 0, log_used = 0;
    std::vector<PinBuf<long long>> log_hdr;  // one pinned header per job slot
};

namespace {

Slot* find_slot(pc_analyzer* a, int32_t frame_id) {
    const int n = (int)a->slots.size();
    Slot& s = a->slots[(size_t)(((frame_id % n) + n) % n)];
    return (s.valid && s.frame_id == frame_id) ? &s : nullptr;
}

// detection of the slot's frame, enqueued on the prep stream in one go; `kps_ready` fires when keypoints and visiting
// order are complete
int detect_dense(pc_analyzer* a, Slot& s) {
    PrepScope prep(a->ctx);
    int rc = detect_enqueue(a->ctx, s.frame, a->grid, a->gopt, s.scratch, s.scratch.bin_hist);
    if (rc != PC_OK) return rc;
    PC_HIP(hipEventRecord(s.kps_ready, a->ctx->prep_stream));
    s.det = DET_ENQUEUED;
    s.supplied = false;
    return PC_OK;
}

// the keypoint count on the host (waits for the detection; a frame beyond the fast path's bounds is redone synchronously)
int detect_finish_slot(pc_analyzer* a, Slot& s) {
    int rc;
    if (s.det == DET_NONE && (rc = detect_dense(a, s)) != PC_OK) return rc;
    {
        PrepScope prep(a->ctx);
        bool redone = false;
        if ((rc = detect_finish(a->ctx, s.frame, a->grid, a->gopt, s.scratch, s.scratch.bin_hist, &redone)) != PC_OK) return rc;
        // Only then: recorded unconditionally the event would sit behind the detection of the frame that was made
        // resident a moment ago, and the LK launch of THIS frame1 would wait for it (rounds 1-2 did exactly that: the
        // "preparation chain" that bounded the step was this false dependency)
        if (redone) PC_HIP(hipEventRecord(s.kps_ready, a->ctx->prep_stream));
    }
    s.det = DET_DONE;
    return PC_OK;
}

}  // namespace

extern "C" {

int pc_analyzer_create(pc_context* ctx, int width, int height, const pc_gftt_options* gftt,
                       const pc_flow_options* flow, int ring_frames, int max_jobs, pc_analyzer** out) {
    if (!ctx || !gftt || !flow || !out) return fail(PC_E_INVALID, "null argument");
    *out = nullptr;
    if (ring_frames < 1 || ring_frames > 4096) return fail(PC_E_INVALID, "ring_frames must be in [1,4096]");
    if (max_jobs < 1 || max_jobs > 64) return fail(PC_E_INVALID, "max_jobs must be in [1,64]");
    pc::GfttGrid grid0;
    {
        int vrc = validate_gftt(gftt, width, height, &grid0);
        if (vrc != PC_OK) return vrc;
    }
    PC_HIP(hipSetDevice(ctx->device));
    // an early return destroys what exists so far (pc_analyzer_destroy)
    std::unique_ptr<pc_analyzer, void (*)(pc_analyzer*)> a(new (std::nothrow) pc_analyzer(), pc_analyzer_destroy);
    if (!a) return fail(PC_E_INVALID, "out of host memory");
    a->ctx = ctx;
    a->one_lane = getenv("POLYCHASE_LK_LANES") && atoi(getenv("POLYCHASE_LK_LANES")) == 1;
    a->w = width;
    a->h = height;
    a->gopt = *gftt;
    a->fopt = *flow;
    a->grid = grid0;
    a->prio.init();
    // spare slots: a frame can be overwritten (prep stream) while the LK launches that read its predecessors in the
    // ring are still running, without the streams waiting on each other, and the drivers make frame1 + 9 resident
    // one step before the first launch that reads it (PC_ANALYZER_LOOKAHEAD) so that its pyramid never sits on
    // the critical path of that launch
    a->slots.resize((size_t)ring_frames + kSpareSlots);
    a->jobs.resize((size_t)max_jobs);
    for (auto& s : a->slots) {
        if (int rc = pc_frame_create(ctx, width, height, flow->window_size, flow->max_level, &s.frame)) return rc;
        // room for a typical frame's keypoints up front: growing later frees device memory, which synchronises
        const int kp0 = std::max(16384, (width * height) / 16);   // candidates of a textured frame: ~1 per 23 px
        if (int rc = ensure_kp_capacity(s.frame, kp0)) return rc;
        PC_HIP(s.frame->d_perm.ensure((size_t)kp0 * 2, /*exact=*/true));
        s.frame->perm_cap = kp0;
        if (int rc = detect_reserve(ctx, width, height, s.scratch, &a->gopt)) return rc;
        PC_HIP(s.scratch.bin_hist.ensure((size_t)pc::bin_num_tiles(width, height) + 1));
        PC_HIP(s.img_ready.create(hipEventDisableTiming));
        PC_HIP(s.kps_ready.create(hipEventDisableTiming));
    }
    for (auto& j : a->jobs) PC_HIP(j.done.create(hipEventDisableTiming));
    for (auto& lane : a->lk_done)
        for (Event& e : lane) PC_HIP(e.create(hipEventDisableTiming));
    {
        // Warm the runtime's copy engines: it picks a free SDMA engine per copy and creates an engine's queue the first
        // time it is used (5-8 ms inside some hipMemcpyAsync, observed twice or three times in the first few dozen
        // frames).  A burst of overlapping downloads makes it create them now.
        const size_t chunk = (size_t)4 << 20, burst = 12;
        Job& j0 = a->jobs[0];
        for (LkLane& lane : ctx->lanes) PC_HIP(lane.pack.ensure(chunk));
        PC_HIP(j0.h_pack.ensure(chunk * burst));
        hipStream_t streams[3] = {ctx->lanes[1].stream, ctx->prep_stream, ctx->lanes[0].stream};
        for (int round = 0; round < 3; round++) {
            hipError_t e = hipSuccess;
            for (size_t k = 0; k < burst; k++) {
                const hipError_t ek = hipMemcpyAsync(j0.h_pack.p + k * chunk, ctx->lanes[k & 1].pack.p, chunk, hipMemcpyDeviceToHost, streams[k % 3]);
                if (e == hipSuccess) e = ek;
            }
            for (hipStream_t st : streams) (void)hipStreamSynchronize(st);
            if (e != hipSuccess) return fail(PC_E_HIP, "copy engine warm-up failed");
        }
    }
    *out = a.release();
    return PC_OK;
}

void pc_analyzer_destroy(pc_analyzer* a) {
    if (!a) return;
    (void)hipSetDevice(a->ctx->device);
    (void)a->ctx->sync_side_streams();
    (void)hipStreamSynchronize(a->ctx->stream);
    for (auto& s : a->slots)
        if (s.frame) pc_frame_destroy(s.frame);
    delete a;
}

int pc_analyzer_reset(pc_analyzer* a) {
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    if (a->job_count != 0) return fail(PC_E_STATE, "%zu jobs in flight: collect them first", a->job_count);
    PC_HIP(hipSetDevice(a->ctx->device));
    PC_HIP(a->ctx->sync_side_streams());
    PC_HIP(hipStreamSynchronize(a->ctx->stream));
    for (auto& s : a->slots) {
        s.valid = false;
        s.det = DET_NONE;
        s.supplied = false;
        s.frame_id = 0;
        s.last_read[0] = s.last_read[1] = nullptr;
        s.scratch.cleared = false;
        if (s.frame) {
            s.frame->mask_on = false;
            s.frame->target_margin = -1;
            s.frame->window_weights = false;
        }
    }
    a->mask_kind = 0;
    a->mask_dev = nullptr;
    a->job_head = 0;
    a->d_log = nullptr;
    a->log_cap = a->log_used = 0;
    a->host_records = true;
    a->put_newest = a->put_previous = 0;
    a->puts = 0;
    a->prio = HelperPriorityControl();
    a->prio.init();
    return PC_OK;
}

static int analyzer_put(pc_analyzer* a, int32_t frame_id, const uint8_t* rgb, size_t row_pitch, int on_device,
                        int will_detect, int channels, int pixel_type) {
    if (!a || !rgb) return fail(PC_E_INVALID, "null argument");
    const int n = (int)a->slots.size();
    Slot& s = a->slots[(size_t)(((frame_id % n) + n) % n)];
    PC_HIP(hipSetDevice(a->ctx->device));
    PrepScope prep(a->ctx);
    HelperPriorityScope prio_scope(a->prio.hi);
    a->put_previous = a->put_newest;
    a->put_newest = frame_id;
    a->puts++;
    // an LK launch in flight may still read the frame this slot holds
    for (hipEvent_t& e : s.last_read) {
        if (e) PC_HIP(hipStreamWaitEvent(a->ctx->prep_stream, e, 0));
        e = nullptr;
    }
    // (the detection of a frame that was never submitted as frame1 is in front of this on prep_stream)
    // the detection that follows expects its counters zeroed: the frame's first kernel does it on the way
    int rc = set_image(a->ctx, s.frame, rgb, row_pitch, on_device, channels, pixel_type, will_detect ? s.scratch.counters.p : nullptr,
                       detect_counter_words(s.scratch));
    s.scratch.cleared = rc == PC_OK && will_detect;
    if (rc != PC_OK) {
        s.valid = false;
        return rc;
    }
    // the mask of this frame's detection, into the slot's own plane, in front of img_ready: pc_analyzer_frame_ingested then
    // also says that a device mask has been read
    // With a target-side margin every frame takes the mask, as a target; its detection reads the plane as before: iff will_detect.
    // ... and so it does with the masked windows, whose planes follow the mask in front of img_ready
    const bool as_target = a->target_margin >= 0 && a->mask_kind != 0;
    const bool weighted = a->mask_windows == 1 && a->mask_kind != 0;
    const bool take_mask = will_detect || as_target || weighted;
    s.frame->mask_on = false;
    s.frame->target_margin = -1;
    s.frame->window_weights = false;
    if (take_mask && a->mask_kind == 1) {
        // TODO(mask-upload): a static mask is uploaded again for every detected frame (w * h bytes; measured -16 % on a whole
        // 1080p call for an all-on mask, DESIGN.md section 7 "Open follow-ups"): skip the copy when the slot's plane holds this mask
        const int g = a->mask_gen;
        if ((rc = upload_mask(s.frame, a->mask_host[g].p, (size_t)a->w, PC_FRAME_PINNED_HOST, a->ctx->prep_stream)) != PC_OK) return rc;
        PC_HIP(hipEventRecord(a->mask_copied[g], a->ctx->prep_stream));
    } else if (take_mask && a->mask_kind == 2) {
        if ((rc = upload_mask(s.frame, a->mask_dev, a->mask_dev_pitch, 1, a->ctx->prep_stream)) != PC_OK) return rc;
    } else if (take_mask && a->mask_kind == 3) {
        const int g = a->poly_gen;
        if ((rc = fill_mask_polygons(s.frame, a->poly_dev[g].p, a->poly_vertices, a->poly_polygons, a->poly_invert, a->ctx->prep_stream)) != PC_OK)
            return rc;
        PC_HIP(hipEventRecord(a->poly_read[g], a->ctx->prep_stream));
    }
    if (as_target) {
        s.frame->mask_on = will_detect != 0;
        if (a->target_margin > 0) {   // (the slot's choked plane exists: ensure_target_planes ran when margin and mask met)
            pc::launch_mask_choke(s.frame->d_mask.p, s.frame->d_choked.p, a->w, a->h, a->target_margin, a->ctx->prep_stream);
            PC_HIP(hipGetLastError());
        }
        s.frame->target_margin = a->target_margin;
    }
    if (weighted) {   // (the slot's weight planes exist: ensure_target_planes ran when switch and mask met)
        if ((rc = make_window_weights(s.frame, a->ctx->prep_stream)) != PC_OK) return rc;
        s.frame->mask_on = will_detect != 0;   // the detection's alone, as under a margin
        s.frame->window_weights = true;
    }
    PC_HIP(hipEventRecord(s.img_ready, a->ctx->prep_stream));
    s.frame_id = frame_id;
    s.valid = true;
    s.det = DET_NONE;
    s.supplied = false;
    if (will_detect) return detect_dense(a, s);
    return PC_OK;
}

int pc_analyzer_put_frame(pc_analyzer* a, int32_t frame_id, const uint8_t* rgb, size_t row_pitch, int on_device,
                          int will_detect) {
    return analyzer_put(a, frame_id, rgb, row_pitch, on_device, will_detect, 3, PC_PIXEL_U8);
}

int pc_analyzer_put_frame_f32(pc_analyzer* a, int32_t frame_id, const float* rgb, size_t row_pitch, int channels,
                              int on_device, int will_detect) {
    return analyzer_put(a, frame_id, reinterpret_cast<const uint8_t*>(rgb), row_pitch, on_device, will_detect, channels, PC_PIXEL_F32);
}

int pc_analyzer_put_frame_pixels(pc_analyzer* a, int32_t frame_id, const void* pixels, size_t row_pitch_bytes, int pixel_type, int channels,
                                 int on_device, int will_detect) {
    if (!a || !pixels) return fail(PC_E_INVALID, "null argument");
    // refused before the slot is touched: the ring stays as it was
    if (int crc = check_pixels(pixels, row_pitch_bytes, pixel_type, channels)) return crc;
    const size_t row_bytes = (size_t)a->w * channels * pc::pixel_type_bytes(pixel_type);
    if (row_pitch_bytes < row_bytes) return fail(PC_E_INVALID, "row_pitch %zu < %zu", row_pitch_bytes, row_bytes);
    return analyzer_put(a, frame_id, static_cast<const uint8_t*>(pixels), row_pitch_bytes, on_device, will_detect, channels, pixel_type);
}

int pc_analyzer_has_frame(const pc_analyzer* a, int32_t frame_id) {
    if (!a) return 0;
    return find_slot(const_cast<pc_analyzer*>(a), frame_id) != nullptr;
}

int pc_analyzer_frame_ingested(const pc_analyzer* a, int32_t frame_id) {
    if (!a) return 1;
    Slot* s = find_slot(const_cast<pc_analyzer*>(a), frame_id);
    if (!s || !s->img_ready) return 1;   // evicted: whatever read it was ordered before the eviction
    return hipEventQuery(s->img_ready) == hipSuccess ? 1 : 0;
}

int pc_analyzer_set_keypoints(pc_analyzer* a, int32_t frame_id, const float* xy, int n) {
    if (!a || n < 0 || (!xy && n > 0)) return fail(PC_E_INVALID, "bad argument");
    Slot* s = find_slot(a, frame_id);
    if (!s) return fail(PC_E_STATE, "frame %d is not resident", frame_id);
    HelperPriorityScope prio_scope(a->prio.hi);
    int rc = ensure_kp_capacity(s->frame, n);
    if (rc != PC_OK) return rc;
    if (n > 0) {
        // resume path (keypoints from the database): pageable source, so the copy is synchronous
        hipStream_t const ds = a->ctx->prep_stream;
        PC_HIP(hipStreamSynchronize(ds));   // a detection of this frame in flight would write the same buffer
        PC_HIP(hipMemcpyAsync(s->frame->d_kps.p, xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, ds));
        PC_HIP(hipStreamSynchronize(ds));
    }
    s->frame->n_kps = n;
    {
        PrepScope prep(a->ctx);
        if ((rc = order_keypoints_spatially(a->ctx, s->frame, s->scratch.bin_hist)) != PC_OK) return rc;
        PC_HIP(hipEventRecord(s->kps_ready, a->ctx->prep_stream));
    }
    s->det = DET_DONE;
    s->supplied = true;
    return PC_OK;
}

// ---- pc_analyzer_submit in its steps, in the one order they have: each is named for what it checks or enqueues ----

static int submit_check(const pc_analyzer* a, const int32_t* targets, int n_targets) {
    if (!a || (n_targets > 0 && !targets)) return fail(PC_E_INVALID, "null argument");
    if (n_targets < 0 || n_targets > PC_MAX_TARGETS) return fail(PC_E_INVALID, "n_targets must be in [0,%d]", PC_MAX_TARGETS);
    if (a->job_count == a->jobs.size()) return fail(PC_E_STATE, "%zu jobs already in flight: call pc_analyzer_collect", a->job_count);
    if (int arc = check_affine(a->affine, a->normalize)) return arc;   // normalize may have been switched on after the refinement
    if (int src = check_search_radius(a->search_radius, a->normalize)) return src;   // ... or after the search
    return check_mask_windows(a->mask_windows, a->normalize, a->affine, a->search_radius, a->min_correlation);
}

static int resolve_slots(pc_analyzer* a, int32_t frame1, const int32_t* targets, int n_targets, JobSlots* s) {
    if (!(s->frame1 = find_slot(a, frame1))) return fail(PC_E_STATE, "frame1 %d is not resident", frame1);
    s->n_targets = n_targets;
    for (int t = 0; t < n_targets; t++) {
        if (!(s->target[t] = find_slot(a, targets[t]))) return fail(PC_E_STATE, "target frame %d is not resident", targets[t]);
        s->target_frame[t] = s->target[t]->frame;
    }
    return PC_OK;
}

// keypoints of frame1: the dense phase ran when the frame became resident; order them now.  *detected: by this run, not supplied
static int finish_frame1_keypoints(pc_analyzer* a, Slot& s1, bool* detected) {
    *detected = !s1.supplied;
    if (s1.det == DET_DONE) return PC_OK;
    SlowSection ss("submit/detect_finish");
    *detected = true;
    return detect_finish_slot(a, s1);
}

// the lane's LK launch needs this frame's keypoints and the pyramids of the frames it reads -- not the detection of frames that
// were made resident for later
static int enqueue_lane_waits(hipStream_t ls, const JobSlots& s) {
    SlowSection ss("submit/waits");
    PC_HIP(hipStreamWaitEvent(ls, s.frame1->kps_ready, 0));
    PC_HIP(hipStreamWaitEvent(ls, s.frame1->img_ready, 0));
    for (int t = 0; t < s.n_targets; t++) PC_HIP(hipStreamWaitEvent(ls, s.target[t]->img_ready, 0));
    return PC_OK;
}

// refused before anything of the job is enqueued: more keypoints than the compaction handles, and a record that does not fit the
// device log (the caller may redirect the log and submit again)
static int refuse_job(const pc_analyzer* a, int n, const pc::RecordLayout& layout) {
    if (n > pc::kCompactMaxKeypoints) return fail(PC_E_CAPACITY, "%d keypoints: more than the compaction handles (%d)", n, pc::kCompactMaxKeypoints);
    const size_t end = a->log_used + pc::RecordLayout::kLogHeaderBytes + layout.bytes;
    if (a->d_log && end > a->log_cap) return fail(PC_E_CAPACITY, "device log full (%zu of %zu bytes)", end, a->log_cap);
    return PC_OK;
}

static int reserve_pack(Job& j, LkLane& lane) {
    SlowSection ss("submit/ensure pack");
    PC_HIP(j.h_pack.ensure(j.layout.bytes));
    PC_HIP(lane.pack.ensure(j.layout.bytes));
    return PC_OK;
}

// the gate between the lanes, then the job's launches, which follow each other on the lane; the gate is the forward launch's
// alone, and the compaction filters on the status the last pass leaves
static int enqueue_lk(pc_analyzer* a, LkLane& lane, const JobSlots& s) {
    pc_context* ctx = a->ctx;
    const pc_frame* const f1 = s.frame1->frame;
    if (a->fopt.window_size != f1->win) return fail(PC_E_INVALID, "window size mismatch");
    SlowSection ss("submit/run_lk");
    uint32_t gate_value = 0;
    if (ctx->gate.on && f1->n_kps > 0) {
        // two job lanes: this launch starts when the one before it (other lane) has handed out its last workgroup --
        // it fills that launch's tail and does not compete with its body
        if (int rc = ctx->gate.wait_and_next(lane.stream, a->gate_armed, &gate_value)) return rc;
        a->gate_armed = true;
    }
    LkPasses passes{.search_radius = a->search_radius, .affine = a->affine, .normalize = a->normalize,
                    .min_correlation = a->min_correlation, .fb_threshold = a->fb_threshold, .mask_windows = a->mask_windows};
    for (int t = 0; t < s.n_targets; t++) {
        const pc_frame* const tg = s.target_frame[t];
        if (tg->target_margin >= 0) passes.plane[t] = tg->target_margin > 0 ? tg->d_choked.p : tg->d_mask.p;
        if (a->mask_windows) passes.weights_tgt[t] = tg->window_weights;
    }
    if (a->mask_windows) passes.weights_f1 = f1->window_weights;
    return run_lk_job(ctx, lane, f1, s.target_frame, s.n_targets, &a->fopt, passes, gate_value);
}

// compaction (status filter) into the lane's pack, frame1's keypoints beside it, and `lk_done`
static int enqueue_records(pc_analyzer* a, LkLane& lane, const JobSlots& s, const Job& j, int lane_i, hipEvent_t lk_done) {
    hipStream_t const ls = lane.stream;
    uint8_t* const pack = lane.pack.p;
    PC_HIP(hipMemsetAsync(pack, 0, pc::RecordLayout::kRowOffsetBytes, ls));
    if (j.n_targets > 0)
        if (int rc = compact_lane(a->ctx, lane, j.n_kps, j.n_targets, reinterpret_cast<long long*>(pack), reinterpret_cast<uint32_t*>(pack + j.layout.o_idx),
                                  reinterpret_cast<float2*>(pack + j.layout.o_xy), reinterpret_cast<float*>(pack + j.layout.o_err)))
            return rc;
    pc::launch_copy_keypoints(s.frame1->frame->d_kps.p, reinterpret_cast<float2*>(pack + j.layout.o_kps), j.n_kps, ls);
    // Everything that reads the resident frames is enqueued: the pyramids (LK), frame1's keypoints (LK, the copy
    // above) and its inverse visiting order (compaction).  A slot may be overwritten once this event has fired.
    PC_HIP(hipEventRecord(lk_done, ls));
    s.frame1->last_read[lane_i] = lk_done;
    for (int t = 0; t < s.n_targets; t++) s.target[t]->last_read[lane_i] = lk_done;
    return PC_OK;
}

// device log: header from pinned memory (that of the job's slot in the ring), the record itself is the pack (one device-to-device
// copy); refuse_job has seen that it fits
static int enqueue_log_append(pc_analyzer* a, LkLane& lane, const Job& j, size_t slot_i) {
    constexpr size_t kHeader = pc::RecordLayout::kLogHeaderBytes;
    if (a->log_hdr.size() != a->jobs.size()) a->log_hdr.resize(a->jobs.size());
    PC_HIP(a->log_hdr[slot_i].ensure(kHeader / sizeof(long long)));
    long long* hh = a->log_hdr[slot_i].p;
    std::memset(hh, 0, kHeader);
    hh[0] = PC_LOG_MAGIC;
    hh[1] = j.frame1;
    hh[2] = j.n_kps;
    hh[3] = j.n_targets;
    for (int t = 0; t < j.n_targets; t++) hh[4 + t] = j.targets[t];
    hh[12] = (long long)j.n_kps * j.n_targets;
    PC_HIP(hipMemcpyAsync(a->d_log + a->log_used, hh, kHeader, hipMemcpyHostToDevice, lane.stream));
    PC_HIP(hipMemcpyAsync(a->d_log + a->log_used + kHeader, lane.pack.p, j.layout.bytes, hipMemcpyDeviceToDevice, lane.stream));
    a->log_used += kHeader + j.layout.bytes;
    return PC_OK;
}

// download: ONE copy with fixed endpoints (the lane's pack -> the job's pinned pack).  The runtime stalls the host for 5-8 ms the
// first time it sees a buffer as a copy source, so per-frame buffers must not appear here.  Then the job's `done`
static int enqueue_download(const pc_analyzer* a, LkLane& lane, Job& j) {
    j.host_records = a->host_records;   // else the row offsets only
    const size_t bytes = j.host_records ? j.layout.bytes : pc::RecordLayout::kRowOffsetBytes;
    PC_HIP(hipMemcpyAsync(j.h_pack.p, lane.pack.p, bytes, hipMemcpyDeviceToHost, lane.stream));
    PC_HIP(hipEventRecord(j.done, lane.stream));
    return PC_OK;
}

int pc_analyzer_submit(pc_analyzer* a, int32_t frame1, const int32_t* targets, int n_targets) {
    int rc = submit_check(a, targets, n_targets);
    if (rc != PC_OK) return rc;
    pc_context* ctx = a->ctx;
    PC_HIP(hipSetDevice(ctx->device));
    HelperPriorityScope prio_scope(a->prio.hi);
    JobSlots s;
    if ((rc = resolve_slots(a, frame1, targets, n_targets, &s)) != PC_OK) return rc;
    bool detected = false;
    if ((rc = finish_frame1_keypoints(a, *s.frame1, &detected)) != PC_OK) return rc;
    const size_t slot_i = (a->job_head + a->job_count) % a->jobs.size();
    Job& j = a->jobs[slot_i];
    hipEvent_t lk_done = nullptr;
    const int lane_i = a->next_lane(&lk_done);
    LkLane& lane = ctx->lanes[lane_i];
    if ((rc = enqueue_lane_waits(lane.stream, s)) != PC_OK) return rc;
    const int n = s.frame1->frame->n_kps;
    const pc::RecordLayout layout((size_t)n, (size_t)n * (size_t)n_targets);
    if ((rc = refuse_job(a, n, layout)) != PC_OK) return rc;
    j.layout = layout;
    if ((rc = reserve_pack(j, lane)) != PC_OK) return rc;
    j.frame1 = frame1;
    j.n_kps = n;
    j.detected = detected;
    j.n_targets = n_targets;
    for (int t = 0; t < n_targets; t++) j.targets[t] = targets[t];
    // Everything of this job goes onto its lane, in order: LK into the lane's records, compaction into the lane's pack,
    // device-log append, download.  The other lane holds the neighbouring jobs, so the next LK launch does not wait for any of it.
    ctx->prep_dirty = true;   // stage-level calls must order themselves behind the side streams
    if (n_targets > 0 && (rc = enqueue_lk(a, lane, s)) != PC_OK) return rc;
    SlowSection ss_post("submit/post enqueue");
    if ((rc = enqueue_records(a, lane, s, j, lane_i, lk_done)) != PC_OK) return rc;
    if (a->d_log && (rc = enqueue_log_append(a, lane, j, slot_i)) != PC_OK) return rc;
    a->submitted++;
    if ((rc = enqueue_download(a, lane, j)) != PC_OK) return rc;
    a->job_count++;
    return PC_OK;
}

int pc_analyzer_pending(const pc_analyzer* a) { return a ? (int)a->job_count : 0; }

int pc_analyzer_set_device_log(pc_analyzer* a, void* d_log, size_t capacity_bytes) {
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    if (d_log && (reinterpret_cast<uintptr_t>(d_log) & 15)) return fail(PC_E_INVALID, "device log must be 16-byte aligned");
    PC_HIP(a->ctx->sync_side_streams());
    PC_HIP(hipStreamSynchronize(a->ctx->stream));
    a->d_log = static_cast<uint8_t*>(d_log);
    a->log_cap = d_log ? capacity_bytes : 0;
    a->log_used = 0;
    return PC_OK;
}

int pc_analyzer_redirect_device_log(pc_analyzer* a, void* d_log, size_t capacity_bytes) {
    if (!a || !d_log) return fail(PC_E_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_log) & 15) return fail(PC_E_INVALID, "device log must be 16-byte aligned");
    // no synchronisation: the appends already enqueued keep their addresses, the next submit writes to the new buffer
    a->d_log = static_cast<uint8_t*>(d_log);
    a->log_cap = capacity_bytes;
    a->log_used = 0;
    return PC_OK;
}

int pc_analyzer_set_host_records(pc_analyzer* a, int enabled) {
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    a->host_records = enabled != 0;
    return PC_OK;
}

int pc_analyzer_set_fb_threshold(pc_analyzer* a, double fb_threshold) {
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    if (int rc = check_fb_threshold(fb_threshold)) return rc;
    a->fb_threshold = fb_threshold;
    return PC_OK;
}

int pc_analyzer_set_min_correlation(pc_analyzer* a, double min_correlation) {
    if (int rc = check_min_correlation(min_correlation)) return rc;   // first: a value is refused whatever the handle
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    a->min_correlation = min_correlation;
    return PC_OK;
}

int pc_analyzer_set_normalize(pc_analyzer* a, int normalize) {
    if (int rc = check_normalize(normalize)) return rc;   // first: a value is refused whatever the handle
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    a->normalize = normalize;
    return PC_OK;
}

int pc_analyzer_set_search_radius(pc_analyzer* a, int search_radius) {
    if (int rc = check_search_radius(search_radius, 0)) return rc;   // first: a value is refused whatever the handle
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    if (int rc = check_search_radius(search_radius, a->normalize)) return rc;
    a->search_radius = search_radius;
    return PC_OK;
}

int pc_analyzer_set_affine_refinement(pc_analyzer* a, int affine) {
    if (int rc = check_affine(affine, 0)) return rc;   // first: a value is refused whatever the handle
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    if (int rc = check_affine(affine, a->normalize)) return rc;
    a->affine = affine;
    return PC_OK;
}

// the choked planes of every slot, when frames put from now on will need them: an allocation inside the running pipeline would stall it
// ... and likewise the weight planes of the masked windows
static int ensure_target_planes(pc_analyzer* a) {
    if (a->mask_kind == 0) return PC_OK;
    if (a->target_margin > 0)
        for (auto& s : a->slots)
            if (int rc = ensure_choked_plane(s.frame)) return rc;
    if (a->mask_windows == 1) {
        PrepScope prep(a->ctx);
        for (auto& s : a->slots)
            if (int rc = alloc_window_weights(s.frame, a->ctx->prep_stream)) return rc;
    }
    return PC_OK;
}

int pc_analyzer_set_mask_windows(pc_analyzer* a, int mask_windows) {
    if (int rc = check_mask_windows(mask_windows, 0, 0, 0, 0.0)) return rc;   // first: a value is refused whatever the handle
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    if (int rc = check_mask_windows(mask_windows, a->normalize, a->affine, a->search_radius, a->min_correlation)) return rc;
    a->mask_windows = mask_windows;
    if (mask_windows == 1 && a->mask_kind != 0) PC_HIP(hipSetDevice(a->ctx->device));
    return ensure_target_planes(a);
}

int pc_analyzer_set_target_mask_margin(pc_analyzer* a, int margin) {
    if (int rc = check_target_margin(margin, true)) return rc;   // first: a margin is refused whatever the handle
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    a->target_margin = margin;
    if (margin > 0 && a->mask_kind != 0) PC_HIP(hipSetDevice(a->ctx->device));
    return ensure_target_planes(a);
}

int pc_analyzer_set_mask(pc_analyzer* a, const uint8_t* mask, size_t row_pitch, int on_device) {
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    if (!mask) {
        a->mask_kind = 0;
        a->mask_dev = nullptr;
        return PC_OK;
    }
    if (row_pitch < (size_t)a->w) return fail(PC_E_INVALID, "row_pitch %zu < %d", row_pitch, a->w);
    PC_HIP(hipSetDevice(a->ctx->device));
    // every slot's plane now: an allocation inside the running pipeline would stall it
    for (auto& s : a->slots)
        if (int rc = ensure_mask_plane(s.frame)) return rc;
    if (on_device == 1) {
        a->mask_kind = 2;
        a->mask_dev = mask;
        a->mask_dev_pitch = row_pitch;
        return ensure_target_planes(a);
    }
    const int g = (a->mask_gen + 1) % pc_analyzer::kMaskGens;
    if (!a->mask_copied[g]) PC_HIP(a->mask_copied[g].create(hipEventDisableTiming));
    else PC_HIP(hipEventSynchronize(a->mask_copied[g]));   // copies out of this buffer, kMaskGens masks ago
    PC_HIP(a->mask_host[g].ensure((size_t)a->w * a->h));
    for (int y = 0; y < a->h; y++) std::memcpy(a->mask_host[g].p + (size_t)y * a->w, mask + (size_t)y * row_pitch, (size_t)a->w);
    a->mask_gen = g;
    a->mask_kind = 1;
    a->mask_dev = nullptr;
    return ensure_target_planes(a);
}

int pc_analyzer_set_mask_polygons(pc_analyzer* a, const float* xy, const int32_t* counts, int n_polygons, int invert) {
    int nv = 0;
    if (int rc = check_polygons(xy, counts, n_polygons, &nv)) return rc;   // first: the polygons are refused whatever the handle
    if (!a) return fail(PC_E_INVALID, "null analyzer");
    PC_HIP(hipSetDevice(a->ctx->device));
    // every slot's plane and the whole vertex ring now: an allocation inside the running pipeline would stall it
    for (auto& s : a->slots)
        if (int rc = ensure_mask_plane(s.frame)) return rc;
    for (int k = 0; k < pc_analyzer::kMaskGens; k++) {
        PC_HIP(a->poly_host[k].ensure((size_t)pc::kPolyWords));
        PC_HIP(a->poly_dev[k].ensure((size_t)pc::kPolyWords, true));
        if (!a->poly_read[k]) PC_HIP(a->poly_read[k].create(hipEventDisableTiming));
    }
    const int g = (a->poly_gen + 1) % pc_analyzer::kMaskGens;
    PC_HIP(hipEventSynchronize(a->poly_read[g]));   // what read this buffer, kMaskGens masks ago (a fresh event is complete)
    const size_t words = snap_polygons(xy, counts, n_polygons, a->poly_host[g].p);
    {
        PrepScope prep(a->ctx);
        PC_HIP(hipMemcpyAsync(a->poly_dev[g].p, a->poly_host[g].p, words * sizeof(int32_t), hipMemcpyHostToDevice, a->ctx->prep_stream));
        PC_HIP(hipEventRecord(a->poly_read[g], a->ctx->prep_stream));
    }
    a->poly_gen = g;
    a->poly_vertices = nv;
    a->poly_polygons = n_polygons;
    a->poly_invert = invert ? 1 : 0;
    a->mask_kind = 3;
    a->mask_dev = nullptr;
    return ensure_target_planes(a);
}

int pc_analyzer_device_log_used(const pc_analyzer* a, size_t* bytes) {
    if (!a || !bytes) return fail(PC_E_INVALID, "null argument");
    *bytes = a->log_used;
    return PC_OK;
}

int pc_analyzer_collect(pc_analyzer* a, pc_frame_result* out) {
    if (!a || !out) return fail(PC_E_INVALID, "null argument");
    if (a->job_count == 0) return fail(PC_E_STATE, "no job in flight");
    Job& j = a->jobs[a->job_head];
    PC_HIP(hipEventSynchronize(j.done));
    // is the preparation stream keeping up?  (HelperPriorityControl)
    if (a->puts >= 2) {
        Slot* const sp = find_slot(a, a->put_previous);
        a->prio.observe(sp && sp->img_ready && hipEventQuery(sp->img_ready) == hipErrorNotReady);
    }
    // let the runtime retire the finished commands of the other streams now, a few at a time: left alone it does
    // so in one batch of several milliseconds every couple of hundred frames, inside some later launch
    for (const LkLane& lane : a->ctx->lanes)
        if (lane.stream) (void)hipStreamQuery(lane.stream);
    (void)hipStreamQuery(a->ctx->prep_stream);
    out->frame1 = j.frame1;
    out->n_keypoints = j.n_kps;
    out->keypoints_detected = j.detected ? 1 : 0;
    out->keypoints_xy = j.host_records ? reinterpret_cast<const float*>(j.h_pack.p + j.layout.o_kps) : nullptr;
    out->n_targets = j.n_targets;
    for (int t = 0; t < PC_MAX_TARGETS; t++) out->targets[t] = t < j.n_targets ? j.targets[t] : 0;
    const long long* h_ro = reinterpret_cast<const long long*>(j.h_pack.p);
    for (int t = 0; t <= PC_MAX_TARGETS; t++) out->row_offset[t] = (int64_t)h_ro[std::min(t, j.n_targets)];
    out->src_indices = j.host_records ? reinterpret_cast<const uint32_t*>(j.h_pack.p + j.layout.o_idx) : nullptr;
    out->tgt_xy = j.host_records ? reinterpret_cast<const float*>(j.h_pack.p + j.layout.o_xy) : nullptr;
    out->flow_err = j.host_records ? reinterpret_cast<const float*>(j.h_pack.p + j.layout.o_err) : nullptr;
    a->job_head = (a->job_head + 1) % a->jobs.size();
    a->job_count--;
    return PC_OK;
}

}  // extern "C"
