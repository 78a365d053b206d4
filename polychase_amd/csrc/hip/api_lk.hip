// api_lk.hip -- the LK stage of the C ABI: the argument checks, run_lk_job (the one sequence of launches behind an LK job, shared
// with the analyzer through api_internal.hpp) and the stage-level pc_lk_track* entry points.  Host-side orchestration only.
#include "api_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pc_api {

int check_lk_args(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                  const pc_flow_options* opt) {
    if (!ctx || !frame1 || !targets || !opt) return fail(PC_E_INVALID, "null argument");
    if (n_targets < 1 || n_targets > PC_MAX_TARGETS) return fail(PC_E_INVALID, "n_targets must be in [1,%d]", PC_MAX_TARGETS);
    if (frame1->n_kps < 0) return fail(PC_E_STATE, "frame1 has no keypoints (call pc_frame_detect or pc_frame_set_keypoints)");
    if (opt->window_size != frame1->win) return fail(PC_E_INVALID, "window_size %d differs from the frame's pyramid padding %d", opt->window_size, frame1->win);
    for (int t = 0; t < n_targets; t++) {
        if (!targets[t]) return fail(PC_E_INVALID, "null target");
        // cv::calcOpticalFlowPyrLK asserts equal level sizes/types (CV_Assert in lkpyramid.cpp)
        if (targets[t]->w != frame1->w || targets[t]->h != frame1->h || targets[t]->win != frame1->win)
            return fail(PC_E_INVALID, "target %d geometry differs from frame1", t);
    }
    return PC_OK;
}

int check_fb_threshold(double fb_threshold) {
    if (!(fb_threshold >= 0.0) || std::isinf(fb_threshold)) return fail(PC_E_INVALID, "fb_threshold must be finite and >= 0");
    return PC_OK;
}

int check_normalize(int normalize) {
    if (normalize != 0 && normalize != 1) return fail(PC_E_INVALID, "normalize must be 0 or 1, got %d", normalize);
    return PC_OK;
}

int check_affine(int affine, int normalize) {
    if (affine != 0 && affine != 1) return fail(PC_E_INVALID, "affine must be 0 or 1, got %d", affine);
    if (affine == 1 && normalize == 1) return fail(PC_E_INVALID, "affine refinement assumes brightness constancy: not together with normalize");
    return PC_OK;
}

int check_search_radius(int search_radius, int normalize) {
    if (search_radius < 0 || search_radius > 256) return fail(PC_E_INVALID, "search_radius must be 0 (off) or 1..256, got %d", search_radius);
    if (search_radius > 0 && normalize == 1) return fail(PC_E_INVALID, "the search prepass assumes brightness constancy: not together with normalize");
    return PC_OK;
}

int check_min_correlation(double min_correlation) {
    if (!(min_correlation >= 0.0 && min_correlation <= 1.0)) return fail(PC_E_INVALID, "min_correlation must be in [0, 1]");   // a NaN fails
    return PC_OK;
}

int check_target_margin(int margin, bool allow_off) {
    if (margin < (allow_off ? -1 : 0) || margin > PC_TARGET_MASK_MAX_MARGIN)
        return fail(PC_E_INVALID, "margin %d, %d..%d allowed", margin, allow_off ? -1 : 0, PC_TARGET_MASK_MAX_MARGIN);
    return PC_OK;
}

int check_mask_windows(int mask_windows, int normalize, int affine, int search_radius, double min_correlation) {
    if (mask_windows != 0 && mask_windows != 1) return fail(PC_E_INVALID, "mask_windows must be 0 or 1, got %d", mask_windows);
    if (mask_windows == 1 && (normalize == 1 || affine == 1 || search_radius > 0 || min_correlation > 0.0))
        return fail(PC_E_INVALID, "normalize, affine refinement, the search prepass and the minimum correlation do not weight their windows: not together with mask_windows");
    return PC_OK;
}

namespace {

// What every launch of one job shares, derived once (lk_job_begin): a pass that derived any of it for itself could pair the
// records with other keypoints, levels or criteria than the forward launch did
struct LkJob {
    const pc_frame* frame1;
    const pc_frame* const* targets;
    int n_targets;
    int n, win;
    int max_level;             // the smallest top level over frame1 and the targets, at most the option's
    int max_iters;             // TermCriteria clamps of calcOpticalFlowPyrLK
    double eps_sq;
    float min_eig_thr;
    int x86_order;
    const uint32_t* perm;      // visiting order (slot -> keypoint); its inverse: LkLane::slot_of
    float4* rec;               // the lane's records, in visiting order
    hipStream_t stream;        // the lane's
};

int lk_job_begin(pc_context* ctx, LkLane& lane, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                 const pc_flow_options* opt, LkJob* j) {
    j->frame1 = frame1;
    j->targets = targets;
    j->n_targets = n_targets;
    j->stream = lane.stream;
    j->n = frame1->n_kps;
    j->win = frame1->win;
    PC_HIP(lane.rec.ensure(((size_t)j->n + 1) * pc::kRecStride));
    j->rec = lane.rec.p;
    lane.slot_of = j->perm = nullptr;
    if (j->n == 0) return PC_OK;
    j->max_level = std::min(opt->max_level, frame1->nlevels - 1);
    for (int t = 0; t < n_targets; t++) j->max_level = std::min(j->max_level, targets[t]->nlevels - 1);
    if (j->max_level < 0) j->max_level = 0;
    j->max_iters = std::min(std::max(opt->term_max_iters, 0), 100);
    const double eps = std::min(std::max(opt->term_epsilon, 0.), 10.);
    j->eps_sq = eps * eps;
    j->min_eig_thr = (float)opt->min_eigen_threshold;
    j->x86_order = (ctx->arith & PC_ARITH_LK_X86_ORDER) ? 1 : 0;
    // visiting order: keypoints binned by image tile (they are stored by corner response); the analyzer
    // prepares it together with the keypoints, the stage-level calls compute it here
    size_t cap = frame1->perm_cap;   // the inverse order lies `cap` entries behind the order
    if (!frame1->perm_valid) {
        cap = (size_t)j->n;
        PC_HIP(ctx->lk_perm.ensure((size_t)j->n * 2));
        PC_HIP(ctx->lk_hist.ensure((size_t)pc::bin_num_tiles(frame1->w, frame1->h) + 1));
        pc::launch_spatial_bins(frame1->d_kps.p, j->n, nullptr, frame1->w, frame1->h, ctx->lk_hist.p, ctx->lk_perm.p, ctx->lk_perm.p + j->n, j->stream);
    }
    j->perm = frame1->perm_valid ? frame1->d_perm.p : ctx->lk_perm.p;
    lane.slot_of = j->perm + cap;
    return PC_OK;
}

int unsupported_window(const LkJob& j) { return fail(PC_E_INVALID, "unsupported window size %d", j.win); }

// forward launch; normalize: the brightness-normalised kernel (include/polychase_hip.h: pc_lk_track_normalized); gate_value: what
// it stores into the context's gate (0: not gated)
int lk_forward(pc_context* ctx, const LkJob& j, int normalize, uint32_t gate_value) {
    pc::LKParams p;
    std::memset(&p, 0, sizeof(p));
    for (int l = 0; l <= j.max_level; l++) {
        p.src[l] = j.frame1->levels[l];
        for (int t = 0; t < j.n_targets; t++) {
            p.tgt[t][l] = j.targets[t]->levels[l].img;
            p.tgt16[t][l] = j.targets[t]->levels[l].img16;
        }
    }
    p.n_targets = j.n_targets;
    p.max_level = j.max_level;
    p.n = j.n;
    p.pts = j.frame1->d_kps.p;
    p.perm = j.perm;
    p.max_iters = j.max_iters;
    p.eps_sq = j.eps_sq;
    p.min_eig_thr = j.min_eig_thr;
    p.out_rec = j.rec;
    p.prof = nullptr;
    p.x86_order = j.x86_order;
    p.x86_stats = ctx->lk_x86_stats.p;
    p.gate = gate_value ? ctx->gate.word.p : nullptr;
    p.gate_value = gate_value;
    if (pc::lk_profile_enabled()) {   // diagnostics build: 16 words per wavefront, the latest launch only
        ctx->lk_prof_rows = (size_t)j.n / 2 + 1;
        PC_HIP(ctx->lk_prof.ensure(ctx->lk_prof_rows * PC_LK_PROFILE_SLOTS));
        PC_HIP(hipMemsetAsync(ctx->lk_prof.p, 0, ctx->lk_prof_rows * PC_LK_PROFILE_SLOTS * sizeof(unsigned long long), j.stream));
        p.prof = ctx->lk_prof.p;
    }
    ScopedTimer tm(ctx, PC_K_LK, j.stream);
    if (!(normalize ? pc::launch_lk_norm(p, j.win, j.stream) : pc::launch_lk(p, j.win, j.stream))) return unsupported_window(j);
    return PC_OK;
}

// search prepass (include/polychase_hip.h: pc_lk_track_search); the displacements and states stay in search_d / search_state,
// [target][n], for lk_backward
int lk_search(pc_context* ctx, const LkJob& j, int search_radius, short2* search_d, uint8_t* search_state) {
    pc::SearchParams p;
    std::memset(&p, 0, sizeof(p));
    for (int l = 0; l <= j.max_level; l++) {
        p.src[l] = j.frame1->levels[l];
        for (int t = 0; t < j.n_targets; t++) p.tgt[t][l] = j.targets[t]->levels[l].img;
    }
    p.n_targets = j.n_targets;
    p.max_level = j.max_level;
    p.n = j.n;
    p.win = j.win;
    pc::search_level_radius(search_radius, j.max_level, &p.s, &p.r);
    p.max_iters = j.max_iters;
    p.eps_sq = j.eps_sq;
    p.min_eig_thr = j.min_eig_thr;
    p.pts = j.frame1->d_kps.p;
    p.perm = j.perm;
    p.rec = j.rec;
    p.search_d = search_d;
    p.search_state = search_state;
    ScopedTimer tm(ctx, PC_K_LK, j.stream);   // no class of its own, as the affine refinement
    if (!pc::launch_lk_search(p, j.stream)) return unsupported_window(j);
    return PC_OK;
}

// affine refinement (include/polychase_hip.h: pc_lk_track_affine); affine_m / affine_state: device arrays [target][n], zeroed, or null
int lk_affine(pc_context* ctx, const LkJob& j, float4* affine_m, uint8_t* affine_state) {
    pc::AffineParams p;
    std::memset(&p, 0, sizeof(p));
    p.f1 = j.frame1->levels[0];
    for (int t = 0; t < j.n_targets; t++) p.timg[t] = j.targets[t]->levels[0].img;
    p.n_targets = j.n_targets;
    p.n = j.n;
    p.win = j.win;
    p.max_iters = j.max_iters;
    p.eps_sq = j.eps_sq;
    p.pts = j.frame1->d_kps.p;
    p.perm = j.perm;
    p.rec = j.rec;
    p.affine_m = affine_m;
    p.affine_state = affine_state;
    ScopedTimer tm(ctx, PC_K_LK, j.stream);   // no class of its own: a job with the option shows two lk launches
    if (!pc::launch_lk_affine(p, j.stream)) return unsupported_window(j);
    return PC_OK;
}

// masked windows (include/polychase_hip.h: pc_lk_track_window_masked): the keypoints frame1's weights touch are tracked again
// under the rule, their records overwritten; touched: device array [n], zeroed, or null
int lk_window_mask(pc_context* ctx, const LkJob& j, uint8_t* touched) {
    pc::LKWMaskParams p;
    std::memset(&p, 0, sizeof(p));
    for (int l = 0; l <= j.max_level; l++) {
        p.src[l] = j.frame1->levels[l];
        p.swt[l] = j.frame1->wt[l];
        for (int t = 0; t < j.n_targets; t++) p.tgt[t][l] = j.targets[t]->levels[l].img;
    }
    p.n_targets = j.n_targets;
    p.max_level = j.max_level;
    p.n = j.n;
    p.win = j.win;
    p.pts = j.frame1->d_kps.p;
    p.perm = j.perm;
    p.max_iters = j.max_iters;
    p.eps_sq = j.eps_sq;
    p.min_eig_thr = j.min_eig_thr;
    p.rec = j.rec;
    p.touched = touched;
    p.x86_order = j.x86_order;
    ScopedTimer tm(ctx, PC_K_LK, j.stream);   // no class of its own, as the affine refinement
    if (!pc::launch_lk_wmask(p, j.stream)) return unsupported_window(j);
    return PC_OK;
}

// target-side masks (include/polychase_hip.h: pc_lk_track_masked): drops the records that end where the plane of their target
// is off (plane[t] null: target t keeps its rows; all null: nothing is enqueued)
int lk_target_mask(const LkJob& j, const uint8_t* const* plane) {
    pc::TargetMaskParams p;
    std::memset(&p, 0, sizeof(p));
    bool any = false;
    for (int t = 0; t < j.n_targets; t++) {
        p.plane[t] = plane[t];
        any = any || plane[t] != nullptr;
    }
    if (!any) return PC_OK;
    p.rec = j.rec;
    p.n = j.n;
    p.n_targets = j.n_targets;
    p.w = j.frame1->w;
    p.h = j.frame1->h;
    pc::launch_lk_target_mask(p, j.stream);
    PC_HIP(hipGetLastError());
    return PC_OK;
}

// minimum correlation (include/polychase_hip.h: pc_lk_track_correlated): drops the rows below min_correlation (0: none) and,
// with `corr` (device, [target][n]), writes the scores
int lk_correlation(pc_context* ctx, const LkJob& j, double min_correlation, float* corr) {
    pc::CorrParams p;
    std::memset(&p, 0, sizeof(p));
    p.f1 = j.frame1->levels[0];
    for (int t = 0; t < j.n_targets; t++) p.timg[t] = j.targets[t]->levels[0].img;
    p.n_targets = j.n_targets;
    p.n = j.n;
    p.win = j.win;
    p.drop = min_correlation > 0.0 ? 1 : 0;
    p.pts = j.frame1->d_kps.p;
    p.perm = j.perm;
    p.t2 = min_correlation * min_correlation;
    p.rec = j.rec;
    p.corr = corr;
    ScopedTimer tm(ctx, PC_K_LK_CORR, j.stream);
    if (!pc::launch_lk_corr(p, j.stream)) return unsupported_window(j);
    return PC_OK;
}

// forward-backward check (include/polychase_hip.h: pc_lk_track_fb); search_d / search_state: lk_search has run, the rows it
// replaced are tracked back by a launch of their own (timed under PC_K_LK_FB too)
int lk_backward(pc_context* ctx, const LkJob& j, const LkPasses& passes, const short2* search_d, const uint8_t* search_state) {
    pc::LKFBParams p;
    std::memset(&p, 0, sizeof(p));
    for (int l = 0; l <= j.max_level; l++) {
        p.f1[l] = j.frame1->levels[l];
        for (int t = 0; t < j.n_targets; t++) {
            p.timg[t][l] = j.targets[t]->levels[l].img;
            p.tder[t][l] = j.targets[t]->levels[l].der;
        }
    }
    p.n_targets = j.n_targets;
    p.max_level = j.max_level;
    p.n = j.n;
    p.win = j.win;
    p.pts = j.frame1->d_kps.p;
    p.perm = j.perm;
    p.max_iters = j.max_iters;
    p.eps_sq = j.eps_sq;
    p.min_eig_thr = j.min_eig_thr;
    p.thr2 = (float)(passes.fb_threshold * passes.fb_threshold);
    p.rec = j.rec;
    p.back_xy = passes.back_xy;
    p.back_status = passes.back_status;
    p.x86_order = j.x86_order;
    p.search_d = search_d;
    p.search_state = search_state;
    bool weighted = false;   // masked windows: a target with weights swaps the weighted launch in
    for (int t = 0; t < j.n_targets; t++) weighted = weighted || (passes.mask_windows && passes.weights_tgt[t]);
    if (weighted) {
        pc::LKWMaskFBParams q;
        std::memset(&q, 0, sizeof(q));
        q.fb = p;
        for (int t = 0; t < j.n_targets; t++)
            for (int l = 0; l <= j.max_level && passes.weights_tgt[t]; l++) q.twt[t][l] = j.targets[t]->wt[l];
        ScopedTimer tm(ctx, PC_K_LK_FB, j.stream);
        if (!pc::launch_lk_wmask_fb(q, j.stream)) return unsupported_window(j);
    } else {
        ScopedTimer tm(ctx, PC_K_LK_FB, j.stream);
        if (!(passes.normalize ? pc::launch_lk_norm_fb(p, j.stream) : pc::launch_lk_fb(p, j.stream))) return unsupported_window(j);
    }
    if (search_d) {
        // the rows the search replaced: tracked back from q with the top level started at q - d
        ScopedTimer tm(ctx, PC_K_LK_FB, j.stream);
        if (!pc::launch_lk_search_fb(p, j.stream)) return unsupported_window(j);
    }
    return PC_OK;
}

}  // namespace

int run_lk_job(pc_context* ctx, LkLane& lane, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
               const pc_flow_options* opt, const LkPasses& passes, uint32_t gate_value) {
    LkJob j;
    int rc = lk_job_begin(ctx, lane, frame1, targets, n_targets, opt, &j);
    if (rc != PC_OK || j.n == 0) return rc;
    const size_t rows = (size_t)j.n * n_targets;
    if ((rc = lk_forward(ctx, j, passes.normalize, gate_value)) != PC_OK) return rc;
    // masked windows: directly after the forward launch (none of the passes it is refused with follows); frame1 without weights:
    // nothing to weight, nothing enqueued but the zeros of `touched`
    if (passes.mask_windows) {
        if (passes.touched) PC_HIP(hipMemsetAsync(passes.touched, 0, (size_t)j.n, j.stream));
        if (passes.weights_f1 && (rc = lk_window_mask(ctx, j, passes.touched)) != PC_OK) return rc;
    }
    // search prepass: directly after the forward launch, in front of the refinement and of every check, which then see the
    // records it replaced
    short2* search_d = nullptr;
    uint8_t* search_state = nullptr;
    if (passes.search_radius > 0) {
        PC_HIP(lane.search_d.ensure(rows));
        PC_HIP(lane.search_state.ensure(rows));
        search_d = lane.search_d.p;
        search_state = lane.search_state.p;
        if ((rc = lk_search(ctx, j, passes.search_radius, search_d, search_state)) != PC_OK) return rc;
    }
    // affine refinement: in front of every check, so that each of them judges the refined end points
    if (passes.affine) {
        if (passes.affine_m) PC_HIP(hipMemsetAsync(passes.affine_m, 0, rows * sizeof(float4), j.stream));
        if (passes.affine_state) PC_HIP(hipMemsetAsync(passes.affine_state, 0, rows, j.stream));
        if ((rc = lk_affine(ctx, j, passes.affine_m, passes.affine_state)) != PC_OK) return rc;
    }
    // target-side masks, then minimum correlation: the rows they drop are rows the backward launch need not look at
    if ((rc = lk_target_mask(j, passes.plane)) != PC_OK) return rc;
    if ((passes.min_correlation > 0.0 || passes.corr) && (rc = lk_correlation(ctx, j, passes.min_correlation, passes.corr)) != PC_OK) return rc;
    // forward-backward check: last, it rewrites the status of the records the caller then unpacks or compacts
    if (passes.fb_threshold > 0.0 && (rc = lk_backward(ctx, j, passes, search_d, search_state)) != PC_OK) return rc;
    return PC_OK;
}

int compact_lane(pc_context* ctx, LkLane& lane, int n, int n_targets, long long* row_offset, uint32_t* src_indices, float2* tgt_xy, float* err) {
    const size_t scratch_cap_before = lane.block_counts.cap;   // a reallocation changes the capacity (the address may repeat)
    PC_HIP(lane.block_counts.ensure(pc::compact_scratch_words(n, n_targets)));
    ScopedTimer t(ctx, PC_K_COMPACT, lane.stream);
    pc::launch_compact(lane.rec.p, lane.slot_of, n, n_targets, lane.block_counts.p, lane.block_counts.cap != scratch_cap_before, row_offset,
                       src_indices, tgt_xy, err, lane.stream);
    return PC_OK;
}

}  // namespace pc_api

using namespace pc_api;

namespace {

// host outputs of a stage call, [target][n] each: the first three are required, the others may be null
struct LkHostOut {
    float* next_xy;
    uint8_t* status;
    float* err;
    float* back_xy;
    uint8_t* back_status;
    float* corr;
    float* affine_m;
    uint8_t* affine_state;
    int16_t* search_d;
    uint8_t* search_state;
    uint8_t* touched;        // [n]
};

// ... and of a filtered one: the status-1 rows of all targets back to back, row_offset[n_targets + 1] (required) delimits them
struct LkFilteredOut {
    uint32_t* src_indices;
    float* tgt_xy;
    float* flow_err;
    int64_t* row_offset;
};

// an optional side array of a stage call whose pass runs: the context's buffer for it, or null where the caller did not ask
template <class T>
int side_reserve(DevBuf<T>& buf, const void* host, size_t rows, T** dev) {
    *dev = nullptr;
    if (!host) return PC_OK;
    PC_HIP(buf.ensure(rows));
    *dev = buf.p;
    return PC_OK;
}

// ... and its way to the host behind the job; dev null: the pass did not run, zeros
template <class T>
int side_download(pc_context* ctx, void* host, const T* dev, size_t rows) {
    if (!host) return PC_OK;
    if (!dev) {
        std::memset(host, 0, rows * sizeof(T));
        return PC_OK;
    }
    PC_HIP(hipMemcpyAsync(host, dev, rows * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return PC_OK;
}

constexpr int kNoMaskTest = -1;

// margin: of the target-side masks, which fill passes.plane here; kNoMaskTest: the targets' masks are not looked at
int lk_track_impl(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets, const pc_flow_options* opt,
                  int margin, LkPasses passes, const LkHostOut& out) {
    int rc = check_target_margin(margin, true);   // first: a margin is refused whatever the handles
    if (rc != PC_OK) return rc;
    if ((rc = check_normalize(passes.normalize)) != PC_OK) return rc;   // ... and so is a switch that is neither off nor on
    if ((rc = check_search_radius(passes.search_radius, passes.normalize)) != PC_OK) return rc;
    if ((rc = check_affine(passes.affine, passes.normalize)) != PC_OK) return rc;
    if ((rc = check_min_correlation(passes.min_correlation)) != PC_OK) return rc;   // ... and so is a correlation
    if ((rc = check_mask_windows(passes.mask_windows, passes.normalize, passes.affine, passes.search_radius, passes.min_correlation)) != PC_OK)
        return rc;
    if ((rc = check_lk_args(ctx, frame1, targets, n_targets, opt)) != PC_OK) return rc;
    if (!out.next_xy || !out.status || !out.err) return fail(PC_E_INVALID, "null output");
    if ((rc = check_fb_threshold(passes.fb_threshold)) != PC_OK) return rc;
    PC_HIP(hipSetDevice(ctx->device));
    if (int jrc = join_prep(ctx)) return jrc;
    LkLane& lane = ctx->lanes[0];
    if (passes.mask_windows) {
        // masked windows: the weight planes of every frame that has a mask on (a cache of the frame, made when the mask changed)
        passes.weights_f1 = frame1->mask_on;
        if (frame1->mask_on && (rc = ensure_window_weights(const_cast<pc_frame*>(frame1), ctx->stream)) != PC_OK) return rc;
        for (int t = 0; t < n_targets && passes.fb_threshold > 0.0; t++) {
            passes.weights_tgt[t] = targets[t]->mask_on;
            if (targets[t]->mask_on && (rc = ensure_window_weights(const_cast<pc_frame*>(targets[t]), ctx->stream)) != PC_OK) return rc;
        }
    }
    const size_t rows = (size_t)frame1->n_kps * n_targets;
    if (rows == 0) {   // nothing to launch and nothing to write
        if ((rc = run_lk_job(ctx, lane, frame1, targets, n_targets, opt, passes)) != PC_OK) return rc;
        PC_HIP(hipStreamSynchronize(ctx->stream));
        return PC_OK;
    }
    if (passes.affine) {
        if ((rc = side_reserve(ctx->lk_affine_m, out.affine_m, rows, &passes.affine_m)) != PC_OK) return rc;
        if ((rc = side_reserve(ctx->lk_affine_state, out.affine_state, rows, &passes.affine_state)) != PC_OK) return rc;
    }
    if (margin >= 0) {
        // target-side masks: each masked target's plane -- choked into the context's scratch when there is a margin
        const size_t plane_bytes = ((size_t)frame1->w * frame1->h + 15) & ~(size_t)15;
        int masked = 0;
        for (int t = 0; t < n_targets; t++) masked += targets[t]->mask_on ? 1 : 0;
        if (margin > 0 && masked > 0) PC_HIP(ctx->lk_choked.ensure((size_t)masked * plane_bytes + 16));
        for (int t = 0, k = 0; t < n_targets; t++) {
            if (!targets[t]->mask_on) continue;
            passes.plane[t] = targets[t]->d_mask.p;
            if (margin > 0) {
                uint8_t* const choked = ctx->lk_choked.p + (size_t)(k++) * plane_bytes;
                pc::launch_mask_choke(targets[t]->d_mask.p, choked, frame1->w, frame1->h, margin, ctx->stream);
                passes.plane[t] = choked;
            }
        }
        PC_HIP(hipGetLastError());
    }
    if ((rc = side_reserve(ctx->lk_corr, out.corr, rows, &passes.corr)) != PC_OK) return rc;
    if (passes.mask_windows && (rc = side_reserve(ctx->lk_touched, out.touched, (size_t)frame1->n_kps, &passes.touched)) != PC_OK) return rc;
    if (passes.fb_threshold > 0.0) {
        if ((rc = side_reserve(ctx->lk_back_xy, out.back_xy, rows, &passes.back_xy)) != PC_OK) return rc;
        if ((rc = side_reserve(ctx->lk_back_status, out.back_status, rows, &passes.back_status)) != PC_OK) return rc;
    }
    if ((rc = run_lk_job(ctx, lane, frame1, targets, n_targets, opt, passes)) != PC_OK) return rc;
    const bool search = passes.search_radius > 0;   // its arrays are the job's own: the backward launches read them
    if ((rc = side_download(ctx, out.search_d, search ? lane.search_d.p : nullptr, rows)) != PC_OK) return rc;
    if ((rc = side_download(ctx, out.search_state, search ? lane.search_state.p : nullptr, rows)) != PC_OK) return rc;
    if ((rc = side_download(ctx, out.affine_m, passes.affine_m, rows)) != PC_OK) return rc;
    if ((rc = side_download(ctx, out.affine_state, passes.affine_state, rows)) != PC_OK) return rc;
    if ((rc = side_download(ctx, out.corr, passes.corr, rows)) != PC_OK) return rc;
    if ((rc = side_download(ctx, out.touched, passes.touched, (size_t)frame1->n_kps)) != PC_OK) return rc;
    if ((rc = side_download(ctx, out.back_xy, passes.back_xy, rows)) != PC_OK) return rc;
    if ((rc = side_download(ctx, out.back_status, passes.back_status, rows)) != PC_OK) return rc;
    // the kernel's records are in visiting order: bring them into the [target][n] arrays of the call
    PC_HIP(ctx->lk_cxy.ensure(rows));
    PC_HIP(ctx->lk_cerr.ensure(rows));
    PC_HIP(ctx->lk_ustatus.ensure(rows));
    pc::launch_unpack_records(lane.rec.p, lane.slot_of, frame1->n_kps, n_targets, ctx->lk_cxy.p, ctx->lk_ustatus.p, ctx->lk_cerr.p, ctx->stream);
    PC_HIP(hipMemcpyAsync(out.next_xy, ctx->lk_cxy.p, rows * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    PC_HIP(hipMemcpyAsync(out.status, ctx->lk_ustatus.p, rows, hipMemcpyDeviceToHost, ctx->stream));
    PC_HIP(hipMemcpyAsync(out.err, ctx->lk_cerr.p, rows * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PC_HIP(hipStreamSynchronize(ctx->stream));
    return PC_OK;
}

int lk_track_filtered_impl(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                           const pc_flow_options* opt, const LkPasses& passes, const LkFilteredOut& out) {
    int rc = check_lk_args(ctx, frame1, targets, n_targets, opt);
    if (rc != PC_OK) return rc;
    if (!out.row_offset) return fail(PC_E_INVALID, "null row_offset");
    if ((rc = check_fb_threshold(passes.fb_threshold)) != PC_OK) return rc;
    PC_HIP(hipSetDevice(ctx->device));
    if (int jrc = join_prep(ctx)) return jrc;
    LkLane& lane = ctx->lanes[0];
    if ((rc = run_lk_job(ctx, lane, frame1, targets, n_targets, opt, passes)) != PC_OK) return rc;
    const int n = frame1->n_kps;
    const size_t rows = (size_t)n * n_targets;
    PC_HIP(ctx->lk_cxy.ensure(rows + 1));
    PC_HIP(ctx->lk_cerr.ensure(rows + 1));
    PC_HIP(ctx->lk_cidx.ensure(rows + 1));
    if (n > pc::kCompactMaxKeypoints) return fail(PC_E_CAPACITY, "%d keypoints: more than the compaction handles (%d)", n, pc::kCompactMaxKeypoints);
    PC_HIP(ctx->lk_row_offset.ensure(PC_MAX_TARGETS + 1));
    PC_HIP(ctx->h_row_offset.ensure(PC_MAX_TARGETS + 1));
    if ((rc = compact_lane(ctx, lane, n, n_targets, ctx->lk_row_offset.p, ctx->lk_cidx.p, ctx->lk_cxy.p, ctx->lk_cerr.p)) != PC_OK) return rc;
    PC_HIP(hipMemcpyAsync(ctx->h_row_offset.p, ctx->lk_row_offset.p, (size_t)(n_targets + 1) * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    PC_HIP(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t <= n_targets; t++) out.row_offset[t] = (int64_t)ctx->h_row_offset.p[t];
    const size_t total = (size_t)out.row_offset[n_targets];
    if (total > 0) {
        if (!out.src_indices || !out.tgt_xy || !out.flow_err) return fail(PC_E_INVALID, "null output");
        PC_HIP(hipMemcpyAsync(out.src_indices, ctx->lk_cidx.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        PC_HIP(hipMemcpyAsync(out.tgt_xy, ctx->lk_cxy.p, total * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
        PC_HIP(hipMemcpyAsync(out.flow_err, ctx->lk_cerr.p, total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        PC_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PC_OK;
}

}  // namespace

extern "C" {

int pc_lk_track(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                const pc_flow_options* opt, float* next_xy, uint8_t* status, float* err) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, kNoMaskTest, LkPasses{}, {.next_xy = next_xy, .status = status, .err = err});
}

int pc_lk_track_fb(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                   const pc_flow_options* opt, double fb_threshold, float* next_xy, uint8_t* status, float* err,
                   float* back_xy, uint8_t* back_status) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, kNoMaskTest, {.fb_threshold = fb_threshold},
                         {.next_xy = next_xy, .status = status, .err = err, .back_xy = back_xy, .back_status = back_status});
}

int pc_lk_track_masked(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                       const pc_flow_options* opt, double fb_threshold, int margin, float* next_xy, uint8_t* status, float* err) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, margin, {.fb_threshold = fb_threshold},
                         {.next_xy = next_xy, .status = status, .err = err});
}

int pc_lk_track_correlated(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                           const pc_flow_options* opt, double min_correlation, double fb_threshold, int margin, float* next_xy,
                           uint8_t* status, float* err, float* corr) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, margin, {.min_correlation = min_correlation, .fb_threshold = fb_threshold},
                         {.next_xy = next_xy, .status = status, .err = err, .corr = corr});
}

int pc_lk_track_normalized(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                           const pc_flow_options* opt, int normalize, double min_correlation, double fb_threshold, int margin,
                           float* next_xy, uint8_t* status, float* err, float* back_xy, uint8_t* back_status) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, margin,
                         {.normalize = normalize, .min_correlation = min_correlation, .fb_threshold = fb_threshold},
                         {.next_xy = next_xy, .status = status, .err = err, .back_xy = back_xy, .back_status = back_status});
}

int pc_lk_track_affine(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                       const pc_flow_options* opt, int affine, int normalize, double min_correlation, double fb_threshold, int margin,
                       float* next_xy, uint8_t* status, float* err, float* back_xy, uint8_t* back_status, float* affine_m,
                       uint8_t* affine_state) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, margin,
                         {.affine = affine, .normalize = normalize, .min_correlation = min_correlation, .fb_threshold = fb_threshold},
                         {.next_xy = next_xy, .status = status, .err = err, .back_xy = back_xy, .back_status = back_status,
                          .affine_m = affine_m, .affine_state = affine_state});
}

int pc_lk_track_search(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                       const pc_flow_options* opt, int search_radius, int affine, int normalize, double min_correlation, double fb_threshold,
                       int margin, float* next_xy, uint8_t* status, float* err, float* back_xy, uint8_t* back_status, float* affine_m,
                       uint8_t* affine_state, int16_t* search_d, uint8_t* search_state) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, margin,
                         {.search_radius = search_radius, .affine = affine, .normalize = normalize, .min_correlation = min_correlation,
                          .fb_threshold = fb_threshold},
                         {.next_xy = next_xy, .status = status, .err = err, .back_xy = back_xy, .back_status = back_status,
                          .affine_m = affine_m, .affine_state = affine_state, .search_d = search_d, .search_state = search_state});
}

int pc_lk_track_window_masked(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                              const pc_flow_options* opt, int mask_windows, double fb_threshold, int margin, float* next_xy, uint8_t* status,
                              float* err, float* back_xy, uint8_t* back_status, uint8_t* touched) {
    return lk_track_impl(ctx, frame1, targets, n_targets, opt, margin, {.fb_threshold = fb_threshold, .mask_windows = mask_windows},
                         {.next_xy = next_xy, .status = status, .err = err, .back_xy = back_xy, .back_status = back_status,
                          .touched = touched});
}

int pc_lk_track_filtered(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                         const pc_flow_options* opt, uint32_t* src_indices, float* tgt_xy, float* flow_err,
                         int64_t* row_offset) {
    return lk_track_filtered_impl(ctx, frame1, targets, n_targets, opt, LkPasses{},
                                  {.src_indices = src_indices, .tgt_xy = tgt_xy, .flow_err = flow_err, .row_offset = row_offset});
}

int pc_lk_track_filtered_fb(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                            const pc_flow_options* opt, double fb_threshold, uint32_t* src_indices, float* tgt_xy,
                            float* flow_err, int64_t* row_offset) {
    return lk_track_filtered_impl(ctx, frame1, targets, n_targets, opt, {.fb_threshold = fb_threshold},
                                  {.src_indices = src_indices, .tgt_xy = tgt_xy, .flow_err = flow_err, .row_offset = row_offset});
}

}  // extern "C"
