// internal.hpp -- host-side structures shared by the api*.hip units (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/polychase_hip.h"
#include "../../../include/polychase_records.h"
#include "kernels.hpp"

static_assert(pc::kMaxLevels == PC_MAX_LEVELS, "LKParams holds PC_MAX_LEVELS levels");

namespace pc {

std::string& last_error();

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}

#define PC_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(PC_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// POLYCHASE_TRACE_ALLOC=1: report every (re)allocation of a scratch buffer (each one stalls the pipeline)
inline bool trace_allocations() {
    static const bool on = getenv("POLYCHASE_TRACE_ALLOC") != nullptr;
    return on;
}

// pc_debug_live_resources: what the four owners below hold in this process, counted where a handle is acquired and let go
enum { kLiveDevice = 0, kLivePinned, kLiveStreams, kLiveEvents };
inline std::atomic<int> g_live[4];
inline void live_add(int kind, int d) { g_live[kind].fetch_add(d, std::memory_order_relaxed); }

// The owners of everything behind the C ABI: a device buffer, a pinned host buffer, a stream, an event.  Each lets go of what
// it holds in its destructor, cannot be copied, and is empty after a move.  None may be a global or a function-local static
// (its destructor would run after the HIP runtime has shut down).  A struct declares its streams and events before the buffers
// that work on them: members are destroyed in reverse order, so the buffers are freed first and the streams destroyed last.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n, bool exact = false) {   // exact: a buffer of fixed size, no room to grow
        if (n <= cap) return hipSuccess;
        const size_t old = cap;
        release();
        size_t want = exact ? n : n + n / 2 + 64;   // generous: a reallocation synchronises the device
        if (trace_allocations()) fprintf(stderr, "[polychase_hip] device buffer %zu -> %zu bytes\n", old * sizeof(T), want * sizeof(T));
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
        if (e != hipSuccess) return e;
        cap = want;
        live_add(kLiveDevice, 1);
        return e;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            live_add(kLiveDevice, -1);
        }
        p = nullptr;
        cap = 0;
    }
};

template <typename T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~PinBuf() { release(); }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        const size_t old = cap;
        release();
        size_t want = n + n / 2 + 64;   // pinned allocations take tens of milliseconds
        if (trace_allocations()) fprintf(stderr, "[polychase_hip] pinned buffer %zu -> %zu bytes\n", old * sizeof(T), want * sizeof(T));
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), want * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return e;
        cap = want;
        live_add(kLivePinned, 1);
        return e;
    }
    void release() {
        if (p) {
            (void)hipHostFree(p);
            live_add(kLivePinned, -1);
        }
        p = nullptr;
        cap = 0;
    }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) {
            release();
            s = std::exchange(o.s, nullptr);
        }
        return *this;
    }
    ~Stream() { release(); }
    hipError_t create(unsigned flags) {   // an empty owner only
        hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e == hipSuccess) live_add(kLiveStreams, 1);
        else s = nullptr;
        return e;
    }
    void release() {
        if (s) {
            (void)hipStreamDestroy(s);
            live_add(kLiveStreams, -1);
        }
        s = nullptr;
    }
    operator hipStream_t() const { return s; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            release();
            e = std::exchange(o.e, nullptr);
        }
        return *this;
    }
    ~Event() { release(); }
    hipError_t create(unsigned flags = hipEventDefault) {   // an empty owner only
        hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc == hipSuccess) live_add(kLiveEvents, 1);
        else e = nullptr;
        return rc;
    }
    void release() {
        if (e) {
            (void)hipEventDestroy(e);
            live_add(kLiveEvents, -1);
        }
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

template <typename Owner>
constexpr bool owns_alone = !std::is_copy_constructible<Owner>::value && !std::is_copy_assignable<Owner>::value &&
                            std::is_nothrow_move_constructible<Owner>::value && std::is_nothrow_move_assignable<Owner>::value;
static_assert(owns_alone<DevBuf<float>> && owns_alone<PinBuf<float>> && owns_alone<Stream> && owns_alone<Event>,
              "owners are not copyable and move without throwing (std::vector<Slot>, std::vector<Job>)");

struct TimedRange {
    int cls;
    Event a, b;
};

}  // namespace pc

using pc::DevBuf;
using pc::Event;
using pc::PinBuf;
using pc::Stream;
using pc::TimedRange;
using pc::fail;

// Per-detection buffers of one frame.  Detection is enqueued in one go, without the host in the loop:
//   min-eig map + per-cell max, threshold + NMS -> candidate keys + state bytes + per-bucket counts, bucket sort of the
//   candidates (counts stay on the device), greedy suppression in priority order, ordered compaction -> keypoints, LK
//   visiting order; the counters go to pinned memory (ev_b).  detect_finish() then reads the keypoint count -- and
//   redoes the frame on the slow path (candidate count on the host, rocPRIM sort) if a fast-path bound was exceeded.
struct DetectScratch {
    Event ev_b;
    DevBuf<unsigned long long> keys, keys_bucketed, keys_sorted;
    DevBuf<unsigned long long> key_slots;  // kSortBuckets x kBucketSlots bucket slots of the fused chain (launch_nms), when it runs
    DevBuf<float> eig;                     // min-eig map (K2 -> K3, K5)
    DevBuf<float> cov;                     // covariance planes of the general corner response (block_size != 3 / Harris), on demand
    DevBuf<double> box_rows;               // row sums of the box filter for large block sizes (kernels.hpp kBoxRowsFromBlock), on demand
    DevBuf<uint8_t> cstate;                // 0 no candidate / 1 candidate / 2 accepted / 3 rejected
    // [0] candidates, [1] keypoints, [2] stuck lanes, [3] fast-path overflow bits, [4] sort range hi, [5] sort shift, [6..7] pad,
    // [8 ..] cell max [kMaxGridCells], bucket counts [kSortBuckets], bucket cursors [kSortBuckets]
    DevBuf<uint32_t> counters;
    DevBuf<uint32_t> bucket_offsets;       // [kSortBuckets + 1]
    DevBuf<uint32_t> per_block;            // accepted candidates per suppression workgroup -> their exclusive scan
    DevBuf<uint32_t> sup_grid;             // min_distance > 64: the accepted corners by grid cell (kernels_gftt.hip), on demand
    DevBuf<uint32_t> bin_hist;             // keypoints per 64x64 tile (the analyzer's detections; stage-level calls use the context's)
    PinBuf<uint32_t> h_counters;           // counters[0..7] after the detection
    uint32_t cand_cap = 0;                 // candidates the fast path holds
    int counter_words = 0;                 // words of `counters` (header, cell maxima, bucket counts + cursors, tickets)
    uint32_t ticket_stride = 0;            // words between the three ticket arrays at the end of `counters`
    bool cleared = false;                  // `counters` were zeroed in front of the coming detection (by the frame's level-0 kernel)
};

// One job lane: the stream a job's launches are enqueued on and what they write.  run_lk_job leaves the records in `rec` and the
// inverse visiting order in `slot_of` (with a search radius the displacements and states in search_d / search_state), the
// analyzer compacts them into `pack`.  pc_context holds two: lane 0 is the stage-level calls' lane, on pc_context::stream; the
// analyzer alternates its jobs over lane 0 and lane 1 (pc_context::stream_b).
struct LkLane {
    hipStream_t stream = nullptr;          // not owned: pc_context::stream or stream_b
    DevBuf<float4> rec;                    // raw records in visiting order (kernels.hpp LKParams::out_rec)
    const uint32_t* slot_of = nullptr;     // not owned (a frame's d_perm or lk_perm): inverse visiting order of the latest job
    DevBuf<uint32_t> block_counts;         // compaction scratch
    DevBuf<short2> search_d;               // pc_lk_track_search: the displacements and the states of the latest job, [target][n]
    DevBuf<uint8_t> search_state;          // (the backward launches read them)
    DevBuf<uint8_t> pack;                  // the analyzer's compacted records of one job (pc::RecordLayout)
};

// The gate between the forward launches of the two lanes (kernels.hpp LKParams::gate): a gated launch stores its value into
// `word` when its last workgroup starts, launch_lk_gate makes the other lane's stream wait for that value.
struct LkGate {
    DevBuf<uint32_t> word;                 // allocated (16 words, zeroed) by the first gated submit
    PinBuf<uint32_t> timed_out;            // raised by a gate kernel that gave up
    uint32_t seq = 0;                      // value the latest gated launch stores
    bool on = true;                        // POLYCHASE_LK_GATE=0 (pc_context_create) and a timed-out wait switch it off
    // Off for good once a wait has timed out: the lanes' streams share a hardware queue, the launch the gate kernel waited for
    // was queued BEHIND it.
    void drop_if_timed_out() {
        if (*static_cast<volatile uint32_t*>(timed_out.p) == 0u) return;
        on = false;
        if (pc::trace_allocations()) fprintf(stderr, "[polychase_hip] LK gate timed out (streams share a hardware queue): gate switched off\n");
    }
    // Makes `s` wait for the previous gated launch, if there is one ahead (`armed`), and hands out the value the coming forward
    // launch must store (run_lk_job's gate_value; never 0, which says "not gated").  Only while `on`.
    int wait_and_next(hipStream_t s, bool armed, uint32_t* value) {
        if (!word.p) {
            PC_HIP(word.ensure(16));
            PC_HIP(hipMemset(word.p, 0, 16 * sizeof(uint32_t)));
            PC_HIP(timed_out.ensure(1));
            timed_out.p[0] = 0u;
        }
        drop_if_timed_out();
        if (armed && on) pc::launch_lk_gate(word.p, seq, timed_out.p, s);
        if (++seq == 0) ++seq;
        *value = seq;
        return PC_OK;
    }
};

struct pc_context {
    int device = 0;
    int arith = PC_ARITH_OPENCV_X86;     // pc_context_set_arithmetic; the default = what a stock x86-64 OpenCV build executes
    // Stage-level calls run on `stream`.  pc_analyzer alternates its jobs (LK launch + compaction + device-log append +
    // record download of one frame1) over two job lanes (`lanes`, on `stream` and `stream_b`): the launches of consecutive frames
    // overlap, so the tail of one launch and the gap before the next are filled by the other lane's wavefronts.
    // (HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues, 4 unless raised, and a stream that shares a queue
    // waits behind the other's commands: pc_runtime_init raises the default before the first HIP call.)
    // (Streams and events stand in front of the buffers: ~pc_context frees the buffers first and destroys the streams last.)
    Stream stream;
    Stream stream_b;
    // pc_analyzer runs frame preparation (gray, pyramid, detection, keypoint ordering) on its own
    // stream so that it overlaps the LK launch of the previous frame1 on `stream`.  `work` is the stream
    // the image / detection helpers enqueue on: `stream` by default, `prep_stream` inside the analyzer.
    Stream prep_stream;
    // Detection follows the image path on prep_stream.
    hipError_t sync_side_streams() const {
        hipError_t e = copy_stream ? hipStreamSynchronize(copy_stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(prep_stream);
        if (lanes[1].stream && e == hipSuccess) e = hipStreamSynchronize(lanes[1].stream);
        return e;
    }
    hipStream_t work = nullptr;          // not owned: `stream` or `prep_stream`
    Event prep_fence;                    // orders `stream` after everything queued on prep_stream so far
    bool prep_dirty = false;
    // pc_context_set_gray_conversion: the channel weights and the float transfer table of the RGB frames put from now on
    int gray_w[3] = {9798, 19235, 3735};
    bool gray_table_on = false;
    DevBuf<uint8_t> gray_table_buf[2];     // PC_TRANSFER_ENTRIES bytes each: the table in force and the one a setter uploads into
    int gray_table_cur = 0;                // ... gray_table_buf[gray_table_cur] is the one in force (swapped once an upload is complete)
    const uint8_t* gray_table_dev() const { return gray_table_on ? gray_table_buf[gray_table_cur].p : nullptr; }
    std::vector<uint8_t> gray_table_host;  // the table in force (pc_context_get_gray_conversion)
    bool gray_default_weights() const { return gray_w[0] == 9798 && gray_w[1] == 19235 && gray_w[2] == 3735; }
    // pc_context_set_lens_map: the map of the frames put from now on (lens_w x lens_h entries in rows of lens_pitch, a multiple
    // of 4), the gray plane of the source the remap reads and the plane it writes for the level-0 kernel (rows of
    // lens_plane_pitch bytes each); all three allocated by the setter and freed when the map is cleared.  lens_w == 0: no map
    DevBuf<int32_t> lens_map;
    DevBuf<uint8_t> lens_gray, lens_out;
    int lens_w = 0, lens_h = 0, lens_pitch = 0, lens_plane_pitch = 0;
    // the analyzer's host frames (PC_FRAME_PINNED_HOST): transfers on a stream of their own, two buffers in turn;
    // staging_ev[b] = {copy into b complete (copy stream), the kernel that reads b has run (preparation stream)}
    Stream copy_stream;                  // POLYCHASE_COPY_STREAM=0: none (the transfer is enqueued in front of the frame's kernels)
    Event staging_ev[2][2];
    int staging_turn = 0;
    // timing
    unsigned timing_mask = 0;   // bit k: time kernel class k with HIP events
    std::vector<TimedRange> ranges;
    std::vector<Event> event_pool;
    // staging of host-provided frames
    DevBuf<uint8_t> staging;
    DevBuf<uint8_t> staging2[2];
    // GFTT scratch
    DevBuf<int2> sup_offsets;              // suppression neighbourhood for sup_min_distance
    DevBuf<int> sup_rows;                  // the same as half-widths per row, [2 * sup_R + 1]
    int sup_R = 0;
    double sup_min_distance = -1.0;
    unsigned long long detect_paths[PC_DETECT_PATH_SLOTS] = {0};   // pc_debug_detection_paths; written by detect_finish only
    int n_sup_offsets = 0;
    // candidates of the latest finished detection + 25 %: the detections enqueued next size their launches for that many
    // (the count itself stays on the device; a frame with more is redone with launches for the full capacity)
    uint32_t cand_hint = 0;
    std::unique_ptr<DetectScratch> detect;   // scratch of the stage-level pc_frame_detect
    DevBuf<uint8_t> sort_temp;
    const pc_frame* eig_owner = nullptr;   // not owned: the frame whose response map `detect` holds
    // pc_frame_set_mask_polygons: the snapped vertices on their way to the device (the call waits for the launch that reads them)
    PinBuf<int32_t> poly_host;
    DevBuf<int32_t> poly_dev;
    // LK scratch
    LkLane lanes[2];                       // behind the streams: the lanes' buffers are freed before the streams are destroyed
    LkGate gate;
    DevBuf<float2> lk_cxy;
    DevBuf<uint8_t> lk_ustatus;            // pc_lk_track: unpacked status
    DevBuf<float> lk_cerr;
    DevBuf<float2> lk_back_xy;             // pc_lk_track_fb: backward end points / status, [target][n]
    DevBuf<uint8_t> lk_back_status;
    DevBuf<float> lk_corr;                 // pc_lk_track_correlated: the scores, [target][n]
    DevBuf<float4> lk_affine_m;            // pc_lk_track_affine: the matrices and the states, [target][n]
    DevBuf<uint8_t> lk_affine_state;
    DevBuf<uint8_t> lk_touched;            // pc_lk_track_window_masked: the keypoints the weights touched, [n]
    DevBuf<uint8_t> lk_choked;             // pc_lk_track_masked, pc_frame_download_choked_mask: the targets' choked planes
    DevBuf<uint32_t> lk_cidx, lk_perm, lk_hist;
    DevBuf<unsigned long long> lk_prof;    // pc_debug_lk_profile: 16 words per wavefront of the latest launch
    size_t lk_prof_rows = 0;
    DevBuf<unsigned long long> lk_x86_stats;   // pc_debug_lk_x86_stats: four counters, or unallocated (not counting)
    DevBuf<long long> lk_row_offset;
    PinBuf<long long> h_row_offset;
    // timing (the events: above)
    int launches[PC_K_COUNT] = {0};
    double total_ms[PC_K_COUNT] = {0};
    double busy_ms[PC_K_COUNT] = {0};    // time during which at least one launch of the class was executing
};

struct pc_frame {
    pc_context* ctx = nullptr;
    int w = 0, h = 0, win = 0, max_level = 0, nlevels = 0;
    pc::Level levels[PC_MAX_LEVELS];
    DevBuf<uint8_t> slab;
    size_t slab_bytes = 0;
    DevBuf<float2> d_kps;
    int kp_cap = 0;
    int n_kps = -1;   // -1: none
    int n_cands = -1;
    DevBuf<uint32_t> d_perm;      // LK visiting order of d_kps (spatial bins) [perm_cap], then its inverse [perm_cap]; valid iff perm_valid
    int perm_cap = 0;
    bool perm_valid = false;
    // detection mask (gftt.cc:45-83): a packed w x h plane of bytes, allocated the first time the frame is given one;
    // mask_on: the next detection of this frame honours it
    DevBuf<uint8_t> d_mask;
    bool mask_on = false;
    // target-side mask of a frame in an analyzer's ring (pc_analyzer_set_target_mask_margin): the margin the frame was put under
    // while a mask was in force -- rows that end in this frame are judged by d_mask (0) or by d_choked, its choked plane (> 0) --
    // or -1: the frame keeps every row.  d_choked is allocated the first time an analyzer needs it.
    int target_margin = -1;
    DevBuf<uint8_t> d_choked;
    // masked windows (pc_lk_track_window_masked): the weight planes W_l of the mask, one per level in the level's image geometry
    // (wt[l]: interior origin; the padding is on), and behind them the packed M_l of the levels >= 1.  One allocation, made the
    // first time the frame needs its weights; weights_valid: the planes are those of the mask in d_mask (every change of the mask
    // clears it).  An analyzer's frame: window_weights says that the frame was put with the option and a mask in force.
    DevBuf<uint8_t> d_weights;
    uint8_t* wt[PC_MAX_LEVELS] = {nullptr};
    uint8_t* wm[PC_MAX_LEVELS] = {nullptr};
    bool weights_valid = false;
    bool window_weights = false;
};

