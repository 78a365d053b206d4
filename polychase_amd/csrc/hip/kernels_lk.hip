// kernels_lk.hip -- what surrounds the pyramidal Lucas-Kanade launch (K8-K10) on gfx950: the dispatch to the LK kernels, the
// plain cross-check kernel, the spatial binning of the keypoints, the gate between job lanes, status compaction and unpacking.
//
// The LK launch replaces cv::calcOpticalFlowPyrLK as called at reference cpp/opticalflow.cc:119-125 and the status==1 filter of
// cpp/opticalflow.cc:130-147.  Arithmetic follows oracle/pc_oracle.c (which restates OpenCV's LKTrackerInvoker): 14-bit
// fixed-point bilinear weights, int16 patches, structure tensor / mismatch vector accumulated EXACTLY in integers (or, under
// PC_ARITH_LK_X86_ORDER, in the fp32 lane order of an x86 OpenCV build), one rounding to fp32, 2x2 solve in fp32 without FMA
// contraction.  The product kernels are kernels_lk3.hip (windows 4..10) and lk4_kernel.hpp (window 3, windows 11..31).
#include <cstdlib>

#include "lk_plain.hpp"

namespace pc {

// The independent cross-check of the product kernels, every window 3 .. PC_MAX_WINDOW: one wavefront per keypoint (visiting order
// p.perm), group g = lane / 8 tracks it into target g with plain_lk_pair (lk_plain.hpp) -- the template is evaluated per group,
// nothing is shared across the wavefront, the target is gathered byte by byte.  A diagnostic, not a fast path.  The mapping and
// the launch geometry are the ones of the kernels that follow the forward launch (lk_pair.hpp).
template <bool X86>
__global__ __launch_bounds__(256) void lk_plain_kernel(const LKParams p, const int win) {
    extern __shared__ __attribute__((aligned(16))) uint2 s_tmpl[];
    lk_signal_dispatched(p);
    LKPair q;
    if (!lk_pair_prologue<false>(q, p)) return;   // whole wavefronts
    if (!q.tgt_active) return;   // whole groups
    const float2 pt = p.pts[q.feat];
    const auto level_of = [&](int level) {
        const Level L = p.src[level];
        return PlainLKLevel{L.w, L.h, L.pitch, L.img, L.der, p.tgt[q.grp][level]};
    };
    const PlainLKResult r = plain_lk_pair<X86, true>(level_of, pt.x, pt.y, win, q.lg, p.max_level, p.max_iters, p.eps_sq, p.min_eig_thr,
                                                     s_tmpl + (size_t)(q.wave * 8 + q.grp) * (win * win));
    // one 16-byte record per (slot, target): the wavefront's results are contiguous
    if (q.lg == 0) p.out_rec[(size_t)q.slot * kRecStride + q.grp] = make_float4(r.nx, r.ny, r.err, __uint_as_float(r.status ? 1u : 0u));
}

static bool launch_lk_plain(const LKParams& p, int win, hipStream_t s) {
    if (!lk_pair_args_ok(win, p.n_targets)) return false;
    if (p.n <= 0) return true;
    launch_plain_geometry(p.x86_order ? lk_plain_kernel<true> : lk_plain_kernel<false>, p.n, win, s, p, win);
    return true;
}

// POLYCHASE_LK_VARIANT=1 sends every window to the plain kernel above (the cross-check of the two product kernels; round 1's
// two-keypoint kernel on the u8 planes, kernels_lk2.hip, was removed in round 3 after its last measurement:
// profiles/r03_c2_lk_variants.jsonl);
// default: the two-keypoint kernel on the uint16 planes (kernels_lk3.hip) for windows 4..10, the eight-lanes-per-target kernel
// (lk4_kernel.hpp) for window 3 and windows 11..31
static int lk_variant() {
    static const int v = [] {
        const char* e = getenv("POLYCHASE_LK_VARIANT");
        return e ? atoi(e) : 0;
    }();
    return v;
}

bool launch_lk(const LKParams& p, int win, hipStream_t s) {
    if (lk_variant() == 1) return launch_lk_plain(p, win, s);
    return launch_lk3(p, win, s) || launch_lk4a(p, win, s) || launch_lk4b(p, win, s) || launch_lk4c(p, win, s);
}

// ------------------------------------------------------------------------------------------------
// Spatial binning of the keypoints (counting sort by 64x64 tile, raster order of tiles): the order
// in which LK visits keypoints.  Keypoints are stored by corner response, i.e. randomly in space;
// visiting them tile by tile keeps the gathers of concurrently running waves inside one image
// region (L2 hits instead of fabric requests).  Results are written by keypoint index, so the order
// inside a tile (atomics) does not affect the output.
// ------------------------------------------------------------------------------------------------
constexpr int BIN_SHIFT = 6;

__global__ __launch_bounds__(256) void bin_count_kernel(const float2* __restrict__ pts, int n_max, const uint32_t* __restrict__ n_dev, int tiles_x, int n_tiles,
                                                        uint32_t* __restrict__ hist, int hi_prio) {
    helper_priority(hi_prio);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = n_dev ? min((int)*n_dev, n_max) : n_max;
    if (i >= n) return;
    const float2 p = pts[i];
    const int t = min(n_tiles - 1, max(0, ((int)p.y >> BIN_SHIFT) * tiles_x + ((int)p.x >> BIN_SHIFT)));
    atomicAdd(&hist[t], 1u);
}

// (256 lanes: beside a running LK launch a workgroup needs its wavefronts resident together, and 1024-lane
// workgroups -- 4 wavefronts per SIMD -- do not fit the registers three LK wavefronts per SIMD leave over; they
// waited for the whole LK launch to drain, measured 2 ms for a 50-us kernel)
__global__ __launch_bounds__(256) void bin_scan_kernel(uint32_t* __restrict__ hist, int n_tiles, int hi_prio) {
    helper_priority(hi_prio);
    __shared__ uint32_t s_sum[256];
    const int per = (n_tiles + 255) / 256;
    const int b = threadIdx.x * per, e = min(b + per, n_tiles);
    uint32_t s = 0;
    for (int i = b; i < e; i++) s += hist[i];
    s_sum[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t v = (threadIdx.x >= (unsigned)d) ? s_sum[threadIdx.x - d] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = s_sum[threadIdx.x] - s;  // exclusive prefix of this lane's range
    for (int i = b; i < e; i++) {
        const uint32_t c = hist[i];
        hist[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(256) void bin_scatter_kernel(const float2* __restrict__ pts, int n_max, const uint32_t* __restrict__ n_dev, int tiles_x, int n_tiles,
                                                          uint32_t* __restrict__ cursor, uint32_t* __restrict__ perm,
                                                          uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ copy_src,
                                                          uint32_t* __restrict__ copy_dst, int copy_words, int hi_prio) {
    helper_priority(hi_prio);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && (int)threadIdx.x < copy_words) copy_dst[threadIdx.x] = copy_src[threadIdx.x];
    const int n = n_dev ? min((int)*n_dev, n_max) : n_max;
    if (i >= n) return;
    const float2 p = pts[i];
    const int t = min(n_tiles - 1, max(0, ((int)p.y >> BIN_SHIFT) * tiles_x + ((int)p.x >> BIN_SHIFT)));
    const uint32_t pos = atomicAdd(&cursor[t], 1u);
    perm[pos] = (uint32_t)i;
    slot_of[i] = pos;
}

// One wavefront that idles until the launch ahead (on another stream) has handed out all its workgroups.
// The launch ahead was enqueued first and normally runs already.  If the two streams share a hardware queue, though (the
// process holds more HIP streams than the runtime has queues), this kernel sits in FRONT of the launch it waits for: after
// ~50 ms it gives up and raises *timed_out (pinned host memory) -- the analyzer then stops using the gate.
__global__ __launch_bounds__(64) void lk_gate_kernel(const uint32_t* gate, uint32_t value, uint32_t* timed_out) {
    if (threadIdx.x != 0) return;
    for (uint32_t spin = 0; spin < 25000u; spin++) {
        const uint32_t v = __hip_atomic_load(const_cast<uint32_t*>(gate), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int32_t)(v - value) >= 0) return;
        __builtin_amdgcn_s_sleep(64);
    }
    if (timed_out) __hip_atomic_store(timed_out, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
void launch_lk_gate(const uint32_t* gate, uint32_t value, uint32_t* timed_out, hipStream_t s) {
    hipLaunchKernelGGL(lk_gate_kernel, dim3(1), dim3(64), 0, s, gate, value, timed_out);
}

int bin_num_tiles(int w, int h) { return ((w + 63) >> BIN_SHIFT) * ((h + 63) >> BIN_SHIFT); }

void launch_spatial_bins(const float2* pts, int n, const uint32_t* n_dev, int w, int h, uint32_t* hist, uint32_t* perm,
                         uint32_t* slot_of, hipStream_t s) {
    if (n <= 0) return;
    const int tiles_x = (w + 63) >> BIN_SHIFT, n_tiles = bin_num_tiles(w, h);
    (void)hipMemsetAsync(hist, 0, (size_t)n_tiles * sizeof(uint32_t), s);
    hipLaunchKernelGGL(bin_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pts, n, n_dev, tiles_x, n_tiles, hist, helper_prio_arg());
    hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(256), 0, s, hist, n_tiles, helper_prio_arg());
    hipLaunchKernelGGL(bin_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pts, n, n_dev, tiles_x, n_tiles, hist, perm, slot_of,
                       (const uint32_t*)nullptr, (uint32_t*)nullptr, 0, helper_prio_arg());
}

void launch_spatial_bins_counted(const float2* pts, int n, const uint32_t* n_dev, int w, int h, uint32_t* hist, uint32_t* perm,
                                 uint32_t* slot_of, const uint32_t* copy_src, uint32_t* copy_dst, int copy_words, hipStream_t s) {
    const int tiles_x = (w + 63) >> BIN_SHIFT, n_tiles = bin_num_tiles(w, h);
    hipLaunchKernelGGL(bin_scatter_kernel, dim3((std::max(n, 1) + 255) / 256), dim3(256), 0, s, pts, n, n_dev, tiles_x, n_tiles, hist, perm,
                       slot_of, copy_src, copy_dst, copy_words, helper_prio_arg());
}

// ------------------------------------------------------------------------------------------------
// Ordered compaction of status == 1 rows (opticalflow.cc:130-147) in TWO launches: count per block of 256 keypoints --
// whose last workgroup turns the counts into offsets (pc::last_workgroup: the scan is the tail of the kernel that
// produces its input, not a launch of its own) -- and scatter.  The LK kernel leaves its records in visiting order
// (8 per slot, 128 contiguous bytes); here lane = (keypoint i, target t) with t the fast index, so the 8 lanes of a
// keypoint read exactly that line through the inverse permutation and write one run per target in ascending keypoint
// order.  A 256-lane workgroup walks its 256 keypoints in 8 passes of 32.
// (Round 2: 32 keypoints per workgroup and a scan kernel of ONE workgroup that walked nblocks x 8 counters in two serial
// passes -- 10 k counters at 1080p, 40 k at 4K: 58 / 294 us on the job lane between the LK launch and the download.)
// scratch: [kCompactTicketWords tickets, zero before the launch and zeroed again by the scatter][n_targets x nblocks counts]
// ------------------------------------------------------------------------------------------------
constexpr int CF = 256;                  // keypoints per workgroup
constexpr int CT = 256;                  // lanes (small workgroups: see bin_scan_kernel)
constexpr int CPASS = CF * kRecStride / CT;   // passes of CT / kRecStride = 32 keypoints
int compact_num_blocks(int n) { return (n + CF - 1) / CF; }
size_t compact_scratch_words(int n, int n_targets) {
    return (size_t)kCompactTicketWords + (size_t)compact_num_blocks(n) * (size_t)std::max(n_targets, 1) + 1;
}

__device__ __forceinline__ unsigned long long target_lanes(int t) { return 0x0101010101010101ull << t; }

// block_counts[t][b] -> exclusive offsets (global, target-major) + row_offset[]; all 256 lanes of one workgroup
__device__ __forceinline__ void compact_scan_body(uint32_t* __restrict__ block_counts, int nblocks, int n_targets,
                                                  long long* __restrict__ row_offset) {
    __shared__ long long s_part[256];
    const int total = nblocks * n_targets;
    const int per = (total + 255) / 256;
    const int b = threadIdx.x * per, e = min(b + per, total);
    long long sum = 0;
    for (int i = b; i < e; i++) sum += block_counts[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // inclusive scan of the 256 partial sums
        const long long v = (threadIdx.x >= (unsigned)d) ? s_part[threadIdx.x - d] : 0ll;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = s_part[threadIdx.x] - sum;   // exclusive
    for (int i = b; i < e; i++) {
        const uint32_t c = block_counts[i];
        if (i % nblocks == 0) row_offset[i / nblocks] = run;
        block_counts[i] = (uint32_t)run;  // total rows < 2^32 (n_targets * n)
        run += c;
    }
    if (e == total && b < e) row_offset[n_targets] = run;
}

__global__ __launch_bounds__(CT) void compact_count_kernel(const float4* __restrict__ rec, const uint32_t* __restrict__ slot_of,
                                                             int n, int n_targets, int nblocks,
                                                             uint32_t* __restrict__ tickets, uint32_t* __restrict__ block_counts,
                                                             long long* __restrict__ row_offset, int hi_prio) {
    helper_priority(hi_prio);
    __shared__ uint32_t s_cnt[kRecStride];
    const int t = threadIdx.x & 7, lane = threadIdx.x & 63;
    if (threadIdx.x < kRecStride) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t mine = 0;   // lanes 0-7 of a wavefront: rows of target `lane` among the wavefront's keypoints
#pragma unroll
    for (int k = 0; k < CPASS; k++) {
        const int i = blockIdx.x * CF + k * (CT / kRecStride) + (int)(threadIdx.x >> 3);
        bool keep = false;
        if (i < n && t < n_targets) keep = __float_as_uint(rec[(size_t)slot_of[i] * kRecStride + t].w) == 1u;
        const unsigned long long b = __ballot(keep);
        if (lane < kRecStride) mine += (uint32_t)__popcll(b & target_lanes(lane));
    }
    if (lane < kRecStride && mine) atomicAdd(&s_cnt[lane], mine);
    __syncthreads();
    // agent-scope store: the workgroup that finishes last reads the counts of all the others (last_workgroup's contract)
    if ((int)threadIdx.x < n_targets) publish(&block_counts[(size_t)threadIdx.x * nblocks + blockIdx.x], s_cnt[threadIdx.x]);
    if (last_workgroup(tickets, (uint32_t)nblocks)) compact_scan_body(block_counts, nblocks, n_targets, row_offset);
}

__global__ __launch_bounds__(CT) void compact_scatter_kernel(const float4* __restrict__ rec, const uint32_t* __restrict__ slot_of,
                                                               int n, int n_targets, int nblocks, uint32_t* __restrict__ tickets,
                                                               const uint32_t* __restrict__ block_offsets,
                                                               uint32_t* __restrict__ out_idx,
                                                               float2* __restrict__ out_xy, float* __restrict__ out_err, int hi_prio) {
    helper_priority(hi_prio);
    // rows of target t in (pass k, wavefront w), then their exclusive prefix in keypoint order = (k, w) order
    __shared__ uint32_t s_cnt[CPASS * (CT / 64)][kRecStride];
    const int t = threadIdx.x & 7, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the tickets of the count kernel are zero again for the next launch on this lane
    if (blockIdx.x == 0)
        for (uint32_t k = threadIdx.x; k < last_workgroup_words((uint32_t)nblocks); k += CT) tickets[k] = 0u;
    float4 r[CPASS];
    unsigned long long bal[CPASS];
#pragma unroll
    for (int k = 0; k < CPASS; k++) {
        const int i = blockIdx.x * CF + k * (CT / kRecStride) + (int)(threadIdx.x >> 3);
        r[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool live = i < n && t < n_targets;
        if (live) r[k] = rec[(size_t)slot_of[i] * kRecStride + t];
        bal[k] = __ballot(live && __float_as_uint(r[k].w) == 1u);
        if (lane < kRecStride) s_cnt[k * (CT / 64) + wave][lane] = (uint32_t)__popcll(bal[k] & target_lanes(lane));
    }
    __syncthreads();
    {
        // lane (q, t): exclusive prefix over q' < q of target t (32 x 8 entries, one per lane)
        const int q = threadIdx.x >> 3;
        uint32_t run = 0;
        for (int qq = 0; qq < q; qq++) run += s_cnt[qq][t];
        __syncthreads();
        s_cnt[q][t] = run;
        __syncthreads();
    }
    const uint32_t base = (t < n_targets) ? block_offsets[(size_t)t * nblocks + blockIdx.x] : 0u;
#pragma unroll
    for (int k = 0; k < CPASS; k++) {
        if ((bal[k] >> lane) & 1ull) {
            const int i = blockIdx.x * CF + k * (CT / kRecStride) + (int)(threadIdx.x >> 3);
            const uint32_t pos = base + s_cnt[k * (CT / 64) + wave][t] +
                                 (uint32_t)__popcll(bal[k] & target_lanes(t) & ((1ull << lane) - 1ull));
            out_idx[pos] = (uint32_t)i;
            out_xy[pos] = make_float2(r[k].x, r[k].y);
            out_err[pos] = r[k].z;
        }
    }
}

// raw records -> the [target][n] arrays of pc_lk_track, keypoint order
__global__ __launch_bounds__(256) void unpack_records_kernel(const float4* __restrict__ rec, const uint32_t* __restrict__ slot_of,
                                                             int n, float2* __restrict__ xy, uint8_t* __restrict__ status,
                                                             float* __restrict__ err, int hi_prio) {
    helper_priority(hi_prio);
    const int i = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (i >= n) return;
    const float4 r = rec[(size_t)slot_of[i] * kRecStride + t];
    const size_t o = (size_t)t * n + i;
    xy[o] = make_float2(r.x, r.y);
    status[o] = (uint8_t)__float_as_uint(r.w);
    err[o] = r.z;
}

void launch_unpack_records(const float4* rec, const uint32_t* slot_of, int n, int n_targets, float2* xy, uint8_t* status,
                           float* err, hipStream_t s) {
    if (n <= 0 || n_targets <= 0) return;
    hipLaunchKernelGGL(unpack_records_kernel, dim3((n + 255) / 256, n_targets), dim3(256), 0, s, rec, slot_of, n, xy, status, err, helper_prio_arg());
}

// keypoints of frame1 -> the job's packed record buffer (device to device, 16 bytes per lane)
__global__ __launch_bounds__(256) void copy_keypoints_kernel(const float2* __restrict__ src, float2* __restrict__ dst, int n, int hi_prio) {
    helper_priority(hi_prio);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // one pair of keypoints
    if (2 * i + 1 < n) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    else if (2 * i < n) dst[2 * i] = src[2 * i];
}
void launch_copy_keypoints(const float2* src, float2* dst, int n, hipStream_t s) {
    if (n <= 0) return;
    const int pairs = (n + 1) / 2;
    hipLaunchKernelGGL(copy_keypoints_kernel, dim3((pairs + 255) / 256), dim3(256), 0, s, src, dst, n, helper_prio_arg());
}

void launch_compact(const float4* rec, const uint32_t* slot_of, int n, int n_targets, uint32_t* scratch, bool scratch_fresh,
                    long long* row_offset, uint32_t* out_idx, float2* out_xy, float* out_err, hipStream_t s) {
    const int nblocks = compact_num_blocks(n);
    uint32_t* const tickets = scratch;
    uint32_t* const block_counts = scratch + kCompactTicketWords;
    // tickets: zero at the first use of a (re)allocated scratch buffer -- also when this call has nothing to compact:
    // the next one no longer knows that the buffer is new --, afterwards the scatter kernel leaves them zero
    if (scratch_fresh) (void)hipMemsetAsync(tickets, 0, (size_t)kCompactTicketWords * sizeof(uint32_t), s);
    if (nblocks == 0 || n_targets <= 0) {
        (void)hipMemsetAsync(row_offset, 0, (size_t)(std::max(n_targets, 0) + 1) * sizeof(long long), s);
        return;
    }
    static_assert((long long)(kCompactTicketWords - 1) * kTicketGroup * CF >= kCompactMaxKeypoints, "tickets for kCompactMaxKeypoints");
    hipLaunchKernelGGL(compact_count_kernel, dim3(nblocks), dim3(CT), 0, s, rec, slot_of, n, n_targets, nblocks, tickets, block_counts,
                       row_offset, helper_prio_arg());
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nblocks), dim3(CT), 0, s, rec, slot_of, n, n_targets, nblocks, tickets,
                       block_counts, out_idx, out_xy, out_err, helper_prio_arg());
}

}  // namespace pc
