/*
 * polychase_hip.h -- C ABI of the MI355X (gfx950) video-analysis hot path.
 *
 * This is the drop-in boundary BELOW the reference's pybind11 module `polychase_core`
 * (/root/reference/cpp/polychase_pybind.cc:29): the reference has no FFI of its own, its host C++
 * calls OpenCV directly.  Each entry point below replaces one OpenCV / in-repo call on the path
 * GenerateOpticalFlowDatabase (cpp/opticalflow.cc:209-321) and cites it.  Plain pointers and sizes
 * only; no torch / Eigen / OpenCV types.  All functions return 0 on success, a negative PC_E_* code
 * on failure; pc_last_error() returns the message of the calling thread's last failure.
 *
 * Memory: "host" pointers are ordinary (or pinned) CPU memory; "device" pointers are HIP device
 * memory of the context's GPU (e.g. torch.Tensor.data_ptr()).  Work is enqueued on the context's HIP
 * stream; functions that return data to the host synchronise that stream themselves.
 *
 * There is NO CPU fallback: every function fails with PC_E_NO_DEVICE when no gfx950 device is
 * usable.
 */
#ifndef POLYCHASE_HIP_H_
#define POLYCHASE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC_OK 0
#define PC_E_INVALID (-1)     /* bad argument / unsupported option */
#define PC_E_NO_DEVICE (-2)   /* no usable HIP device */
#define PC_E_HIP (-3)         /* a HIP runtime call failed */
#define PC_E_CAPACITY (-4)    /* caller buffer too small */
#define PC_E_STATE (-5)       /* call sequence error (e.g. frame has no keypoints) */

#define PC_MAX_TARGETS 8      /* the reference tracks each frame into <= 8 neighbours (opticalflow.cc:76-77) */
#define PC_MAX_LEVELS 16      /* a pyramid ends where the next level would be <= the window (>= 3 px): 14 levels at most for the
                                 2^30 pixels a frame may have; any max_level >= 0 is accepted (OpenCV: maxLevel is free) */
#define PC_MAX_WINDOW 31      /* OpticalFlowOptions.window_size is free in the reference (opticalflow.h:27-33); OpenCV's own default is 21.
                                 3: lk4, 4..10: the two-keypoint kernel (lk3), 11..31: lk4 (one keypoint per wavefront, 8 lanes per target) */

typedef struct pc_context pc_context;
typedef struct pc_frame pc_frame;

/* GFTTOptions, cpp/feature_detection/gftt.h:5-21 (same fields, same defaults) */
typedef struct pc_gftt_options {
    double quality_level; /* 0.01 */
    double min_distance;  /* 5.0   (any value >= 0: up to 64 the table-driven parallel suppression, above it the reference's loop against a grid of accepted corners on one wavefront) */
    int block_size;       /* 3   (any size >= 1: 3 runs the tiled kernel, others the general pair of kernels) */
    int gradient_size;    /* 3   (aperture of cornerEigenValsVecs' derivative: Sobel 3 / 5 / 7, or -1 = Scharr; anything else: PC_E_INVALID) */
    int max_corners;      /* 0 = unlimited */
    int use_harris;       /* 0   (1: cornerHarris, gftt.cc:31-33 -- calcHarris' scalar expression (k in double) in the canonical
                                 mode; under PC_ARITH_SOBEL_FMA the first width / 4 * 4 columns of a row as the vector loop of an
                                 x86 build computes them, in float with (float)k, and the scalar expression for the rest;
                                 bit-exact against the oracle's restatement of either -- the reference's addon never takes
                                 this branch) */
    double harris_k;      /* 0.04 */
    int grid_rows;        /* 4 */
    int grid_cols;        /* 4 */
} pc_gftt_options;

/* OpticalFlowOptions, cpp/opticalflow.h:27-33 */
typedef struct pc_flow_options {
    int window_size;            /* 10  (3..PC_MAX_WINDOW) */
    int max_level;              /* 3   (any value >= 0: the pyramid ends where the next level would be <= the window, as in OpenCV) */
    int term_max_iters;         /* 30 */
    double term_epsilon;        /* 0.01 */
    double min_eigen_threshold; /* 1e-4 */
} pc_flow_options;

void pc_gftt_default_options(pc_gftt_options* o);
void pc_flow_default_options(pc_flow_options* o);

const char* pc_last_error(void);
/* Library / build identification ("polychase_hip gfx950 ..."). */
const char* pc_version(void);

/* Process-wide preparation of the HIP runtime for the engine's streams: raises GPU_MAX_HW_QUEUES to 16 unless the
 * environment already holds a value (the engine keeps five streams busy; the runtime maps all streams of a process onto
 * that many hardware queues, 4 by default, and two streams on one queue wait for each other's commands: DESIGN.md
 * section 3).  The runtime reads the variable when the process FIRST touches HIP, so this must run before that;
 * pc_context_create calls it, hosts that initialise HIP themselves (torch, Cycles) call it earlier -- the polychase_core
 * module does when it is imported.  Idempotent.  *runtime_was_up (may be null) = 1 when the ROCm runtime of this process
 * was already initialised at the first call (the setting then has no effect on this process); *hw_queues (may be null) =
 * the value of the variable after the call.  Nothing happens at dlopen any more (round 3 used a library constructor). */
int pc_runtime_init(int* runtime_was_up, int* hw_queues);

/* ---- context: one per GPU (one process per GPU in multi-GPU runs) ---- */
int pc_context_create(int device_index, pc_context** out);
void pc_context_destroy(pc_context* ctx);
int pc_context_synchronize(pc_context* ctx);
/* "0000:c1:00.0" of the context's GPU (hipDeviceGetPCIBusId): the host side looks up the GPU's NUMA node with it (csrc/host/numa_pin.h) */
int pc_context_pci_bus_id(pc_context* ctx, char* buf, int len);
/* Arithmetic mode: where OpenCV's result depends on how the host executes it, which execution the GPU reproduces.
 *   PC_ARITH_CANONICAL      no FMA anywhere; the LK sums (structure tensor, mismatch vector) exact in integers, rounded once
 *   PC_ARITH_LK_X86_ORDER   the LK sums in fp32 in the order of LKTrackerInvoker's CV_SIMD128 path on x86 (four vector lanes
 *                           over the first (win / 8) * 8 columns, a scalar accumulator over the rest; calcOpticalFlowPyrLK,
 *                           cpp/opticalflow.cc:119-125): differs from the canonical order only where a window's partial
 *                           sums exceed 2^24 (step edges), by <= ~2e-3 px.  The kernels run the canonical integer data
 *                           path plus a proof that the fp32 sums are exact, and the x86 order itself where the proof fails
 *                           (+10-18 % on the LK launch at windows 4-10)
 *   PC_ARITH_SOBEL_FMA      the fused multiply-add of the AVX2-dispatched symmetric column filter of Sobel inside
 *                           cornerMinEigenVal (cpp/feature_detection/gftt.cc:35): same corners, the (value, address)
 *                           order of near-ties -- i.e. keypoint indices -- as a stock x86 build produces them; with
 *                           use_harris also calcHarris' vector loop (float, (float)k) over the first width / 4 * 4 columns
 *   PC_ARITH_OPENCV_X86     both
 *   PC_ARITH_SOBEL_ROW_FMA  (not part of the default) additionally the ROW pass of Dy -- the smoothing taps [1, 2, 1] * scale
 *                           over the 8-bit pixels -- as a fused chain t = k0 a; t = fma(k1, b, t); t = fma(k0, c, t): what the
 *                           8u -> 32f vector row filter computes IF the linked OpenCV has one and dispatches it to AVX2 (a
 *                           second hypothesis about the real build; `tests/opencv_crosscheck.py` on a machine with cv2 tells
 *                           which one holds and names the POLYCHASE_ARITH value to use)
 * Bit for bit what oracle/pc_oracle.c computes under pco_set_opencv_emulation(flags).  Default: PC_ARITH_OPENCV_X86 -- the
 * execution of the OpenCV build the reference links (vcpkg, x86-64: SSE baseline, AVX2 / FMA3 dispatched)
 * -- or the environment variable POLYCHASE_ARITH = canonical | opencv_x86 | lk_x86 | sobel_fma | sobel_fma_rows | opencv_x86_rows at
 * context creation. */
#define PC_ARITH_CANONICAL 0
#define PC_ARITH_LK_X86_ORDER 1
#define PC_ARITH_SOBEL_FMA 2
#define PC_ARITH_SOBEL_ROW_FMA 4
#define PC_ARITH_OPENCV_X86 3
/* Synchronous copy of `bytes` bytes of this context's device memory to host memory (debug dump of frames that were handed
 * over as device memory, cpp/opticalflow.cc:80-96). */
int pc_context_download(pc_context* ctx, void* dst_host, const void* src_device, size_t bytes);
int pc_context_set_arithmetic(pc_context* ctx, int flags);
int pc_context_get_arithmetic(const pc_context* ctx);

/* ---- gray conversion (not in the reference): which channels are tracked, and a transfer curve for float frames ----
 * How an RGB frame becomes the gray plane that detection and LK read.  The default is the reference's: cv::cvtColor's
 * Y = (9798 R + 19235 G + 3735 B + 2^14) >> 15 on u8 channels, float channels first through the addon's `(x * 255).astype(uint8)`
 * (pc_frame_set_rgb_f32).  A conversion replaces either part:
 *   weights      three integers weight_r, weight_g, weight_b, each 0 .. 32768, sum exactly 32768:
 *                Y = (weight_r R + weight_g G + weight_b B + 2^14) >> 15 on the u8 channel values in unsigned 32-bit; always
 *                0 .. 255; (32768, 0, 0) gives exactly R.  Callers quantise user weights (r, g, b), finite, >= 0, s = r + g + b > 0,
 *                in fp64 as q_c = floor((c / s) * 32768.0 + 0.5) and add the residual 32768 - (q_r + q_g + q_b) to the channel
 *                with the largest input weight, ties in the order R, G, B.  (0.299, 0.587, 0.114) quantises to (9798, 19234,
 *                3736), NOT to the default's constants: the reference's bits come from the default alone.
 *   float_table  a host pointer to PC_TRANSFER_ENTRIES bytes, or NULL = the `(x * 255)` rule.  With a table a float channel
 *                value v with fp32 pattern `bits` becomes table[idx]: idx = 0 unless v >= 2^-16 (NaN, negatives, zeros,
 *                denormals and tiny values), else idx = min((bits >> 13) - (111 << 10) + 1, PC_TRANSFER_ENTRIES - 1).  Entry
 *                i >= 1 thus covers [x_i, x_i + 2^e / 1024) with e = -16 + (i - 1) / 1024, m = (i - 1) mod 1024,
 *                x_i = 2^e (1 + m / 1024): 20 octaves in 1024 steps each; values >= 16 and +inf read the last entry, so
 *                highlights clamp where the `(x * 255)` rule wraps.  Alpha is ignored.  The three channel values then go through
 *                the weights.  No floating-point arithmetic happens on the device: the kernels look the value up.
 * pc_context_set_gray_conversion: NULL = the default.  Weights outside 0 .. 32768 or with another sum: PC_E_INVALID (checked
 * before the handle), and the previous conversion stays in force.  The table is copied into device memory the context owns.  A
 * per-run call: it may wait for the context's streams.  It takes effect for every frame put afterwards through pc_frame_set_rgb,
 * pc_frame_set_rgb_f32 and pc_analyzer_put_frame[_f32] of this context; weights apply to u8 and float RGB, the table to float
 * frames only; gray sources (pc_frame_set_gray) are untouched.  With the default conversion these calls enqueue exactly what
 * they enqueue without this call ever made.
 * pc_context_get_gray_conversion: the conversion in force; c->float_table is NULL without a table and otherwise `table_out` (may
 * be NULL), which then receives the PC_TRANSFER_ENTRIES bytes.
 * pc_float_transfer_table: the built-in tables, computed on the host in fp64 (no device, no context): entry 0 is 0; for i >= 1
 * y = (x_i + 2^e / 2048) * 2^exposure, the interval's midpoint under an exposure of `exposure` stops, and
 * code = floor(255 * min(f(y), 1) + 0.5) with
 *   PC_TRANSFER_SRGB   f = y <= 0.0031308 ? 12.92 y : 1.055 pow(y, 1 / 2.4) - 0.055   (gamma unused)
 *   PC_TRANSFER_GAMMA  f = pow(y, 1 / gamma)
 * 1 <= gamma <= 4, |exposure| <= 16, both finite; anything else, or another kind: PC_E_INVALID.
 * pc_gray_quantize_weights: the quantisation above of user weights rgb[3] into out->weight_r / _g / _b (float_table is left as it
 * is), on the host -- the one quantiser the driver, polychase_core and the ctypes binding use; a weight that is negative or not
 * finite, or a sum that is not positive: PC_E_INVALID, `out` untouched.
 * pc_float_transfer_index: the table entry idx of each of n float values, computed on the host by the function the kernels
 * compile (testing aid: the rule above is a float compare and a shift, the kernels test an integer range). */
#define PC_TRANSFER_ENTRIES 20481
#define PC_TRANSFER_SRGB 1
#define PC_TRANSFER_GAMMA 2
typedef struct pc_gray_conversion {
    int32_t weight_r, weight_g, weight_b;
    const uint8_t* float_table;
} pc_gray_conversion;
void pc_gray_default_conversion(pc_gray_conversion* c);
int pc_context_set_gray_conversion(pc_context* ctx, const pc_gray_conversion* c);
int pc_context_get_gray_conversion(const pc_context* ctx, pc_gray_conversion* c, uint8_t* table_out);
int pc_float_transfer_table(int kind, double gamma, double exposure, uint8_t* out);
int pc_gray_quantize_weights(const double* rgb, pc_gray_conversion* out);
int pc_float_transfer_index(const float* values, int n, uint32_t* out);

/* ---- lens undistortion at ingest (not in the reference): frames are made pinhole as they are put ----
 * Everything behind the gray plane -- detection, LK, masks, the tracker and the refiner -- assumes a pinhole camera.  With a lens
 * map set, every frame put into the context is resampled into the undistorted camera's pixel grid, so keypoints, flow rows and
 * masks live in ONE undistorted pixel space and none of that code knows a lens existed.  All arithmetic is integer on the device
 * and fp64 on the host; every result is defined bit for bit.
 *   lens map     int32 q[h][w][2]: for the undistorted pixel (u, v) the source position (sx, sy) in the original frame in units of
 *                1 / 256 px (PC_LENS_FRAC_BITS = 8), pixel centres at integers (as in the polygon masks):
 *                q = floor(s * 256 + 0.5), computed in fp64 and clamped to +-2^24.  A source position with a component that is not
 *                finite writes PC_LENS_INVALID (INT32_MIN) to BOTH components.
 *   remap        of the gray plane G (w x h, u8) into U, per (u, v) with entry (qx, qy): an entry with a component equal to
 *                PC_LENS_INVALID gives U = 0.  Otherwise ix = qx >> 8 (arithmetic shift), wx = qx & 255, likewise iy, wy; the four
 *                taps a, b, c, d are G at (clamp(ix, 0, w - 1) | clamp(ix + 1, 0, w - 1), clamp(iy, 0, h - 1) | clamp(iy + 1, 0, h - 1));
 *                top = a (256 - wx) + b wx, bot = c (256 - wx) + d wx, U = (top (256 - wy) + bot wy + 32768) >> 16.
 *                With q = 256 (u, v) this is G itself, bit for bit.
 *   order        GRAY CONVERSION COMES FIRST: an RGB or float source is converted to gray per SOURCE pixel by the context's gray
 *                conversion (default, weights or transfer table, exactly as without a map), and the gray plane is then remapped:
 *                gray kernel -> remap kernel -> level kernel.  (A kernel that fuses the three would have to convert each tap
 *                before blending.)
 *   validity     pixel (u, v) is valid iff 0 <= qx <= (w - 1) 256 and 0 <= qy <= (h - 1) 256: a property of the map, computed on
 *                the host.
 * Two ways to a map, both host-only (no device, no context, like pc_float_transfer_table):
 * pc_lens_build_map: the polynomial model.  The undistorted camera has the focal lengths fx zoom, fy zoom and the same principal
 * point; in fp64, every operation rounded on its own in the order written (the library is built with contraction off):
 *   x = (u - cx) / (fx zoom), y = (v - cy) / (fy zoom), r2 = x x + y y, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *   xd = x rad + 2 p1 x y + p2 (r2 + 2 x x), yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y, sx = xd fx + cx, sy = yd fy + cy.
 * pc_lens_default_model: fx = fy = 1, zoom = 1, everything else 0.
 * pc_lens_map_from_stmap: a float32 st[h][w][2] in [0, 1] that another tool has written (anamorphic and fisheye lenses), pixel
 * centre i at (i + 0.5) / w: sx = (double)s w - 0.5, sy = flip_v ? (1 - (double)t) h - 0.5 : (double)t h - 0.5.  Values outside
 * [0, 1] are taken as they are (the remap clamps its taps); a NaN or an infinity makes the entry PC_LENS_INVALID.
 * pc_lens_map_valid: the validity plane, 255 / 0, eroded: with erode = m >= 0 a pixel stays on iff every pixel of the (2m + 1)^2 box
 * around it that lies inside the frame is valid.  *all_valid (may be null) = 1 iff every byte of `out` is 255.
 * These four refuse with PC_E_INVALID and leave their output untouched: a null argument, a model value that is not finite, fx, fy
 * or zoom <= 0, w or h outside what pc_frame_create takes (>= 1, w h <= 2^30), erode outside 0 .. PC_LENS_MAX_ERODE.
 * pc_context_set_lens_map: q is host memory, copied into device memory the context owns together with two w x h planes; NULL
 * clears the map and frees all three.  A per-run call: it may wait for the context's streams.  It takes effect for every frame put
 * afterwards through pc_frame_set_rgb, _rgb_f32, _gray and pc_analyzer_put_frame[_f32] of this context, with every `on_device`
 * value.  A frame whose size differs from the map's: PC_E_INVALID, the frame left untouched.  A refused setter (null context, a
 * size pc_frame_create would not take) leaves the map in force.  Without a map these calls enqueue exactly what they enqueue
 * without this call ever made.  The remap launch is counted under PC_K_GRAY.
 * pc_context_get_lens_map_size: the size of the map in force, 0 x 0 without one. */
#define PC_LENS_FRAC_BITS 8
#define PC_LENS_INVALID INT32_MIN
#define PC_LENS_MAX_ERODE 64
typedef struct pc_lens_model {
    double fx, fy, cx, cy; /* of the ORIGINAL frames, pixels */
    double k1, k2, k3;     /* radial */
    double p1, p2;         /* tangential */
    double zoom;           /* 1: the undistorted camera keeps fx, fy */
} pc_lens_model;
void pc_lens_default_model(pc_lens_model* m);
int pc_lens_build_map(const pc_lens_model* m, int w, int h, int32_t* q);
int pc_lens_map_from_stmap(const float* st, int w, int h, int flip_v, int32_t* q);
int pc_lens_map_valid(const int32_t* q, int w, int h, int erode, uint8_t* out /* 255 / 0 */, int* all_valid);
int pc_context_set_lens_map(pc_context* ctx, const int32_t* q /* host */, int w, int h);
int pc_context_get_lens_map_size(const pc_context* ctx, int* w, int* h);
/* hipStream_t the context enqueues on (for callers that time with HIP events / torch streams). */
void* pc_context_stream(pc_context* ctx);
/* Timing of the context's kernels with HIP events on the stream each launch is enqueued on.  `class_mask` bit k
 * enables kernel class PC_K_k (0 = off, 0x3ff = all); enabled classes accumulate (launches, total ms).
 * Two event records per timed launch: keep the mask to the class of interest inside timed regions.
 * pc_analyzer overlaps the LK launches of consecutive frames (two job lanes), so `total_ms` -- the sum of the
 * launches' own start-to-end durations -- exceeds the time the class kept the GPU busy; pc_context_get_busy_time
 * returns that: the length of the union of the launches' intervals. */
int pc_context_enable_timing(pc_context* ctx, int class_mask);
int pc_context_get_timing(pc_context* ctx, int kernel_class, int* launches, double* total_ms);
int pc_context_get_busy_time(pc_context* ctx, int kernel_class, double* busy_ms);
int pc_context_reset_timing(pc_context* ctx);
/* Diagnostics of the LK kernel (only a library compiled with -DPC_LK_PROFILE counts anything; otherwise all zeros):
 * shader-clock cycles summed over the wavefronts of the latest launch, per phase --
 * [0] I-side staging, [1] I-side evaluation + 2x2 system, [2] patch pick-up, [3] J-region staging, [4] iterations,
 * [5] error pass, [6] wavefront life time, [7] wavefronts, [8] wavefront-iterations, [9] region stagings. */
#define PC_LK_PROFILE_SLOTS 16
int pc_debug_lk_profile(pc_context* ctx, unsigned long long* out /* [PC_LK_PROFILE_SLOTS] */);
/* Diagnostics of PC_ARITH_LK_X86_ORDER on the two-keypoint LK kernel (windows 4-11).  That kernel runs the canonical
 * integer data path and proves, per level and per iteration, that the fp32 sums of the x86 order would be exact (then
 * they equal the canonical values); only where the proof fails it evaluates the sums in the x86 order.  out (may be
 * null) receives the counters accumulated since counting was enabled: [0] (pair, iteration)s decided by the proof,
 * [1] evaluated in the x86 order, [2] (keypoint, level)s, [3] of those with the structure tensor in the x86 order.
 * enable != 0 (re)starts counting from zero, 0 stops it.  Counting costs a few atomics per wavefront. */
int pc_debug_lk_x86_stats(pc_context* ctx, int enable, unsigned long long* out /* [4] */);
/* Diagnostics of the detection: how the detections of this context ended, counted on the host where a detection's counters
 * arrive (stage calls and analyzers alike) -- [0] detections finished, [1] of those on the fast path, then the detections
 * redone on the slow path, one counter per reason (a detection can have several): [2] more candidates than the candidate
 * buffers hold, [3] the keypoint count at the frame's keypoint capacity, [4] overflow bit 1 (a value bucket of the sort beyond
 * its slots), [5] overflow bit 2, [6] overflow bit 4 (more candidates than the launches covered), [7] POLYCHASE_GFTT_SLOW_PATH.
 * out (may be null) receives the counters; reset != 0 zeroes them afterwards.  No device work. */
#define PC_DETECT_PATH_SLOTS 8
int pc_debug_detection_paths(pc_context* ctx, int reset, unsigned long long* out /* [PC_DETECT_PATH_SLOTS] */);
/* Diagnostics of the device-resident PnP solver: ONE damped 9x9 system through the in-kernel float32 Cholesky
 * factorisation and solve that pc_pnp_solve uses (row-major a81, only the lower triangle is read; l81 receives the
 * factor, x9 the solution of L L^T x = b; *positive_definite = 0 and x9 = 0 when the factorisation fails).  Exists so
 * that the reference's known-answer test (cpp/examples/levmarq_ill_conditioned_float32_issue.cpp:16-63) runs on the
 * device copy of the solver, not only on the host one. */
int pc_debug_llt9(pc_context* ctx, const float* a81, const float* b9, float* l81, float* x9, int* positive_definite);
#define PC_K_GRAY 0
#define PC_K_PYRAMID 1
#define PC_K_MINEIG 2
#define PC_K_NMS 3
#define PC_K_SORT 4
#define PC_K_SUPPRESS 5
#define PC_K_LK 6
#define PC_K_COMPACT 7
#define PC_K_LK_FB 8   /* the backward launch of the forward-backward check (pc_lk_track_fb, pc_analyzer_set_fb_threshold) */
#define PC_K_LK_CORR 9 /* the correlation launch of the minimum-correlation check (pc_lk_track_correlated, pc_analyzer_set_min_correlation) */
#define PC_K_COUNT 10

/* ---- frame: gray image + LK pyramid (+ Scharr derivative planes) + keypoints, resident in HBM ----
 * Replaces the per-frame state of cpp/opticalflow.cc:223-226 (frame1_gray, features, frame1_pyramid)
 * and OpticalFlowCache (:18-37). */
int pc_frame_create(pc_context* ctx, int width, int height, int window_size, int max_level,
                    pc_frame** out);
/* Values of the `on_device` argument of the pc_frame_set_* / pc_analyzer_put_frame* calls:
 * 0 = pageable host memory (copied synchronously: the caller may reuse it when the call returns), 1 = memory the GPU can
 * read (device memory, or pc_host_buffer_alloc memory read over PCIe by the kernels), PC_FRAME_PINNED_HOST = page-locked
 * host memory (pc_host_buffer_alloc) that the caller leaves untouched until the frame has been consumed
 * (pc_analyzer_frame_ingested; for pc_frame_set_*: the next synchronising call): fetched by the copy engine, no wait. */
#define PC_FRAME_PINNED_HOST 2
void pc_frame_destroy(pc_frame* f);

/* cv::cvtColor(COLOR_RGB2GRAY) (opticalflow.cc:259,:298) + cv::buildOpticalFlowPyramid
 * (opticalflow.cc:180-187) in one call.  rgb: H rows of W*3 bytes, row_pitch bytes apart.
 * on_device != 0: rgb is a device pointer; otherwise host memory (copied to the GPU first).
 * Clears the frame's keypoints. */
int pc_frame_set_rgb(pc_context* ctx, pc_frame* f, const uint8_t* rgb, size_t row_pitch, int on_device);
/* Same, from the float32 image Blender hands out: H rows of W*channels floats (channels = 3 or 4,
 * alpha ignored), row_pitch BYTES apart.  Replaces the addon's numpy conversion
 * `(image_data * 255).astype(np.uint8)` (blender_addon/operators/analysis.py:221-233) followed by
 * cvtColor: the same fp32 multiply and truncating cast, on the GPU. */
int pc_frame_set_rgb_f32(pc_context* ctx, pc_frame* f, const float* rgb, size_t row_pitch, int channels, int on_device);
/* Page-locked host memory that the GPU reads directly (hipHostMalloc): a frame copied into such a buffer
 * can be handed to pc_frame_set_rgb* / pc_analyzer_put_frame* with on_device = 1 -- the gray kernel then
 * pulls the pixels over PCIe itself, asynchronously, instead of a blocking pageable copy into a staging
 * buffer.  The buffer must stay untouched until the frame has been converted (for the analyzer: until 4
 * more frames have been put).  Replaces the cv::Mat clone of opticalflow_thread.h:120-132. */
int pc_host_buffer_alloc(size_t bytes, void** out);
void pc_host_buffer_free(void* buffer);
/* Same, from an 8-bit gray image (tests / callers that already hold gray). */
int pc_frame_set_gray(pc_context* ctx, pc_frame* f, const uint8_t* gray, size_t row_pitch, int on_device);
/* Same, from pixels of any type the library takes: H rows of W * channels channels of `pixel_type`, row_pitch_bytes apart (the
 * last row need not have a full pitch).  Every channel becomes a byte on the GPU, by the rule of its type, and the frame is from
 * then on what the byte frame would be (gray conversion by the context's weights, planes of 8 bits):
 *   PC_PIXEL_U8   channels 1 (gray), 3 (RGB) or 4 (RGBA, alpha ignored): the byte itself.  1 and 3 are pc_frame_set_gray and
 *                 pc_frame_set_rgb, bit for bit.
 *   PC_PIXEL_U16  channels 3 or 4 (alpha ignored): b = (v * 255 + 32895) >> 16 in 32-bit unsigned arithmetic, the integer nearest
 *                 to v / 257 (there are no ties).  v = 257 k gives k: a uint8 clip expanded by x * 257 gives the uint8 clip's
 *                 planes.  (NOT the top byte v >> 8, which differs on 16256 values.)  No transfer curve applies, as for uint8.
 *   PC_PIXEL_F16  channels 3 or 4 (alpha ignored): IEEE binary16, widened exactly to binary32 (subnormals, +-0, +-inf kept, NaN
 *                 to a NaN), then the float32 rule -- the `(x * 255).astype(uint8)` rule or, under a float transfer table of
 *                 pc_context_set_gray_conversion, the table entry of the widened value.  A frame h gives the planes of the
 *                 float32 frame h.astype(float32), bit for bit.
 *   PC_PIXEL_F32  channels 3 or 4: pc_frame_set_rgb_f32, bit for bit.
 * PC_E_INVALID, with the frame's planes left as they were: pixels or row_pitch_bytes not a multiple of the channel's size (2 for
 * the 16-bit types, 4 for float32), row_pitch_bytes below a row's bytes, any other channel count, an unknown pixel type. */
enum pc_pixel_type { PC_PIXEL_U8 = 0, PC_PIXEL_U16 = 1, PC_PIXEL_F16 = 2, PC_PIXEL_F32 = 3 };
int pc_frame_set_pixels(pc_context* ctx, pc_frame* f, const void* pixels, size_t row_pitch_bytes, int pixel_type, int channels,
                        int on_device);

int pc_frame_num_levels(const pc_frame* f); /* = maxLevel returned by buildOpticalFlowPyramid + 1 */
int pc_frame_level_size(const pc_frame* f, int level, int* width, int* height);
/* Read-back (tests, debugging).  Layouts are tightly packed, matching OpenCV's padded pyramid:
 * image  (h + 2*win) x (w + 2*win) u8, REFLECT_101 border;
 * deriv  (h + 2*win) x (w + 2*win) x 2 int16 (dx,dy interleaved), zero border. */
int pc_frame_download_gray(pc_context* ctx, const pc_frame* f, uint8_t* out_gray);
int pc_frame_download_level(pc_context* ctx, const pc_frame* f, int level, uint8_t* out_padded);
int pc_frame_download_deriv(pc_context* ctx, const pc_frame* f, int level, int16_t* out_padded);
/* The plane the LK kernels read: (h + 2*win) x (w + 2*win) uint16, every value of the padded image plane << 7. */
int pc_frame_download_level16(pc_context* ctx, const pc_frame* f, int level, uint16_t* out_padded);

/* GoodFeaturesToTrack (cpp/feature_detection/gftt.cc:14-192, called at opticalflow.cc:160) on the
 * frame's gray image; keypoints stay on the device, in acceptance order. */
int pc_frame_detect(pc_context* ctx, pc_frame* f, const pc_gftt_options* opt);
/* The `mask` argument of GoodFeaturesToTrack (gftt.cc:45-83) for the next pc_frame_detect of this frame: H rows of W bytes,
 * row_pitch bytes apart, host memory (on_device = 0, copied before the call returns) or device memory (on_device = 1, read
 * stream-ordered: keep it until the next synchronising call).  Any non-zero byte is "on".  As in the reference, the response
 * map is that of the whole image; a grid cell's maxVal is the maximum over its pixels that are on (0.0 for a cell with none,
 * what cv::minMaxLoc reports for an empty mask); the threshold maxVal * quality_level and the 3x3 dilation apply to every
 * pixel, on or off; and only a pixel that is on can become a candidate.  This is NOT the unmasked result filtered by the mask:
 * a pixel that is off still suppresses its neighbours in the dilation, and masking out a cell's brightest region lowers that
 * cell's threshold.  Sort, greedy suppression, max_corners and the keypoint order are untouched.  The mask stays with the
 * frame until it is replaced or cleared (mask = NULL); a frame that never had one allocates nothing and runs the unmasked
 * kernels.  Null context or frame, or row_pitch < W: PC_E_INVALID. */
int pc_frame_set_mask(pc_context* ctx, pc_frame* f, const uint8_t* mask, size_t row_pitch, int on_device);
/* The same mask given as outlines and rasterised on the GPU (kernels_mask.hip), so that no plane crosses the bus: a list of
 * n_polygons closed polygons (0..PC_MASK_MAX_POLYGONS), polygon k with counts[k] >= 3 vertices, PC_MASK_MAX_VERTICES in all;
 * xy holds them one after another, (x, y) float32 in pixel coordinates: pixel (px, py) has its centre at (px, py).  A polygon
 * closes from its last vertex to its first; it may lie partly or wholly outside the frame.  The fill rule is exact, in integers:
 *   1. every coordinate is snapped to X = rint(x * PC_MASK_SUBPIXEL), round-half-to-even (on the host);
 *   2. with P = (16 px, 16 py), an edge A -> B is crossed when (Ay <= Py) != (By <= Py); a crossed edge lies to the right of P
 *      when d = (Bx - Ax)(Py - Ay) - (Px - Ax)(By - Ay) is > 0 for By > Ay, < 0 for By < Ay (64-bit integers);
 *   3. a pixel is inside a polygon when an odd number of that polygon's edges are crossed to its right (even-odd), on when it
 *      is inside at least one polygon (union), and `invert` flips the result.
 * So an integer-cornered rectangle (x0, y0)-(x1, y1) turns on x0 <= px < x1, y0 <= py < y1; polygons that share an edge share
 * no pixel; orientation does not matter; horizontal and zero-length edges never cross.  Holes are not expressible (a polygon
 * inside another adds nothing to the union): pass a keyhole outline.  0 polygons: everything off (on with invert).
 * The effect on the next pc_frame_detect is that of pc_frame_set_mask with the plane the rule gives; pc_frame_set_mask(NULL)
 * clears it.  xy and counts are host memory, consumed before the call returns.  PC_E_INVALID, with the previous mask left in
 * force: a null handle or array, n_polygons outside 0..PC_MASK_MAX_POLYGONS, a count below 3, more than PC_MASK_MAX_VERTICES
 * vertices, a coordinate that is not finite or has |x| > 32768. */
#define PC_MASK_MAX_POLYGONS 32
#define PC_MASK_MAX_VERTICES 4096
#define PC_MASK_SUBPIXEL     16
int pc_frame_set_mask_polygons(pc_context* ctx, pc_frame* f, const float* xy, const int32_t* counts, int n_polygons, int invert);
/* tests, debugging: the frame's current mask plane, w*h bytes (255 / 0 for a polygon mask, the caller's bytes for a byte
 * mask); PC_E_STATE when the frame has no mask on */
int pc_frame_download_mask(pc_context* ctx, const pc_frame* f, uint8_t* out);
/* tests, debugging: the choked plane C_margin of the frame's current mask (target-side masks below: pc_lk_track_masked), w*h
 * bytes, 255 / 0; margin 0: the mask read as on/off.  PC_E_STATE when the frame has no mask on, PC_E_INVALID for a margin
 * outside 0..PC_TARGET_MASK_MAX_MARGIN. */
#define PC_TARGET_MASK_MAX_MARGIN 31
int pc_frame_download_choked_mask(pc_context* ctx, const pc_frame* f, int margin, uint8_t* out);
/* cv::cornerMinEigenVal map of the last pc_frame_detect (gftt.cc:35), w*h floats (tests). */
int pc_frame_download_min_eig(pc_context* ctx, const pc_frame* f, float* out_eig);
/* Number of local-maximum candidates of the last pc_frame_detect (gftt.cc:76-86) (tests). */
int pc_frame_num_candidates(pc_context* ctx, const pc_frame* f, int* out_n);
int pc_frame_num_keypoints(pc_context* ctx, const pc_frame* f, int* out_n);
int pc_frame_download_keypoints(pc_context* ctx, const pc_frame* f, float* out_xy, int capacity);
/* Keypoints read back from the database on resume (opticalflow.cc:168-178). host pointer, n x 2. */
int pc_frame_set_keypoints(pc_context* ctx, pc_frame* f, const float* xy, int n);

/* cv::calcOpticalFlowPyrLK(frame1 pyramid, target pyramid, frame1 keypoints, ...) (opticalflow.cc:119-125)
 * for n_targets targets in one launch.  Raw outputs (host pointers), target-major:
 *   next_xy [n_targets][N][2], status [n_targets][N], err [n_targets][N],  N = keypoints of frame1. */
int pc_lk_track(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                const pc_flow_options* opt, float* next_xy, uint8_t* status, float* err);

/* Same + the status==1 filter of opticalflow.cc:130-147, compacted on the device, ascending
 * keypoint index.  Host outputs, each with room for n_targets*N rows; rows of target t start at
 * row_offset[t] (row_offset has n_targets+1 entries; row_offset[n_targets] = total rows). */
int pc_lk_track_filtered(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets,
                         int n_targets, const pc_flow_options* opt, uint32_t* src_indices,
                         float* tgt_xy, float* flow_err, int64_t* row_offset);

/* ---- forward-backward consistency check (Kalal et al., 2010; not in the reference, off by default) ----
 * fb_threshold (pixels at level 0) > 0: every row with forward status 1 is tracked back,
 * calcOpticalFlowPyrLK(prev = target, next = frame1, pts = {q}, the same options, no initial flow), from the fp32 end point
 * q the forward pass stored, in one additional launch (kernels_lk_fb.hip), bit for bit the oracle's pco_lk in the context's
 * arithmetic mode.  With b the backward end point, p the keypoint, dx = b.x - p.x, dy = b.y - p.y, d2 = dx * dx + dy * dy
 * (every operation rounded to fp32 on its own) and thr2 = (float)((double)fb_threshold * fb_threshold), the row's final status
 * is 1 iff status_f == 1 && status_b == 1 && d2 <= thr2 (a NaN fails).  next_xy and err stay the forward pass's values.
 * fb_threshold == 0: exactly pc_lk_track / pc_lk_track_filtered (nothing else is enqueued).  Negative, NaN or infinite:
 * PC_E_INVALID.
 * pc_lk_track_fb: `status` is the final status; back_xy [n_targets][N][2] and back_status [n_targets][N] (either may be NULL)
 * receive b and status_b -- (0, 0) and 0 where the forward status is 0, and everywhere when fb_threshold == 0. */
int pc_lk_track_fb(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                   const pc_flow_options* opt, double fb_threshold, float* next_xy, uint8_t* status, float* err,
                   float* back_xy, uint8_t* back_status);
/* pc_lk_track_filtered on the final status. */
int pc_lk_track_filtered_fb(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets,
                            int n_targets, const pc_flow_options* opt, double fb_threshold, uint32_t* src_indices,
                            float* tgt_xy, float* flow_err, int64_t* row_offset);

/* ---- target-side masks (not in the reference, off by default) ----
 * A detection mask keeps keypoints out of a region of frame1; this keeps ROWS out that END in the masked-out region of their
 * target (a background keypoint that a matted-out actor covers in the target frame).  on(x, y): the target's mask byte is
 * non-zero.  Choked plane of margin r, 0 <= r <= PC_TARGET_MASK_MAX_MARGIN: C_r(x, y) = 255 when on(x', y') holds for every
 * pixel of the frame with |x' - x| <= r and |y' - y| <= r, else 0 -- pixels outside the frame are ignored; C_0 is the mask read
 * as on/off (kernels_mask.hip: mask_choke_kernel).  A forward record (q, err, status_f == 1) is judged at the pixel
 *   ix = (int) fminf(fmaxf(floorf(q.x + 0.5f), 0.f), (float)(w - 1)),   iy likewise with q.y and h,
 * every operation rounded to fp32: an end point outside the frame (OpenCV keeps such rows) by the nearest border pixel, a NaN
 * by pixel 0.  The row's status becomes 0 when its target has a mask on (pc_frame_set_mask / _polygons) and C_r(ix, iy) == 0;
 * next_xy and err are untouched, and a target without a mask keeps every row.  With fb_threshold > 0 the final status is the
 * AND of both checks; the mask test runs first, so the backward launch does no work for the rows it dropped.
 * pc_lk_track_masked: pc_lk_track_fb without the back outputs, under the margin.  margin == -1: exactly pc_lk_track_fb
 * (nothing else is enqueued); margin outside -1..PC_TARGET_MASK_MAX_MARGIN: PC_E_INVALID. */
int pc_lk_track_masked(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                       const pc_flow_options* opt, double fb_threshold, int margin, float* next_xy, uint8_t* status, float* err);

/* ---- minimum correlation (not in the reference, off by default) ----
 * The patch error `err` is OpenCV's L1 difference, which is not invariant to exposure: a gain or bias change between the frames
 * raises it for every row.  This check judges a row by the normalised cross-correlation of the two windows LK itself compared.
 * Take a forward record of a pair (keypoint p of frame1, target t) with status 1 and stored fp32 end point q; win = window_size,
 * n = win * win, half = (float)(win - 1) * 0.5f.
 *   I window   the win x win values ival that LK's template pass takes at level 0 from frame1's u8 plane at p - half: floor, fp32
 *              fractions a, b, the 14-bit weights with iw11 = 2^14 - iw00 - iw01 - iw10 (which may be -1), DESCALE(., 9): values
 *              x 32 in 0..8160.
 *   J window   the same expression at q - half in the target's level-0 u8 plane: the window the err pass evaluates, before I is
 *              subtracted.
 *   bounds     a status-1 record has passed OpenCV's bounds test for both windows on these same floats; the kernel repeats the
 *              test and drops a record that fails it, and never reads outside the padded plane, whatever it is handed.
 *   sums       exact integers (int64: n * sum(I^2) <= 961 * 961 * 8160^2 ~ 6.2e13): cov = n sum(IJ) - sum(I) sum(J),
 *              vI = n sum(I^2) - sum(I)^2, vJ = n sum(J^2) - sum(J)^2.
 *   decision   without a square root: t2 = (double)min_correlation * (double)min_correlation, computed once on the host; the row
 *              keeps status 1 iff cov > 0 && (double)cov * (double)cov >= ((double)vI * (double)vJ) * t2, every operation rounded
 *              to fp64 on its own (no contraction; the int64 -> double conversions are exact).  A flat window (vI == 0 or
 *              vJ == 0) gives cov == 0 and is dropped.  next_xy and err of the rows that stay are untouched.
 *   score      (stage-level call only) corr = (float)((double)cov / sqrt((double)vI * (double)vJ)), or 0 when either variance is 0.
 * min_correlation == 0: no filter; valid values are 0 <= v <= 1; NaN, negative or > 1: PC_E_INVALID.  The final status is the AND
 * of all enabled checks; the order on the lane is target mask, correlation, forward-backward, so the backward launch does no work
 * for rows already dropped (kernels_lk_corr.hip; the rule restated in numpy: tests/lk_correlation_ref.py).
 * pc_lk_track_correlated: pc_lk_track_masked plus the check.  corr ([n_targets][N], may be NULL) receives the score, 0 wherever
 * the record reached the pass with status 0.  min_correlation == 0 and corr == NULL: exactly pc_lk_track_masked (nothing else is
 * enqueued); min_correlation == 0 and corr != NULL: the pass runs and only writes scores. */
int pc_lk_track_correlated(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                           const pc_flow_options* opt, double min_correlation, double fb_threshold, int margin, float* next_xy,
                           uint8_t* status, float* err, float* corr);

/* ---- brightness normalisation (not in the reference, off by default) ----
 * LK assumes brightness constancy: its mismatch vector is b = sum (J - I) grad I, and a bias c between the two frames adds
 * c sum grad I to it -- non-zero for every window with a net gradient, so an exposure ramp or a flicker displaces every end point.
 * With normalize == 1 every LK pass of the call (the forward launch, and the backward launch of the forward-backward check where
 * fb_threshold > 0) runs the rule below instead: Gauss-Newton on g (J - mean J) - (I - mean I), g the ratio of the two windows'
 * standard deviations.  The residual has zero sum, so the gradient means drop out of b and a bias changes nothing at all.
 * The rule is OpenCV's pass (oracle/pc_oracle.c: pco_lk; lk_plain.hpp: plain_lk_pair) level by level -- the bounds tests, the
 * bilinear weights, the template values ival (0..8160), ix, iy (DESCALE by 9 / 14), the interpolation of the searched plane, the
 * 2x2 solve, the epsilon test, the oscillation exit and the level-0 L1 patch error are identical in fp32 -- with two
 * replacements.  n = win * win; every sum is an exact integer (int64), every fp64 operation is rounded on its own (no
 * contraction), and the arithmetic mode (pc_context_set_arithmetic) plays no part.
 *   template, once per level   over the window (x = ix, y = iy, I = ival): S_I, S_II, S_x, S_y, S_xx, S_xy, S_yy, S_Ix, S_Iy;
 *              G11 = n S_xx - S_x^2, G12 = n S_xy - S_x S_y, G22 = n S_yy - S_y^2, C_Ix = n S_Ix - S_I S_x, C_Iy = n S_Iy - S_I S_y,
 *              vI = n S_II - S_I^2 (all below 2^53);  A11 = (float)((double)G11 / (double)n) * FLT_SCALE, A12 and A22 likewise:
 *              the centred Gram matrix.  The bias is eliminated, so a pure ramp is degenerate: the unchanged D / min_eig test
 *              refuses it.
 *   each iteration   over the J window (J = the interpolated value, 0..8160): T_J, T_JJ, T_Jx = sum J ix, T_Jy = sum J iy;
 *              vJ = n T_JJ - T_J^2, C_Jx = n T_Jx - T_J S_x, C_Jy = n T_Jy - T_J S_y;
 *              gain: vI > 0 && vJ > 0 ? g = (float)sqrt((double)vI / (double)vJ) clamped to [0.25f, 4.0f] : g = 1.0f;
 *              b1 = (float)(((double)g * (double)C_Jx - (double)C_Ix) / (double)n) * FLT_SCALE, b2 likewise with C_Jy, C_Iy.
 * The stored err stays OpenCV's un-normalised L1 patch error; min_correlation is the gain-invariant measure of a row, and the two
 * options compose (the correlation pass judges the normalised rows like any others).  Records, target-mask test, correlation pass,
 * compaction and unpacking are unchanged (kernels_lk_norm.hip; the rule restated in numpy: tests/lk_normalized_ref.py).
 * pc_lk_track_normalized: normalize == 0 is exactly pc_lk_track_correlated without scores, plus the back outputs of
 * pc_lk_track_fb (nothing else is enqueued); normalize == 1 swaps the LK launches, timed under PC_K_LK and PC_K_LK_FB as before.
 * Any other value: PC_E_INVALID. */
int pc_lk_track_normalized(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                           const pc_flow_options* opt, int normalize, double min_correlation, double fb_threshold, int margin,
                           float* next_xy, uint8_t* status, float* err, float* back_xy, uint8_t* back_status);

/* ---- affine refinement (not in the reference, off by default) ----
 * Every LK pass tracks a translating window.  Between frames up to 8 apart a rolling or zooming camera rotates and scales the
 * window's content, and the translational fit then lands a fraction of a pixel off.  With affine == 1 ONE additional launch,
 * directly after the forward launch, refines the end point of every forward record with status 1 at level 0 under a 6-parameter
 * warp of the window (Blender's tracker calls it the affine motion model).  It is a refinement, not a check: it overwrites
 * (q.x, q.y, err) of the record when the result is accepted, leaves the record untouched bit for bit otherwise, and never changes a
 * status.  It runs before the target-mask test, the correlation pass and the backward launch, which judge the refined end points.
 * win = window_size, n = win * win, half = (float)(win - 1) * 0.5f.  Every fp32 and fp64 operation is rounded on its own (no
 * contraction), every sum is an exact integer (int64), and the arithmetic mode (pc_context_set_arithmetic) plays no part.
 *   template   the correlation pass's I window plus the derivatives: at p - half in frame1's level-0 planes, floor, the bounds
 *              test, the 14-bit weights and the template values ival (0..8160), ix, iy (DESCALE by 9 / 14) of LK's template pass,
 *              per window pixel (c, r).  A template that fails the bounds test: no refinement for any of the keypoint's rows.
 *   Jacobian   U = 2c - (win - 1), V = 2r - (win - 1) (twice the offset from the window centre); per pixel
 *              g = (ix U, ix V, iy U, iy V, ix, iy); H[i][j] = sum g_i g_j: 21 exact integers below 2^53.
 *   factor     once per keypoint, lower Cholesky of (double)H in fp64, column by column, j = 0..5: s = H[j][j]; for ascending
 *              k < j: s = s - L[j][k] * L[j][k]; no refinement unless s > 0; L[j][j] = sqrt(s); for i > j: s = H[i][j]; for
 *              ascending k < j: s = s - L[i][k] * L[j][k]; L[i][j] = s / L[j][j].
 *   state      per row: centre (cx, cy) = q, the stored fp32 end point; m11 = m22 = 1.0f, m12 = m21 = 0.0f.
 *   warped J window   pixel (c, r): u = (float)U * 0.5f, v = (float)V * 0.5f; xj = (cx + m11 * u) + m12 * v,
 *              yj = (cy + m21 * u) + m22 * v; fx = floorf(xj), fy = floorf(yj).  The window FAILS unless -win <= fx <= w + win - 2
 *              and -win <= fy <= h + win - 2 hold for every pixel (a NaN fails): every tap then lies inside the padded plane, so
 *              the kernel never reads outside it, whatever it is handed.  The pixel's weights are LK's 14-bit ones of
 *              (xj - fx, yj - fy) with w11 = 2^14 - w00 - w01 - w10; jv = DESCALE(., 9) of the four taps of the target's level-0
 *              u8 plane, 0..8160.
 *   iteration  at most term_max_iters times (clamped to 0..100 as in LK; eps = term_epsilon clamped to [0, 10]): evaluate the
 *              warped window -- a failed window ends the refinement with the row unchanged --; e = jv - ival; b_i = sum e g_i, six
 *              exact integers below 2^44; solve L L^T t = -b in fp64: forward, i = 0..5: s = -(double)b_i; for ascending k < i:
 *              s = s - L[i][k] * y_k; y_i = s / L[i][i]; backward, i = 5..0: s = y_i; for ascending k > i: s = s - L[k][i] * t_k;
 *              t_i = s / L[i][i].  Update in fp32: m11 += (float)(2.0 * t0), m12 += (float)(2.0 * t1), m21 += (float)(2.0 * t2),
 *              m22 += (float)(2.0 * t3), cx += (float)t4, cy += (float)t5.  Stop when
 *              (t4^2 + t5^2) + (double)(win - 1)^2 * (((t0^2 + t1^2) + t2^2) + t3^2) <= eps^2 in fp64.
 *   final      the warped window once more at the final parameters (a failed window leaves the row unchanged):
 *              err_a = (float)sum |jv - ival| / (float)(32 * n).
 *   acceptance in fp32, all of: err_a <= err (the record's stored patch error); 0.5f <= m11 * m22 - m12 * m21 <= 2.0f;
 *              |m11 - 1|, |m12|, |m21|, |m22 - 1| <= 0.5f; (cx - q.x)^2 + (cy - q.y)^2 <= half^2.  Accepted: the record becomes
 *              (cx, cy, err_a, status 1); otherwise it stays (q.x, q.y, err, 1).
 * A target identical to frame1 has e = 0 everywhere: every row whose template has a factor is accepted and stays bit-identical, m
 * exactly the identity.  A row is never replaced by one that matches its patch worse.  At wide windows six parameters fit noise:
 * rows of an unrelated target are accepted too, and dropping them stays the job of the checks that follow.
 * The residual assumes brightness constancy: affine == 1 together with normalize == 1 is PC_E_INVALID (a gain-aware affine
 * residual is a follow-up).  Records, compaction, unpacking and everything downstream are unchanged (kernels_lk_affine.hip; the
 * rule restated in numpy: tests/lk_affine_ref.py).
 * pc_lk_track_affine: affine == 0 is exactly pc_lk_track_normalized (nothing else is enqueued); affine == 1 adds the launch, timed
 * under PC_K_LK (a call then shows two launches of that class).  affine_m ([n_targets][N][4] floats (m11, m12, m21, m22), may be
 * NULL) receives the matrix the refinement ended with; affine_state ([n_targets][N] bytes, may be NULL): 0 = not run (forward
 * status 0, or affine == 0), 1 = accepted, 2 = run and left unchanged.  affine_m is zero where the state is 0.  Any value other than
 * 0 and 1: PC_E_INVALID. */
int pc_lk_track_affine(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                       const pc_flow_options* opt, int affine, int normalize, double min_correlation, double fb_threshold, int margin,
                       float* next_xy, uint8_t* status, float* err, float* back_xy, uint8_t* back_status, float* affine_m,
                       uint8_t* affine_state);

/* ---- search prepass (not in the reference, off by default) ----
 * Pyramidal LK starts at zero displacement and reaches about a window's width per level.  Past that the rows are not dropped: they
 * come back with status 1 and a wrong end point.  With search_radius = R > 0 ONE additional launch, directly after the forward
 * launch, finds per (keypoint, target) pair an integer displacement d by block matching, runs LK once more from p + d and keeps
 * whichever of the two records has the smaller stored patch error (Blender's tracker calls the brute-force search its prepass).  It
 * is a rescue, not a check: a record is never replaced by one with a larger patch error, and a row with forward status 0 can gain
 * status 1.  It runs before the affine refinement, the target-mask test, the correlation pass and the backward launch, which judge
 * the chosen end points unchanged.  Every fp32 and fp64 operation is rounded on its own, every sum is an exact integer, and the
 * arithmetic mode (pc_context_set_arithmetic) plays no part.  T = the top level both pyramids have, min(max_level, levels - 1).
 *   level, radius  s = the smallest level >= 0 with ceil(R / 2^s) <= 16, clamped to T; r = min(16, ceil(R / 2^s)).  w_s, h_s: the
 *              level's interior size.  The block is 8 x 8 u8 pixels of the interior planes at level s.
 *   template   lscale = 1.f / (float)(1 << s); cx = (int)floorf(p.x * lscale + 0.5f), cy likewise; origin (ox, oy) = (cx - 4,
 *              cy - 4).  The block is inside when 0 <= ox, ox + 8 <= w_s, 0 <= oy and oy + 8 <= h_s.  A keypoint whose block is
 *              not inside (a non-finite or out-of-frame p included) is not searched: state 0, d = 0, record untouched.
 *   candidates all integer (dx, dy), |dx|, |dy| <= r, whose block at (ox + dx, oy + dy) in the target's level-s plane is inside by
 *              the same test.  No padding pixel is ever compared, and the kernel never reads outside the planes, whatever it is
 *              handed.  SAD = the sum over the 64 pixels of |J - I|, an exact integer <= 16320.
 *   choice     the candidate with the smallest key (SAD, dx^2 + dy^2, dy, dx), compared lexicographically.  It is accepted when
 *              4 * SAD_best <= 3 * SAD_zero, SAD_zero the SAD of (0, 0), which is always a candidate; otherwise d = 0.
 *              d = (dx << s, dy << s) in level-0 pixels.  d = 0: state 0, nothing more for this pair.
 *   guided pass   for d != 0: the canonical (integer-exact) plain LK pass with the patch error, pco_lk under PCO_EMU_CANONICAL,
 *              template at p, with ONE change: at level T the search starts at guess * lscale_T instead of p * lscale_T, guess =
 *              (p.x + (float)d.x, p.y + (float)d.y) -- OPTFLOW_USE_INITIAL_FLOW.  Bounds tests, weights, template values, the
 *              2 x 2 solve, the epsilon test, the oscillation exit, the level-0 error and the status rules are unchanged.
 *              -> (q_g, err_g, status_g).
 *   keep the better   the forward record (q_f, err_f, status_f) becomes (q_g, err_g, 1) iff status_g == 1 && (status_f == 0 ||
 *              err_g < err_f), compared in fp32 (a NaN fails): state 1.  Otherwise it stays bit for bit: state 2.
 *   forward-backward   rows in state 1 are tracked back by the same canonical pass from template q in the target, searched in
 *              frame1, with level T started at (q.x - (float)d.x, q.y - (float)d.y), and judged by the d2 <= thr2 rule of
 *              pc_lk_track_fb into the same back_xy / back_status; every other row goes through the usual backward launch.
 * The block matching assumes brightness constancy: search_radius > 0 together with normalize == 1 is PC_E_INVALID (a gain-aware
 * search is a follow-up), and so is a radius outside 0 .. 256.  Records, compaction, unpacking and everything downstream are
 * unchanged (kernels_lk_search.hip; the rule restated in numpy: tests/lk_search_ref.py).
 * pc_lk_track_search: search_radius == 0 is exactly pc_lk_track_affine (nothing else is enqueued); > 0 adds the launch, timed under
 * PC_K_LK, and with fb_threshold > 0 one small backward launch for the rows in state 1, timed under PC_K_LK_FB.  search_d
 * ([n_targets][N][2] int16, may be NULL) receives d of every pair, zero in state 0; search_state ([n_targets][N] bytes, may be
 * NULL): 0 = no displacement (or search_radius == 0), 1 = record replaced, 2 = searched and record kept. */
int pc_lk_track_search(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                       const pc_flow_options* opt, int search_radius, int affine, int normalize, double min_correlation,
                       double fb_threshold, int margin, float* next_xy, uint8_t* status, float* err, float* back_xy,
                       uint8_t* back_status, float* affine_m, uint8_t* affine_state, int16_t* search_d, uint8_t* search_state);

/* ---- masked windows (Blender's use_mask; not in the reference, off by default) ----
 * A detection mask decides which keypoints exist and a target-side mask which rows survive; neither decides what a row's window
 * looks at.  A keypoint inside the mask but closer than half a window to its outline builds its template partly from pixels outside
 * the mask -- another layer, moving differently -- and its translational fit is a compromise between two motions.  With
 * mask_windows = 1 the template pixels outside the mask carry no weight.  on(x, y): the frame's mask byte is non-zero
 * (pc_frame_set_mask / _polygons); a frame without a mask on has no weights and is tracked exactly as without the option.
 *   weight planes   one per pyramid level.  M_0 = on.  For level l >= 1 of size (w_l, h_l): M_l(x, y) = the AND over dx, dy in
 *              -2 .. 2 of M_{l-1}(r(2x + dx, w_{l-1}), r(2y + dy, h_{l-1})), r the BORDER_REFLECT_101 index map -- exactly the pixels
 *              pyrDown read to make that pixel: a level pixel is on only if no off pixel contributed to it.  W_l(x, y) = the AND of
 *              M_l over |dx|, |dy| <= 1, the Scharr support; neighbours outside the level count as on, and every position outside
 *              the level (the padding) is on (kernels_mask.hip; pc_frame_download_window_weights).
 *   sample weight   the template sample (x, y) of the window with integer origin (ipx, ipy) reads the four taps (ipx + x + {0, 1},
 *              ipy + y + {0, 1}); it is on iff all four are on in W_l.  The bilinear weights do not enter the test.  n_on = the
 *              number of on samples of the window.
 *   the pass   the plain pass -- pco_lk of the oracle, lk_plain.hpp's plain_lk_pair -- with four changes, everything else the same
 *              fp32 and integer expression in the same order, canonical or PC_ARITH_LK_X86_ORDER:
 *              1. ix and iy of an off sample are 0 (ival is kept), so off samples add exact zeros to the A and b sums in either
 *                 accumulation order;
 *              2. if 4 * n_on < win * win the level fails like the min-eig test: status 0 at level 0, level skipped otherwise;
 *              3. the min-eig divisor is (float)(2 * n_on);
 *              4. the level-0 patch error sums |diff| over the on samples only and divides by (float)(32 * n_on).
 *              With every sample on every expression is the plain pass's: a window that touches no off sample gives its bits.
 *   which weights   those of the template image: frame1's in the forward pass; in the backward pass of the forward-backward check
 *              the target's, if the target has a mask on -- otherwise the plain backward pass.
 * A keypoint is TOUCHED when, at some level that passes the bounds test, its template window has an off sample.  One more launch
 * directly after the forward launch tracks the touched keypoints again under the rule and overwrites their records
 * (kernels_lk_wmask.hip; timed under PC_K_LK); the records of every other keypoint are the product kernel's, bit for bit.  With
 * fb_threshold > 0 and a masked target the weighted backward launch replaces the plain one (timed under PC_K_LK_FB).
 * fb_threshold and the target-side margin compose with the option.  normalize, the affine refinement, the search prepass and a
 * minimum correlation do not weight their windows: an analyzer or a job with one of them and mask_windows = 1 is PC_E_INVALID,
 * before anything is launched, and so is a mask_windows other than 0 or 1.  (The rule restated in numpy:
 * tests/lk_window_mask_ref.py.)
 * pc_lk_track_window_masked: mask_windows == 0 is exactly pc_lk_track_masked plus the back outputs of pc_lk_track_fb (nothing
 * else is enqueued).  touched ([N] bytes, may be NULL) receives 1 for the touched keypoints, 0 elsewhere and everywhere when the
 * option is off or frame1 has no mask on. */
int pc_lk_track_window_masked(pc_context* ctx, const pc_frame* frame1, const pc_frame* const* targets, int n_targets,
                              const pc_flow_options* opt, int mask_windows, double fb_threshold, int margin, float* next_xy,
                              uint8_t* status, float* err, float* back_xy, uint8_t* back_status, uint8_t* touched);
/* tests, debugging: the weight plane W_level of the frame's current mask with its padding, (w_l + 2 win) x (h_l + 2 win) bytes,
 * 255 / 0, the layout of pc_frame_download_level.  Makes the planes if the mask changed since they were made.  PC_E_STATE when the
 * frame has no mask on, PC_E_INVALID for a level the frame does not have. */
int pc_frame_download_window_weights(pc_context* ctx, pc_frame* f, int level, uint8_t* out_padded);

/* ---- analyzer: the pipelined per-clip engine behind GenerateOpticalFlowDatabase ----
 * (cpp/opticalflow.cc:209-321).  Holds a ring of resident frames (the reference's 17-frame
 * SequentialWrapper cache, cpp/opticalflow_thread.h:34-79, generalised), builds every frame's gray
 * image and pyramid ONCE (the reference rebuilds them per pair, opticalflow.cc:298-302), and runs
 * frame1 jobs asynchronously: submit() enqueues, collect() hands back the records of the oldest
 * job in pinned host memory.  Internally three HIP streams: frame preparation (gray, pyramid,
 * detection, keypoint ordering) and two job lanes that take the frame1 jobs alternately -- a job's LK
 * launch, its compaction, device-log append and record download stay on one lane, so the launches of
 * consecutive frames overlap; per-slot events carry the dependencies.
 * One analyzer per context; calls are not thread-safe. */
typedef struct pc_analyzer pc_analyzer;

typedef struct pc_frame_result {
    int32_t frame1;
    int32_t n_keypoints;
    int32_t keypoints_detected;            /* 1: detected by this run (a new `keypoints` row), 0: supplied */
    const float* keypoints_xy;             /* n_keypoints x 2 (gftt.cc acceptance order) */
    int32_t n_targets;
    int32_t targets[PC_MAX_TARGETS];       /* frame ids, in submit order */
    int64_t row_offset[PC_MAX_TARGETS + 1];/* rows of target t: [row_offset[t], row_offset[t+1]) */
    const uint32_t* src_indices;           /* src_keypoints_indices, ascending per target */
    const float* tgt_xy;                   /* tgt_keypoints, rows x 2 */
    const float* flow_err;                 /* flow_errors */
} pc_frame_result;

#define PC_ANALYZER_SPARE_SLOTS 3
#define PC_ANALYZER_LOOKAHEAD 1
int pc_analyzer_create(pc_context* ctx, int width, int height, const pc_gftt_options* gftt,
                       const pc_flow_options* flow, int ring_frames, int max_jobs, pc_analyzer** out);
void pc_analyzer_destroy(pc_analyzer* a);
/* Back to the state after pc_analyzer_create -- no resident frame, no job, no device log -- keeping every allocation
 * (frame slabs, detection scratch, pinned result buffers, streams and events): the next clip of the same geometry and
 * options starts without the tens of milliseconds of creation and destruction (analysis_driver.cc keeps one idle engine
 * per process).  Fails with PC_E_STATE while jobs are in flight.  Synchronises the analyzer's streams. */
int pc_analyzer_reset(pc_analyzer* a);
/* Make `frame_id` resident (evicting the frame ring_frames + PC_ANALYZER_SPARE_SLOTS ids back: the ring holds three
 * slots more than asked for, so that a put never waits for LK launches that still read older frames and the caller
 * can run PC_ANALYZER_LOOKAHEAD = 1 frame ahead of the window frame1 - 8 .. frame1 + 8 of the current submit):
 * RGB->gray + pyramid, and, when will_detect != 0, the dense part of GoodFeaturesToTrack.
 * Replaces RequestFrame + cvtColor + GeneratePyramid (opticalflow.cc:249-263, :287-302). */
int pc_analyzer_put_frame(pc_analyzer* a, int32_t frame_id, const uint8_t* rgb, size_t row_pitch,
                          int on_device, int will_detect);
/* pc_analyzer_put_frame for a float32 frame (see pc_frame_set_rgb_f32). */
int pc_analyzer_put_frame_f32(pc_analyzer* a, int32_t frame_id, const float* rgb, size_t row_pitch, int channels,
                              int on_device, int will_detect);
/* pc_analyzer_put_frame for pixels of any type the library takes: the pixel types, channel counts, per-channel rules (uint16:
 * (v * 255 + 32895) >> 16; float16: widened exactly, then the float32 rule; a fourth channel is ignored) and refusals of
 * pc_frame_set_pixels.  A refused call leaves the ring as it was. */
int pc_analyzer_put_frame_pixels(pc_analyzer* a, int32_t frame_id, const void* pixels, size_t row_pitch_bytes, int pixel_type,
                                 int channels, int on_device, int will_detect);
int pc_analyzer_has_frame(const pc_analyzer* a, int32_t frame_id);
/* 1 when the pixels handed to pc_analyzer_put_frame for `frame_id` are no longer read (its gray conversion has
 * finished, or the frame has left the ring), 0 while the GPU may still read them.  Device / pinned sources are read
 * asynchronously: the caller keeps such a buffer alive, and unmodified, until this returns 1. */
int pc_analyzer_frame_ingested(const pc_analyzer* a, int32_t frame_id);
/* Keypoints already stored in the database for this frame (resume, opticalflow.cc:168-178). */
int pc_analyzer_set_keypoints(pc_analyzer* a, int32_t frame_id, const float* xy, int n);
/* Enqueue one iteration of the outer loop (opticalflow.cc:259-309) for frame1 and the given
 * resident target frames (0..PC_MAX_TARGETS of them; the caller has already dropped pairs whose
 * flow exists, opticalflow.cc:286).  Fails with PC_E_STATE when max_jobs jobs are in flight. */
int pc_analyzer_submit(pc_analyzer* a, int32_t frame1, const int32_t* targets, int n_targets);
int pc_analyzer_pending(const pc_analyzer* a);
/* Device-resident record log (multi-GPU stitch): when set, every submitted job also appends its
 * records to `d_log` (device memory owned by the caller, e.g. a torch tensor that is later handed
 * to an RCCL all-gather) without a host round trip.  Layout per job, all little-endian, 16-B aligned:
 *   int64 hdr[16] = {PC_LOG_MAGIC, frame1, n_keypoints, n_targets, targets[8], rows_capacity, 0, 0, 0}
 *   int64 row_offset[16]      (first n_targets+1 valid; written by the GPU)
 *   float  keypoints[n_keypoints][2]
 *   uint32 src_indices[rows_capacity]; float tgt_xy[rows_capacity][2]; float flow_err[rows_capacity]
 * with rows_capacity = n_keypoints * n_targets (rows beyond row_offset[n_targets] are unspecified).
 * Passing NULL detaches the log.  Appending fails with PC_E_CAPACITY when the buffer is full. */
#define PC_LOG_MAGIC 0x50434c4f47303031ll /* "PCLOG001" */
int pc_analyzer_set_device_log(pc_analyzer* a, void* d_log, size_t capacity_bytes);
int pc_analyzer_device_log_used(const pc_analyzer* a, size_t* bytes);
/* The jobs submitted from now on append to another buffer, from its offset 0, without waiting for anything (set_device_log
 * synchronises the streams): the multi-GPU driver hands the log over piece by piece while the analysis keeps running
 * (analysis_driver.cc, polychase_amd/analyze.py -- the store of cpp/opticalflow.cc:149-151 overlapped with the analysis).
 * The bytes of the previous buffer are complete once the last job submitted into it has been collected.
 * A job whose record does not fit is refused by pc_analyzer_submit with PC_E_CAPACITY BEFORE anything of it is enqueued:
 * the caller can redirect the log and submit the same frame1 again. */
int pc_analyzer_redirect_device_log(pc_analyzer* a, void* d_log, size_t capacity_bytes);
/* enabled = 0: the records of the following jobs are not downloaded to pinned host memory (a rank whose records leave
 * through the device log only); pc_analyzer_collect then returns counts and NULL array pointers.  Default 1. */
int pc_analyzer_set_host_records(pc_analyzer* a, int enabled);
/* Forward-backward check (pc_lk_track_fb) for the jobs submitted from now on: the backward launch goes onto the job's lane
 * between the LK launch and the compaction, so rejected rows are simply absent from the records.  0 (the default): off, the
 * jobs enqueue what they always did.  Negative, NaN or infinite: PC_E_INVALID.  pc_analyzer_reset keeps the value. */
int pc_analyzer_set_fb_threshold(pc_analyzer* a, double fb_threshold);
/* Minimum correlation (pc_lk_track_correlated) of the jobs submitted FROM NOW ON: 0 = off (the default), else every job drops,
 * between the target-side mask test and the forward-backward check, the rows whose windows correlate below the value.  Jobs
 * already submitted keep theirs; pc_analyzer_reset keeps the value.  NaN, negative or > 1, or a null analyzer: PC_E_INVALID. */
int pc_analyzer_set_min_correlation(pc_analyzer* a, double min_correlation);
/* Brightness normalisation (pc_lk_track_normalized) of the jobs submitted FROM NOW ON: 0 = off (the default), 1 = the forward
 * launch, and the backward launch where the forward-backward check is on, run the normalised rule.  Jobs already submitted keep
 * theirs; pc_analyzer_reset keeps the value.  Any other value, or a null analyzer: PC_E_INVALID. */
int pc_analyzer_set_normalize(pc_analyzer* a, int normalize);
/* Affine refinement (pc_lk_track_affine) of the jobs submitted FROM NOW ON: 0 = off (the default), 1 = every job refines its
 * forward records in one more launch directly after the forward one.  Jobs already submitted keep theirs; pc_analyzer_reset keeps
 * the value.  Any other value, a null analyzer, or 1 while normalize is 1: PC_E_INVALID; pc_analyzer_submit refuses a job while
 * both are 1. */
int pc_analyzer_set_affine_refinement(pc_analyzer* a, int affine);
/* Search prepass (pc_lk_track_search) of the jobs submitted FROM NOW ON: 0 = off (the default), 1..256 = the radius in level-0
 * pixels; every job then runs the search launch directly after its forward launch.  Jobs already submitted keep theirs;
 * pc_analyzer_reset keeps the value.  Any other value, a null analyzer, or > 0 while normalize is 1: PC_E_INVALID;
 * pc_analyzer_submit refuses a job while both are set. */
int pc_analyzer_set_search_radius(pc_analyzer* a, int search_radius);
/* Detection mask (pc_frame_set_mask, gftt.cc:45-83) of the frames put FROM NOW ON with will_detect != 0; NULL: no mask (the
 * default).  Detection is enqueued inside pc_analyzer_put_frame, so every slot of the ring keeps a mask plane of its own: a
 * detection already enqueued keeps the mask it was enqueued with, and the mask may change from frame to frame.  A host mask
 * (on_device = 0) is consumed before the call returns; a device mask (on_device = 1) is read when a frame is put and must
 * stay alive and unmodified until pc_analyzer_frame_ingested says so for the frames put under it.  Frames put with
 * will_detect = 0 (their keypoints come from the caller, or they are detected without a mask when submitted as frame1) never
 * take the mask -- unless a target-side margin is on (pc_analyzer_set_target_mask_margin below), and then as targets only.  The
 * planes are allocated by the first call with a mask; an analyzer that never sees one allocates nothing
 * and enqueues what it always did.  pc_analyzer_reset clears the mask.  Null analyzer, or row_pitch < width: PC_E_INVALID. */
int pc_analyzer_set_mask(pc_analyzer* a, const uint8_t* mask, size_t row_pitch, int on_device);
/* As pc_analyzer_set_mask, the mask of the frames put from now on with will_detect != 0, given as polygons
 * (pc_frame_set_mask_polygons: arguments, fill rule, refusals).  The snapped vertices go through a small page-locked ring to
 * the device; each frame's plane is rasterised into its slot on the preparation stream when the frame is put, so the mask may
 * change with every frame and nothing of the size of a plane crosses the bus.  The first call allocates the slots' planes and
 * the vertex ring; later calls allocate nothing.  pc_analyzer_set_mask(a, NULL, ..) and pc_analyzer_reset clear it. */
int pc_analyzer_set_mask_polygons(pc_analyzer* a, const float* xy, const int32_t* counts, int n_polygons, int invert);
/* Target-side masks (pc_lk_track_masked) for the frames put FROM NOW ON: -1 = off (the default), 0..PC_TARGET_MASK_MAX_MARGIN =
 * the margin.  While it is >= 0 and a mask is in force (pc_analyzer_set_mask / _polygons), every frame put takes the mask into
 * its slot's plane whatever will_detect is, and with margin > 0 also gets the choked plane, made on the preparation stream in
 * front of the frame's "image ready" event.  The jobs submitted then drop, between the forward launch and the forward-backward
 * check, the rows that end where the target's plane is off; the margin a frame was put under is the one applied to the rows
 * that end in it, and a frame put without a mask in force keeps every row tracked into it.  Whether a frame's DETECTION reads
 * the mask stays as pc_analyzer_set_mask says: a frame put with will_detect = 0 is never detected under a mask.  The planes are
 * allocated by the first call that needs them: an analyzer that never sees a margin >= 0 together with a mask allocates and
 * enqueues what it always did.  pc_analyzer_reset keeps the margin (like the forward-backward threshold) and clears the mask.
 * Null analyzer, or a margin outside -1..PC_TARGET_MASK_MAX_MARGIN: PC_E_INVALID. */
int pc_analyzer_set_target_mask_margin(pc_analyzer* a, int margin);
/* Masked windows (pc_lk_track_window_masked) for the frames put and the jobs submitted FROM NOW ON: 0 = off (the default), 1 = on.
 * While it is on and a mask is in force (pc_analyzer_set_mask / _polygons), every frame put takes the mask into its slot's plane
 * whatever will_detect is -- as under a target-side margin, and as little a reason for its detection to read the mask -- and gets
 * its weight planes, made on the preparation stream in front of the frame's "image ready" event.  A job submitted while it is on
 * runs the masked launch behind its forward launch when frame1 was put that way, and, with a forward-backward threshold, the
 * weighted backward launch when a target was; a frame put without a mask in force, or with the option off, has no weights.  The
 * planes are allocated by the first call that needs them: an analyzer that never sees the switch together with a mask allocates
 * and enqueues what it always did.  pc_analyzer_reset keeps the switch and clears the mask.  A value other than 0 or 1, a null
 * analyzer, or 1 while normalize, the affine refinement, a search radius or a minimum correlation is set: PC_E_INVALID;
 * pc_analyzer_submit refuses a job while the switch and one of them are set (they may have been switched on afterwards). */
int pc_analyzer_set_mask_windows(pc_analyzer* a, int mask_windows);
/* Wait for the oldest submitted job.  Pointers stay valid until the job slot is reused, i.e. for
 * the next max_jobs-1 submits. */
int pc_analyzer_collect(pc_analyzer* a, pc_frame_result* out);

/* ---- "Track Sequence" path (cpp/tracker.cc:36-131): batched ray casting + PnP accumulation ---- */
typedef struct pc_mesh pc_mesh;
typedef struct pc_pnp_problem pc_pnp_problem;

/* Mesh of AcceleratedMesh (cpp/ray_casting.cc:21-63): vertices n_vertices x 3 f32 row-major,
 * triangles n_triangles x 3 u32 (host pointers; copied to the GPU). */
int pc_mesh_create(pc_context* ctx, const float* vertices, int n_vertices, const uint32_t* triangles,
                   int n_triangles, pc_mesh** out);
/* masked_triangles bitset (cpp/geometry.h:58-66), n_words >= ceil(n_triangles / 32). */
int pc_mesh_set_mask(pc_context* ctx, pc_mesh* mesh, const uint32_t* mask_words, int n_words);
void pc_mesh_destroy(pc_mesh* mesh);

/* Camera of GetRayObjectSpace (cpp/ray_casting.h:53-63): inv = (view * model)^-1. */
typedef struct pc_ray_camera {
    float dir_matrix[9]; /* inv.block<3,3>(0,0), row-major */
    float origin[3];     /* inv.col(3).head<3>() */
    float fx, fy, cx, cy;
    float unproject_sign; /* CameraIntrinsics::Unproject: +1 OpenCV convention, -1 OpenGL (types.h:95-98) */
} pc_ray_camera;

/* RayCast(accel_mesh, scene_transform, pos, check_mask) (cpp/ray_casting.cc:123-133) for n pixel
 * positions in one launch.  Closest hit, no back-face culling; a masked closest triangle is a miss.
 * Host in/out: xy n x 2; hit n bytes; pos n x 3 (barycentric point, object space); prim n;
 * uvt n x 3 = (u, v, t). */
int pc_raycast_pixels(pc_context* ctx, const pc_mesh* mesh, const pc_ray_camera* cam, const float* xy, int n,
                      int check_mask, uint8_t* hit, float* pos, uint32_t* prim, float* uvt);
/* The same result by an exhaustive sweep over every triangle instead of the hierarchy pc_mesh_create
 * builds (Embree's BVH in the reference, ray_casting.cc:23-63): the validation path of that hierarchy. */
int pc_raycast_pixels_sweep(pc_context* ctx, const pc_mesh* mesh, const pc_ray_camera* cam, const float* xy, int n,
                            int check_mask, uint8_t* hit, float* pos, uint32_t* prim, float* uvt);

/* Mesh render: the mesh as a width x height frame sees it, in one launch and without a pixel list.  Pixel (px, py),
 * 0 <= px < width, 0 <= py < height, casts exactly the ray pc_raycast_pixels casts for xy = ((float)px, (float)py) -- same
 * unprojection, same camera, same Moeller-Trumbore; the closest hit wins, among equal t the lowest triangle index -- so pixel
 * centres sit at integer coordinates, where GFTT puts its keypoints and the polygon masks their pixels.  Three packed planes
 * (row pitch = width), each may be NULL (not computed, not written), not all three:
 *   prim   int32: index of the closest triangle, -1 on a miss, WHATEVER the mesh's mask bits say (the ids a caller paints
 *          masked_triangles with: the addon's triangle-index buffer, blender_addon/operators/pin_mode/masking_3d.py:17-45);
 *   depth  float32: t of that triangle's hit, 0.0f on a miss: uvt[2] of pc_raycast_pixels with check_mask = 0.  The direction
 *          is not normalised and its camera-space z is +-1: under a rigid model-view, the distance along the optical axis;
 *   mask   uint8, 255 / 0: (1) on = hit && !(check_mask && closest triangle masked) -- a masked closest triangle is a miss, not
 *          a pass-through (ray_casting.cc:104-106): hit[] of pc_raycast_pixels; (2) invert != 0 flips on; (3) the plane is
 *          eroded by `margin` pixels, 0..PC_TARGET_MASK_MAX_MARGIN, by the choke rule of pc_lk_track_masked (square of
 *          2 margin + 1 pixels, pixels outside the frame count as on).  Polarity first, erosion second: invert = 0 keeps the
 *          object `margin` px inside its own silhouette, invert = 1 keeps everything else `margin` px away from it.
 * Consequence: with invert = 0 every pixel that is on, cast by pc_raycast_pixels (RayCast, the tracker) under the same camera
 * and check_mask at its integer coordinates, hits.
 * on_device = 0: host pointers, filled before the call returns.  on_device = 1: device memory of the mesh's GPU, complete when
 * the call returns -- the call synchronises the context's stream, so another context's stream may read the planes afterwards
 * (pc_analyzer_set_mask(on_device = 1)).  Scratch (the un-eroded plane; the planes of a host call) lives with the mesh and is
 * allocated by the first call that needs it.  PC_E_INVALID: a null handle or camera; all three planes NULL; width or height < 1
 * or > PC_MESH_RENDER_MAX_SIDE; margin outside 0..PC_TARGET_MASK_MAX_MARGIN; mask == NULL with invert or margin set; a context
 * other than the one the mesh was created in. */
#define PC_MESH_RENDER_MAX_SIDE 65536
int pc_mesh_render(pc_context* ctx, const pc_mesh* mesh, const pc_ray_camera* cam, int width, int height, int check_mask,
                   int invert, int margin, int on_device, int32_t* prim, float* depth, uint8_t* mask);

/* ---- 3D-2D correspondences of the frame being solved, built and kept on the GPU (cpp/tracker.cc:52-97) ----
 * SolveFrame gathers, per source frame that already has a pose, the matches of the flow source -> frame: the
 * source keypoint is cast onto the mesh under the source camera (tracker.cc:64-78), a hit is moved to world space
 * with the model matrix (:80-82) and paired with the tracked position (:86).  pc_corr_set_append does that for one
 * source in one pass on the device -- gather, ray cast, transform, order-preserving compaction -- and appends to
 * the set; nothing but a counter comes back to the host.  The PnP problem then reads the set in place. */
typedef struct pc_corr_set pc_corr_set;
int pc_corr_set_create(pc_context* ctx, pc_corr_set** out);
void pc_corr_set_destroy(pc_corr_set* set);
int pc_corr_set_clear(pc_context* ctx, pc_corr_set* set);
/* Makes a set fit for an unrelated run without giving its device memory back: waits for the set's own work (its copy stream
 * and the context's stream), forgets the cached keypoint arrays (they are keyed by frame id: another database may use the same
 * ids) and empties the set.  The host side parks ONE set per process between TrackSequence calls (csrc/host/track_sequence.cc):
 * creating the set's streams, page-locked words and device arrays is 6-8 ms of a call (cpp/tracker.cc:133-192 has no such
 * state: the reference allocates per frame on the host). */
int pc_corr_set_recycle(pc_context* ctx, pc_corr_set* set);
/* keypoints_xy: n_keypoints x 2 of the source frame; src_idx / tgt_xy: the n_matches rows of the flow
 * (src_keypoints_indices, tgt_keypoints).  Host pointers (pinned memory from pc_host_buffer_alloc is copied
 * asynchronously: it must stay untouched until pc_corr_set_size or a PnP call has returned).  keypoints_key >= 0
 * names the keypoint array (e.g. the source frame id): the set keeps the device copies of the last 16 keys and
 * skips the upload when it sees one again (a frame is a source for up to 8 targets); -1 = always upload.
 * model_matrix: row-major 4x4, rows 0-2 used.  An index >= n_keypoints is an error (tracker.cc:61). */
int pc_corr_set_append(pc_context* ctx, pc_corr_set* set, const pc_mesh* mesh, const pc_ray_camera* cam,
                       const float* model_matrix, long long keypoints_key, const float* keypoints_xy, int n_keypoints,
                       const uint32_t* src_idx, const float* tgt_xy, int n_matches, int check_mask);
/* number of correspondences so far (waits for the appends). */
int pc_corr_set_size(pc_context* ctx, pc_corr_set* set, int* n);
/* debugging / tests: world points n x 3 and image points n x 2, in append order. */
int pc_corr_set_download(pc_context* ctx, pc_corr_set* set, float* world_xyz, float* image_xy);
/* A PnP problem over the set's arrays, no copy: the set must stay unchanged while the problem is alive. */
int pc_pnp_problem_from_set(pc_context* ctx, pc_corr_set* set, pc_pnp_problem** out);

/* PnPProblem (cpp/pnp/pnp_problem.h:11-142): object points X n x 3, image points x n x 2,
 * optional per-residual weights (NULL = 1). Host pointers; copied to the GPU once per frame. */
int pc_pnp_problem_create(pc_context* ctx, const float* X, const float* x, const float* weights, int n,
                          pc_pnp_problem** out);
void pc_pnp_problem_destroy(pc_pnp_problem* prob);

typedef struct pc_pnp_params {
    float R[9];               /* rotation matrix of the pose (row-major) */
    float t[3];
    float fx, fy, cx, cy, aspect_ratio;
    int convention_opencv;    /* CameraConvention::OpenCV ? 1 : 0 */
    int optimize_focal_length, optimize_principal_point;
    int loss_type;            /* BundleOptions::LossType: 0 TRIVIAL, 1 HUBER, 2 CAUCHY */
    float loss_scale;
} pc_pnp_params;

/* LevMarqDenseSolver::BuildNormalEquations (cpp/pnp/lev_marq.h:231-297) without the diagonal
 * clamp: JtJ lower triangle packed row-major (45), Jtr (9), number of valid residuals. */
int pc_pnp_normal_equations(pc_context* ctx, const pc_pnp_problem* prob, const pc_pnp_params* params,
                            float* jtj_lower45, float* jtr9, int* valid);
/* The same sweep also returns TotalCost of `params` (bit for bit what pc_pnp_total_cost returns): the LM loop
 * (lev_marq.h:132-228) gets a candidate's cost and -- should the step be accepted -- the next iteration's normal
 * equations from one launch and one read-back instead of two. */
int pc_pnp_normal_equations_cost(pc_context* ctx, const pc_pnp_problem* prob, const pc_pnp_params* params,
                                 float* jtj_lower45, float* jtr9, int* valid, float* cost);
/* ---- the whole of SolvePnPIterative on the device (cpp/pnp/solvers.cc:11-71, lev_marq.h:132-228) ----
 * The LM loop alternates residual sweeps with 9x9 algebra that decides what to evaluate next; driven from the
 * host every decision costs a launch + read-back + synchronisation.  pc_pnp_solve keeps the solver's state in
 * device memory: a one-lane kernel takes the decision (same fp32 arithmetic, same order of operations), the host
 * enqueues [sweep, reduce, decide] rounds without waiting and reads the state back once per batch of rounds. */
typedef struct pc_pnp_camera {
    float q_xyzw[4];          /* pose rotation (Eigen order) */
    float t[3];
    float fx, fy, cx, cy, aspect_ratio;
    int convention_opencv;
} pc_pnp_camera;
typedef struct pc_pnp_solve_options {
    int max_iterations;                                   /* BundleOptions (pnp/types.h:200-215) */
    float initial_lambda, min_lambda, max_lambda, gradient_tol, step_tol;
    int loss_type;
    float loss_scale;
    int optimize_focal_length, optimize_principal_point;
    float f_low, f_high, cx_low, cx_high, cy_low, cy_high; /* CameraIntrinsics::GetBounds (types.h:156-192) */
    float max_inlier_error;                               /* <= 0: no inlier pass */
    int rounds_hint;                                      /* rounds enqueued before the first read-back (0 = default) */
} pc_pnp_solve_options;
typedef struct pc_pnp_solve_result {
    pc_pnp_camera camera;
    int iterations, invalid_steps;                        /* BundleStats (pnp/types.h:217-225) */
    float initial_cost, cost, lambda, step_norm, grad_norm;
    int inliers;                                          /* residuals below max_inlier_error (solvers.cc:31-47) */
} pc_pnp_solve_result;
int pc_pnp_solve(pc_context* ctx, pc_pnp_problem* prob, const pc_pnp_camera* initial, const pc_pnp_solve_options* options,
                 pc_pnp_solve_result* result);
/* Diagnostics of the device-resident solver: its DECISION step -- everything lev_marq.h:146-221 does between two residual
 * sweeps -- run on scripted sums instead of a scene.  A decision depends only on the 56 sums of a sweep ([0..44] JtJ lower
 * triangle packed row-major, [45..53] Jtr, [54] valid count, [55] cost), so every branch of it can be reached without a mesh.
 * One launch, one workgroup per script; the state starts as pc_pnp_solve's and pc_track_solve_frame's does and is handed
 * round by round to the solver's own code:
 *   mode 0  the wavefront decision of the persistent tracking launch (the default of pc_track_solve_frame),
 *   mode 1  its one-lane cross-check (POLYCHASE_TRACK_SERIAL_DECISION=1),
 *   mode 2  the bare one-lane decision of pc_pnp_solve: no correspondence-count rules, no round limit (max_rounds ignored).
 * options[i].rounds_hint > 0 is script i's round limit in place of max_rounds (modes 0 and 1).
 * states[i * n_rounds + r] is the state after round r of script i.  Once a script is done, modes 0 and 1 skip its remaining
 * rounds as the tracking launch leaves its loop; mode 2 still makes the call, as pc_pnp_solve's rounds enqueued past
 * convergence do, and the solver returns at once: in every mode the remaining snapshots repeat the final state.
 * PC_E_INVALID, with nothing launched: a null pointer, mode outside 0..2, n_scripts outside 1..1024, n_rounds outside 1..16.
 * The struct is 4-byte words only (PC_LM_DEBUG_STATE_WORDS of them): the solver's state without its configuration and its
 * copy of the latest accepted sums. */
#define PC_LM_DEBUG_STATE_WORDS 169
typedef struct pc_lm_debug_state {
    pc_pnp_camera cam, cam_new;                           /* accepted parameters, latest candidate */
    float R[9], t[3], fx, fy, cx, cy, aspect_ratio;       /* what the next sweep evaluates (the accepted ones once done) */
    int convention_opencv, sweep_optimize_focal, sweep_optimize_pp;
    float JtJ[81], diag[9], Jtr[9], step[9];              /* JtJ row-major: lower triangle, clamped diagonal; the rest stays 0 */
    float cost, initial_cost, lambda, v, grad_norm, step_norm;
    int iterations, invalid_steps, rebuild, phase, done;
    int n_valid, status;                                  /* modes 0, 1: 0 ok, 1 fewer than 3 correspondences, 3 round limit */
    int optimize_focal, optimize_pp;                      /* as the solver holds them: cleared when n_valid == 3 */
} pc_lm_debug_state;
int pc_debug_lm_decide(pc_context* ctx, int mode, int n_scripts, int n_rounds, int max_rounds,
                       const pc_pnp_solve_options* options /* [n_scripts] */, const pc_pnp_camera* initial /* [n_scripts] */,
                       const float* sums /* [n_scripts][n_rounds][56] */, pc_lm_debug_state* states /* [n_scripts][n_rounds] */);
/* tests, debugging: device allocations, pinned allocations, streams and events currently owned by objects of this library
 * in this process (what pc_peer_buffer_alloc / pc_host_buffer_alloc handed out is the caller's and is not counted). */
int pc_debug_live_resources(int out[4]);
/* ---- SolveFrame in one call (cpp/tracker.cc:36-131): the correspondences of EVERY source frame + SolvePnPIterative ----
 * Two launches and one wait per frame: one ray-cast launch over the matches of all sources (each under its own
 * camera; world points stay on the GPU, no compaction), then the whole Levenberg-Marquardt loop and the inlier pass as
 * ONE persistent launch -- the workgroups keep their correspondences, meet at a grid barrier once per evaluated
 * parameter set, one workgroup takes the solver's decision (lev_marq.h:146-221) and the rounds stop when it is done; the
 * result is written to pinned host memory by the kernel.  (pc_corr_set_append + pc_pnp_solve -- 12 + 28 launches per
 * frame -- remain as the building blocks and as the cross-check: same world points bit for bit, poses equal to fp32
 * summation order.)
 * sources[k]: camera of source frame k (already solved), its keypoints (cached by keypoints_key like
 * pc_corr_set_append) and where its matches -- src_keypoints_indices (n_matches x uint32 at idx_offset) and
 * tgt_keypoints (n_matches x 2 floats at tgt_offset; byte offsets, 4- / 8-aligned) -- lie inside the block `matches`
 * of matches_bytes bytes: the block travels to the GPU in ONE transfer (host memory; pc_host_buffer_alloc memory is
 * fetched by the copy engine without a staging copy).
 * options->optimize_*: what the caller ASKS for; intrinsics are only optimised with more than 3 correspondences
 * (pnp_problem.h:34-35), decided on the device where the count is known.
 * result->n_correspondences < 3: "not enough features" (tracker.cc:95-97), nothing was solved. */
typedef struct pc_track_source {
    pc_ray_camera cam;
    long long keypoints_key;
    const float* keypoints_xy;    /* host, n_keypoints x 2 */
    int n_keypoints;
    int n_matches;
    size_t idx_offset, tgt_offset;
} pc_track_source;
typedef struct pc_track_solve_result {
    pc_pnp_solve_result pnp;
    int n_matches;                /* rows of all sources */
    int n_correspondences;        /* ... whose ray hit the (unmasked) mesh */
    int rounds;                   /* parameter sets evaluated by the persistent launch */
    /* where the persistent launch spent its time, measured by its deciding workgroup in 100 MHz ticks and summed over the
     * rounds: [0] residual sweep + publishing the partial sums, [1] waiting for the other workgroups, [2] adding the
     * partials, [3] the decision (9x9 algebra; by a wavefront since round 6), [4] publishing it, [5] fetching the next parameters,
     * [6] inlier pass, [7] the whole launch */
    unsigned lm_ticks[8];
    unsigned long long lm_begin_tick, lm_end_tick;   /* the GPU's 100 MHz clock when the LM kernel began / handed over its result */
} pc_track_solve_result;
int pc_track_solve_frame(pc_context* ctx, pc_corr_set* set, const pc_mesh* mesh, const float* model_matrix, int check_mask,
                         const pc_track_source* sources, int n_sources, const void* matches, size_t matches_bytes,
                         const pc_pnp_camera* initial, const pc_pnp_solve_options* options, pc_track_solve_result* result);
/* The same in three steps, so that a caller overlaps the host's part and the transfer of frame f + 1 with the launches of
 * frame f (csrc/host/track_sequence.cc): upload = the matches block (and the keypoints of sources the set has not cached yet)
 * on the set's own copy stream, into the next of three device blocks -- callable while frames are in flight, before the
 * cameras of its sources are known; launch = the two launches behind that upload, for the block uploaded last; finish =
 * wait + result.  `matches` and the keypoint arrays must stay untouched until the frame's finish. */
int pc_track_frame_upload(pc_context* ctx, pc_corr_set* set, const void* matches, size_t matches_bytes, const pc_track_source* sources,
                          int n_sources);
int pc_track_frame_launch(pc_context* ctx, pc_corr_set* set, const pc_mesh* mesh, const float* model_matrix, int check_mask,
                          const pc_track_source* sources, int n_sources, const pc_pnp_camera* initial, const pc_pnp_solve_options* options);
/* Allocates what the first tracked frame of a clip with up to n_matches matches per frame and n_keypoints keypoints per source
 * frame would otherwise allocate inside pc_track_frame_upload / _launch (the set's copy stream and event, the three match blocks,
 * the per-match arrays, the barrier words, the page-locked result words, `n_cached` keypoint arrays): 6-8 ms of a process's
 * first TrackSequence call.  Everything still grows on demand. */
int pc_corr_set_reserve(pc_context* ctx, pc_corr_set* set, int n_matches, int n_keypoints, int n_cached);
/* The launch with its inputs taken from the launch enqueued JUST BEFORE it on this set, on the device: up to TWO frames may be in
 * flight (finished in launch order), so that the GPU goes from frame f to frame f + 1 without the host in between -- SolveFrame of
 * f + 1 needs the pose of f twice (tracker.cc:43-50: f is one of its source frames; :111-119: f's pose is its initial guess), and
 * both are left on the device by f's launch.
 *   chained_source  index into `sources` of the source frame whose camera (pc_track_source::cam is ignored for it) is the result
 *                   of the previous launch, or -1;
 *   chain_initial   != 0: the initial camera is the previous launch's result (`initial` is ignored);
 * both require that a launch of this set has run since it was created / recycled.  Sources of a second frame in flight must
 * have keypoints_key >= 0.  If the previous launch fails, this one runs on whatever it left (bounded by max_iterations) and the
 * caller, who learns of the failure first, drops its result. */
int pc_track_frame_launch_chained(pc_context* ctx, pc_corr_set* set, const pc_mesh* mesh, const float* model_matrix, int check_mask,
                                  const pc_track_source* sources, int n_sources, int chained_source, const pc_pnp_camera* initial,
                                  int chain_initial, const pc_pnp_solve_options* options);
/* waits for the OLDEST frame in flight */
int pc_track_frame_finish(pc_context* ctx, pc_corr_set* set, pc_track_solve_result* result);
/* debugging / tests: (world x, y, z, hit ? 1 : 0) of the first n matches of the last pc_track_solve_frame, in match order
 * (source after source). */
int pc_track_download_points(pc_context* ctx, pc_corr_set* set, int n, float* world_xyzw);

/* LevMarqDenseSolver::TotalCost (lev_marq.h:316-356) and the inlier count of SolvePnPIterative
 * (cpp/pnp/solvers.cc:31-47) in one pass. */
int pc_pnp_total_cost(pc_context* ctx, const pc_pnp_problem* prob, const pc_pnp_params* params,
                      float max_inlier_error_sq, float* cost, int* valid, int* inliers);

/* ---- "Refine Sequence" path (cpp/refiner.cc:199-725, cpp/pnp/lev_marq.h:391-871) ----
 * The segment's keypoints and flows live on the GPU; per LM iteration the host sends the camera
 * trajectory and receives the cost or the per-edge normal-equation blocks. */
typedef struct pc_refine_problem pc_refine_problem;

typedef struct pc_refine_desc {
    int n_frames;                 /* frames of the segment, index 0 = first frame */
    int n_edges;                  /* flows (image_id_from -> image_id_to) inside the segment */
    const int32_t* kp_offset;     /* [n_frames + 1]: keypoints of frame f = kp_xy[kp_offset[f] .. kp_offset[f+1]) */
    const float* kp_xy;           /* all (bbox-filtered) keypoints, x y */
    const int32_t* edge_src;      /* [n_edges] frame index of image_id_from */
    const int32_t* edge_tgt;      /* [n_edges] frame index of image_id_to */
    const int32_t* edge_offset;   /* [n_edges + 1] into the residual arrays */
    const uint32_t* res_src_kp;   /* per residual: keypoint index within the source frame */
    const float* res_tgt_xy;      /* per residual: tracked position in the target frame */
    const float* edge_weight;     /* [n_edges] GlobalRefinementProblem::EdgeWeight (refiner.cc:596-599) */
    float model_matrix[16];       /* object -> world, row-major */
    float model_matrix_inv[16];
    int block_len;                /* parameters per camera: 6, or 9 when intrinsics are optimised */
    int optimize_focal_length, optimize_principal_point;
} pc_refine_desc;

/* one camera of the trajectory, 20 floats */
typedef struct pc_refine_camera {
    float R[9];
    float t[3];
    float fx, fy, cx, cy, aspect_ratio;
    float unproject_sign;         /* +1 OpenCV, -1 OpenGL */
    float reserved[2];
} pc_refine_camera;

int pc_refine_problem_create(pc_context* ctx, const pc_mesh* mesh, const pc_refine_desc* desc,
                             pc_refine_problem** out);
/* The same problem with its three large arrays handed over in pieces: the keypoints and the residuals of consecutive runs of
 * frames (what the reader threads of CachedDatabase's replacement each hold -- a 300-frame 1080p segment is 1.2 GB, and joining
 * the pieces on the host first costs as much as reading them).  desc->kp_xy, res_src_kp and res_tgt_xy must be NULL; the parts,
 * in order, make up kp_offset[n_frames] keypoints and edge_offset[n_edges] residuals.  A residual that names a keypoint its
 * source frame does not have is found on the device and refused like pc_refine_problem_create refuses it. */
typedef struct pc_refine_part {
    const float* kp_xy;           /* n_keypoints (x, y) */
    int64_t n_keypoints;
    const uint32_t* res_src_kp;   /* n_residuals */
    const float* res_tgt_xy;      /* n_residuals (x, y) */
    int64_t n_residuals;
} pc_refine_part;
int pc_refine_problem_create_parts(pc_context* ctx, const pc_mesh* mesh, const pc_refine_desc* desc, const pc_refine_part* parts,
                                   int n_parts, pc_refine_problem** out);
void pc_refine_problem_destroy(pc_refine_problem* prob);
/* LevMarqSparseSolver::TotalCost (lev_marq.h:773-824) over RefinementProblemBase::Evaluate
 * (refiner.cc:274-361); updates the per-keypoint triangle cache like the reference does. */
int pc_refine_total_cost(pc_context* ctx, pc_refine_problem* prob, const pc_refine_camera* cameras,
                         int loss_type, float loss_scale, double* cost);
/* LevMarqSparseSolver::BuildNormalEquations (lev_marq.h:653-771) without the scatter: per edge the
 * lower triangle of the (2B x 2B) block (packed row-major, (2B)(2B+1)/2 doubles) followed by the 2B
 * gradient entries, normalised by the edge's valid-residual count (returned in edge_valid).
 * Jacobians are evaluated in fp32 like the reference; the sums are fp64 so that J^T J stays positive
 * semi-definite to rounding (long weakly-damped chains need it). */
int pc_refine_normal_equations(pc_context* ctx, pc_refine_problem* prob, const pc_refine_camera* cameras,
                               int loss_type, float loss_scale, double* edge_blocks, int* edge_valid);

/* GPU time of the sweeps of this problem so far: HIP events on the context's stream around the kernel of every
 * pc_refine_total_cost / pc_refine_normal_equations call (launches, summed milliseconds).  Any pointer may be NULL. */
int pc_refine_problem_timing(const pc_refine_problem* prob, int* cost_launches, double* cost_ms, int* normal_eq_launches,
                             double* normal_eq_ms);

/* ---- record exchange between the ranks of a multi-GPU analysis (one process per GPU) --------------------------------
 * The stitch of the flow database (the reference's store, cpp/opticalflow.cc:149-151, sharded): a rank exports a
 * device buffer, its peers map it INTO THEIR OWN device's address space (HIP IPC) and write their record pieces into it with
 * device-to-device copies on a stream of their own device -- xGMI is point to point, the copy engines move the bytes, no
 * kernel and no queue on the peer's GPU is involved.  polychase_amd/distributed.py: PeerLogStitch. */
#define PC_PEER_HANDLE_BYTES 64
int pc_peer_buffer_alloc(int device_index, size_t bytes, void** device_ptr);           /* hipMalloc on that device */
int pc_peer_buffer_free(int device_index, void* device_ptr);
int pc_peer_buffer_export(int device_index, void* device_ptr, unsigned char handle[PC_PEER_HANDLE_BYTES]);
/* maps a peer's exported buffer for `device_index` (this process's GPU); *device_ptr is valid for copies issued here */
int pc_peer_buffer_open(int device_index, const unsigned char handle[PC_PEER_HANDLE_BYTES], void** device_ptr);
int pc_peer_buffer_close(int device_index, void* device_ptr);
/* hipMemcpyAsync(dst, src, bytes, device-to-device) on `stream` (a hipStream_t of device_index; NULL = the null stream) */
int pc_peer_copy_async(int device_index, void* dst, const void* src, size_t bytes, void* stream);
/* blocking device-to-host copy (verification of what the peers wrote) */
int pc_peer_buffer_download(int device_index, void* dst_host, const void* src_device, size_t bytes);

/* ---- the same exchange over RCCL, for C / C++ hosts (no torch): api_comm.hip ---------------------------------------------
 * One communicator per rank (= process = GPU).  Rank 0 makes the id (ncclGetUniqueId) and hands its PC_COMM_ID_BYTES bytes
 * to the other ranks by any means (csrc/host/multi_gpu.cc: a TCP socket); every rank then calls pc_comm_create, which is
 * collective (ncclCommInitRank).  librccl.so.1 is loaded at the first of these calls: PC_E_NO_DEVICE when it is missing.
 *   pc_comm_all_gather_log   BASELINE.json's "RCCL all-gather of the flow DB": every rank contributes `bytes` bytes at
 *                            `piece` (device memory; sizes may differ) and receives all ranks' pieces in `recv` (device
 *                            memory, world * slot_bytes; rank r's piece at r * slot_bytes, sizes_host[r] bytes of it valid).
 *                            Two ncclAllGather calls (the sizes as uint64, then the payload padded to slot_bytes) on the
 *                            communicator's own stream; returns when both are complete.
 *   pc_comm_send / _recv     the ordered gather of the product: ncclSend / ncclRecv of exactly `bytes` bytes of device
 *                            memory, blocking until the transfer is complete.
 * What they replace in the reference: nothing it has (cpp/opticalflow.cc:209-321 is one process) -- the hand-over of
 * opticalflow.cc:149-151 (flows -> database) when the frames were analysed on another GPU. */
typedef struct pc_comm pc_comm;
#define PC_COMM_ID_BYTES 128
int pc_comm_unique_id(void* id /* [PC_COMM_ID_BYTES] */);
int pc_comm_create(pc_context* ctx, const void* id /* [PC_COMM_ID_BYTES] */, int world_size, int rank, pc_comm** out);
void pc_comm_destroy(pc_comm* comm);
int pc_comm_world_size(const pc_comm* comm);
int pc_comm_rank(const pc_comm* comm);
int pc_comm_all_gather_log(pc_comm* comm, const void* piece_device, uint64_t bytes, void* recv_device, uint64_t slot_bytes,
                           uint64_t* sizes_host /* [world_size] */);
int pc_comm_send(pc_comm* comm, const void* src_device, uint64_t bytes, int dst_rank);
int pc_comm_recv(pc_comm* comm, void* dst_device, uint64_t bytes, int src_rank);

#ifdef __cplusplus
}
#endif
#endif /* POLYCHASE_HIP_H_ */
