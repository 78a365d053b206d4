// api_lens.hip -- lens undistortion at ingest (include/polychase_hip.h has the rule): the host-only makers of a lens map -- the
// polynomial model, an STmap, the validity plane -- and the context's setter.  The remap itself is kernels_lens.hip, launched by
// pc_api::set_image (api.hip).
//
// The model is fp64 with every operation rounded on its own, in the order the header writes them: this unit, like the whole
// library, is compiled with -ffp-contract=off (polychase_amd/build.py), and no expression below is rearranged.
#include "api_internal.hpp"

#include <limits>

using namespace pc_api;

static_assert(pc::kLensFracBits == PC_LENS_FRAC_BITS && pc::kLensInvalid == PC_LENS_INVALID, "kernels.hpp holds the header's constants");

namespace {

constexpr double kLensClamp = 16777216.0;   // 2^24

// w and h as pc_frame_create takes them
int check_lens_size(int w, int h) {
    if (w < 1 || h < 1 || (long long)w * h > (1ll << 30)) return fail(PC_E_INVALID, "bad lens map size %dx%d", w, h);
    return PC_OK;
}

// q = floor(s * 256 + 0.5) clamped to +-2^24 (s finite)
inline int32_t lens_quantize(double s) {
    double v = std::floor(s * 256.0 + 0.5);
    if (v > kLensClamp) v = kLensClamp;
    if (v < -kLensClamp) v = -kLensClamp;
    return (int32_t)v;
}

inline void lens_store(int32_t* q, double sx, double sy) {
    if (!(std::isfinite(sx) && std::isfinite(sy))) {
        q[0] = PC_LENS_INVALID;
        q[1] = PC_LENS_INVALID;
        return;
    }
    q[0] = lens_quantize(sx);
    q[1] = lens_quantize(sy);
}

}  // namespace

extern "C" {

void pc_lens_default_model(pc_lens_model* m) {
    if (!m) return;
    m->fx = m->fy = 1.0;
    m->cx = m->cy = 0.0;
    m->k1 = m->k2 = m->k3 = 0.0;
    m->p1 = m->p2 = 0.0;
    m->zoom = 1.0;
}

int pc_lens_build_map(const pc_lens_model* m, int w, int h, int32_t* q) {
    if (!m || !q) return fail(PC_E_INVALID, "null argument");
    const double vals[10] = {m->fx, m->fy, m->cx, m->cy, m->k1, m->k2, m->k3, m->p1, m->p2, m->zoom};
    for (int k = 0; k < 10; k++)
        if (!std::isfinite(vals[k])) return fail(PC_E_INVALID, "lens model: value %d is not finite", k);
    if (!(m->fx > 0.0 && m->fy > 0.0 && m->zoom > 0.0)) return fail(PC_E_INVALID, "lens model: fx, fy and zoom must be > 0");
    if (int rc = check_lens_size(w, h)) return rc;
    const double fx = m->fx, fy = m->fy, cx = m->cx, cy = m->cy, k1 = m->k1, k2 = m->k2, k3 = m->k3, p1 = m->p1, p2 = m->p2;
    const double fxz = fx * m->zoom, fyz = fy * m->zoom;
    for (int v = 0; v < h; v++) {
        const double y = ((double)v - cy) / fyz;
        for (int u = 0; u < w; u++) {
            const double x = ((double)u - cx) / fxz;
            const double r2 = x * x + y * y;
            const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
            const double xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
            const double yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
            const double sx = xd * fx + cx;
            const double sy = yd * fy + cy;
            lens_store(q + ((size_t)v * w + u) * 2, sx, sy);
        }
    }
    return PC_OK;
}

int pc_lens_map_from_stmap(const float* st, int w, int h, int flip_v, int32_t* q) {
    if (!st || !q) return fail(PC_E_INVALID, "null argument");
    if (int rc = check_lens_size(w, h)) return rc;
    const double dw = (double)w, dh = (double)h;
    for (size_t i = 0, n = (size_t)w * h; i < n; i++) {
        const double s = (double)st[2 * i], t = (double)st[2 * i + 1];
        const double sx = s * dw - 0.5;
        const double sy = flip_v ? (1.0 - t) * dh - 0.5 : t * dh - 0.5;
        lens_store(q + 2 * i, sx, sy);
    }
    return PC_OK;
}

int pc_lens_map_valid(const int32_t* q, int w, int h, int erode, uint8_t* out, int* all_valid) {
    if (!q || !out) return fail(PC_E_INVALID, "null argument");
    if (int rc = check_lens_size(w, h)) return rc;
    if (erode < 0 || erode > PC_LENS_MAX_ERODE) return fail(PC_E_INVALID, "erode must be in 0..%d, got %d", PC_LENS_MAX_ERODE, erode);
    const int m = erode;
    const int32_t xmax = (int32_t)(((long long)w - 1) * 256 > 0x7fffffffll ? 0x7fffffffll : ((long long)w - 1) * 256);
    const int32_t ymax = (int32_t)(((long long)h - 1) * 256 > 0x7fffffffll ? 0x7fffffffll : ((long long)h - 1) * 256);
    // rows first: a pixel stays on iff no invalid pixel lies within m columns of it (prefix counts of the invalid pixels of the
    // row); then the columns the same way, with a running count per column of the rows y - m .. y + m that are off
    std::vector<uint8_t> rows_on((size_t)w * h);
    std::vector<int> prefix((size_t)w + 1);
    for (int y = 0; y < h; y++) {
        const int32_t* r = q + (size_t)y * w * 2;
        prefix[0] = 0;
        for (int x = 0; x < w; x++) {
            const bool ok = r[2 * x] >= 0 && r[2 * x] <= xmax && r[2 * x + 1] >= 0 && r[2 * x + 1] <= ymax;
            prefix[(size_t)x + 1] = prefix[(size_t)x] + (ok ? 0 : 1);
        }
        uint8_t* o = rows_on.data() + (size_t)y * w;
        for (int x = 0; x < w; x++) o[x] = prefix[(size_t)std::min(w, x + m + 1)] == prefix[(size_t)std::max(0, x - m)] ? 1 : 0;
    }
    std::vector<int> off((size_t)w, 0);
    for (int y = 0; y < std::min(h, m); y++)   // rows 0 .. m - 1: the window of row 0 without the row that enters below
        for (int x = 0; x < w; x++) off[(size_t)x] += rows_on[(size_t)y * w + x] ? 0 : 1;
    bool all = true;
    for (int y = 0; y < h; y++) {
        if (y + m < h)
            for (int x = 0; x < w; x++) off[(size_t)x] += rows_on[(size_t)(y + m) * w + x] ? 0 : 1;
        if (y - m - 1 >= 0)
            for (int x = 0; x < w; x++) off[(size_t)x] -= rows_on[(size_t)(y - m - 1) * w + x] ? 0 : 1;
        uint8_t* o = out + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            o[x] = off[(size_t)x] == 0 ? 255 : 0;
            all = all && off[(size_t)x] == 0;
        }
    }
    if (all_valid) *all_valid = all ? 1 : 0;
    return PC_OK;
}

int pc_context_set_lens_map(pc_context* c, const int32_t* q, int w, int h) {
    if (!c) return fail(PC_E_INVALID, "null context");
    if (q)
        if (int rc = check_lens_size(w, h)) return rc;
    PC_HIP(hipSetDevice(c->device));
    if (!q && c->lens_w == 0) return PC_OK;   // nothing to clear: not even a wait
    // launches of the map in force may still read it and the two planes
    if (c->prep_stream) PC_HIP(c->sync_side_streams());
    PC_HIP(hipStreamSynchronize(c->stream));
    if (!q) {
        c->lens_w = c->lens_h = c->lens_pitch = c->lens_plane_pitch = 0;
        c->lens_map.release();
        c->lens_gray.release();
        c->lens_out.release();
        return PC_OK;
    }
    // into buffers of their own, which take the place of those in force only once the copy is complete: a failure on the way
    // leaves the map in force untouched
    const int pitch = (w + 3) / 4 * 4, plane_pitch = (w + 63) / 64 * 64;
    DevBuf<int32_t> map;
    DevBuf<uint8_t> gray, out;
    PC_HIP(map.ensure((size_t)pitch * h * 2, /*exact=*/true));
    PC_HIP(gray.ensure((size_t)plane_pitch * h, /*exact=*/true));
    PC_HIP(out.ensure((size_t)plane_pitch * h, /*exact=*/true));
    if (pitch != w) PC_HIP(hipMemset(map.p, 0, (size_t)pitch * h * 2 * sizeof(int32_t)));   // the entries behind a row's end are read, never used
    PC_HIP(hipMemcpy2D(map.p, (size_t)pitch * 2 * sizeof(int32_t), q, (size_t)w * 2 * sizeof(int32_t), (size_t)w * 2 * sizeof(int32_t), (size_t)h,
                       hipMemcpyHostToDevice));
    c->lens_map = std::move(map);
    c->lens_gray = std::move(gray);
    c->lens_out = std::move(out);
    c->lens_w = w;
    c->lens_h = h;
    c->lens_pitch = pitch;
    c->lens_plane_pitch = plane_pitch;
    return PC_OK;
}

int pc_context_get_lens_map_size(const pc_context* c, int* w, int* h) {
    if (!c) return fail(PC_E_INVALID, "null context");
    if (w) *w = c->lens_w;
    if (h) *h = c->lens_h;
    return PC_OK;
}

}  // extern "C"
