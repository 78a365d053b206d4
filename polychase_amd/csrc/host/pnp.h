// pnp.h -- SolvePnPIterative of the reference (cpp/pnp/solvers.h:22-29): dense Levenberg-Marquardt
// over 9 parameters (so(3) step, translation, fy, cx, cy) with a robust loss.
#pragma once

#include "../../../include/polychase_hip.h"
#include "types.h"

// object_points: n x 3, image_points: n x 2, weights: n or nullptr.
void SolvePnPIterative(const float* object_points, const float* image_points, const float* weights, size_t n,
                       const PnPOptions& opts, PnPResult& result);

// The same solver over a problem that already lives on the GPU (pc_pnp_problem_create / pc_pnp_problem_from_set);
// n = its number of correspondences.
void SolvePnPIterativeOnGpu(pc_pnp_problem* problem, size_t n, const PnPOptions& opts, PnPResult& result);

// ---- host types <-> the C ABI of the device solver (pc_pnp_solve, pc_track_frame_*) ----
inline pc_pnp_camera ToPnpCamera(const CameraState& s) {
    pc_pnp_camera c;
    c.q_xyzw[0] = s.pose.q.x;
    c.q_xyzw[1] = s.pose.q.y;
    c.q_xyzw[2] = s.pose.q.z;
    c.q_xyzw[3] = s.pose.q.w;
    for (int i = 0; i < 3; i++) c.t[i] = s.pose.t[i];
    c.fx = s.intrinsics.fx;
    c.fy = s.intrinsics.fy;
    c.cx = s.intrinsics.cx;
    c.cy = s.intrinsics.cy;
    c.aspect_ratio = s.intrinsics.aspect_ratio;
    c.convention_opencv = s.intrinsics.convention == CameraConvention::OpenCV ? 1 : 0;
    return c;
}

// pose and the four intrinsics onto an existing state (aspect ratio, size and convention are not the solver's to change)
inline void FromPnpCamera(const pc_pnp_camera& c, CameraState& s) {
    s.pose.q.x = c.q_xyzw[0];
    s.pose.q.y = c.q_xyzw[1];
    s.pose.q.z = c.q_xyzw[2];
    s.pose.q.w = c.q_xyzw[3];
    for (int i = 0; i < 3; i++) s.pose.t[i] = c.t[i];
    s.intrinsics.fx = c.fx;
    s.intrinsics.fy = c.fy;
    s.intrinsics.cx = c.cx;
    s.intrinsics.cy = c.cy;
}

inline pc_pnp_solve_options ToPnpSolveOptions(const BundleOptions& bo, const CameraIntrinsics::Bounds& bounds, bool opt_f,
                                              bool opt_pp, Float max_inlier_error) {
    pc_pnp_solve_options so;
    so.max_iterations = static_cast<int>(bo.max_iterations);
    so.initial_lambda = bo.initial_lambda;
    so.min_lambda = bo.min_lambda;
    so.max_lambda = bo.max_lambda;
    so.gradient_tol = bo.gradient_tol;
    so.step_tol = bo.step_tol;
    so.loss_type = static_cast<int>(bo.loss_type);
    so.loss_scale = bo.loss_scale;
    so.optimize_focal_length = opt_f ? 1 : 0;
    so.optimize_principal_point = opt_pp ? 1 : 0;
    so.f_low = bounds.f_low;
    so.f_high = bounds.f_high;
    so.cx_low = bounds.cx_low;
    so.cx_high = bounds.cx_high;
    so.cy_low = bounds.cy_low;
    so.cy_high = bounds.cy_high;
    so.max_inlier_error = max_inlier_error;
    so.rounds_hint = 0;
    return so;
}

inline BundleStats ToBundleStats(const pc_pnp_solve_result& r) {
    BundleStats st;
    st.iterations = static_cast<size_t>(r.iterations);
    st.invalid_steps = static_cast<size_t>(r.invalid_steps);
    st.initial_cost = r.initial_cost;
    st.cost = r.cost;
    st.lambda = r.lambda;
    st.step_norm = r.step_norm;
    st.grad_norm = r.grad_norm;
    return st;
}
