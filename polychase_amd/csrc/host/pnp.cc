// pnp.cc -- LevMarqDenseSolver (cpp/pnp/lev_marq.h:99-389) + PnPProblem::Step
// (cpp/pnp/pnp_problem.h:101-131) on the host; residual sweeps (normal equations, cost, inliers)
// on the GPU through pc_pnp_* (one deterministic two-stage reduction per call).
#include "pnp.h"

#include <cmath>
#include <cstdlib>
#include <stdexcept>

#include "gpu_context.h"
#include "lm_loop.h"
#include "stage_clock.h"

namespace {

struct Params {  // PnPProblem::Parameters
    CameraState cam;
    Mat3f R;
};

pc_pnp_params ToGpu(const Params& p, bool opt_f, bool opt_pp, const BundleOptions& o) {
    pc_pnp_params g;
    for (int i = 0; i < 9; i++) g.R[i] = p.R[i];
    for (int i = 0; i < 3; i++) g.t[i] = p.cam.pose.t[i];
    g.fx = p.cam.intrinsics.fx;
    g.fy = p.cam.intrinsics.fy;
    g.cx = p.cam.intrinsics.cx;
    g.cy = p.cam.intrinsics.cy;
    g.aspect_ratio = p.cam.intrinsics.aspect_ratio;
    g.convention_opencv = p.cam.intrinsics.convention == CameraConvention::OpenCV ? 1 : 0;
    g.optimize_focal_length = opt_f ? 1 : 0;
    g.optimize_principal_point = opt_pp ? 1 : 0;
    g.loss_type = static_cast<int>(o.loss_type);
    g.loss_scale = o.loss_scale;
    return g;
}

struct GpuProblem {
    pc_context* ctx;
    pc_pnp_problem* prob = nullptr;
    ~GpuProblem() { pc_pnp_problem_destroy(prob); }
};

[[noreturn]] void ThrowHip(const char* what) { throw std::runtime_error(std::string(what) + ": " + pc_last_error()); }

void CheckArguments(size_t n, const PnPOptions& opts) {
    CHECK_GE(n, static_cast<size_t>(3));  // solvers.cc:54-55
    const int lt = static_cast<int>(opts.bundle_opts.loss_type);
    if (lt < 0 || lt > 2) throw std::runtime_error("Unknown loss type: " + std::to_string(lt));
}

// LevMarqDenseSolver over PnPProblem, as lm_loop.h wants it: 9x9 fp32 algebra on the host, the residual sweeps on the GPU.
// One sweep returns the cost of a parameter set AND its normal equations (pc_pnp_normal_equations_cost): the
// candidate of every LM step is evaluated that way, so an accepted step already holds the system the
// reference would build at the top of the next iteration (lev_marq.h:146-160) -- same numbers, half the
// GPU round trips.
struct DenseProblem {
    using Scalar = Float;
    struct System {
        float lower[45];
        float Jtr[9];
        float cost = 0;
    };

    pc_context* ctx;
    pc_pnp_problem* prob;
    const BundleOptions& bo;
    const bool opt_f, opt_pp;
    const CameraIntrinsics::Bounds bounds;
    Params params, params_new;
    System current, candidate;
    float JtJ[81];  // row-major, lower triangle meaningful
    float L[81];
    float diag[9], Jtr[9], step[9];

    void Sweep(const Params& p, System& out) {
        const pc_pnp_params g = ToGpu(p, opt_f, opt_pp, bo);
        int valid = 0;
        if (pc_pnp_normal_equations_cost(ctx, prob, &g, out.lower, out.Jtr, &valid, &out.cost) != PC_OK)
            ThrowHip("pc_pnp_normal_equations");
    }

    Float InitialCost() {
        Sweep(params, current);
        return current.cost;  // kShouldNormalize == false
    }
    Float Linearize() {  // unpacks the system that came with the accepted parameters' cost
        int o = 0;
        for (int a = 0; a < 9; a++)
            for (int b = 0; b <= a; b++) JtJ[9 * a + b] = current.lower[o++];
        for (int a = 0; a < 9; a++) Jtr[a] = current.Jtr[a];
        // JtJ_diag = diag.cwiseMax(1e-6).cwiseMin(1e32)  (:296)
        for (int a = 0; a < 9; a++) diag[a] = std::min(std::max(JtJ[10 * a], 1e-6f), 1e32f);
        float g2 = 0;
        for (int a = 0; a < 9; a++) g2 += Jtr[a] * Jtr[a];
        return std::sqrt(g2);
    }
    bool Factorize(Float lambda) {  // ComputeStep (:299-314): multiplicative damping, LLT of the lower triangle
        for (int a = 0; a < 9; a++)
            for (int b = 0; b <= a; b++) L[9 * a + b] = JtJ[9 * a + b];
        for (int a = 0; a < 9; a++) L[10 * a] = diag[a] * (1.0f + lambda);
        for (int a = 0; a < 9; a++) JtJ[10 * a] = diag[a];  // "remove dampening" leaves the clamped diagonal
        return CholeskyLower<9>(L);
    }
    Float Solve() {
        CholeskySolve<9>(L, Jtr, step);
        for (int a = 0; a < 9; a++) step[a] = -step[a];
        float s2 = 0;
        for (int a = 0; a < 9; a++) s2 += step[a] * step[a];
        return std::sqrt(s2);
    }
    Float EvaluateCandidate() {
        params_new.cam = params.cam;
        StepCamera(params_new.cam, step, opt_f, opt_pp, bounds);
        params_new.R = params_new.cam.pose.R();
        Sweep(params_new, candidate);
        return candidate.cost;
    }
    Float ExpectedChange() const {  // step^T (2 Jtr + JtJ_sym step)   (:183-186), fp32 like the reference
        Float expected = 0;
        for (int a = 0; a < 9; a++) {
            Float row = 0;
            for (int b = 0; b < 9; b++) row += (b <= a ? JtJ[9 * a + b] : JtJ[9 * b + a]) * step[b];
            expected += step[a] * (2.0f * Jtr[a] + row);
        }
        return expected;
    }
    void Accept() {
        params = params_new;
        current = candidate;
    }
    bool Report(const BundleStats&) { return true; }
};

}  // namespace

void SolvePnPIterative(const float* object_points, const float* image_points, const float* weights, size_t n,
                       const PnPOptions& opts, PnPResult& result) {
    CheckArguments(n, opts);
    GpuSection section;
    GpuProblem gp{SharedGpuContext()};
    {
        StageClock::Scope sc("pnp/create+upload");
        if (pc_pnp_problem_create(gp.ctx, object_points, image_points, weights, static_cast<int>(n), &gp.prob) != PC_OK)
            ThrowHip("pc_pnp_problem_create");
    }
    SolvePnPIterativeOnGpu(gp.prob, n, opts, result);
}

void SolvePnPIterativeOnGpu(pc_pnp_problem* problem, size_t n, const PnPOptions& opts, PnPResult& result) {
    CheckArguments(n, opts);
    const BundleOptions& bo = opts.bundle_opts;
    // PnPProblem: intrinsics are only optimised with more than 3 points (pnp_problem.h:34-35)
    const bool opt_f = opts.optimize_focal_length && n > 3;
    const bool opt_pp = opts.optimize_principal_point && n > 3;
    const CameraIntrinsics::Bounds bounds = result.camera.intrinsics.GetBounds();
    GpuSection section;
    pc_context* ctx = SharedGpuContext();

    // The solver runs on the device (pc_pnp_solve: the LM state lives in device memory, a one-lane kernel takes the
    // decisions between the residual sweeps).  POLYCHASE_PNP_HOST_LM=1 runs the same loop on the host instead,
    // one read-back per sweep -- the cross-check of the device state machine.
    const char* host_lm_env = std::getenv("POLYCHASE_PNP_HOST_LM");   // read per call: the tests flip it
    const bool host_lm = host_lm_env && host_lm_env[0] == '1';
    if (!host_lm) {
        const pc_pnp_camera init = ToPnpCamera(result.camera);
        const pc_pnp_solve_options so = ToPnpSolveOptions(bo, bounds, opt_f, opt_pp, opts.max_inlier_error);
        pc_pnp_solve_result sr;
        if (pc_pnp_solve(ctx, problem, &init, &so, &sr) != PC_OK) ThrowHip("pc_pnp_solve");
        FromPnpCamera(sr.camera, result.camera);
        result.bundle_stats = ToBundleStats(sr);
        result.inlier_ratio = static_cast<Float>(sr.inliers) / static_cast<Float>(n);
        return;
    }

    const Params start{result.camera, result.camera.pose.R()};
    DenseProblem dense{ctx, problem, bo, opt_f, opt_pp, bounds, start, start};
    result.bundle_stats = LevMarqLoop(bo, dense);  // LevMarqDenseSolver::Solve (lev_marq.h:132-228)
    result.camera = dense.params.cam;

    // inlier ratio (solvers.cc:31-47)
    int inliers = 0;
    if (opts.max_inlier_error > 0.0f) {
        const pc_pnp_params g = ToGpu(dense.params, opt_f, opt_pp, bo);
        float cost = 0;
        int valid = 0;
        if (pc_pnp_total_cost(ctx, problem, &g, opts.max_inlier_error * opts.max_inlier_error, &cost, &valid, &inliers) != PC_OK)
            ThrowHip("pc_pnp_total_cost");
    }
    result.inlier_ratio = static_cast<Float>(inliers) / static_cast<Float>(n);
}
