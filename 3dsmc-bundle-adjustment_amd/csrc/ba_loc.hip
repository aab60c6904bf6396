// ba_loc.hip — ba_localize's kernel (ba_loc.h): pose-only Levenberg-Marquardt of one camera per workgroup, the whole
// trust-region loop in one launch.
//
// With the points and the intrinsics constant a camera's problem has six parameters, so the "linear solver" is a 6x6
// Cholesky one lane does in registers and the observation pass is all the parallel work there is. Per LM iteration the
// workgroup makes ONE pass over the camera's observations, at the candidate pose, with lin_obs: it yields the
// candidate's cost (the decision needs it) and, should the step be accepted, the next iteration's J^T J and J^T f, so
// an accepted step costs no second pass and a rejected one keeps the sums of the pose it returns to and only
// re-damps. Iteration 0 is the same pass at the given pose.
//
// Sums: per thread 20 entries of J^T J (upper-packed; U(0,1) is structurally zero, ba_device.h), 6 of J^T f, the cost
// and the count of failed evaluations; DPP sum inside a wave, then the four wave sums added in wave order through LDS.
// Thread t takes the camera's observations t, t + 256, ... of its own list, so every sum's order is set by the
// observation's position among its camera's observations and by nothing else in the call.
//
// The serial part (scaling, damping, Cholesky, solve, se3_plus, model cost change, decision) runs on thread 0 with its
// state in LDS; what it decides reaches the workgroup through LocLds::action behind a barrier, and every barrier sits
// in workgroup-uniform control flow. No workgroup reads anything another one writes.
//
// Thread t's first observation (pixel, depth, point: 6 doubles) stays in registers across the iterations; a camera
// with more than 256 observations re-reads the rest through the L2 every pass.
#include "ba_loc.h"

#include "ba_common.h"

namespace miba {

namespace {

constexpr int LOC_NW = LOC_TPB / 64;
// the pass's sums: U without U(0,1) (20) | g (6) | cost | failed evaluations
constexpr int LOC_NS = 28;
constexpr int S_G = 20, S_COST = 26, S_BAD = 27;

enum { LOC_STOP = 0, LOC_RUN = 1 };

// thread 0's LM state (Ceres 2.0 TrustRegionMinimizer + LevenbergMarquardtStrategy bookkeeping of one camera)
struct LocState {
    double x[7];      // the accepted pose
    double H[21];     // J^T J at x, upper-packed (i <= j): q = 6 i - i (i - 1) / 2 + (j - i)
    double g[6];      // J^T f at x
    double scale[6];  // Jacobi scaling, taken at iteration 0
    double radius, decrease_factor, x_cost, xnorm2, gmax, final_cost, initial_cost, mcc;
    int iter, n_succ, n_unsucc, n_invalid, step_ok, termination, msg;
};

struct LocLds {
    double part[LOC_NW][LOC_NS];
    double sum[LOC_NS];  // the last pass's sums
    double pose[7];      // the pose the next pass evaluates (the candidate)
    LocState S;
    int action;
};

struct LocObs {
    double u, v, d, X[3];
};

__device__ __forceinline__ LocObs loc_load(const LocArgs& a, int o) {
    const int k = a.idx[o];
    const double2 uv = a.uv[k];
    const double* X = a.pts + 3 * (size_t)a.obs_pt[k];
    return LocObs{uv.x, uv.y, a.depth[k], {X[0], X[1], X[2]}};
}

__host__ __device__ constexpr int hq(int i, int j) { return 6 * i - (i * (i - 1)) / 2 + (j - i); }  // i <= j

// One pass over the camera's observations at L.pose; L.sum valid for every thread after it.
__device__ __forceinline__ void loc_pass(const LocArgs& a, const BaConsts& c, const LocCam& w, const double K[4],
                                         const LocObs& first, LocLds& L) {
    const int tid = threadIdx.x;
    double pose[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) pose[j] = L.pose[j];
    double acc[LOC_NS];
#pragma unroll
    for (int i = 0; i < LOC_NS; ++i) acc[i] = 0.0;
    auto take = [&](const LocObs& ob) {
        ObsEval ev;
        double jc[18], jp[9], jk[8];
        lin_obs(c, pose, ob.X, K, ob.u, ob.v, ob.d, ev, jc, jp, jk);
        if (ev.ok) cam_accum_u(acc, jc, ev.f, ev.cost, true);
        else acc[S_BAD] += 1.0;
    };
    // the thread's first observation from its registers, the rest (a camera of more than LOC_TPB) through the L2
    if (w.begin + tid < w.end) take(first);
    for (int o = w.begin + tid + LOC_TPB; o < w.end; o += LOC_TPB) take(loc_load(a, o));
    wave_sum_dpp<LOC_NS>(acc);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < LOC_NS; ++i) L.part[wave][i] = acc[i];
    __syncthreads();
    if (tid < LOC_NS) {
        double s = L.part[0][tid];
#pragma unroll
        for (int k = 1; k < LOC_NW; ++k) s += L.part[k][tid];
        L.sum[tid] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ void loc_log(const LocArgs& a, int row, double cost, double dc, double gm, double sn,
                                        double rho, double radius, double acc) {
    if (a.log_wg != (int)blockIdx.x || row >= a.log_max_rows) return;
    double* r = a.log + (size_t)row * LOG_W;
    r[0] = cost; r[1] = dc; r[2] = gm; r[3] = sn; r[4] = rho; r[5] = radius; r[6] = acc; r[7] = 0.0;
}

// thread 0: the pass's sums become the linearisation at S.x (H, g, the cost) and the gradient max-norm
// ||x - Plus(x, -g)||_inf is taken (Ceres 2.0 trust_region_minimizer)
__device__ __forceinline__ void loc_absorb(LocLds& L) {
    LocState& S = L.S;
#pragma unroll
    for (int q = 0; q < 21; ++q) S.H[q] = q == 0 ? L.sum[0] : (q == 1 ? 0.0 : L.sum[q - 1]);
    double ng[6], x[7], tp[7];
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        S.g[d] = L.sum[S_G + d];
        ng[d] = -L.sum[S_G + d];
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = S.x[j];
    se3_plus(x, ng, tp);
    double gm = 0.0, xn2 = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        gm = fmax(gm, fabs(x[j] - tp[j]));
        xn2 += x[j] * x[j];
    }
    S.gmax = gm;
    S.xnorm2 = xn2;
    S.x_cost = L.sum[S_COST];
}

// thread 0: from the state to the next candidate (L.pose, S.mcc, action LOC_RUN) or to the end (LOC_STOP). Invalid
// steps need no pass (the cost at x is known), so they loop here; every trip counts an iteration, so the loop is
// bounded by max_num_iterations.
__device__ __forceinline__ void loc_next_step(const LocArgs& a, const BaConsts& c, const LmParams& prm, LocLds& L) {
    LocState& S = L.S;
    for (;;) {
        // FinalizeIterationAndCheckIfMinimizerCanContinue
        const bool t_iter = S.iter >= prm.max_iter;
        const bool t_grad = !t_iter && S.step_ok && S.gmax <= prm.gradient_tolerance;
        const bool t_rad = !t_iter && !t_grad && S.radius <= prm.min_radius;
        if (t_iter || t_grad || t_rad) {
            S.termination = t_iter ? 1 : 0;
            S.msg = t_iter ? MSG_MAX_ITER : (t_grad ? MSG_GRAD_TOL : MSG_MIN_RADIUS);
            L.action = LOC_STOP;
            return;
        }
        S.iter += 1;
        // the damped, Jacobi-scaled system A y = b: A = s H s + clamp(diag(s H s)) / radius, b = s g
        double sc[6], A[6][6], y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) sc[i] = S.scale[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) A[j][i] = sc[i] * S.H[hq(i, j)] * sc[j];
            const double u = A[i][i];
            A[i][i] = u + fmin(fmax(u, c.min_diag), c.max_diag) / S.radius;
            y[i] = sc[i] * S.g[i];
        }
        // (scheduling barriers between the phases of the step, here and below: left alone, the scheduler interleaves
        // the unrolled system build, Cholesky, solves, model cost change and se3_plus, whose operands are then all live
        // at once: 255 VGPRs and 28 B of scratch per lane for the whole kernel against 195 and none with them)
        __builtin_amdgcn_sched_barrier(0);
        // Cholesky A = L L^T in the lower triangle; a non-positive or non-finite pivot is a linear-solver failure
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double d = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
            const bool ok = d > 0.0 && d < INFINITY;
            bad = bad || !ok;
            const double l = sqrt(ok ? d : 1.0);
            A[j][j] = l;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double v = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
                A[i][j] = v / l;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {  // L z = b
            double v = y[i];
#pragma unroll
            for (int k = 0; k < i; ++k) v -= A[i][k] * y[k];
            y[i] = v / A[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {  // L^T y = z
            double v = y[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) v -= A[k][i] * y[k];
            y[i] = v / A[i][i];
        }
        __builtin_amdgcn_sched_barrier(0);
        double delta[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            delta[i] = -sc[i] * y[i];
            bad = bad || !isfinite(delta[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
        // model cost change -(J d)^T (f + J d / 2) = -(d^T g + d^T H d / 2), from the unscaled sums
        double dg = 0.0, dHd = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double hd = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) hd += S.H[i <= j ? hq(i, j) : hq(j, i)] * delta[j];
            dHd += delta[i] * hd;
            dg += delta[i] * S.g[i];
        }
        __builtin_amdgcn_sched_barrier(0);
        const double mcc = -(dg + 0.5 * dHd);
        const bool valid = !bad && isfinite(mcc) && mcc > 0.0;
        if (!valid) {  // HandleInvalidStep
            S.n_unsucc += 1;
            if (++S.n_invalid >= prm.max_invalid) {
                S.termination = 2;
                S.msg = MSG_INVALID;
                loc_log(a, S.iter, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 0.0);
                L.action = LOC_STOP;
                return;
            }
            S.radius /= S.decrease_factor;
            S.decrease_factor *= 2.0;
            S.step_ok = 0;
            loc_log(a, S.iter, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 0.0);
            continue;
        }
        S.n_invalid = 0;
        __builtin_amdgcn_sched_barrier(0);
        S.mcc = mcc;
        double x[7], xc[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) x[j] = S.x[j];
        se3_plus(x, delta, xc);
#pragma unroll
        for (int j = 0; j < 7; ++j) L.pose[j] = xc[j];
        L.action = LOC_RUN;
        return;
    }
}

// thread 0: the decision on the candidate L.pose whose sums the pass left in L.sum. Returns true when the loop ends.
__device__ __forceinline__ bool loc_decide(const LocArgs& a, const LmParams& prm, LocLds& L) {
    LocState& S = L.S;
    double cand = L.sum[S_COST];
    if (L.sum[S_BAD] > 0.0 || !isfinite(cand)) cand = DBL_MAX;
    double sn2 = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double df = S.x[j] - L.pose[j];
        sn2 += df * df;
    }
    const double step_norm = sqrt(sn2);
    const double xnorm = sqrt(S.xnorm2);
    const double cost_change = S.x_cost - cand;
    const bool t_par = step_norm <= prm.parameter_tolerance * (xnorm + prm.parameter_tolerance);
    const bool t_fun = !t_par && fabs(cost_change) <= prm.function_tolerance * S.x_cost;
    if (t_par || t_fun) {
        S.termination = 0;
        S.msg = t_par ? MSG_PARAM_TOL : MSG_FUNC_TOL;
        loc_log(a, S.iter, cand, cost_change, S.gmax, step_norm, 0.0, S.radius, -1.0);
        return true;
    }
    const double rho = (cand >= DBL_MAX) ? -DBL_MAX : cost_change / S.mcc;
    if (rho > prm.min_relative_decrease) {  // HandleSuccessfulStep + LM StepAccepted
#pragma unroll
        for (int j = 0; j < 7; ++j) S.x[j] = L.pose[j];
        loc_absorb(L);
        const double t = 2.0 * rho - 1.0;
        S.radius = S.radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
        S.radius = fmin(prm.max_radius, S.radius);
        S.decrease_factor = 2.0;
        S.step_ok = 1;
        S.n_succ += 1;
        S.final_cost = fmin(S.final_cost, S.x_cost);
        loc_log(a, S.iter, S.x_cost, cost_change, S.gmax, step_norm, rho, S.radius, 1.0);
    } else {  // HandleUnsuccessfulStep + LM StepRejected: the sums at x stay as they are
        S.radius /= S.decrease_factor;
        S.decrease_factor *= 2.0;
        S.step_ok = 0;
        S.n_unsucc += 1;
        S.final_cost = fmin(S.final_cost, cand);
        loc_log(a, S.iter, cand, cost_change, S.gmax, step_norm, rho, S.radius, 0.0);
    }
    return false;
}

__global__ __launch_bounds__(LOC_TPB) void k_loc_lm(LocArgs a, BaConsts c, LmParams prm) {
    __shared__ LocLds L;
    const int tid = threadIdx.x;
    const LocCam w = a.wg[blockIdx.x];
    c.sw_r = w.sw_r;
    c.sw_d = w.sw_d;
    const double K[4] = {a.K[0], a.K[1], a.K[2], a.K[3]};
    LocObs first = LocObs{0.0, 0.0, 0.0, {0.0, 0.0, 0.0}};
    if (w.begin + tid < w.end) first = loc_load(a, w.begin + tid);
    if (tid < 7) {
        const double v = a.cams[7 * (size_t)w.cam + tid];
        L.pose[tid] = v;
        L.S.x[tid] = v;
    }
    __syncthreads();
    loc_pass(a, c, w, K, first, L);  // iteration 0: the pass at the given pose
    if (tid == 0) {
        LocState& S = L.S;
        S.radius = a.initial_radius;
        S.decrease_factor = 2.0;
        S.mcc = 0.0;
        S.iter = 0; S.n_succ = 1; S.n_unsucc = 0; S.n_invalid = 0; S.step_ok = 1;
        S.termination = -1; S.msg = MSG_NONE;
        loc_absorb(L);
        if (L.sum[S_BAD] > 0.0 || !isfinite(S.x_cost)) {  // "Residual and Jacobian evaluation failed."
            S.x_cost = S.initial_cost = S.final_cost = __builtin_nan("");
            S.termination = 2;
            S.msg = MSG_EVAL_FAIL;
            L.action = LOC_STOP;
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) S.scale[i] = a.jacobi_scaling ? 1.0 / (1.0 + sqrt(S.H[hq(i, i)])) : 1.0;
            S.initial_cost = S.final_cost = S.x_cost;
            loc_log(a, 0, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 1.0);
            loc_next_step(a, c, prm, L);
        }
    }
    __syncthreads();
    while (L.action == LOC_RUN) {  // (workgroup-uniform: written by thread 0 before the barrier above / below)
        loc_pass(a, c, w, K, first, L);
        if (tid == 0) {
            if (loc_decide(a, prm, L)) L.action = LOC_STOP;
            else loc_next_step(a, c, prm, L);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const LocState& S = L.S;
        double* st = a.stats + (size_t)blockIdx.x * LOC_STAT;
        st[0] = (double)(w.end - w.begin);
        st[1] = S.initial_cost;
        st[2] = S.final_cost;
        st[3] = (double)S.iter;
        st[4] = (double)S.n_succ;
        st[5] = (double)S.n_unsucc;
        st[6] = (double)S.termination;
        st[7] = (double)S.msg;
    }
    if (tid < 7) a.cams[7 * (size_t)w.cam + tid] = L.S.x[tid];
}

}  // namespace

hipError_t launch_loc_lm(const LocArgs& a, const BaConsts& c, const LmParams& prm, int n_wg, hipStream_t s) {
    if (n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_loc_lm, dim3((unsigned)n_wg), dim3(LOC_TPB), 0, s, a, c, prm);
    return hipGetLastError();
}

}  // namespace miba
