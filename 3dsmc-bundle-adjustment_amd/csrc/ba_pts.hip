// ba_pts.hip — ba_refine_points' kernel (ba_pts.h): structure-only Levenberg-Marquardt of one point per row of 16
// lanes, the whole trust-region loop in one launch.
//
// With the cameras and the intrinsics constant a point's problem has three parameters and about ten observations
// (10^5 problems of ~10 observations where ba_localize has 10^2 of ~200), so a workgroup per problem would idle 246
// of its 256 lanes. Here a point owns one DPP row: lane j of the row takes the point's observations j, j + 16, ... of
// its own list, dpp_row_sum (ba_solve_util.h) leaves every sum in all 16 lanes with fixed bits, and a wave carries
// four points, a workgroup 16. No LDS, no barrier: a point never waits on anything outside its row.
//
// Per LM iteration the row makes ONE pass over the point's observations, at the candidate position, with lin_obs: it
// yields the candidate's cost (the decision needs it) and, should the step be accepted, the next iteration's
// Jp^T Jp and Jp^T f, so an accepted step costs no second pass and a rejected one keeps the sums of the position it
// returns to and only re-damps (k_loc_lm's restatement of the loop). Iteration 0 is the same pass at the given
// position.
//
// Sums: per lane 6 entries of Jp^T Jp (upper-packed), 3 of Jp^T f, the cost and the count of failed evaluations. Every
// sum's order is set by the observation's position among its point's observations and by nothing else in the call.
//
// The serial part (scaling, damping, 3x3 Cholesky, step, model cost change, decision) runs redundantly in all 16
// lanes of the row on registers: the same inputs through the same instructions, so the lanes hold the same bits and
// nothing has to be broadcast. Lane 0 of the row writes the log, the statistics and the position.
//
// The loop is wave-uniform: it runs while any row of the wave is active (a ballot), so the DPP sums always execute
// with all 64 lanes. A finished row is predicated off: it takes no observation and its state is frozen, so its result
// does not depend on how long its wave-mates run.
//
// Lane j's first observation (pixel, depth and its camera's pose: 10 doubles) stays in registers across the
// iterations; a point with more than 16 observations re-reads the rest through the L2 every pass.
#include "ba_pts.h"

#include "ba_common.h"

namespace miba {

namespace {

// the pass's sums: Jp^T Jp upper-packed (6) | Jp^T f (3) | cost | failed evaluations
constexpr int PTS_NS = 11;
constexpr int P_G = 6, P_COST = 9, P_BAD = 10;

// a row's LM state (Ceres 2.0 TrustRegionMinimizer + LevenbergMarquardtStrategy bookkeeping of one point), the same
// bits in each of its lanes
struct PtsState {
    double x[3];      // the accepted position
    double xc[3];     // the position the next pass evaluates (the candidate)
    double H[6];      // Jp^T Jp at x, upper-packed (i <= j): q = 3 i - i (i - 1) / 2 + (j - i)
    double g[3];      // Jp^T f at x
    double scale[3];  // Jacobi scaling, taken at iteration 0
    double radius, decrease_factor, x_cost, xnorm2, gmax, final_cost, initial_cost, mcc;
    int iter, n_succ, n_unsucc, n_invalid, step_ok, termination, msg;
};

struct PtsObs {
    double u, v, d, pose[7];
};

__device__ __forceinline__ PtsObs pts_load(const PtsArgs& a, int o) {
    const int k = a.idx[o];
    const double2 uv = a.uv[k];
    const double* T = a.cams + 7 * (size_t)a.obs_cam[k];
    return PtsObs{uv.x, uv.y, a.depth[k], {T[0], T[1], T[2], T[3], T[4], T[5], T[6]}};
}

__host__ __device__ constexpr int pq(int i, int j) { return 3 * i - (i * (i - 1)) / 2 + (j - i); }  // i <= j

// One pass over the point's observations at X; sum valid in every lane of the row after it. Called in wave-uniform
// control flow (the DPP sums); a row that is not `on` takes no observation.
__device__ __forceinline__ void pts_pass(const PtsArgs& a, const BaConsts& c, const PtsRec& w, const double K[4],
                                         const PtsObs& first, const double X[3], int j, bool on,
                                         double (&sum)[PTS_NS]) {
#pragma unroll
    for (int i = 0; i < PTS_NS; ++i) sum[i] = 0.0;
    auto take = [&](const PtsObs& ob) {
        ObsEval ev;
        double jc[18], jp[9], jk[8];
        lin_obs(c, ob.pose, X, K, ob.u, ob.v, ob.d, ev, jc, jp, jk);
        if (ev.ok) {
            sum[0] += jp[0] * jp[0] + jp[3] * jp[3] + jp[6] * jp[6];
            sum[1] += jp[0] * jp[1] + jp[3] * jp[4] + jp[6] * jp[7];
            sum[2] += jp[0] * jp[2] + jp[3] * jp[5] + jp[6] * jp[8];
            sum[3] += jp[1] * jp[1] + jp[4] * jp[4] + jp[7] * jp[7];
            sum[4] += jp[1] * jp[2] + jp[4] * jp[5] + jp[7] * jp[8];
            sum[5] += jp[2] * jp[2] + jp[5] * jp[5] + jp[8] * jp[8];
            sum[P_G + 0] += jp[0] * ev.f[0] + jp[3] * ev.f[1] + jp[6] * ev.f[2];
            sum[P_G + 1] += jp[1] * ev.f[0] + jp[4] * ev.f[1] + jp[7] * ev.f[2];
            sum[P_G + 2] += jp[2] * ev.f[0] + jp[5] * ev.f[1] + jp[8] * ev.f[2];
            sum[P_COST] += ev.cost;
        } else {
            sum[P_BAD] += 1.0;
        }
    };
    if (on) {
        // the lane's first observation from its registers, the rest (a point of more than PTS_LANES) through the L2
        if (w.begin + j < w.end) take(first);
        for (int o = w.begin + j + PTS_LANES; o < w.end; o += PTS_LANES) take(pts_load(a, o));
    }
#pragma unroll
    for (int i = 0; i < PTS_NS; ++i) sum[i] = dpp_row_sum(sum[i]);
}

__device__ __forceinline__ void pts_log(const PtsArgs& a, bool logon, int row, double cost, double dc, double gm,
                                        double sn, double rho, double radius, double acc) {
    if (!logon || row >= a.log_max_rows) return;
    double* r = a.log + (size_t)row * LOG_W;
    r[0] = cost; r[1] = dc; r[2] = gm; r[3] = sn; r[4] = rho; r[5] = radius; r[6] = acc; r[7] = 0.0;
}

// the pass's sums become the linearisation at S.x (H, g, the cost) and the gradient max-norm ||x - (x + -g)||_inf is
// taken as point_tail (ba_common.h) forms it
__device__ __forceinline__ void pts_absorb(PtsState& S, const double (&sum)[PTS_NS]) {
#pragma unroll
    for (int q = 0; q < 6; ++q) S.H[q] = sum[q];
    double gm = 0.0, xn2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        S.g[i] = sum[P_G + i];
        gm = fmax(gm, fabs(S.x[i] - (S.x[i] + -S.g[i])));
        xn2 += S.x[i] * S.x[i];
    }
    S.gmax = gm;
    S.xnorm2 = xn2;
    S.x_cost = sum[P_COST];
}

// From the state to the next candidate (S.xc, S.mcc; returns true) or to the end (false). Invalid steps need no pass
// (the cost at x is known), so they loop here; every trip counts an iteration, so the loop is bounded by
// max_num_iterations.
__device__ __forceinline__ bool pts_next_step(const PtsArgs& a, const BaConsts& c, const LmParams& prm, PtsState& S,
                                              bool logon) {
    for (;;) {
        // FinalizeIterationAndCheckIfMinimizerCanContinue
        const bool t_iter = S.iter >= prm.max_iter;
        const bool t_grad = !t_iter && S.step_ok && S.gmax <= prm.gradient_tolerance;
        const bool t_rad = !t_iter && !t_grad && S.radius <= prm.min_radius;
        if (t_iter || t_grad || t_rad) {
            S.termination = t_iter ? 1 : 0;
            S.msg = t_iter ? MSG_MAX_ITER : (t_grad ? MSG_GRAD_TOL : MSG_MIN_RADIUS);
            return false;
        }
        S.iter += 1;
        // the damped, Jacobi-scaled system A y = b: A = s H s + clamp(diag(s H s)) / radius, b = s g
        double sc[3], A[3][3], y[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) sc[i] = S.scale[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = i; k < 3; ++k) A[k][i] = sc[i] * S.H[pq(i, k)] * sc[k];
            const double u = A[i][i];
            A[i][i] = u + fmin(fmax(u, c.min_diag), c.max_diag) / S.radius;
            y[i] = sc[i] * S.g[i];
        }
        __builtin_amdgcn_sched_barrier(0);
        // Cholesky A = L L^T in the lower triangle (IEEE square root and division); a non-positive or non-finite
        // pivot is a linear-solver failure
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double d = A[k][k];
#pragma unroll
            for (int m = 0; m < k; ++m) d -= A[k][m] * A[k][m];
            const bool ok = d > 0.0 && d < INFINITY;
            bad = bad || !ok;
            const double l = sqrt(ok ? d : 1.0);
            A[k][k] = l;
#pragma unroll
            for (int i = k + 1; i < 3; ++i) {
                double v = A[i][k];
#pragma unroll
                for (int m = 0; m < k; ++m) v -= A[i][m] * A[k][m];
                A[i][k] = v / l;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {  // L z = b
            double v = y[i];
#pragma unroll
            for (int m = 0; m < i; ++m) v -= A[i][m] * y[m];
            y[i] = v / A[i][i];
        }
#pragma unroll
        for (int i = 2; i >= 0; --i) {  // L^T y = z
            double v = y[i];
#pragma unroll
            for (int m = i + 1; m < 3; ++m) v -= A[m][i] * y[m];
            y[i] = v / A[i][i];
        }
        __builtin_amdgcn_sched_barrier(0);
        double delta[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            delta[i] = -sc[i] * y[i];
            bad = bad || !isfinite(delta[i]);
        }
        // model cost change -(J d)^T (f + J d / 2) = -(d^T g + d^T H d / 2), from the unscaled sums
        double dg = 0.0, dHd = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double hd = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) hd += S.H[i <= k ? pq(i, k) : pq(k, i)] * delta[k];
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
                pts_log(a, logon, S.iter, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 0.0);
                return false;
            }
            S.radius /= S.decrease_factor;
            S.decrease_factor *= 2.0;
            S.step_ok = 0;
            pts_log(a, logon, S.iter, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 0.0);
            continue;
        }
        S.n_invalid = 0;
        S.mcc = mcc;
#pragma unroll
        for (int i = 0; i < 3; ++i) S.xc[i] = S.x[i] + delta[i];
        return true;
    }
}

// The decision on the candidate S.xc whose sums the pass left in `sum`. Returns true when the loop ends.
__device__ __forceinline__ bool pts_decide(const PtsArgs& a, const LmParams& prm, PtsState& S,
                                           const double (&sum)[PTS_NS], bool logon) {
    double cand = sum[P_COST];
    if (sum[P_BAD] > 0.0 || !isfinite(cand)) cand = DBL_MAX;
    double sn2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double df = S.x[i] - S.xc[i];
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
        pts_log(a, logon, S.iter, cand, cost_change, S.gmax, step_norm, 0.0, S.radius, -1.0);
        return true;
    }
    const double rho = (cand >= DBL_MAX) ? -DBL_MAX : cost_change / S.mcc;
    if (rho > prm.min_relative_decrease) {  // HandleSuccessfulStep + LM StepAccepted
#pragma unroll
        for (int i = 0; i < 3; ++i) S.x[i] = S.xc[i];
        pts_absorb(S, sum);
        const double t = 2.0 * rho - 1.0;
        S.radius = S.radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
        S.radius = fmin(prm.max_radius, S.radius);
        S.decrease_factor = 2.0;
        S.step_ok = 1;
        S.n_succ += 1;
        S.final_cost = fmin(S.final_cost, S.x_cost);
        pts_log(a, logon, S.iter, S.x_cost, cost_change, S.gmax, step_norm, rho, S.radius, 1.0);
    } else {  // HandleUnsuccessfulStep + LM StepRejected: the sums at x stay as they are
        S.radius /= S.decrease_factor;
        S.decrease_factor *= 2.0;
        S.step_ok = 0;
        S.n_unsucc += 1;
        S.final_cost = fmin(S.final_cost, cand);
        pts_log(a, logon, S.iter, cand, cost_change, S.gmax, step_norm, rho, S.radius, 0.0);
    }
    return false;
}

__global__ __launch_bounds__(PTS_TPB) void k_pts_lm(PtsArgs a, BaConsts c, LmParams prm) {
    const int tid = threadIdx.x;
    const int j = tid & (PTS_LANES - 1);
    const size_t rec = (size_t)blockIdx.x * PTS_PER_WG + (size_t)(tid / PTS_LANES);
    const bool valid = rec < (size_t)a.n_rec;  // (the last workgroup's rows past the records idle through the loop)
    PtsRec w = PtsRec{0, 0, 0, 0, 0.0, 0.0};
    if (valid) w = a.rec[rec];
    c.sw_r = w.sw_r;
    c.sw_d = w.sw_d;
    const double K[4] = {a.K[0], a.K[1], a.K[2], a.K[3]};
    PtsObs first = PtsObs{0.0, 0.0, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    if (valid && w.begin + j < w.end) first = pts_load(a, w.begin + j);
    const bool logon = valid && j == 0 && a.log_rec >= 0 && rec == (size_t)a.log_rec;

    PtsState S;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        S.x[i] = valid ? a.pts[3 * (size_t)w.pt + i] : 0.0;
        S.xc[i] = S.x[i];
        S.g[i] = 0.0;
        S.scale[i] = 1.0;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) S.H[q] = 0.0;
    S.radius = a.initial_radius;
    S.decrease_factor = 2.0;
    S.mcc = 0.0;
    S.x_cost = S.xnorm2 = S.gmax = S.final_cost = S.initial_cost = 0.0;
    S.iter = 0; S.n_succ = 1; S.n_unsucc = 0; S.n_invalid = 0; S.step_ok = 1;
    S.termination = -1; S.msg = MSG_NONE;

    double sum[PTS_NS];
    pts_pass(a, c, w, K, first, S.xc, j, valid, sum);  // iteration 0: the pass at the given position
    bool active = false;
    if (valid) {
        pts_absorb(S, sum);
        if (sum[P_BAD] > 0.0 || !isfinite(S.x_cost)) {  // "Residual and Jacobian evaluation failed."
            S.x_cost = S.initial_cost = S.final_cost = __builtin_nan("");
            S.termination = 2;
            S.msg = MSG_EVAL_FAIL;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) S.scale[i] = a.jacobi_scaling ? 1.0 / (1.0 + sqrt(S.H[pq(i, i)])) : 1.0;
            S.initial_cost = S.final_cost = S.x_cost;
            pts_log(a, logon, 0, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 1.0);
            active = pts_next_step(a, c, prm, S, logon);
        }
    }
    while (__ballot(active) != 0ull) {  // wave-uniform: all 64 lanes make the pass while any row is active
        pts_pass(a, c, w, K, first, S.xc, j, active, sum);
        if (active) {
            if (pts_decide(a, prm, S, sum, logon)) active = false;
            else active = pts_next_step(a, c, prm, S, logon);
        }
    }
    if (valid && j == 0) {
        double* st = a.stats + rec * PTS_STAT;
        st[0] = (double)(w.end - w.begin);
        st[1] = S.initial_cost;
        st[2] = S.final_cost;
        st[3] = (double)S.iter;
        st[4] = (double)S.n_succ;
        st[5] = (double)S.n_unsucc;
        st[6] = (double)S.termination;
        st[7] = (double)S.msg;
#pragma unroll
        for (int i = 0; i < 3; ++i) a.xout[3 * rec + i] = S.x[i];
    }
}

}  // namespace

hipError_t launch_pts_lm(const PtsArgs& a, const BaConsts& c, const LmParams& prm, hipStream_t s) {
    if (a.n_rec <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pts_lm, dim3((unsigned)pts_workgroups((size_t)a.n_rec)), dim3(PTS_TPB), 0, s, a, c, prm);
    return hipGetLastError();
}

}  // namespace miba
