// ba_block_lm.h — the trust-region loop of one small dense block (device, internal): Levenberg-Marquardt of a problem
// whose N-dimensional step one lane solves in registers. k_loc_lm (ba_loc.hip: N = 6, a pose of P = 7 numbers) and
// k_pts_lm (ba_pts.hip: N = P = 3, a position) are its two instances.
//
// Per LM iteration the kernel makes ONE pass over the problem's observations, at the candidate: it yields the
// candidate's cost (the decision needs it) and, should the step be accepted, the next iteration's J^T J and J^T f, so
// an accepted step costs no second pass and a rejected one keeps the sums of the x it returns to and only re-damps.
// Iteration 0 is the same pass at the given x. The kernel owns the pass, its reduction, the mapping of the pass's sums
// to H / g / cost (the `load` it hands to block_lm_absorb) and the control skeleton; everything between two passes is
// here:
//
//     block_lm_init; pass; block_lm_absorb; if (block_lm_first) run = block_lm_next_step;
//     while (run) { pass at xc; run = !block_lm_decide && block_lm_next_step; }
//     block_lm_write_stats
//
// The bookkeeping is Ceres 2.0's TrustRegionMinimizer with the LevenbergMarquardtStrategy: the termination tests in
// their order, the Jacobi scaling taken at iteration 0, the clamped diagonal over the radius, HandleInvalidStep, the
// step-quality radius update. The candidate xc stays where the kernel keeps it (LDS or registers) and is passed by
// reference; the state may live in LDS (one thread steps it) or in registers (lanes step it redundantly).
//
// Retract: the stage's manifold, `static void plus(const double (&x)[P], const double (&d)[N], double (&out)[P])`.
#pragma once
#include "ba_common.h"

namespace miba {

// upper-packed index of (i, j), i <= j, in an N x N symmetric matrix
template <int N>
__host__ __device__ constexpr int upq(int i, int j) { return N * i - (i * (i - 1)) / 2 + (j - i); }

template <int N, int P>
struct BlockLmState {
    double x[P];                  // the accepted parameters
    double H[N * (N + 1) / 2];    // J^T J at x, upper-packed (upq<N>)
    double g[N];                  // J^T f at x
    double scale[N];              // Jacobi scaling, taken at iteration 0
    double radius, decrease_factor, x_cost, xnorm2, gmax, final_cost, initial_cost, mcc;
    int iter, n_succ, n_unsucc, n_invalid, step_ok, termination, msg;
};

// where the problem's iteration rows go (on: this lane's problem is the logged one and this lane writes for it)
struct BlockLmLog {
    double* rows;  // [max_rows * LOG_W]
    int max_rows;
    bool on;
};

__device__ __forceinline__ void block_lm_log(const BlockLmLog& lg, int row, double cost, double dc, double gm, double sn,
                                             double rho, double radius, double acc) {
    if (!lg.on || row >= lg.max_rows) return;
    double* r = lg.rows + (size_t)row * LOG_W;
    r[0] = cost; r[1] = dc; r[2] = gm; r[3] = sn; r[4] = rho; r[5] = radius; r[6] = acc; r[7] = 0.0;
}

// the iteration-0 state at the given x0
template <int N, int P>
__device__ __forceinline__ void block_lm_init(BlockLmState<N, P>& S, const double (&x0)[P], double initial_radius) {
#pragma unroll
    for (int j = 0; j < P; ++j) S.x[j] = x0[j];
#pragma unroll
    for (int q = 0; q < N * (N + 1) / 2; ++q) S.H[q] = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        S.g[i] = 0.0;
        S.scale[i] = 1.0;
    }
    S.radius = initial_radius;
    S.decrease_factor = 2.0;
    S.mcc = 0.0;
    S.x_cost = S.xnorm2 = S.gmax = S.final_cost = S.initial_cost = 0.0;
    S.iter = 0; S.n_succ = 1; S.n_unsucc = 0; S.n_invalid = 0; S.step_ok = 1;
    S.termination = -1; S.msg = MSG_NONE;
}

// the pass's sums become the linearisation at S.x: load(S) sets S.H, S.g and S.x_cost from them, and the gradient
// max-norm ||x - Plus(x, -g)||_inf is taken (Ceres 2.0 trust_region_minimizer)
template <class Retract, int N, int P, class Load>
__device__ __forceinline__ void block_lm_absorb(BlockLmState<N, P>& S, Load&& load) {
    load(S);
    double ng[N], x[P], tp[P];
#pragma unroll
    for (int d = 0; d < N; ++d) ng[d] = -S.g[d];
#pragma unroll
    for (int j = 0; j < P; ++j) x[j] = S.x[j];
    Retract::plus(x, ng, tp);
    double gm = 0.0, xn2 = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        gm = fmax(gm, fabs(x[j] - tp[j]));
        xn2 += x[j] * x[j];
    }
    S.gmax = gm;
    S.xnorm2 = xn2;
}

// after the first absorb: false when the evaluation at the given x failed (`bad`: an observation's evaluation failed),
// the loop never starts then; else the Jacobi scaling and log row 0
template <int N, int P>
__device__ __forceinline__ bool block_lm_first(BlockLmState<N, P>& S, bool bad, int jacobi_scaling,
                                               const BlockLmLog& lg) {
    if (bad || !isfinite(S.x_cost)) {  // "Residual and Jacobian evaluation failed."
        S.x_cost = S.initial_cost = S.final_cost = __builtin_nan("");
        S.termination = 2;
        S.msg = MSG_EVAL_FAIL;
        return false;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) S.scale[i] = jacobi_scaling ? 1.0 / (1.0 + sqrt(S.H[upq<N>(i, i)])) : 1.0;
    S.initial_cost = S.final_cost = S.x_cost;
    block_lm_log(lg, 0, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 1.0);
    return true;
}

// From the state to the next candidate (xc, S.mcc; returns true) or to the end (false). Invalid steps need no pass
// (the cost at x is known), so they loop here; every trip counts an iteration, so the loop is bounded by
// max_num_iterations.
template <class Retract, int N, int P>
__device__ __forceinline__ bool block_lm_next_step(BlockLmState<N, P>& S, double (&xc)[P], const BaConsts& c,
                                                   const LmParams& prm, const BlockLmLog& lg) {
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
        double sc[N], A[N][N], y[N];
#pragma unroll
        for (int i = 0; i < N; ++i) sc[i] = S.scale[i];
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = i; j < N; ++j) A[j][i] = sc[i] * S.H[upq<N>(i, j)] * sc[j];
            const double u = A[i][i];
            A[i][i] = u + fmin(fmax(u, c.min_diag), c.max_diag) / S.radius;
            y[i] = sc[i] * S.g[i];
        }
        // (scheduling barriers between the phases of the step, here and below: left alone, the scheduler interleaves
        // the unrolled system build, Cholesky, solves, model cost change and se3_plus, whose operands are then all live
        // at once: 255 VGPRs and 28 B of scratch per lane for the whole of k_loc_lm against 195 and none with them)
        __builtin_amdgcn_sched_barrier(0);
        // Cholesky A = L L^T in the lower triangle (IEEE square root and division); a non-positive or non-finite
        // pivot is a linear-solver failure
        bool bad = false;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double d = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
            const bool ok = d > 0.0 && d < INFINITY;
            bad = bad || !ok;
            const double l = sqrt(ok ? d : 1.0);
            A[j][j] = l;
#pragma unroll
            for (int i = j + 1; i < N; ++i) {
                double v = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
                A[i][j] = v / l;
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {  // L z = b
            double v = y[i];
#pragma unroll
            for (int k = 0; k < i; ++k) v -= A[i][k] * y[k];
            y[i] = v / A[i][i];
        }
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {  // L^T y = z
            double v = y[i];
#pragma unroll
            for (int k = i + 1; k < N; ++k) v -= A[k][i] * y[k];
            y[i] = v / A[i][i];
        }
        __builtin_amdgcn_sched_barrier(0);
        double delta[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            delta[i] = -sc[i] * y[i];
            bad = bad || !isfinite(delta[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
        // model cost change -(J d)^T (f + J d / 2) = -(d^T g + d^T H d / 2), from the unscaled sums
        double dg = 0.0, dHd = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double hd = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) hd += S.H[i <= j ? upq<N>(i, j) : upq<N>(j, i)] * delta[j];
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
                block_lm_log(lg, S.iter, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 0.0);
                return false;
            }
            S.radius /= S.decrease_factor;
            S.decrease_factor *= 2.0;
            S.step_ok = 0;
            block_lm_log(lg, S.iter, S.x_cost, 0.0, S.gmax, 0.0, 0.0, S.radius, 0.0);
            continue;
        }
        S.n_invalid = 0;
        __builtin_amdgcn_sched_barrier(0);
        S.mcc = mcc;
        double x[P], t[P];
#pragma unroll
        for (int j = 0; j < P; ++j) x[j] = S.x[j];
        Retract::plus(x, delta, t);
#pragma unroll
        for (int j = 0; j < P; ++j) xc[j] = t[j];
        return true;
    }
}

// The decision on the candidate xc, whose pass gave `cost` (`bad`: an observation's evaluation failed). An accepted
// candidate becomes S.x and its sums are absorbed through `load`. Returns true when the loop ends.
template <class Retract, int N, int P, class Load>
__device__ __forceinline__ bool block_lm_decide(BlockLmState<N, P>& S, const double (&xc)[P], double cost, bool bad,
                                                const LmParams& prm, const BlockLmLog& lg, Load&& load) {
    double cand = cost;
    if (bad || !isfinite(cand)) cand = DBL_MAX;
    double sn2 = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double df = S.x[j] - xc[j];
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
        block_lm_log(lg, S.iter, cand, cost_change, S.gmax, step_norm, 0.0, S.radius, -1.0);
        return true;
    }
    const double rho = (cand >= DBL_MAX) ? -DBL_MAX : cost_change / S.mcc;
    if (rho > prm.min_relative_decrease) {  // HandleSuccessfulStep + LM StepAccepted
#pragma unroll
        for (int j = 0; j < P; ++j) S.x[j] = xc[j];
        block_lm_absorb<Retract>(S, load);
        const double t = 2.0 * rho - 1.0;
        S.radius = S.radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
        S.radius = fmin(prm.max_radius, S.radius);
        S.decrease_factor = 2.0;
        S.step_ok = 1;
        S.n_succ += 1;
        S.final_cost = fmin(S.final_cost, S.x_cost);
        block_lm_log(lg, S.iter, S.x_cost, cost_change, S.gmax, step_norm, rho, S.radius, 1.0);
    } else {  // HandleUnsuccessfulStep + LM StepRejected: the sums at x stay as they are
        S.radius /= S.decrease_factor;
        S.decrease_factor *= 2.0;
        S.step_ok = 0;
        S.n_unsucc += 1;
        S.final_cost = fmin(S.final_cost, cand);
        block_lm_log(lg, S.iter, cand, cost_change, S.gmax, step_norm, rho, S.radius, 0.0);
    }
    return false;
}

// the 8-double record of ba_loc_request.cam_stats / ba_pts_request.pt_stats
template <int N, int P>
__device__ __forceinline__ void block_lm_write_stats(const BlockLmState<N, P>& S, int n_obs, double* st) {
    st[0] = (double)n_obs;
    st[1] = S.initial_cost;
    st[2] = S.final_cost;
    st[3] = (double)S.iter;
    st[4] = (double)S.n_succ;
    st[5] = (double)S.n_unsucc;
    st[6] = (double)S.termination;
    st[7] = (double)S.msg;
}

}  // namespace miba
