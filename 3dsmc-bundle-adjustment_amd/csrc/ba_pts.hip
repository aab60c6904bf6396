// ba_pts.hip — ba_refine_points' kernel (ba_pts.h): structure-only Levenberg-Marquardt of one point per row of 16
// lanes, the whole trust-region loop in one launch.
//
// With the cameras and the intrinsics constant a point's problem has three parameters and about ten observations
// (10^5 problems of ~10 observations where ba_localize has 10^2 of ~200), so a workgroup per problem would idle 246
// of its 256 lanes. Here a point owns one DPP row: lane j of the row takes the point's observations j, j + 16, ... of
// its own list, dpp_row_sum (ba_solve_util.h) leaves every sum in all 16 lanes with fixed bits, and a wave carries
// four points, a workgroup 16. No LDS, no barrier: a point never waits on anything outside its row.
//
// The loop is ba_block_lm.h's (N = 3, a component-wise add), one pass over the point's observations with lin_obs per
// LM iteration.
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

#include "ba_block_lm.h"

namespace miba {

namespace {

// the pass's sums: Jp^T Jp upper-packed (6) | Jp^T f (3) | cost | failed evaluations
constexpr int PTS_NS = 11;
constexpr int P_G = 6, P_COST = 9, P_BAD = 10;

// (the gradient max-norm then is ||x - (x + -g)||_inf, as point_tail (ba_common.h) forms it)
struct AddRetract {
    static __device__ __forceinline__ void plus(const double (&x)[3], const double (&d)[3], double (&out)[3]) {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = x[i] + d[i];
    }
};
using PtsState = BlockLmState<3, 3>;  // a row's LM state of one point, the same bits in each of its lanes

struct PtsObs {
    double u, v, d, pose[7];
};

__device__ __forceinline__ PtsObs pts_load(const PtsArgs& a, int o) {
    const int k = a.idx[o];
    const double2 uv = a.uv[k];
    const double* T = a.cams + 7 * (size_t)a.obs_cam[k];
    return PtsObs{uv.x, uv.y, a.depth[k], {T[0], T[1], T[2], T[3], T[4], T[5], T[6]}};
}

// One pass over the point's observations at X; sum valid in every lane of the row after it. Called in wave-uniform
// control flow (the DPP sums); a row that is not `on` takes no observation.
__device__ __forceinline__ void pts_pass(const PtsArgs& a, const BaConsts& c, const BlockRec& w, const double K[4],
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

// the pass's sums as the linearisation at S.x (block_lm_absorb's load)
__device__ __forceinline__ auto pts_load_sums(const double (&sum)[PTS_NS]) {
    return [&sum](PtsState& S) {
#pragma unroll
        for (int q = 0; q < 6; ++q) S.H[q] = sum[q];
#pragma unroll
        for (int i = 0; i < 3; ++i) S.g[i] = sum[P_G + i];
        S.x_cost = sum[P_COST];
    };
}

__global__ __launch_bounds__(PTS_TPB) void k_pts_lm(PtsArgs a, BaConsts c, LmParams prm) {
    const int tid = threadIdx.x;
    const int j = tid & (PTS_LANES - 1);
    const size_t rec = (size_t)blockIdx.x * PTS_PER_WG + (size_t)(tid / PTS_LANES);
    const bool valid = rec < (size_t)a.n_rec;  // (the last workgroup's rows past the records idle through the loop)
    BlockRec w = BlockRec{0, 0, 0, 0, 0.0, 0.0};
    if (valid) w = a.rec[rec];
    c.sw_r = w.sw_r;
    c.sw_d = w.sw_d;
    const double K[4] = {a.K[0], a.K[1], a.K[2], a.K[3]};
    PtsObs first = PtsObs{0.0, 0.0, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    if (valid && w.begin + j < w.end) first = pts_load(a, w.begin + j);
    const BlockLmLog lg{a.log, a.log_max_rows, valid && j == 0 && a.log_rec >= 0 && rec == (size_t)a.log_rec};

    double xc[3];  // the position the next pass evaluates (the candidate)
#pragma unroll
    for (int i = 0; i < 3; ++i) xc[i] = valid ? a.pts[3 * (size_t)w.id + i] : 0.0;
    PtsState S;
    block_lm_init(S, xc, a.initial_radius);

    double sum[PTS_NS];
    pts_pass(a, c, w, K, first, xc, j, valid, sum);  // iteration 0: the pass at the given position
    bool active = false;
    if (valid) {
        block_lm_absorb<AddRetract>(S, pts_load_sums(sum));
        active = block_lm_first(S, sum[P_BAD] > 0.0, a.jacobi_scaling, lg) &&
                 block_lm_next_step<AddRetract>(S, xc, c, prm, lg);
    }
    while (__ballot(active) != 0ull) {  // wave-uniform: all 64 lanes make the pass while any row is active
        pts_pass(a, c, w, K, first, xc, j, active, sum);
        if (active)
            active = !block_lm_decide<AddRetract>(S, xc, sum[P_COST], sum[P_BAD] > 0.0, prm, lg, pts_load_sums(sum)) &&
                     block_lm_next_step<AddRetract>(S, xc, c, prm, lg);
    }
    if (valid && j == 0) {
        block_lm_write_stats(S, w.end - w.begin, a.stats + rec * PTS_STAT);
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
