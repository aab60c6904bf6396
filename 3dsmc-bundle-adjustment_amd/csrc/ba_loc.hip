// ba_loc.hip — ba_localize's kernel (ba_loc.h): pose-only Levenberg-Marquardt of one camera per workgroup, the whole
// trust-region loop in one launch.
//
// With the points and the intrinsics constant a camera's problem has six parameters, so the "linear solver" is a 6x6
// Cholesky one lane does in registers and the observation pass is all the parallel work there is: the loop is
// ba_block_lm.h's (N = 6, se3_plus), one pass over the camera's observations with lin_obs per LM iteration.
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

#include "ba_block_lm.h"

namespace miba {

namespace {

constexpr int LOC_NW = LOC_TPB / 64;
// the pass's sums: U without U(0,1) (20) | g (6) | cost | failed evaluations
constexpr int LOC_NS = 28;
constexpr int S_G = 20, S_COST = 26, S_BAD = 27;

enum { LOC_STOP = 0, LOC_RUN = 1 };

struct Se3Retract {
    static __device__ __forceinline__ void plus(const double (&x)[7], const double (&d)[6], double (&out)[7]) {
        se3_plus(x, d, out);
    }
};
using LocState = BlockLmState<6, 7>;  // thread 0's LM state of one camera

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

// One pass over the camera's observations at L.pose; L.sum valid for every thread after it.
__device__ __forceinline__ void loc_pass(const LocArgs& a, const BaConsts& c, const BlockRec& w, const double K[4],
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

// thread 0: the pass's sums as the linearisation at S.x (block_lm_absorb's load)
__device__ __forceinline__ auto loc_load_sums(const LocLds& L) {
    return [&L](LocState& S) {
#pragma unroll
        for (int q = 0; q < 21; ++q) S.H[q] = q == 0 ? L.sum[0] : (q == 1 ? 0.0 : L.sum[q - 1]);
#pragma unroll
        for (int d = 0; d < 6; ++d) S.g[d] = L.sum[S_G + d];
        S.x_cost = L.sum[S_COST];
    };
}

__global__ __launch_bounds__(LOC_TPB) void k_loc_lm(LocArgs a, BaConsts c, LmParams prm) {
    __shared__ LocLds L;
    const int tid = threadIdx.x;
    const BlockRec w = a.wg[blockIdx.x];
    c.sw_r = w.sw_r;
    c.sw_d = w.sw_d;
    const double K[4] = {a.K[0], a.K[1], a.K[2], a.K[3]};
    LocObs first = LocObs{0.0, 0.0, 0.0, {0.0, 0.0, 0.0}};
    if (w.begin + tid < w.end) first = loc_load(a, w.begin + tid);
    if (tid < 7) L.pose[tid] = a.cams[7 * (size_t)w.id + tid];
    __syncthreads();
    loc_pass(a, c, w, K, first, L);  // iteration 0: the pass at the given pose
    const BlockLmLog lg{a.log, a.log_max_rows, (int)blockIdx.x == a.log_wg};
    LocState& S = L.S;
    if (tid == 0) {
        block_lm_init(S, L.pose, a.initial_radius);
        block_lm_absorb<Se3Retract>(S, loc_load_sums(L));
        L.action = LOC_STOP;
        if (block_lm_first(S, L.sum[S_BAD] > 0.0, a.jacobi_scaling, lg) &&
            block_lm_next_step<Se3Retract>(S, L.pose, c, prm, lg))
            L.action = LOC_RUN;
    }
    __syncthreads();
    while (L.action == LOC_RUN) {  // (workgroup-uniform: written by thread 0 before the barrier above / below)
        loc_pass(a, c, w, K, first, L);
        if (tid == 0) {
            const bool end = block_lm_decide<Se3Retract>(S, L.pose, L.sum[S_COST], L.sum[S_BAD] > 0.0, prm, lg,
                                                         loc_load_sums(L));
            if (end || !block_lm_next_step<Se3Retract>(S, L.pose, c, prm, lg)) L.action = LOC_STOP;
        }
        __syncthreads();
    }
    if (tid == 0) block_lm_write_stats(S, w.end - w.begin, a.stats + (size_t)blockIdx.x * LOC_STAT);
    if (tid < 7) a.cams[7 * (size_t)w.id + tid] = S.x[tid];
}

}  // namespace

hipError_t launch_loc_lm(const LocArgs& a, const BaConsts& c, const LmParams& prm, int n_wg, hipStream_t s) {
    if (n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_loc_lm, dim3((unsigned)n_wg), dim3(LOC_TPB), 0, s, a, c, prm);
    return hipGetLastError();
}

}  // namespace miba
