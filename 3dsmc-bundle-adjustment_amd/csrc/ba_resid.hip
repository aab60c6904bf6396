// ba_resid.hip — the residual report (ba_residuals): per-observation errors in physical units, flags and cost
// shares, statistics per point and per camera, window totals.
//
//   k_res_obs      one thread per point-major slot: obs_project / obs_residual / huber of ba_device.h, as the
//                  solver's candidate evaluation runs them -> errors, cost share, flags in slot order
//   k_res_scatter  one thread per observation of the caller: its slot's values through po_dest (NaN and
//                  BA_RES_INADMISSIBLE where the solver skips the observation)
//   k_res_point    eight lanes per active point over its pt_ptr range, each lane every eighth observation in
//                  order, the lanes combined by xor shuffles
//   k_res_seg      one workgroup per camera-major sub-segment, evaluating the co_* records again
//   k_res_cam      one workgroup: each camera's sub-segments in order, then the window totals in camera order
//
// No floating-point atomic anywhere: every sum has one fixed order (given the window's sub-segments), so the report
// is bitwise reproducible.
#include "../../include/ba.h"
#include "ba_resid.h"
#include "ba_tail.h"

namespace miba {

namespace {

static constexpr int RES_PT_LANES = 8;  // lanes per active point of k_res_point

struct ResObs {
    double du, dv, dd, z, cost;
    int flags;
};

// What the statistics add per observation, from the reported errors: one spelling for every kernel, no contraction
// (a caller reproduces them from obs_err with IEEE multiply, add and square root).
__device__ __forceinline__ void res_terms(double du, double dv, double dd, double& s2, double& hyp, double& dd2) {
#pragma clang fp contract(off)
    s2 = du * du + dv * dv;
    hyp = sqrt(s2);
    dd2 = dd * dd;
}

__device__ __forceinline__ void res_eval(const BaConsts& c, const ResThresholds& t, const double* __restrict__ pose,
                                         const double* __restrict__ X, const double* __restrict__ K, double uo,
                                         double vo, double depth, ResObs& o) {
#pragma clang fp contract(off)
    double R[9], x, y, z, iz, u, v, r0, r1, r2, s_uv;
    obs_project(pose, X, K, R, x, y, z, iz, u, v);
    obs_residual(c, u, v, z, uo, vo, depth, r0, r1, r2, s_uv);
    const double s_d = r2 * r2;
    double rr, gr, rd, gd;
    huber(s_uv, c.a_r, c.b_r, rr, gr);
    huber(s_d, c.a_d, c.b_d, rd, gd);
    o.cost = 0.5 * rr + 0.5 * rd;
    o.du = u - uo;
    o.dv = v - vo;
    o.dd = depth - z;
    o.z = z;
    double s2, hyp, dd2;
    res_terms(o.du, o.dv, o.dd, s2, hyp, dd2);
    int f = 0;
    if (!(z > 0.0) || !isfinite(u) || !isfinite(v)) f |= BA_RES_BEHIND;
    if (t.reproj_on && hyp > t.max_reproj) f |= BA_RES_REPROJ;
    if (t.depth_on && fabs(o.dd) > t.depth_abs + t.depth_rel * depth) f |= BA_RES_DEPTH;
    if (s_uv > c.b_r) f |= BA_RES_HUBER_REPR;
    if (s_d > c.b_d) f |= BA_RES_HUBER_UNPR;
    o.flags = f;
}

// One admissible observation into a partial: a[0 .. 10) the sums (RES_PART_N order without the two maxima:
// 0 1 2 4 5 6 7 8 9 10), mh / md the maxima.
__device__ __forceinline__ void res_accum(double (&a)[10], double& mh, double& md, double du, double dv, double dd,
                                          double cost, int f) {
    a[0] += 1.0;
    a[1] += (f & BA_RES_OUTLIER) ? 1.0 : 0.0;
    if (!(f & BA_RES_BEHIND)) {
        double s2, hyp, dd2;
        res_terms(du, dv, dd, s2, hyp, dd2);
        a[2] += s2;
        a[3] += dd2;
        mh = fmax(mh, hyp);
        md = fmax(md, fabs(dd));
    }
    a[4] += cost;
    a[5] += (f & BA_RES_BEHIND) ? 1.0 : 0.0;
    a[6] += (f & BA_RES_REPROJ) ? 1.0 : 0.0;
    a[7] += (f & BA_RES_DEPTH) ? 1.0 : 0.0;
    a[8] += (f & BA_RES_HUBER_REPR) ? 1.0 : 0.0;
    a[9] += (f & BA_RES_HUBER_UNPR) ? 1.0 : 0.0;
}
// sums a[k] -> RES_PART_N slot
__device__ __forceinline__ int res_sum_slot(int k) { return k < 3 ? k : (k == 3 ? 4 : k + 1); }

template <bool O32>
__global__ __launch_bounds__(TPB) void k_res_obs(DevProblem P, BaConsts c, ResThresholds t, double* __restrict__ err,
                                                 double* __restrict__ cost, int* __restrict__ flags) {
    const int q = blockIdx.x * TPB + threadIdx.x;
    if (q >= P.n_adm) return;
    const ObsRaw<O32> o = po_obs<O32>(P, q);
    ResObs r;
    res_eval(c, t, P.cams[0] + 7 * (size_t)o.idx(), P.pts[0] + 3 * (size_t)P.po_pt[q], P.K[0], o.u(), o.v(), o.d(), r);
    reinterpret_cast<double4*>(err)[q] = double4{r.du, r.dv, r.dd, r.z};
    cost[q] = r.cost;
    flags[q] = r.flags;
}

__global__ __launch_bounds__(TPB) void k_res_scatter(const int* __restrict__ po_dest, int n_obs,
                                                     const double* __restrict__ po_err,
                                                     const double* __restrict__ po_cost,
                                                     const int* __restrict__ po_flags, double* __restrict__ err,
                                                     double* __restrict__ cost, int* __restrict__ flags) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= n_obs) return;
    const int q = po_dest[k];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double4 e = double4{nan, nan, nan, nan};
    double cs = nan;
    int f = BA_RES_INADMISSIBLE;
    if (q >= 0) {
        e = reinterpret_cast<const double4*>(po_err)[q];
        cs = po_cost[q];
        f = po_flags[q];
    }
    reinterpret_cast<double4*>(err)[k] = e;
    cost[k] = cs;
    flags[k] = f;
}

__global__ __launch_bounds__(TPB) void k_res_point(DevProblem P, const double* __restrict__ po_err,
                                                   const double* __restrict__ po_cost,
                                                   const int* __restrict__ po_flags, double* __restrict__ point_stats) {
    const int g = (blockIdx.x * TPB + threadIdx.x) / RES_PT_LANES, l = threadIdx.x & (RES_PT_LANES - 1);
    const bool live = g < P.n_ap;  // (every lane takes part in the shuffles)
    double a[10], mh = 0.0, md = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) a[i] = 0.0;
    if (live) {
        const int q1 = P.pt_ptr[g + 1];
        for (int q = P.pt_ptr[g] + l; q < q1; q += RES_PT_LANES) {
            const double4 e = reinterpret_cast<const double4*>(po_err)[q];
            res_accum(a, mh, md, e.x, e.y, e.z, po_cost[q], po_flags[q]);
        }
    }
#pragma unroll
    for (int off = RES_PT_LANES / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 5; ++i) a[i] += __shfl_xor(a[i], off);
        mh = fmax(mh, __shfl_xor(mh, off));
    }
    if (live && l == 0) {
        double* out = point_stats + BA_RES_STAT_N * (size_t)P.pt_idx[g];
        out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = mh; out[4] = a[3]; out[5] = a[4];
    }
}

template <bool O32>
__global__ __launch_bounds__(TPB) void k_res_seg(DevProblem P, BaConsts c, ResThresholds t,
                                                 double* __restrict__ seg_part) {
    __shared__ double lds[4 * 10], out[10];
    const int sg = blockIdx.x;
    const int q0 = P.seg_ptr[sg], q1 = P.seg_ptr[sg + 1];
    const double* pose = P.cams[0] + 7 * (size_t)P.seg_cam[sg];
    double a[10], mh = 0.0, md = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) a[i] = 0.0;
    for (int q = q0 + (int)threadIdx.x; q < q1; q += TPB) {
        const ObsRaw<O32> o = co_obs<O32>(P, q);
        ResObs r;
        res_eval(c, t, pose, P.pts[0] + 3 * (size_t)o.idx(), P.K[0], o.u(), o.v(), o.d(), r);
        res_accum(a, mh, md, r.du, r.dv, r.dd, r.cost, r.flags);
    }
    block_sum<10>(a, lds, out);
    mh = block_max(mh, lds);
    md = block_max(md, lds);
    double* dst = seg_part + RES_PART_N * (size_t)sg;
    if (threadIdx.x < 10) dst[res_sum_slot(threadIdx.x)] = out[threadIdx.x];
    if (threadIdx.x == 0) { dst[3] = mh; dst[11] = md; }
}

// slot 3 and slot 11 are maxima, the others sums
__device__ __forceinline__ double res_combine(int slot, double a, double b) {
    return (slot == 3 || slot == 11) ? fmax(a, b) : a + b;
}

// The cameras in rounds of TPB: a thread per camera sums its sub-segments in order into LDS (row stride 13 doubles:
// the column reads below hit distinct banks), then thread i < 12 adds the round's cameras to total i in camera
// order. (The totals read from global memory instead, one dependent load per camera, took 48 us of C4's call and
// 341 us of C5's.)
__global__ __launch_bounds__(TPB) void k_res_cam(DevProblem P, BaConsts c, const double* __restrict__ seg_part,
                                                 double* __restrict__ cam_stats, double* __restrict__ totals) {
    __shared__ double sh[TPB * (RES_PART_N + 1)];
    double v = 0.0;
    for (int base = 0; base < P.n_cams; base += TPB) {
        const int cam = base + (int)threadIdx.x;
        if (cam < P.n_cams) {
            int lo = 0, hi = P.n_seg;  // the camera's first sub-segment (seg_cam is non-decreasing)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (P.seg_cam[mid] < cam) lo = mid + 1; else hi = mid;
            }
            double a[RES_PART_N];
#pragma unroll
            for (int i = 0; i < RES_PART_N; ++i) a[i] = 0.0;
            for (int sg = lo; sg < P.n_seg && P.seg_cam[sg] == cam; ++sg)
#pragma unroll
                for (int i = 0; i < RES_PART_N; ++i) a[i] = res_combine(i, a[i], seg_part[RES_PART_N * (size_t)sg + i]);
#pragma unroll
            for (int i = 0; i < RES_PART_N; ++i) sh[threadIdx.x * (RES_PART_N + 1) + i] = a[i];
#pragma unroll
            for (int i = 0; i < BA_RES_STAT_N; ++i) cam_stats[BA_RES_STAT_N * (size_t)cam + i] = a[i];
        }
        __syncthreads();
        if (threadIdx.x < RES_PART_N) {
            const int n = min(TPB, P.n_cams - base);
#pragma unroll 8
            for (int k = 0; k < n; ++k) v = res_combine(threadIdx.x, v, sh[k * (RES_PART_N + 1) + threadIdx.x]);
        }
        __syncthreads();
    }
    if (threadIdx.x < RES_PART_N) {
        totals[threadIdx.x] = v;
    } else if (threadIdx.x == RES_TOT_PRIOR) {  // the IntrinsicsPrior block (intr_lin's order)
        double pc = 0.0;
        for (int m = 0; m < 4; ++m) {
            const double fk = c.sw_k * (P.prior[m] - P.K[0][m]);
            pc += fk * fk;
        }
        totals[RES_TOT_PRIOR] = 0.5 * pc;
    } else if (threadIdx.x < RES_TOTALS_N) {
        totals[threadIdx.x] = 0.0;
    }
}

static inline int nblocks(size_t n, int t) { return (int)((n + t - 1) / t); }

}  // namespace

#define CK(x)                            \
    do {                                 \
        hipError_t e_ = (x);             \
        if (e_ != hipSuccess) return e_; \
    } while (0)

hipError_t launch_resid(const DevProblem& P, const BaConsts& c, const PrepRaw& R, int n_points,
                        const ResThresholds& t, const ResBufs& b, hipStream_t s) {
    if (P.n_adm > 0) {
        if (P.obs32) hipLaunchKernelGGL(k_res_obs<true>, dim3(nblocks(P.n_adm, TPB)), dim3(TPB), 0, s, P, c, t, b.po_err, b.po_cost, b.po_flags);
        else hipLaunchKernelGGL(k_res_obs<false>, dim3(nblocks(P.n_adm, TPB)), dim3(TPB), 0, s, P, c, t, b.po_err, b.po_cost, b.po_flags);
        CK(hipGetLastError());
    }
    if (b.obs_err && R.n_obs > 0) {
        hipLaunchKernelGGL(k_res_scatter, dim3(nblocks(R.n_obs, TPB)), dim3(TPB), 0, s, R.po_dest, R.n_obs, b.po_err,
                           b.po_cost, b.po_flags, b.obs_err, b.obs_cost, b.obs_flags);
        CK(hipGetLastError());
    }
    if (b.point_stats && n_points > 0) {
        CK(hipMemsetAsync(b.point_stats, 0, sizeof(double) * BA_RES_STAT_N * (size_t)n_points, s));
        if (P.n_ap > 0) {
            hipLaunchKernelGGL(k_res_point, dim3(nblocks((size_t)P.n_ap * RES_PT_LANES, TPB)), dim3(TPB), 0, s, P,
                               b.po_err, b.po_cost, b.po_flags, b.point_stats);
            CK(hipGetLastError());
        }
    }
    if (P.n_seg > 0) {
        if (P.obs32) hipLaunchKernelGGL(k_res_seg<true>, dim3(P.n_seg), dim3(TPB), 0, s, P, c, t, b.seg_part);
        else hipLaunchKernelGGL(k_res_seg<false>, dim3(P.n_seg), dim3(TPB), 0, s, P, c, t, b.seg_part);
        CK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_res_cam, dim3(1), dim3(TPB), 0, s, P, c, b.seg_part, b.cam_stats, b.totals);
    return hipGetLastError();
}

}  // namespace miba
