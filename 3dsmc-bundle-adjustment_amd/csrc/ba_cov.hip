// ba_cov.hip — covariance of the estimate (ba_covariance): the dense inverse of the undamped, Jacobi-scaled
// reduced camera system on the f64 matrix cores, and the points' marginal covariances from it.
//
//   k_cov_copy      work matrix A <- lower triangle of W.S, padded to a multiple of 64 with an identity diagonal
//   per 64-column block k (the host loops and enqueues; every dependency between workgroups is a launch boundary):
//     k_cov_diag    one workgroup: A_kk = L_kk L_kk^T in LDS, pivot extrema, Z_kk = L_kk^-1
//     k_cov_panel   L_ik = A_ik L_kk^-T (i > k)   and   Z_kj = L_kk^-1 B_kj (j < k)
//     k_cov_trail   A_ij -= L_ik L_jk^T (i >= j > k)   and   B_ij -= L_ik Z_kj (i > k >= j)
//                   (B starts as the identity: the right-looking solve of L Z = I rides along the factorisation,
//                   so Z = L^-1 is complete after the last column)
//   k_cov_ztz       A_ij <- sum_m Z_mi^T Z_mj (lower blocks): the inverse of the scaled system
//   k_cov_unscale   Cv <- s_i s_j A_ij, both triangles (Cv overwrites Z)
//   k_cov_pairs     the requested 6x6 / 6x4 / 4x4 blocks
//   k_cov_points    one thread per requested point: V^-1 + V^-1 E^T Cv[cols, cols] E V^-1
// The tile products (panel, trail, ztz) run on v_mfma_f64_16x16x4_f64: a wave owns a 32x32 quad of a 64x64 block.
// Every kernel but the copy (which resets the status) checks the device failure flag first and exits on it.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ba_common.h"
#include "ba_cov.h"
#include "ba_device.h"
#include "ba_kernels.h"
#include "ba_tail.h"
#include "ba_tile64.h"

namespace miba {

namespace {

constexpr int CB = COV_B;
constexpr int CTPB = 256;    // 4 waves: one 32x32 quad each
constexpr int CLD = CB + 1;  // LDS row stride of a staged block

__device__ __forceinline__ bool cov_rank_bad(const CovStat* st, double rcond) {
    return st->flag != 0 || !(st->pmin / st->pmax >= rcond);
}

__global__ __launch_bounds__(CTPB) void k_cov_copy(const double* __restrict__ S, int lds, int n, double* __restrict__ A,
                                                   int ld, CovStat* __restrict__ stat) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stat->flag = 0;
        stat->pad = 0;
        stat->pmin = INFINITY;
        stat->pmax = 0.0;
    }
    const size_t total = (size_t)ld * ld;
    for (size_t e = (size_t)blockIdx.x * CTPB + threadIdx.x; e < total; e += (size_t)gridDim.x * CTPB) {
        const int i = (int)(e / ld), j = (int)(e % ld);
        double v = i == j ? 1.0 : 0.0;
        if (i < n && j <= i) v = S[(size_t)i * lds + j];
        A[e] = v;
    }
}

// One workgroup: the diagonal block's Cholesky factor (into A_kk) and its inverse (into Z_kk, zeros above the
// diagonal) in one elimination (tile_chol_inv, ba_tile64.h). Pivots of the padded rows (>= n, exactly 1) do not count
// for the extrema; a failing pivot does (the extrema are taken before it is judged).
__global__ __launch_bounds__(CTPB) void k_cov_diag(double* __restrict__ A, double* __restrict__ Zm, int ld, int k, int n,
                                                   CovStat* __restrict__ stat) {
    if (stat->flag) return;
    __shared__ double Ls[CB * CLD];
    __shared__ double Xs[CB * (CB + 1) / 2];  // L^-1, lower triangle packed by rows
    __shared__ double Dg[CB];                 // diag(L)
    const int tid = threadIdx.x;
    double* Akk = A + ((size_t)k * CB) * ld + (size_t)k * CB;
    double* Zkk = Zm + ((size_t)k * CB) * ld + (size_t)k * CB;
    for (int e = tid; e < CB * CB; e += CTPB) {
        const int i = e / CB, j = e % CB;
        Ls[i * CLD + j] = j <= i ? Akk[(size_t)i * ld + j] : 0.0;
    }
    for (int e = tid; e < CB * (CB + 1) / 2; e += CTPB) Xs[e] = 0.0;
    double pmin = stat->pmin, pmax = stat->pmax;
    __syncthreads();
    const bool bad = tile_chol_inv<CTPB, CLD, true>(Ls, Xs, Dg, [&](int j, double d) __attribute__((always_inline)) {
        if (k * CB + j < n) { pmin = fmin(pmin, d); pmax = fmax(pmax, d); }
    });
    if (bad) {
        if (tid == 0) {
            stat->flag = 1;
            // a non-finite pivot does not pass through fmin / fmax: report the failure in the extrema too
            stat->pmin = fmin(pmin, 0.0);
            stat->pmax = pmax;
        }
        return;
    }
    for (int e = tid; e < CB * CB; e += CTPB) {
        const int i = e / CB, j = e % CB;
        Akk[(size_t)i * ld + j] = j < i ? Ls[i * CLD + j] : (j == i ? Dg[i] : 0.0);
        Zkk[(size_t)i * ld + j] = j <= i ? Xs[i * (i + 1) / 2 + j] : 0.0;
    }
    if (tid == 0) { stat->pmin = pmin; stat->pmax = pmax; }
}

// Workgroups [0, nblk - 1 - k): L_ik = A_ik Z_kk^T for i = k + 1 + b, in place through an LDS copy of A_ik;
// the next k workgroups: Z_kj = Z_kk B_kj for j = b - (nblk - 1 - k), in place through an LDS copy of B_kj.
__global__ __launch_bounds__(CTPB) void k_cov_panel(double* __restrict__ A, double* __restrict__ Zm, int ld, int nblk,
                                                    int k, const CovStat* __restrict__ stat) {
    if (stat->flag) return;
    __shared__ double T[CB * CLD];
    const int tid = threadIdx.x, wave = tid >> 6, qi = wave >> 1, qj = wave & 1;
    const int nl = nblk - 1 - k, b = blockIdx.x;
    const double* Zkk = Zm + ((size_t)k * CB) * ld + (size_t)k * CB;
    double* X = b < nl ? A + ((size_t)(k + 1 + b) * CB) * ld + (size_t)k * CB
                       : Zm + ((size_t)k * CB) * ld + (size_t)(b - nl) * CB;
    for (int e = tid; e < CB * CB; e += CTPB) T[(e / CB) * CLD + e % CB] = X[(size_t)(e / CB) * ld + e % CB];
    __syncthreads();
    d4 acc[2][2] = {};
    if (b < nl)  // C(i, j) = sum_m T(i, m) Zkk(j, m)
        tile_mma(acc, T + 32 * qi * CLD, CLD, 1, Zkk + (size_t)(32 * qj) * ld, ld, 1, CB);
    else  // C(i, j) = sum_m Zkk(i, m) T(m, j)
        tile_mma(acc, Zkk + (size_t)(32 * qi) * ld, ld, 1, T + 32 * qj, 1, CLD, CB);
    tile_store<TILE_SET>(acc, X, ld, qi, qj);
}

// Workgroup (x = j, y = i - (k + 1)), j <= i: j > k: A_ij -= L_ik L_jk^T; j <= k: B_ij -= L_ik Z_kj.
__global__ __launch_bounds__(CTPB) void k_cov_trail(double* __restrict__ A, double* __restrict__ Zm, int ld, int k,
                                                    const CovStat* __restrict__ stat) {
    if (stat->flag) return;
    const int j = blockIdx.x, i = k + 1 + blockIdx.y;
    if (j > i) return;
    const int wave = threadIdx.x >> 6, qi = wave >> 1, qj = wave & 1;
    const double* Lik = A + ((size_t)i * CB + 32 * qi) * ld + (size_t)k * CB;
    d4 acc[2][2] = {};
    if (j > k) {
        const double* Ljk = A + ((size_t)j * CB + 32 * qj) * ld + (size_t)k * CB;
        tile_mma(acc, Lik, ld, 1, Ljk, ld, 1, CB);
        tile_store<TILE_SUB>(acc, A + ((size_t)i * CB) * ld + (size_t)j * CB, ld, qi, qj);
    } else {
        const double* Zkj = Zm + ((size_t)k * CB) * ld + (size_t)j * CB + 32 * qj;
        tile_mma(acc, Lik, ld, 1, Zkj, 1, ld, CB);
        tile_store<TILE_SUB>(acc, Zm + ((size_t)i * CB) * ld + (size_t)j * CB, ld, qi, qj);
    }
}

// Workgroup (x = j, y = i), j <= i: A_ij = sum over the rows r >= 64 i of Z(r, block i)^T Z(r, block j)
// (Z is lower triangular with explicit zeros inside its diagonal blocks).
__global__ __launch_bounds__(CTPB) void k_cov_ztz(double* __restrict__ A, const double* __restrict__ Zm, int ld, int nblk,
                                                  double rcond, const CovStat* __restrict__ stat) {
    if (cov_rank_bad(stat, rcond)) return;
    const int j = blockIdx.x, i = blockIdx.y;
    if (j > i) return;
    const int wave = threadIdx.x >> 6, qi = wave >> 1, qj = wave & 1;
    const double* Zi = Zm + ((size_t)i * CB) * ld + (size_t)i * CB + 32 * qi;
    const double* Zj = Zm + ((size_t)i * CB) * ld + (size_t)j * CB + 32 * qj;
    d4 acc[2][2] = {};
    tile_mma(acc, Zi, 1, ld, Zj, 1, ld, (nblk - i) * CB);
    tile_store<TILE_SET>(acc, A + ((size_t)i * CB) * ld + (size_t)j * CB, ld, qi, qj);
}

// Cv(i, j) = Cv(j, i) = s_hi * A(hi, lo) * s_lo for i, j < n (the same expression on both sides of the diagonal)
__global__ __launch_bounds__(CTPB) void k_cov_unscale(const double* __restrict__ A, double* __restrict__ Cv, int ld, int n,
                                                      const double* __restrict__ scale, int kb, int off_k, double rcond,
                                                      const CovStat* __restrict__ stat) {
    if (cov_rank_bad(stat, rcond)) return;
    const size_t total = (size_t)n * n;
    for (size_t e = (size_t)blockIdx.x * CTPB + threadIdx.x; e < total; e += (size_t)gridDim.x * CTPB) {
        const int i = (int)(e / n), j = (int)(e % n);
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        const double sh = scale[hi < kb ? hi : off_k + (hi - kb)], sl = scale[lo < kb ? lo : off_k + (lo - kb)];
        Cv[(size_t)i * ld + j] = (sh * A[(size_t)hi * ld + lo]) * sl;
    }
}

__global__ __launch_bounds__(CTPB) void k_cov_pairs(const double* __restrict__ Cv, int ld, int kb,
                                                    const int* __restrict__ ia, const int* __restrict__ ib, int n_pairs,
                                                    double* __restrict__ out, double rcond,
                                                    const CovStat* __restrict__ stat) {
    if (cov_rank_bad(stat, rcond)) return;
    const int t = blockIdx.x * CTPB + threadIdx.x;
    if (t >= 36 * n_pairs) return;
    const int p = t / 36, e = t % 36;
    const int a = ia[p], b = ib[p];
    const int da = a == COV_PAIR_INTR ? 4 : 6, db = b == COV_PAIR_INTR ? 4 : 6;
    double v = 0.0;
    if (e < da * db) {
        if (a == COV_PAIR_NAN || b == COV_PAIR_NAN) v = __builtin_nan("");
        else if (a != COV_PAIR_ZERO && b != COV_PAIR_ZERO) {
            const int r = (a >= 0 ? 6 * a : kb) + e / db, c = (b >= 0 ? 6 * b : kb) + e % db;
            v = Cv[(size_t)r * ld + c];
        }
    }
    out[t] = v;
}

// One thread per requested point. Pass 1 over the point's observations (lin_obs, as the back-substitution does):
// V = sum Jp^T Jp, K = sum Jk^T Jp (4x3), and W_o = Jc^T Jp (6x3) of every observation of an active camera into
// wbuf (18 doubles per observation: any track length). Pass 2: M = E^T Cv[cols, cols] E over the pairs of those
// observations and the intrinsics rows, E = [W ; K] (two observations of one camera add up, as E's rows do).
template <bool O32>
__global__ __launch_bounds__(CTPB) void k_cov_points(DevProblem P, BaConsts c, const LmState* __restrict__ st,
                                                     const double* __restrict__ Cv, int ld, const int* __restrict__ apv,
                                                     int n_req, double* __restrict__ wbuf, double* __restrict__ out,
                                                     double rcond, const CovStat* __restrict__ stat) {
    if (cov_rank_bad(stat, rcond)) return;
    const int t = blockIdx.x * CTPB + threadIdx.x;
    if (t >= n_req) return;
    double* o9 = out + 9 * (size_t)t;
    const int ap = apv[t];
    if (ap < 0) {
        for (int i = 0; i < 9; ++i) o9[i] = __builtin_nan("");
        return;
    }
    const int cur = st->cur;
    const double* X = P.pts[cur] + 3 * P.pt_idx[ap];
    const double* K = P.K[cur];
    const int o0 = P.pt_ptr[ap], o1 = P.pt_ptr[ap + 1];
    double V[6] = {0, 0, 0, 0, 0, 0}, Kt[12];
    for (int i = 0; i < 12; ++i) Kt[i] = 0.0;
    for (int o = o0; o < o1; ++o) {
        const ObsRaw<O32> r = po_obs<O32>(P, o);
        ObsEval ev;
        double jc[18], jp[9], jk[8];
        lin_obs(c, P.cams[cur] + 7 * r.idx(), X, K, r.u(), r.v(), r.d(), ev, jc, jp, jk);
        V[0] += jp[0] * jp[0] + jp[3] * jp[3] + jp[6] * jp[6];
        V[1] += jp[0] * jp[1] + jp[3] * jp[4] + jp[6] * jp[7];
        V[2] += jp[0] * jp[2] + jp[3] * jp[5] + jp[6] * jp[8];
        V[3] += jp[1] * jp[1] + jp[4] * jp[4] + jp[7] * jp[7];
        V[4] += jp[1] * jp[2] + jp[4] * jp[5] + jp[7] * jp[8];
        V[5] += jp[2] * jp[2] + jp[5] * jp[5] + jp[8] * jp[8];
        for (int i = 0; i < 3; ++i) {  // jk row 0 is [k0, 0, su, 0], row 1 [0, k1, 0, su]
            Kt[0 * 3 + i] += jk[0] * jp[i];
            Kt[1 * 3 + i] += jk[5] * jp[3 + i];
            Kt[2 * 3 + i] += jk[2] * jp[i];
            Kt[3 * 3 + i] += jk[7] * jp[3 + i];
        }
        if (P.po_ac[o] >= 0) {
            double* w = wbuf + 18 * (size_t)o;
            for (int d = 0; d < 6; ++d)
                for (int i = 0; i < 3; ++i) w[3 * d + i] = jc[d] * jp[i] + jc[6 + d] * jp[3 + i] + jc[12 + d] * jp[6 + i];
        }
    }
    // V^-1 by Cholesky
    double Vi[9];
    {
        const double l00 = sqrt(V[0]);
        const double l10 = V[1] / l00, l20 = V[2] / l00;
        const double d11 = V[3] - l10 * l10;
        const double l11 = sqrt(d11);
        const double l21 = (V[4] - l20 * l10) / l11;
        const double d22 = V[5] - l20 * l20 - l21 * l21;
        const double l22 = sqrt(d22);
        if (!(V[0] > 0.0 && d11 > 0.0 && d22 > 0.0 && isfinite(d22))) {
            for (int i = 0; i < 9; ++i) o9[i] = __builtin_nan("");
            return;
        }
        // G = L^-1 (lower), V^-1 = G^T G
        const double g00 = 1.0 / l00, g11 = 1.0 / l11, g22 = 1.0 / l22;
        const double g10 = -l10 * g00 * g11;
        const double g21 = -l21 * g11 * g22;
        const double g20 = -(l20 * g00 + l21 * g10) * g22;
        Vi[0] = g00 * g00 + g10 * g10 + g20 * g20;
        Vi[1] = g10 * g11 + g20 * g21;
        Vi[2] = g20 * g22;
        Vi[4] = g11 * g11 + g21 * g21;
        Vi[5] = g21 * g22;
        Vi[8] = g22 * g22;
        Vi[3] = Vi[1]; Vi[6] = Vi[2]; Vi[7] = Vi[5];
    }
    // M = E^T Cv E (the intrinsics rows K ride in the point's 12-double slot behind the observations' W_o)
    double* kt = wbuf + 18 * (size_t)P.n_adm + 12 * (size_t)t;
#pragma unroll
    for (int i = 0; i < 12; ++i) kt[i] = Kt[i];
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = 0.0;
    const int kb = P.kb;
    for (int a = o0; a <= o1; ++a) {  // a == o1: the intrinsics rows
        const bool ak = a == o1;
        const int aca = ak ? 0 : P.po_ac[a];
        if (aca < 0) continue;
        const int ra = ak ? kb : 6 * aca, na = ak ? 4 : 6;
        double y[18];  // rows of Cv[rows_a, cols] E
#pragma unroll
        for (int i = 0; i < 18; ++i) y[i] = 0.0;
        for (int b = o0; b <= o1; ++b) {
            const bool bk = b == o1;
            const int acb = bk ? 0 : P.po_ac[b];
            if (acb < 0) continue;
            const int rb = bk ? kb : 6 * acb, nb = bk ? 4 : 6;
            const double* Eb = bk ? kt : wbuf + 18 * (size_t)b;
            for (int q = 0; q < nb; ++q) {
                const double e0 = Eb[3 * q], e1 = Eb[3 * q + 1], e2 = Eb[3 * q + 2];
#pragma unroll
                for (int p = 0; p < 6; ++p)
                    if (p < na) {
                        const double s = Cv[(size_t)(ra + p) * ld + rb + q];
                        y[3 * p] += s * e0; y[3 * p + 1] += s * e1; y[3 * p + 2] += s * e2;
                    }
            }
        }
        const double* Ea = ak ? kt : wbuf + 18 * (size_t)a;
#pragma unroll
        for (int p = 0; p < 6; ++p)
            if (p < na) {
                const double a0 = Ea[3 * p], a1 = Ea[3 * p + 1], a2 = Ea[3 * p + 2];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    M[j] += a0 * y[3 * p + j];
                    M[3 + j] += a1 * y[3 * p + j];
                    M[6 + j] += a2 * y[3 * p + j];
                }
            }
    }
    // Vi + Vi M Vi, symmetrised
    double MV[9], R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) MV[3 * i + j] = M[3 * i] * Vi[j] + M[3 * i + 1] * Vi[3 + j] + M[3 * i + 2] * Vi[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = Vi[3 * i + j] + (Vi[3 * i] * MV[j] + Vi[3 * i + 1] * MV[3 + j] + Vi[3 * i + 2] * MV[6 + j]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o9[3 * i + j] = 0.5 * (R[3 * i + j] + R[3 * j + i]);
}

inline int cov_grid(size_t total) { return (int)std::min<size_t>((total + CTPB - 1) / CTPB, 8192); }

}  // namespace

hipError_t launch_cov_copy(const double* S, int lds, int n, double* A, int ld, CovStat* stat, hipStream_t s) {
    hipLaunchKernelGGL(k_cov_copy, dim3(cov_grid((size_t)ld * ld)), dim3(CTPB), 0, s, S, lds, n, A, ld, stat);
    return hipGetLastError();
}

hipError_t launch_cov_column(double* A, double* Zm, int ld, int nblk, int k, int n, CovStat* stat, hipStream_t s) {
    hipLaunchKernelGGL(k_cov_diag, dim3(1), dim3(CTPB), 0, s, A, Zm, ld, k, n, stat);
    if (nblk - 1 > 0)  // (nblk - 1 - k) panel blocks of L + k row blocks of Z
        hipLaunchKernelGGL(k_cov_panel, dim3(nblk - 1), dim3(CTPB), 0, s, A, Zm, ld, nblk, k, stat);
    if (nblk - 1 - k > 0)
        hipLaunchKernelGGL(k_cov_trail, dim3(nblk, nblk - 1 - k), dim3(CTPB), 0, s, A, Zm, ld, k, stat);
    return hipGetLastError();
}

hipError_t launch_cov_finish(double* A, double* Zm, int ld, int nblk, int n, const double* scale, int kb, int off_k,
                             double rcond, CovStat* stat, hipStream_t s) {
    hipLaunchKernelGGL(k_cov_ztz, dim3(nblk, nblk), dim3(CTPB), 0, s, A, Zm, ld, nblk, rcond, stat);
    hipLaunchKernelGGL(k_cov_unscale, dim3(cov_grid((size_t)n * n)), dim3(CTPB), 0, s, A, Zm, ld, n, scale, kb, off_k,
                       rcond, stat);
    return hipGetLastError();
}

hipError_t launch_cov_pairs(const double* Cv, int ld, int kb, const int* ia, const int* ib, int n_pairs, double* out,
                            double rcond, const CovStat* stat, hipStream_t s) {
    if (n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_cov_pairs, dim3((36 * n_pairs + CTPB - 1) / CTPB), dim3(CTPB), 0, s, Cv, ld, kb, ia, ib, n_pairs,
                       out, rcond, stat);
    return hipGetLastError();
}

hipError_t launch_cov_points(const DevProblem& P, const BaConsts& c, const LmState* st, const double* Cv, int ld,
                             const int* ap, int n_req, double* wbuf, double* out, double rcond, const CovStat* stat,
                             hipStream_t s) {
    if (n_req <= 0) return hipSuccess;
    const dim3 g((n_req + CTPB - 1) / CTPB), b(CTPB);
    if (P.obs32) hipLaunchKernelGGL(k_cov_points<true>, g, b, 0, s, P, c, st, Cv, ld, ap, n_req, wbuf, out, rcond, stat);
    else hipLaunchKernelGGL(k_cov_points<false>, g, b, 0, s, P, c, st, Cv, ld, ap, n_req, wbuf, out, rcond, stat);
    return hipGetLastError();
}

}  // namespace miba
