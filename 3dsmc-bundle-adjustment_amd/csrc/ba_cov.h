// ba_cov.h — launchers of the covariance kernels (ba_cov.hip, internal).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_kernels.h"

namespace miba {

// block size of the dense inverse: the blocked Cholesky's (ba_dense.h), the two share the tile kit of ba_tile64.h
static constexpr int COV_B = DENSE_B;
inline int cov_nblk(int n) { return (n + COV_B - 1) / COV_B; }

// Device status of one ba_covariance call: flag != 0 once a pivot was <= 0 or not finite (every later launch
// exits on it); pmin / pmax the smallest / largest squared Cholesky diagonal of the real (unpadded) rows.
struct CovStat {
    int flag, pad;
    double pmin, pmax;
};

// pair codes of launch_cov_pairs (an active camera index is >= 0)
static constexpr int COV_PAIR_INTR = -1;  // the intrinsics block
static constexpr int COV_PAIR_ZERO = -2;  // the gauge camera: a constant block
static constexpr int COV_PAIR_NAN = -3;   // a camera without an admissible observation

// A <- lower triangle of S (n rows, leading dimension lds) padded to ld = 64 * nblk with an identity diagonal,
// zero elsewhere; *stat reset.
hipError_t launch_cov_copy(const double* S, int lds, int n, double* A, int ld, CovStat* stat, hipStream_t s);
// Block column k of the blocked Cholesky A = L L^T with Z = L^-1 carried along in Zm (lower blocks zero and the
// diagonal blocks unwritten on entry): three launches.
hipError_t launch_cov_column(double* A, double* Zm, int ld, int nblk, int k, int n, CovStat* stat, hipStream_t s);
// A (lower blocks) <- Z^T Z, then Zm (n x n, both triangles) <- s_i s_j A_ij; rcond: the pivot-ratio threshold
hipError_t launch_cov_finish(double* A, double* Zm, int ld, int nblk, int n, const double* scale, int kb, int off_k,
                             double rcond, CovStat* stat, hipStream_t s);
// out[36 k ..] <- block (ia[k], ib[k]) of the unscaled inverse Cv (leading dimension ld), zero / NaN rules applied
hipError_t launch_cov_pairs(const double* Cv, int ld, int kb, const int* ia, const int* ib, int n_pairs, double* out,
                            double rcond, const CovStat* stat, hipStream_t s);
// out[9 k ..] <- marginal covariance of active point ap[k] (ap[k] < 0: NaN); wbuf: 18 doubles per admissible
// observation, then 12 per requested point
inline size_t cov_wbuf_doubles(int n_adm, int n_req) { return 18 * (size_t)n_adm + 12 * (size_t)n_req; }
hipError_t launch_cov_points(const DevProblem& P, const BaConsts& c, const LmState* st, const double* Cv, int ld,
                             const int* ap, int n_req, double* wbuf, double* out, double rcond, const CovStat* stat,
                             hipStream_t s);

}  // namespace miba
