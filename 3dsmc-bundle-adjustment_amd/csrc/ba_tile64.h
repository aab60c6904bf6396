// ba_tile64.h — the 64x64 f64 tile kit of the two blocked Cholesky factorisations (device code, internal):
// ba_dense.hip (the reduced solve of wide windows) and ba_cov.hip (the dense inverse of ba_covariance). A workgroup's
// wave owns a 32x32 quad of a DENSE_B x DENSE_B block: the quad's product on v_mfma_f64_16x16x4_f64, its store, and
// the one-workgroup elimination of a diagonal block that leaves L and L^-1.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "ba_dense.h"

namespace miba {

typedef double d4 __attribute__((ext_vector_type(4)));

// acc[ti][tj] += sum_k A(16 ti + r, k) B(16 tj + c, k), k in [0, K), K a multiple of 4;
// A(i, k) = A[i * sai + k * sak], B(j, k) = B[j * sbj + k * sbk] (global memory or LDS; constant strides fold).
// f64 MFMA lane map: lane l feeds A(row l & 15, k = l >> 4) and B(col l & 15, k = l >> 4) per k-step of 4, and
// holds the results (row (l >> 4) + 4 g, col l & 15) in element g.
__device__ __forceinline__ void tile_mma(d4 (&acc)[2][2], const double* __restrict__ A, size_t sai, size_t sak,
                                         const double* __restrict__ B, size_t sbj, size_t sbk, int K) {
    const int lane = threadIdx.x & 63, rr = lane & 15, kk = lane >> 4;
    const double* a0 = A + rr * sai + kk * sak;
    const double* a1 = a0 + 16 * sai;
    const double* b0 = B + rr * sbj + kk * sbk;
    const double* b1 = b0 + 16 * sbj;
    const size_t da = 4 * sak, db = 4 * sbk;
    for (int s = 0; s < K; s += 4) {
        const double x0 = *a0, x1 = *a1, y0 = *b0, y1 = *b1;
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, acc[1][1], 0, 0, 0);
        a0 += da; a1 += da; b0 += db; b1 += db;
    }
}

// the wave's quad (qi, qj) of the 64x64 block at C (leading dimension ld): C = acc, or C -= acc
enum TileStore { TILE_SET, TILE_SUB };
template <TileStore MODE>
__device__ __forceinline__ void tile_store(const d4 (&acc)[2][2], double* __restrict__ C, size_t ld, int qi, int qj) {
    const int lane = threadIdx.x & 63, rr = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                double* p = C + (size_t)(32 * qi + 16 * ti + kk + 4 * g) * ld + 32 * qj + 16 * tj + rr;
                if constexpr (MODE == TILE_SUB) *p -= acc[ti][tj][g];
                else *p = acc[ti][tj][g];
            }
}

// One workgroup of NT threads: the Cholesky factor of a diagonal block and its inverse in one elimination: the row
// operations that reduce A to L^T, applied to the identity, leave L^-1 (L^-1 [A | I] = [L^T | L^-1]). On entry Ls
// (LDS, row stride LD) holds the block's lower triangle and Xs (LDS, the lower triangle packed by rows) zeros; the
// caller has put a barrier behind both. Column j: l_ij = a_ij / sqrt(d), row j of X scaled by 1 / sqrt(d); then row
// i > j subtracts l_ij times row j over its i + 1 live entries (NT / 64 threads per row): columns c <= j of X,
// columns j < c <= i of A's lower triangle. Two barriers per column. On return Ls holds L below the diagonal (the
// diagonal still the pivots d_j) and Xs = L^-1; with DIAG, Dg[j] = sqrt(d_j) = diag(L) (else Dg is not used).
// on_pivot(j, d) is called by every thread for every column before the pivot is judged, the failing one included.
// The pivot is read by every thread, so a failure (d <= 0 or not finite) ends the loop uniformly: true is returned.
// (The square root stays behind the pivot test: taken before it, k_cov_diag ran 4 % slower.)
template <int NT, int LD, bool DIAG, class OnPivot>
__device__ __forceinline__ bool tile_chol_inv(double* __restrict__ Ls, double* __restrict__ Xs, double* __restrict__ Dg,
                                              OnPivot on_pivot) {
    constexpr int B = DENSE_B;
    const int tid = threadIdx.x;
    bool bad = false;
    const int ri = tid & (B - 1), cg = tid >> 6;  // elimination: row ri, columns cg, cg + NT / 64, ...
    for (int j = 0; j < B; ++j) {
        const double d = Ls[j * LD + j];  // (not written during the elimination)
        on_pivot(j, d);
        if (!(d > 0.0) || !isfinite(d)) { bad = true; break; }
        const double sd = sqrt(d), inv = 1.0 / sd;
        if (tid < B) {
            if (tid > j) Ls[tid * LD + j] *= inv;
            else if (DIAG && tid == j) Dg[j] = sd;
        } else if (tid < 2 * B) {
            const int c = tid - B;
            if (c < j) Xs[j * (j + 1) / 2 + c] *= inv;
            else if (c == j) Xs[j * (j + 1) / 2 + j] = inv;
        }
        __syncthreads();
        if (ri > j) {
            const double lij = Ls[ri * LD + j];
            for (int c = cg; c <= ri; c += NT / B) {
                if (c <= j) Xs[ri * (ri + 1) / 2 + c] -= lij * Xs[j * (j + 1) / 2 + c];
                else Ls[ri * LD + c] -= lij * Ls[c * LD + j];
            }
        }
        __syncthreads();
    }
    return bad;
}

}  // namespace miba
