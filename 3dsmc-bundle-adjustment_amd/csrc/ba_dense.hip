// ba_dense.hip — the reduced solve of wide co-visibility windows (BA_LS_BLOCKED): a right-looking blocked Cholesky
// over 64-column blocks of the envelope, spread over many workgroups, with the forward solve riding along and a
// backward solve per block column. Every dependency between workgroups is a launch boundary: no flags, no polling,
// no atomics in the arithmetic, a fixed summation order (bitwise reproducible given S and rhs).
//
//   k_dense_copy     A <- the envelope's 64x64 blocks of S (identity on the pad diagonal), bz <- rhs
//   per block column K (launch_dense loops; the same launch list every iteration):
//     k_dense_diag   one workgroup, in LDS: A_KK = L L^T, Z_K = L^-1, z_K = Z_K b_K
//     k_dense_panel  L_IK = A_IK Z_K^T for the block rows I of column K's list
//     k_dense_trail  A_IJ -= L_IK L_JK^T over the list's pairs J <= I, and b_I -= L_IK z_K
//   per block column K, last to first:
//     k_dense_back   one workgroup: y_K = Z_K^T (z_K - sum_I L_IK^T y_I), into bz and rhs
// The tile products run on v_mfma_f64_16x16x4_f64 with both operands staged in LDS (row stride 66 doubles: the
// 16 rows x 2 k-columns a 32-lane half reads fall on 64 distinct banks); a wave owns a 32x32 quad of a block.
// The factor lives in a packed private copy of the envelope (DenseWork::A), so S keeps its invariant — written by
// the assembly only, zero outside the envelope — also when a pivot fails.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ba_dense.h"
#include "ba_kernels.h"
#include "ba_tile64.h"

namespace miba {

namespace {

constexpr int DB = DENSE_B;
constexpr int DTPB = 256;   // 4 waves: one 32x32 quad each
// threads of k_dense_diag: its columns are bound by LDS latency, and 8 waves hide it better than 4 (measured 101 /
// 61 / 58 us per launch with 256 / 512 / 1024 threads)
constexpr int DIAG_TPB = 512;
constexpr int DLD = DB + 2; // LDS row stride of a staged MFMA operand block
constexpr int DLDD = DB + 1;  // LDS row stride of the diagonal block's elimination
constexpr size_t DENSE_LDS2 = sizeof(double) * 2 * DB * DLD;  // two staged blocks (dynamic: above 64 KB)

__device__ __forceinline__ double* dense_blk(const DenseWork& D, int I, int J) {
    return D.A + (size_t)(D.rowstart[I] + J - D.bfcol[I]) * DENSE_BB;
}
__device__ __forceinline__ bool dense_off(const LmState* st, const int* flag) {
    return skip_step(st) || (*flag & FLAG_NOT_PD);
}

// global 64x64 block (row stride 64) -> LDS (row stride DLD)
__device__ __forceinline__ void dense_stage(double* __restrict__ T, const double* __restrict__ X) {
    const double2* X2 = reinterpret_cast<const double2*>(X);  // (blocks are 32 KB apart; DLD is even)
#pragma unroll
    for (int e = threadIdx.x; e < DENSE_BB / 2; e += DTPB)
        *reinterpret_cast<double2*>(T + (e >> 5) * DLD + 2 * (e & 31)) = X2[e];
}

// Workgroups [0, n_env): one envelope block each; the last workgroup: the right-hand side.
__global__ __launch_bounds__(DTPB) void k_dense_copy(const LmState* __restrict__ st, const double* __restrict__ S,
                                                     int npad, const double* __restrict__ rhs, DenseWork D) {
    if (skip_step(st)) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b == D.n_env) {
        for (int i = tid; i < D.nblk * DB; i += DTPB) D.bz[i] = i < npad ? rhs[i] : 0.0;
        return;
    }
    const int2 ij = D.blk[b];
    double* X = dense_blk(D, ij.x, ij.y);
    for (int e = tid; e < DENSE_BB; e += DTPB) {
        const int gi = DB * ij.x + (e >> 6), gj = DB * ij.y + (e & 63);
        double v = gi == gj ? 1.0 : 0.0;
        if (gi < npad && gj < npad) v = S[(size_t)gi * npad + gj];
        X[e] = v;
    }
}

// One workgroup: the diagonal block's Cholesky factor and its inverse in one elimination (tile_chol_inv,
// ba_tile64.h, NT / 64 threads per row). Only Z_K = L^-1 is kept (the panel, the forward and the backward solve all
// multiply by it), and z_K = Z_K b_K.
// (Measured alternatives, DESIGN §4.9: the rows in registers with one hand-off buffer and one barrier per column ran
// 1.5x - 2.5x slower at 256 threads: those variants execute every row's 16 entries under predicates where this
// loop runs the live entries only.)
template <int NT>
__global__ __launch_bounds__(NT) void k_dense_diag(const LmState* __restrict__ st, DenseWork D, int K,
                                                   int* __restrict__ flag) {
    if (dense_off(st, flag)) return;
    __shared__ double Ls[DB * DLDD];
    __shared__ double Xs[DB * (DB + 1) / 2];  // L^-1, lower triangle packed by rows
    __shared__ double bs[DB];
    const int tid = threadIdx.x;
    const double* Akk = dense_blk(D, K, K);
    for (int e = tid; e < DENSE_BB; e += NT) {
        const int i = e >> 6, j = e & 63;
        Ls[i * DLDD + j] = j <= i ? Akk[e] : 0.0;
    }
    for (int e = tid; e < DB * (DB + 1) / 2; e += NT) Xs[e] = 0.0;
    if (tid < DB) bs[tid] = D.bz[DB * K + tid];
    __syncthreads();
    if (tile_chol_inv<NT, DLDD, false>(Ls, Xs, nullptr, [](int, double) {})) {
        if (tid == 0) *flag |= FLAG_NOT_PD;  // (the only writer between the assembly and k_final on this path)
        return;
    }
    double* Zk = D.Zd + (size_t)K * DENSE_BB;
    for (int e = tid; e < DENSE_BB; e += NT) {
        const int i = e >> 6, j = e & 63;
        Zk[e] = j <= i ? Xs[i * (i + 1) / 2 + j] : 0.0;
    }
    if (tid < DB) {
        double z = 0.0;
        for (int c = 0; c <= tid; ++c) z += Xs[tid * (tid + 1) / 2 + c] * bs[c];
        D.bz[DB * K + tid] = z;
    }
}

// Workgroup b: L_IK = A_IK Z_K^T for I = crows[crptr[K] + b], in place.
__global__ __launch_bounds__(DTPB) void k_dense_panel(const LmState* __restrict__ st, DenseWork D, int K,
                                                      const int* __restrict__ flag) {
    if (dense_off(st, flag)) return;
    extern __shared__ __attribute__((aligned(16))) double dn_lds[];
    double* T0 = dn_lds;
    double* T1 = dn_lds + DB * DLD;
    const int wave = threadIdx.x >> 6, qi = wave >> 1, qj = wave & 1;
    const int I = D.crows[D.crptr[K] + blockIdx.x];
    double* X = dense_blk(D, I, K);
    dense_stage(T0, X);
    dense_stage(T1, D.Zd + (size_t)K * DENSE_BB);
    __syncthreads();
    d4 acc[2][2] = {};
    // C(i, j) = sum_m X(i, m) Z(j, m); Z is lower triangular: m <= j < 32 (qj + 1)
    tile_mma(acc, T0 + 32 * qi * DLD, DLD, 1, T1 + 32 * qj * DLD, DLD, 1, 32 * (qj + 1));
    tile_store<TILE_SET>(acc, X, DB, qi, qj);
}

// Workgroup (x = q, y = p) with q <= p < nr: A_IJ -= L_IK L_JK^T for I = rows[p], J = rows[q] of column K's list;
// workgroup (x, y = nr): b_I -= L_IK z_K for I = rows[x].
__global__ __launch_bounds__(DTPB) void k_dense_trail(const LmState* __restrict__ st, DenseWork D, int K,
                                                      const int* __restrict__ flag) {
    if (dense_off(st, flag)) return;
    extern __shared__ __attribute__((aligned(16))) double dn_lds[];
    const int r0 = D.crptr[K], nr = D.crptr[K + 1] - r0;
    const int tid = threadIdx.x;
    if ((int)blockIdx.y == nr) {
        const int I = D.crows[r0 + blockIdx.x];
        const double* L = dense_blk(D, I, K);
        const double* z = D.bz + DB * K;
        const int c = tid & 63, part = tid >> 6;  // thread (c, part): row c of L, its columns part * 16 .. + 15
        double* red = dn_lds;
        double s = 0.0;
        const double* row = L + c * DB + part * 16;
#pragma unroll
        for (int m = 0; m < 16; ++m) s += row[m] * z[part * 16 + m];
        red[part * DB + c] = s;
        __syncthreads();
        if (tid < DB) D.bz[DB * I + tid] -= ((red[tid] + red[DB + tid]) + red[2 * DB + tid]) + red[3 * DB + tid];
        return;
    }
    const int p = blockIdx.y, q = blockIdx.x;
    if (q > p) return;
    const int wave = tid >> 6, qi = wave >> 1, qj = wave & 1;
    const int I = D.crows[r0 + p], J = D.crows[r0 + q];
    double* T0 = dn_lds;
    double* T1 = p == q ? T0 : dn_lds + DB * DLD;
    dense_stage(T0, dense_blk(D, I, K));
    if (p != q) dense_stage(T1, dense_blk(D, J, K));
    __syncthreads();
    if (p == q && qj > qi) return;  // a diagonal block: its lower triangle only
    d4 acc[2][2] = {};
    tile_mma(acc, T0 + 32 * qi * DLD, DLD, 1, T1 + 32 * qj * DLD, DLD, 1, DB);
    tile_store<TILE_SUB>(acc, dense_blk(D, I, J), DB, qi, qj);
}

// One workgroup: t = z_K - sum over column K's list of L_IK^T y_I (thread (c, part) sums the rows part * 16 .. + 15
// of every block, the four parts added in a fixed order), then y_K = Z_K^T t.
__global__ __launch_bounds__(DTPB) void k_dense_back(const LmState* __restrict__ st, DenseWork D, int K,
                                                     double* __restrict__ y_out, int npad,
                                                     const int* __restrict__ flag) {
    if (dense_off(st, flag)) return;
    __shared__ double red[4 * DB];
    __shared__ double ts[DB];
    const int tid = threadIdx.x, c = tid & 63, part = tid >> 6;
    const int r0 = D.crptr[K], r1 = D.crptr[K + 1];
    double s = 0.0;
    for (int t = r0; t < r1; ++t) {
        const int I = D.crows[t];
        const double* L = dense_blk(D, I, K) + (part * 16) * DB + c;
        const double* y = D.bz + DB * I + part * 16;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += L[r * DB] * y[r];
    }
    red[part * DB + c] = s;
    __syncthreads();
    if (tid < DB) ts[tid] = D.bz[DB * K + tid] - (((red[tid] + red[DB + tid]) + red[2 * DB + tid]) + red[3 * DB + tid]);
    __syncthreads();
    if (tid < DB) {
        const double* Zk = D.Zd + (size_t)K * DENSE_BB;
        double v = 0.0;
        for (int r = tid; r < DB; ++r) v += Zk[r * DB + tid] * ts[r];
        D.bz[DB * K + tid] = v;
        if (DB * K + tid < npad) y_out[DB * K + tid] = v;
    }
}

#define DPL(kid, ...)                                   \
    do {                                                \
        if (pf) pf->begin(kid, s);                      \
        hipLaunchKernelGGL(__VA_ARGS__);                \
        if (pf) pf->end(s);                             \
        const hipError_t e_ = hipGetLastError();        \
        if (e_ != hipSuccess) return e_;                \
    } while (0)

}  // namespace

hipError_t launch_dense(const LmState* st, const double* S, int npad, double* rhs, int* chol_flag, const DenseWork& D,
                        hipStream_t s, Prof* pf) {
    static DeviceOnce attr;
    const hipError_t ea = attr([]() -> hipError_t {
        hipError_t e = hipFuncSetAttribute((const void*)k_dense_panel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)DENSE_LDS2);
        if (e != hipSuccess) return e;
        return hipFuncSetAttribute((const void*)k_dense_trail, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)DENSE_LDS2);
    });
    if (ea != hipSuccess) return ea;
    DPL(K_DENSE_COPY, k_dense_copy, dim3(D.n_env + 1), dim3(DTPB), 0, s, st, S, npad, rhs, D);
    for (int K = 0; K < D.nblk; ++K) {
        const int nr = D.h_crptr[K + 1] - D.h_crptr[K];
        DPL(K_DENSE_DIAG, k_dense_diag<DIAG_TPB>, dim3(1), dim3(DIAG_TPB), 0, s, st, D, K, chol_flag);
        if (nr > 0) {
            DPL(K_DENSE_PANEL, k_dense_panel, dim3(nr), dim3(DTPB), DENSE_LDS2, s, st, D, K, chol_flag);
            DPL(K_DENSE_TRAIL, k_dense_trail, dim3(nr, nr + 1), dim3(DTPB), DENSE_LDS2, s, st, D, K, chol_flag);
        }
    }
    for (int K = D.nblk - 1; K >= 0; --K)
        DPL(K_DENSE_BACK, k_dense_back, dim3(1), dim3(DTPB), 0, s, st, D, K, rhs, npad, chol_flag);
    return hipSuccess;
}

}  // namespace miba
