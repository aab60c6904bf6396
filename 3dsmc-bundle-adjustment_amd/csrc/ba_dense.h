// ba_dense.h — the multi-workgroup blocked Cholesky of wide co-visibility windows (ba_dense.hip, internal):
// its block envelope (host) and its launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace miba {

struct LmState;
struct Prof;

static constexpr int DENSE_B = 64;  // block size: the tile of ba_tile64.h (the covariance's COV_B is this one)
static constexpr int DENSE_BB = DENSE_B * DENSE_B;
// Default selection: where the solver choice lands on the one-workgroup envelope kernel (k_chol), windows of
// npad >= BLOCKED_MIN_NPAD take this path instead (measured crossover; MIBA_BLOCKED_MIN overrides).
static constexpr int BLOCKED_MIN_NPAD = 256;
inline int dense_nblk(int npad) { return (npad + DENSE_B - 1) / DENSE_B; }

// The envelope of S at 64-block granularity, from the plan's fcol (first 16-block column of every 16-block row):
// block row I holds the block columns bfcol[I]..I, stored contiguously from block slot rowstart[I]; block column K
// is coupled to the block rows crows[crptr[K]..crptr[K + 1]) (I > K with bfcol[I] <= K), as rptr / rows are at 16.
// The fill of the factorisation stays inside this envelope.
struct DensePlan {
    int nblk = 0;
    std::vector<int> bfcol, rowstart, crptr, crows, blk;  // blk: (I, J) of every envelope block, row-major
    int n_env() const { return (int)blk.size() / 2; }
};

inline void dense_plan(const std::vector<int>& fcol, int npad, DensePlan& dp) {
    const int nb = npad / 16, nblk = dense_nblk(npad);
    dp.nblk = nblk;
    dp.bfcol.assign(nblk, 0);
    for (int I = 0; I < nblk; ++I) {
        int f = I;
        for (int i = 4 * I; i < std::min(4 * I + 4, nb); ++i) f = std::min(f, fcol[i] / 4);
        dp.bfcol[I] = f;
    }
    dp.rowstart.assign(nblk + 1, 0);
    dp.blk.clear();
    for (int I = 0; I < nblk; ++I) {
        dp.rowstart[I + 1] = dp.rowstart[I] + (I - dp.bfcol[I] + 1);
        for (int J = dp.bfcol[I]; J <= I; ++J) {
            dp.blk.push_back(I);
            dp.blk.push_back(J);
        }
    }
    dp.crptr.assign(nblk + 1, 0);
    dp.crows.clear();
    for (int K = 0; K < nblk; ++K) {
        for (int I = K + 1; I < nblk; ++I)
            if (dp.bfcol[I] <= K) dp.crows.push_back(I);
        dp.crptr[K + 1] = (int)dp.crows.size();
    }
}

// Device side of the path (DevWork::dense). A: the envelope's 64x64 blocks, packed (row-major inside a block); a
// private copy of S, so S itself is never written. Zd: the inverses of the diagonal blocks' factors. bz: the
// right-hand side padded to 64 nblk (rhs -> z -> y). h_crptr: the host's copy of crptr (the grids).
struct DenseWork {
    double* A = nullptr;
    double* Zd = nullptr;
    double* bz = nullptr;
    const int* bfcol = nullptr;
    const int* rowstart = nullptr;
    const int* crptr = nullptr;
    const int* crows = nullptr;
    const int2* blk = nullptr;
    int nblk = 0, n_env = 0;
    const int* h_crptr = nullptr;
};

// The whole reduced solve: y (into rhs) from S (npad x npad, envelope tiles) and rhs. One copy launch, then per
// block column diag / panel / trail, then one backward launch per block column; a pivot failure raises
// FLAG_NOT_PD in chol_flag and the remaining launches exit on it.
hipError_t launch_dense(const LmState* st, const double* S, int npad, double* rhs, int* chol_flag, const DenseWork& D,
                        hipStream_t s, Prof* pf);

}  // namespace miba
