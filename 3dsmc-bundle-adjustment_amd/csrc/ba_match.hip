// ba_match.hip — ba_match's kernels (ba_match.h): the slices' two nearest trains of every query, then the merge with
// the acceptance chain, then the ordered compaction. Integers throughout.
#include "ba_match.h"
#include "ba_scan.h"
#include "ba_top2.h"

#include "../../include/ba.h"

namespace miba {

namespace {

static_assert(MATCH_SCAN_TPB == SCAN_TPB, "the host's launch limit counts ba_scan.h's workgroup");

using i32x4 = __attribute__((ext_vector_type(4))) int;

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return (unsigned long long)hi << 32 | lo;
}

// What a workgroup of k_match_nn works on: its pair, its queries and its slice of the pair's trains.
struct NnWork {
    int j, qb, nq, tb, q0, s0, s1, slice;
};
__device__ __forceinline__ NnWork nn_work(const MatchNnArgs& a) {
    NnWork w;
    const int tile = (int)(blockIdx.x / (unsigned)a.n_slices);
    w.slice = (int)(blockIdx.x % (unsigned)a.n_slices);
    w.j = owner_of(a.tile_begin, a.n_pairs, tile);
    const int* r = a.range + 4 * (size_t)w.j;
    const int o = a.swap ? 2 : 0;
    w.qb = r[o];
    w.nq = r[o + 1] - r[o];
    w.tb = r[2 - o];
    const int nt = r[3 - o] - r[2 - o];
    w.q0 = (tile - a.tile_begin[w.j]) * MATCH_QTILE;
    // whole LDS tiles per slice; the last slices of a short pair are empty
    const int per = ((nt + a.n_slices - 1) / a.n_slices + MATCH_TTILE - 1) / MATCH_TTILE * MATCH_TTILE;
    const long long b = (long long)w.slice * per;
    w.s0 = (int)(b < nt ? b : nt);
    w.s1 = (int)(b + per < nt ? b + per : nt);
    return w;
}
__device__ __forceinline__ void nn_store(const MatchNnArgs& a, const NnWork& w, int q, unsigned long long k0,
                                         unsigned long long k1) {
    unsigned long long* out = a.top + ((size_t)(a.row_begin[w.j] + q) * (size_t)a.n_slices + (size_t)w.slice) * (size_t)a.keep;
    out[0] = k0;
    if (a.keep == 2) out[1] = k1;
}

// HAMMING. NDW: the descriptor's dwords rounded up to 8, 16, 32 or 64 (zeros on both sides add no bit).
template <int NDW>
__global__ __launch_bounds__(MATCH_TPB_HAMMING) void k_match_nn_hamming(MatchNnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned tile[MATCH_TTILE * NDW];
    const NnWork w = nn_work(a);
    const int lane = (int)threadIdx.x, q = w.q0 + lane, ndw = a.desc_bytes >> 2;
    const bool live = q < w.nq;
    const unsigned* Q = reinterpret_cast<const unsigned*>(a.query) + (size_t)(w.qb + (live ? q : 0)) * (size_t)ndw;
    const unsigned* T = reinterpret_cast<const unsigned*>(a.train);
    unsigned qd[NDW];
#pragma unroll
    for (int k = 0; k < NDW; ++k) qd[k] = live && k < ndw ? Q[k] : 0u;
    unsigned long long k0 = MATCH_NONE, k1 = MATCH_NONE;
    for (int base = w.s0; base < w.s1; base += MATCH_TTILE) {
        const int len = min(MATCH_TTILE, w.s1 - base);
        __syncthreads();  // the previous tile has been read by every lane
        for (int e = lane; e < len * NDW; e += MATCH_TPB_HAMMING) {
            const int i = e / NDW, k = e - i * NDW;
            tile[e] = k < ndw ? T[(size_t)(w.tb + base + i) * (size_t)ndw + k] : 0u;
        }
        __syncthreads();
        for (int i = 0; i < len; ++i) {
            unsigned d = 0;
#pragma unroll
            for (int k = 0; k < NDW; ++k) d += (unsigned)__popc(qd[k] ^ tile[i * NDW + k]);
            // (equal distances at a larger index than the second's cannot enter, at a smaller one they must)
            if (d <= (unsigned)(k1 >> 32)) top2_push((unsigned long long)d << 32 | (unsigned)(base + i), k0, k1);
        }
    }
    if (live) nn_store(a, w, q, k0, k1);
}

// the sum of the squares of a dword's four i8
__device__ __forceinline__ int sq4(unsigned v) {
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int x = (int)(signed char)(v >> (8 * b));
        s += x * x;
    }
    return s;
}

// L2_U8. The descriptors shifted by -128 (byte-wise ^ 0x80), padded with zeros to whole k-steps. Wave v owns the
// queries v * MATCH_MFMA .. of the tile as the B operand (the columns); a lane holds column lane & 15 and, of every
// k-step, the bytes 16 (lane >> 4) .. + 16. The trains are the A operand through the same byte map, so the order of k
// inside a step does not matter. C: column lane & 15, rows 4 (lane >> 4) + r in register r.
static constexpr int L2_MAX_STEPS = BA_MATCH_MAX_BYTES / MATCH_KSTEP;
static constexpr int L2_STRIDE = BA_MATCH_MAX_BYTES / 4 + 4;  // dwords of a train's row in LDS (16-byte aligned, off the power of two)

__global__ __launch_bounds__(MATCH_TPB_L2) void k_match_nn_l2(MatchNnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned tile[MATCH_TTILE * L2_STRIDE];
    __shared__ int tnorm[MATCH_TTILE];
    const NnWork w = nn_work(a);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
    const int ndw = a.desc_bytes >> 2, ksteps = (a.desc_bytes + MATCH_KSTEP - 1) / MATCH_KSTEP, kdw = ksteps * (MATCH_KSTEP / 4);
    const int q = w.q0 + wave * MATCH_MFMA + col;
    const bool live = q < w.nq;
    const unsigned* Q = reinterpret_cast<const unsigned*>(a.query) + (size_t)(w.qb + (live ? q : 0)) * (size_t)ndw;
    const unsigned* T = reinterpret_cast<const unsigned*>(a.train);
    i32x4 bq[L2_MAX_STEPS];
    int qn = 0;
#pragma unroll
    for (int ks = 0; ks < L2_MAX_STEPS; ++ks) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = ks * (MATCH_KSTEP / 4) + g * 4 + c;
            const unsigned v = live && k < ndw ? Q[k] ^ 0x80808080u : 0u;
            bq[ks][c] = (int)v;
            qn += sq4(v);
        }
    }
    qn += __shfl_xor(qn, 16, 64);
    qn += __shfl_xor(qn, 32, 64);

    unsigned long long k0 = MATCH_NONE, k1 = MATCH_NONE;
    for (int base = w.s0; base < w.s1; base += MATCH_TTILE) {
        const int len = min(MATCH_TTILE, w.s1 - base);
        __syncthreads();  // the previous tile has been read by every wave
        {
            // four threads per train: the shifted bytes into LDS, the norm beside them (rows past len: zeros)
            const int i = tid >> 2, part = tid & 3;
            int s = 0;
            for (int k = part; k < kdw; k += 4) {
                const unsigned v = i < len && k < ndw ? T[(size_t)(w.tb + base + i) * (size_t)ndw + k] ^ 0x80808080u : 0u;
                tile[i * L2_STRIDE + k] = v;
                s += sq4(v);
            }
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if (part == 0) tnorm[i] = s;
        }
        __syncthreads();
        for (int sub = 0; sub * MATCH_MFMA < len; ++sub) {
            i32x4 acc = {0, 0, 0, 0};
            const unsigned* arow = tile + (sub * MATCH_MFMA + col) * L2_STRIDE + g * 4;
#pragma unroll
            for (int ks = 0; ks < L2_MAX_STEPS; ++ks)
                if (ks < ksteps) {
                    const i32x4 af = *reinterpret_cast<const i32x4*>(arow + ks * (MATCH_KSTEP / 4));
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bq[ks], acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = sub * MATCH_MFMA + g * 4 + r;
                const unsigned d = (unsigned)(qn + tnorm[i] - 2 * acc[r]);
                if (i < len && d <= (unsigned)(k1 >> 32))
                    top2_push((unsigned long long)d << 32 | (unsigned)(base + i), k0, k1);
            }
        }
    }
    // the four lanes of a column hold disjoint trains
#pragma unroll
    for (int m = 16; m <= 32; m <<= 1) {
        const unsigned long long b0 = shfl_xor_u64(k0, m), b1 = shfl_xor_u64(k1, m);
        top2_merge(b0, b1, k0, k1);
    }
    if (live && g == 0) nn_store(a, w, q, k0, k1);
}

__global__ __launch_bounds__(SCAN_TPB) void k_match_pick(MatchPickArgs a) {
    const long long row = (long long)blockIdx.x * SCAN_TPB + threadIdx.x;
    if (row < a.n_pairs) {
        const int* r = a.range + 4 * (size_t)row;
        a.counts[MATCH_COUNT * (size_t)row] = r[1] - r[0];
        a.counts[MATCH_COUNT * (size_t)row + 1] = r[3] - r[2];
    }
    if (row >= a.n_rows) return;
    const int j = owner_of(a.row_begin, a.n_pairs, row);
    const int ql = (int)(row - a.row_begin[j]);
    unsigned long long k0 = MATCH_NONE, k1 = MATCH_NONE;
    const unsigned long long* t = a.top + (size_t)row * (size_t)a.n_slices * 2;
    for (int s = 0; s < a.n_slices; ++s) top2_merge(t[2 * s], t[2 * s + 1], k0, k1);
    const bool has0 = k0 != MATCH_NONE, has1 = k1 != MATCH_NONE;
    const int i0 = has0 ? (int)(unsigned)k0 : -1, d0 = has0 ? (int)(k0 >> 32) : -1;
    const int i1 = has1 ? (int)(unsigned)k1 : -1, d1 = has1 ? (int)(k1 >> 32) : -1;
    a.nn_idx[2 * (size_t)row] = i0; a.nn_idx[2 * (size_t)row + 1] = i1;
    a.nn_dist[2 * (size_t)row] = d0; a.nn_dist[2 * (size_t)row + 1] = d1;

    int at = 2;  // the count this row falls into: accepted, or the first condition it fails
    if (!has1) {
        at = 3;
    } else {
        const bool ratio_ok = a.kind == BA_MATCH_HAMMING ? (float)d0 < a.ratio * (float)d1
                                                         : (double)d0 < a.ratio2 * (double)d1;
        if (!ratio_ok) {
            at = 4;
        } else if (a.max_distance > 0 && d0 > a.max_distance) {
            at = 5;
        } else if (a.cross_check) {
            // the smallest query of the chosen train under (distance, query index), over the swapped launch's slices
            const unsigned long long* c = a.cross + (size_t)(a.col_begin[j] + i0) * (size_t)a.n_slices;
            unsigned long long m = MATCH_NONE;
            for (int s = 0; s < a.n_slices; ++s) m = c[s] < m ? c[s] : m;
            if ((int)(unsigned)m != ql) at = 6;
        }
    }
    a.accept[row] = at == 2 ? 1 : 0;
    atomicAdd(&a.counts[MATCH_COUNT * (size_t)j + at], 1);
}

// One workgroup: match_begin, the exclusive scan of the pairs' accepted counts, in chunks of SCAN_TPB pairs.
__global__ __launch_bounds__(SCAN_TPB) void k_match_begin(MatchPickArgs a) {
    __shared__ int sh[SCAN_TPB / 64];
    const int tid = (int)threadIdx.x;
    int at = 0;
    for (int base = 0; base < a.n_pairs; base += SCAN_TPB) {
        const int j = base + tid;
        const int c = j < a.n_pairs ? a.counts[MATCH_COUNT * (size_t)j + 2] : 0;
        int sum;
        const int pos = at + block_excl(c, sh, sum);
        if (j < a.n_pairs) a.match_begin[j] = pos;
        at += sum;
    }
    if (tid == 0) a.match_begin[a.n_pairs] = at;
}

// One workgroup per pair: the ordered scan over the pair's rows, from match_begin[j].
__global__ __launch_bounds__(SCAN_TPB) void k_match_compact(MatchPickArgs a) {
    __shared__ int sh[SCAN_TPB / 64];
    const int j = (int)blockIdx.x, tid = (int)threadIdx.x;
    int at = a.match_begin[j];
    const long long r0 = a.row_begin[j];
    const int n = (int)(a.row_begin[j + 1] - r0);
    for (int base = 0; base < n; base += SCAN_TPB) {
        const int ql = base + tid;
        const int f = ql < n ? (int)a.accept[r0 + ql] : 0;
        int sum;
        const int pos = at + block_excl(f, sh, sum);
        if (f) {
            a.matches[2 * (size_t)pos] = ql;
            a.matches[2 * (size_t)pos + 1] = a.nn_idx[2 * (size_t)(r0 + ql)];
        }
        at += sum;
    }
}

}  // namespace

hipError_t launch_match_nn(int kind, const MatchNnArgs& a, int n_tiles, hipStream_t s) {
    const dim3 grid((unsigned)n_tiles * (unsigned)a.n_slices);
    if (kind == BA_MATCH_HAMMING) {
        const int ndw = a.desc_bytes >> 2;
        const dim3 block(MATCH_TPB_HAMMING);
        if (ndw <= 8) hipLaunchKernelGGL(k_match_nn_hamming<8>, grid, block, 0, s, a);
        else if (ndw <= 16) hipLaunchKernelGGL(k_match_nn_hamming<16>, grid, block, 0, s, a);
        else if (ndw <= 32) hipLaunchKernelGGL(k_match_nn_hamming<32>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_match_nn_hamming<64>, grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL(k_match_nn_l2, grid, dim3(MATCH_TPB_L2), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_match_pick(const MatchPickArgs& a, hipStream_t s) {
    const long long n = a.n_rows > a.n_pairs ? a.n_rows : a.n_pairs;
    hipLaunchKernelGGL(k_match_pick, dim3((unsigned)((n + SCAN_TPB - 1) / SCAN_TPB)), dim3(SCAN_TPB), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_begin(const MatchPickArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_match_begin, dim3(1), dim3(SCAN_TPB), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_match_compact(const MatchPickArgs& a, hipStream_t s) {
    if (!a.matches) return hipSuccess;  // (match_begin alone: k_match_begin wrote it)
    hipLaunchKernelGGL(k_match_compact, dim3((unsigned)a.n_pairs), dim3(SCAN_TPB), 0, s, a);
    return hipGetLastError();
}

}  // namespace miba
