// ba_align.hip — ba_align's kernels (ba_align.h): the hypotheses' inlier counts, then the pick, the refit and the
// outputs of a pair. All f64; the model code is ba_align_fit.h's, the samples ba_align_sample.h's.
#include "ba_align.h"
#include "ba_align_fit.h"

namespace miba {

namespace {

// the sample of hypothesis h of pair j (n >= 3 correspondences from b0) and its model; false for a degenerate sample
__device__ __forceinline__ bool hyp_model(const AlignArgs& a, int j, int h, int b0, int n, AlignModel& m) {
    uint32_t idx[3];
    align_sample(a.seed, (uint32_t)j, (uint32_t)h, (uint32_t)n, idx);
    double s1[3][3], s2[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const size_t at = 3 * ((size_t)b0 + idx[i]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s1[i][k] = a.p1[at + k];
            s2[i][k] = a.p2[at + k];
        }
    }
    return align_fit3(s1, s2, a.min_cross2, m);
}

__global__ __launch_bounds__(ALIGN_TPB) void k_align_hyp(AlignArgs a, int n_hblk) {
    // x1 | y1 | z1 | x2 | y2 | z2 of the tile's correspondences
    __shared__ double tile[6][ALIGN_TILE];
    const int j = (int)(blockIdx.x / (unsigned)n_hblk), hb = (int)(blockIdx.x % (unsigned)n_hblk);
    const int tid = (int)threadIdx.x, h = hb * ALIGN_TPB + tid;
    const int b0 = a.pair_begin[j], n = a.pair_begin[j + 1] - b0;
    const bool live = h < a.n_hyp;
    int* out = a.hyp_count + (size_t)j * (size_t)a.n_hyp;
    if (n < 3) {  // (the whole workgroup: nothing to sample from)
        if (live) out[h] = -1;
        return;
    }
    AlignModel m;
    const bool ok = live && hyp_model(a, j, h, b0, n, m);
    int cnt = 0;
    for (int base = 0; base < n; base += ALIGN_TILE) {
        const int len = min(ALIGN_TILE, n - base);
        const size_t g0 = 3 * ((size_t)b0 + (size_t)base);
        __syncthreads();  // the previous tile has been read by every lane
        for (int e = tid; e < 3 * len; e += ALIGN_TPB) {
            const int i = e / 3, c = e - 3 * i;
            tile[c][i] = a.p1[g0 + e];
            tile[3 + c][i] = a.p2[g0 + e];
        }
        __syncthreads();
        if (ok) {
            for (int i = 0; i < len; ++i) {
                const double d2 = align_dist2(m, tile[0][i], tile[1][i], tile[2][i], tile[3][i], tile[4][i], tile[5][i]);
                cnt += d2 < a.thr2 ? 1 : 0;
            }
        }
    }
    if (live) out[h] = ok ? cnt : -1;
}

// fixed-shape tree sums of NV values per thread over the workgroup; every thread returns with the totals in v
template <class T, int NV>
__device__ __forceinline__ void block_sum(T (&v)[NV], T (*buf)[ALIGN_TPB]) {
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) buf[k][tid] = v[k];
    __syncthreads();
    for (int s = ALIGN_TPB / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < NV; ++k) buf[k][tid] = buf[k][tid] + buf[k][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = buf[k][0];
    __syncthreads();
}

__global__ __launch_bounds__(ALIGN_TPB) void k_align_pick(AlignArgs a) {
    __shared__ unsigned long long s_key[ALIGN_TPB];
    __shared__ int s_int[2][ALIGN_TPB];
    __shared__ double s_red[9][ALIGN_TPB];
    __shared__ AlignModel s_m[2];  // the current model, the round's candidate
    __shared__ int s_ok;
    const int j = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int b0 = a.pair_begin[j], n = a.pair_begin[j + 1] - b0;
    const double* P1 = a.p1 + 3 * (size_t)b0;
    const double* P2 = a.p2 + 3 * (size_t)b0;
    double* pose = a.poses + 7 * (size_t)j;
    double* st = a.stats + (size_t)ALIGN_STAT * (size_t)j;
    unsigned char* mask = a.inlier + b0;

    // the best count, the smallest h among equals: the largest (count + 1) << 32 | (2^32 - 1 - h)
    unsigned long long key = 0;
    int iv[2] = {0, 0};  // degenerate samples | (pass C) changed flags
    if (n >= 3) {
        const int* hc = a.hyp_count + (size_t)j * (size_t)a.n_hyp;
        for (int h = tid; h < a.n_hyp; h += ALIGN_TPB) {
            const int c = hc[h];
            iv[0] += c < 0 ? 1 : 0;
            const unsigned long long k = (unsigned long long)(unsigned)(c + 1) << 32 | (0xFFFFFFFFu - (unsigned)h);
            key = k > key ? k : key;
        }
    }
    s_key[tid] = key;
    __syncthreads();
    for (int s = ALIGN_TPB / 2; s > 0; s >>= 1) {
        if (tid < s) s_key[tid] = s_key[tid + s] > s_key[tid] ? s_key[tid + s] : s_key[tid];
        __syncthreads();
    }
    key = s_key[0];
    block_sum<int, 2>(iv, s_int);
    const int n_degenerate = iv[0];
    const int best_cnt = (int)(key >> 32) - 1;
    const int best_h = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    if (n < 3 || best_cnt < 0) {  // no model: the identity, no inlier
        for (int i = tid; i < n; i += ALIGN_TPB) mask[i] = 0;
        if (tid == 0) {
            pose[0] = pose[1] = pose[2] = 0.0; pose[3] = 1.0;
            pose[4] = pose[5] = pose[6] = 0.0;
            st[0] = n < 3 ? 1.0 : 2.0;  // BA_ALIGN_TOO_FEW, BA_ALIGN_NO_MODEL
            st[1] = (double)n; st[2] = 0.0; st[3] = -1.0; st[4] = (double)n_degenerate; st[5] = 0.0; st[6] = 0.0; st[7] = 0.0;
        }
        return;
    }
    if (tid == 0) (void)hyp_model(a, j, best_h, b0, n, s_m[0]);  // bitwise the model k_align_hyp scored
    __syncthreads();

    AlignModel cur = s_m[0];
    auto dist2_of = [&](const AlignModel& m, int i) {
        const size_t o = 3 * (size_t)i;
        return align_dist2(m, P1[o], P1[o + 1], P1[o + 2], P2[o], P2[o + 1], P2[o + 2]);
    };
    auto inlier_of = [&](const AlignModel& m, int i) { return dist2_of(m, i) < a.thr2; };
    iv[0] = iv[1] = 0;
    for (int i = tid; i < n; i += ALIGN_TPB) iv[0] += inlier_of(cur, i) ? 1 : 0;
    block_sum<int, 2>(iv, s_int);
    int m_cur = iv[0];
    const int m_sample = m_cur;

    for (int round = 0; round < a.refit && m_cur >= 3; ++round) {
        // the centroids of the current inliers, then H about them: lane t sums i = t, t + ALIGN_TPB, ... in that
        // order, the tree joins the lanes
        double sv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) sv[k] = 0.0;
        for (int i = tid; i < n; i += ALIGN_TPB)
            if (inlier_of(cur, i)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    sv[k] = sv[k] + P1[3 * (size_t)i + k];
                    sv[3 + k] = sv[3 + k] + P2[3 * (size_t)i + k];
                }
            }
        block_sum<double, 9>(sv, s_red);
        double c1[3], c2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c1[k] = sv[k] / (double)m_cur;
            c2[k] = sv[3 + k] / (double)m_cur;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) sv[k] = 0.0;
        for (int i = tid; i < n; i += ALIGN_TPB)
            if (inlier_of(cur, i)) {
#pragma clang fp contract(off)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) sv[3 * r + k] = sv[3 * r + k] + (P2[3 * (size_t)i + r] - c2[r]) * (P1[3 * (size_t)i + k] - c1[k]);
            }
        block_sum<double, 9>(sv, s_red);
        if (tid == 0) {
            align_fit_H(sv, c1, c2, s_m[1]);
            s_ok = align_model_finite(s_m[1]) ? 1 : 0;
        }
        __syncthreads();
        if (!s_ok) break;
        const AlignModel cand = s_m[1];
        iv[0] = iv[1] = 0;
        for (int i = tid; i < n; i += ALIGN_TPB) {
            const bool f = inlier_of(cand, i);
            iv[0] += f ? 1 : 0;
            iv[1] += f != inlier_of(cur, i) ? 1 : 0;
        }
        block_sum<int, 2>(iv, s_int);
        if (iv[0] < m_cur) break;  // fewer inliers: the previous pose stays
        cur = cand;
        m_cur = iv[0];
        if (iv[1] == 0) break;  // the set did not change
    }

    // the mask and the inliers' RMS distance
    double dsum[1] = {0.0};
    for (int i = tid; i < n; i += ALIGN_TPB) {
        const double d2 = dist2_of(cur, i);
        const bool f = d2 < a.thr2;
        mask[i] = f ? 1 : 0;
        if (f) dsum[0] = dsum[0] + d2;
    }
    block_sum<double, 1>(dsum, s_red);
    if (tid == 0) {
        pose[0] = cur.q[0]; pose[1] = cur.q[1]; pose[2] = cur.q[2]; pose[3] = cur.q[3];
        pose[4] = cur.t[0]; pose[5] = cur.t[1]; pose[6] = cur.t[2];
        st[0] = 0.0;  // BA_ALIGN_OK
        st[1] = (double)n; st[2] = (double)m_cur; st[3] = (double)best_h; st[4] = (double)n_degenerate;
        st[5] = m_cur > 0 ? sqrt(dsum[0] / (double)m_cur) : 0.0;
        st[6] = (double)m_sample; st[7] = 0.0;
    }
}

}  // namespace

hipError_t launch_align_hyp(const AlignArgs& a, hipStream_t s) {
    const int n_hblk = align_hyp_blocks(a.n_hyp);
    hipLaunchKernelGGL(k_align_hyp, dim3((unsigned)a.n_pairs * (unsigned)n_hblk), dim3(ALIGN_TPB), 0, s, a, n_hblk);
    return hipGetLastError();
}

hipError_t launch_align_pick(const AlignArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_align_pick, dim3((unsigned)a.n_pairs), dim3(ALIGN_TPB), 0, s, a);
    return hipGetLastError();
}

}  // namespace miba
