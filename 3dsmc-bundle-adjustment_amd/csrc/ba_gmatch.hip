// ba_gmatch.hip — ba_guided_match's kernels (ba_gmatch.h): the keypoints of every distinct range binned into a pixel
// grid, then per candidate row the projection, the window's two nearest descriptors and the acceptance chain, then
// the one-to-one pick and the ordered compaction. Floating point for the projection and the two gates alone.
#include "ba_gmatch.h"
#include "ba_device.h"
#include "ba_obs.h"
#include "ba_scan.h"
#include "ba_top2.h"

#include "../../include/ba.h"

namespace miba {

namespace {

static_assert(GMATCH_TPB == SCAN_TPB, "the host's launch limit counts ba_scan.h's workgroup");
static_assert(GMATCH_COUNT == BA_GMATCH_COUNT_N, "the kernel writes the header's record width");

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// the grid, the keypoint and the cell of thread t of k_gm_count / k_gm_scatter
struct BinWork {
    int g, local, cell;
};
__device__ __forceinline__ BinWork bin_work(const GmArgs& a, int t) {
    BinWork w;
    w.g = owner_of(a.grid_kp_begin, a.n_grids, t);
    w.local = t - a.grid_kp_begin[w.g];
    const size_t k = (size_t)(a.grid_range[2 * w.g] + w.local);
    const int cx = gm_cell_of(a.kp_uv[2 * k], a.inv_cell, a.gw), cy = gm_cell_of(a.kp_uv[2 * k + 1], a.inv_cell, a.gh);
    w.cell = cy * a.gw + cx;
    return w;
}

__global__ __launch_bounds__(GMATCH_TPB) void k_gm_count(GmArgs a) {
    const long long t = (long long)blockIdx.x * GMATCH_TPB + threadIdx.x;
    if (t >= a.n_binned) return;
    const BinWork w = bin_work(a, (int)t);
    atomicAdd(&a.cell_count[(size_t)w.g * (size_t)a.cells + (size_t)w.cell], 1);
}

// One workgroup per grid: cell_off of its cells (slots of cell_list, from grid_kp_begin[g]); the counts are cleared.
__global__ __launch_bounds__(GMATCH_TPB) void k_gm_offsets(GmArgs a) {
    __shared__ int sh[SCAN_TPB / 64];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    int* cnt = a.cell_count + (size_t)g * (size_t)a.cells;
    int* off = a.cell_off + (size_t)g * ((size_t)a.cells + 1);
    int at = a.grid_kp_begin[g];
    for (int base = 0; base < a.cells; base += GMATCH_TPB) {
        const int c = base + tid;
        const int n = c < a.cells ? cnt[c] : 0;
        int sum;
        const int pos = at + block_excl(n, sh, sum);
        if (c < a.cells) {
            off[c] = pos;
            cnt[c] = 0;
        }
        at += sum;
    }
    if (tid == 0) off[a.cells] = at;
}

__global__ __launch_bounds__(GMATCH_TPB) void k_gm_scatter(GmArgs a) {
    const long long t = (long long)blockIdx.x * GMATCH_TPB + threadIdx.x;
    if (t >= a.n_binned) return;
    const BinWork w = bin_work(a, (int)t);
    const int pos = atomicAdd(&a.cell_count[(size_t)w.g * (size_t)a.cells + (size_t)w.cell], 1);
    a.cell_list[a.cell_off[(size_t)w.g * ((size_t)a.cells + 1) + (size_t)w.cell] + pos] = w.local;
}

// the sum of the squares of a dword's four u8, and the dot product of two dwords' u8, added to acc
__device__ __forceinline__ unsigned dot4_u8(unsigned x, unsigned y, unsigned acc) {
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(x, y, acc, false);
#else
#pragma unroll
    for (int b = 0; b < 4; ++b) acc += ((x >> (8 * b)) & 255u) * ((y >> (8 * b)) & 255u);
    return acc;
#endif
}

// The window test, in the header's order of operations.
__device__ __forceinline__ bool in_disc(double ku, double kv, double u, double v, double r2) {
#pragma clang fp contract(off)
    const double du = ku - u, dv = kv - v;
    return (du * du) + (dv * dv) <= r2;
}
__device__ __forceinline__ bool depth_ok(double dk, double z, double tol) {
#pragma clang fp contract(off)
    return !obs_admissible(dk) || fabs(dk - z) <= tol * z;
}

// One row per lane. NDW: the descriptor's dwords rounded up to 8, 16, 32 or 64. L2: BA_MATCH_L2_U8.
template <int NDW, bool L2>
__global__ __launch_bounds__(GMATCH_SEARCH_TPB) void k_gm_search(GmArgs a) {
    const long long row64 = (long long)blockIdx.x * GMATCH_SEARCH_TPB + threadIdx.x;
    if (row64 >= a.n_rows) return;
    const int row = (int)row64;
    const int f = owner_of(a.cand_begin, a.n_frames, row);
    const int pt = a.cand_pt[row], ndw = a.desc_bytes >> 2;

    double R[9], x, y, z, iz, u, v;
    obs_project(a.frame_pose + 7 * (size_t)f, a.points + 3 * (size_t)pt, a.K, R, x, y, z, iz, u, v);
    int st = 0;
    if (!(z > a.min_depth)) {
        st = 1;
        u = v = 0.0;
    } else if (!(u >= 0.0 && u < (double)a.width && v >= 0.0 && v < (double)a.height)) {
        st = 2;
    }
    a.proj[3 * (size_t)row] = u;
    a.proj[3 * (size_t)row + 1] = v;
    a.proj[3 * (size_t)row + 2] = z;

    unsigned long long k0 = TOP2_NONE, k1 = TOP2_NONE;
    int n_win = 0;
    if (st == 0) {
        const unsigned* Q = reinterpret_cast<const unsigned*>(a.pt_desc) + (size_t)pt * (size_t)ndw;
        unsigned qd[NDW];
        unsigned qn = 0;
#pragma unroll
        for (int k = 0; k < NDW; ++k) {
            qd[k] = k < ndw ? Q[k] : 0u;
            if (L2) qn = dot4_u8(qd[k], qd[k], qn);
        }
        const bool vec = (ndw & 3) == 0;  // whole 16-byte groups: the rows of kp_desc are 16-byte aligned then
        const bool gate = a.kp_depth && a.depth_tol > 0.0;
        const int rb = a.frame_range[2 * f];
        const int* off = a.cell_off + (size_t)a.frame_grid[f] * ((size_t)a.cells + 1);
        int xlo, xhi, ylo, yhi;
        gm_cell_span(u, a.radius, a.inv_cell, a.gw, xlo, xhi);
        gm_cell_span(v, a.radius, a.inv_cell, a.gh, ylo, yhi);
        for (int cy = ylo; cy <= yhi; ++cy) {
            // the cells xlo .. xhi of a grid row are one run of cell_list
            const int i1 = off[cy * a.gw + xhi + 1];
            for (int i = off[cy * a.gw + xlo]; i < i1; ++i) {
                const int kl = a.cell_list[i];
                const size_t k = (size_t)(rb + kl);
                if (!in_disc(a.kp_uv[2 * k], a.kp_uv[2 * k + 1], u, v, a.r2)) continue;
                if (gate && !depth_ok(a.kp_depth[k], z, a.depth_tol)) continue;
                ++n_win;
                const unsigned* T = reinterpret_cast<const unsigned*>(a.kp_desc) + k * (size_t)ndw;
                unsigned d = 0, tn = 0, dot = 0;
#pragma unroll
                for (int k4 = 0; k4 < NDW / 4; ++k4) {
                    if (4 * k4 >= ndw) break;
                    u32x4 t;
                    if (vec) {
                        t = *reinterpret_cast<const u32x4*>(T + 4 * k4);
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c) t[c] = 4 * k4 + c < ndw ? T[4 * k4 + c] : 0u;
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (L2) {
                            tn = dot4_u8(t[c], t[c], tn);
                            dot = dot4_u8(qd[4 * k4 + c], t[c], dot);
                        } else {
                            d += (unsigned)__popc(qd[4 * k4 + c] ^ t[c]);
                        }
                    }
                }
                if (L2) d = qn + tn - 2u * dot;  // |a - b|^2, exact: every term is below 2^25
                top2_push(top2_key(d, (unsigned)kl), k0, k1);
            }
        }
    }
    const bool has0 = k0 != TOP2_NONE, has1 = k1 != TOP2_NONE;
    const int i0 = has0 ? (int)top2_index(k0) : -1, d0 = has0 ? (int)top2_dist(k0) : -1;
    const int i1 = has1 ? (int)top2_index(k1) : -1, d1 = has1 ? (int)top2_dist(k1) : -1;
    if (st == 0) {
        if (!has0) {
            st = 3;
        } else if (has1 && !(L2 ? (double)d0 < a.ratio2 * (double)d1 : (float)d0 < a.ratio * (float)d1)) {
            st = 4;
        } else if (a.max_distance > 0 && d0 > a.max_distance) {
            st = 5;
        }
    }
    a.nn_kp[2 * (size_t)row] = i0; a.nn_kp[2 * (size_t)row + 1] = i1;
    a.nn_dist[2 * (size_t)row] = d0; a.nn_dist[2 * (size_t)row + 1] = d1;
    a.n_in_window[row] = n_win;
    a.status[row] = (unsigned char)st;
    if (st == 0 && a.one_to_one)
        atomicMin(&a.o2o[(size_t)a.o2o_begin[f] + (size_t)i0], top2_key((unsigned)d0, (unsigned)(row - a.cand_begin[f])));
}

__global__ __launch_bounds__(GMATCH_TPB) void k_gm_pick(GmArgs a) {
    const long long t = (long long)blockIdx.x * GMATCH_TPB + threadIdx.x;
    if (t < a.n_frames) {
        a.counts[GMATCH_COUNT * (size_t)t] = a.cand_begin[t + 1] - a.cand_begin[t];
        a.counts[GMATCH_COUNT * (size_t)t + 1] = a.frame_range[2 * t + 1] - a.frame_range[2 * t];
    }
    if (t >= a.n_rows) return;
    const int row = (int)t;
    const int f = owner_of(a.cand_begin, a.n_frames, row);
    int st = (int)a.status[row];
    if (st == 0 && a.one_to_one) {
        const unsigned long long win = a.o2o[(size_t)a.o2o_begin[f] + (size_t)a.nn_kp[2 * (size_t)row]];
        if (top2_index(win) != (unsigned)(row - a.cand_begin[f])) {
            st = 6;
            a.status[row] = 6;
        }
    }
    atomicAdd(&a.counts[GMATCH_COUNT * (size_t)f + 2 + st], 1);
}

// One workgroup: match_begin, the exclusive scan of the frames' accepted counts, in chunks of SCAN_TPB frames.
__global__ __launch_bounds__(GMATCH_TPB) void k_gm_begin(GmArgs a) {
    __shared__ int sh[SCAN_TPB / 64];
    const int tid = (int)threadIdx.x;
    int at = 0;
    for (int base = 0; base < a.n_frames; base += GMATCH_TPB) {
        const int f = base + tid;
        const int c = f < a.n_frames ? a.counts[GMATCH_COUNT * (size_t)f + 2] : 0;
        int sum;
        const int pos = at + block_excl(c, sh, sum);
        if (f < a.n_frames) a.match_begin[f] = pos;
        at += sum;
    }
    if (tid == 0) a.match_begin[a.n_frames] = at;
}

// One workgroup per frame entry: the ordered scan over its rows, from match_begin[f].
__global__ __launch_bounds__(GMATCH_TPB) void k_gm_compact(GmArgs a) {
    __shared__ int sh[SCAN_TPB / 64];
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    int at = a.match_begin[f];
    const int r0 = a.cand_begin[f], n = a.cand_begin[f + 1] - r0;
    for (int base = 0; base < n; base += GMATCH_TPB) {
        const int q = base + tid;
        const int ok = q < n && a.status[r0 + q] == 0 ? 1 : 0;
        int sum;
        const int pos = at + block_excl(ok, sh, sum);
        if (ok) {
            a.matches[2 * (size_t)pos] = a.cand_pt[r0 + q];
            a.matches[2 * (size_t)pos + 1] = a.nn_kp[2 * (size_t)(r0 + q)];
        }
        at += sum;
    }
}

unsigned blocks(long long n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

template <bool L2>
void launch_search(const GmArgs& a, hipStream_t s) {
    const dim3 grid(blocks(a.n_rows, GMATCH_SEARCH_TPB)), block(GMATCH_SEARCH_TPB);
    const int ndw = a.desc_bytes >> 2;
    if (ndw <= 8) hipLaunchKernelGGL((k_gm_search<8, L2>), grid, block, 0, s, a);
    else if (ndw <= 16) hipLaunchKernelGGL((k_gm_search<16, L2>), grid, block, 0, s, a);
    else if (ndw <= 32) hipLaunchKernelGGL((k_gm_search<32, L2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_gm_search<64, L2>), grid, block, 0, s, a);
}

}  // namespace

hipError_t launch_gm_bin(const GmArgs& a, hipStream_t s) {
    if (!a.n_grids) return hipSuccess;
    if (a.n_binned) hipLaunchKernelGGL(k_gm_count, dim3(blocks(a.n_binned, GMATCH_TPB)), dim3(GMATCH_TPB), 0, s, a);
    hipLaunchKernelGGL(k_gm_offsets, dim3((unsigned)a.n_grids), dim3(GMATCH_TPB), 0, s, a);
    if (a.n_binned) hipLaunchKernelGGL(k_gm_scatter, dim3(blocks(a.n_binned, GMATCH_TPB)), dim3(GMATCH_TPB), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gm_search(const GmArgs& a, hipStream_t s) {
    if (a.n_rows) {
        if (a.kind == BA_MATCH_L2_U8) launch_search<true>(a, s);
        else launch_search<false>(a, s);
    }
    const long long n = a.n_rows > a.n_frames ? a.n_rows : a.n_frames;
    if (n) hipLaunchKernelGGL(k_gm_pick, dim3(blocks(n, GMATCH_TPB)), dim3(GMATCH_TPB), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gm_compact(const GmArgs& a, hipStream_t s) {
    if (!a.n_frames) return hipSuccess;
    hipLaunchKernelGGL(k_gm_begin, dim3(1), dim3(GMATCH_TPB), 0, s, a);
    if (a.matches) hipLaunchKernelGGL(k_gm_compact, dim3((unsigned)a.n_frames), dim3(GMATCH_TPB), 0, s, a);
    return hipGetLastError();
}

}  // namespace miba
