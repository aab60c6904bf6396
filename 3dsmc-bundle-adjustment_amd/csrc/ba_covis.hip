// ba_covis.hip — the keyframe co-visibility graph of a window on the device (gfx950).
//
// B is the n_cams x n_points incidence matrix of the admissible observations, one bit per entry, a camera's row
// packed into 64-bit words. The weights are W = B B^T: W[a][b] = popcount(row a & row b), the distinct points both
// cameras see (a point seen twice by a camera is one bit). Everything is integer: bit sets by atomicOr (idempotent),
// sums by integer atomicAdd, spans by atomicMin / atomicMax, all order-independent.
#include "ba_covis.h"
#include "ba_obs.h"

namespace miba {

static constexpr int COVIS_TPB = 256;
static_assert(COVIS_TILE * COVIS_TILE == COVIS_TPB, "one thread per camera pair of a tile");
// LDS row stride of a staged panel in 64-bit words. The 16 lanes of a half wave that read word w of 16 different
// rows (ds_read_b64, bank = (byte address / 4) % 64) hit dword banks 2 * (row * stride + w) % 64: an odd stride makes
// row -> row * stride % 32 a bijection, so the 16 rows take 16 different bank pairs.
static constexpr int COVIS_LDS_STRIDE = COVIS_SLICE_WORDS + 1;
static_assert(COVIS_LDS_STRIDE % 2 == 1, "odd row stride: the rows of a panel start on different banks");

__global__ __launch_bounds__(COVIS_TPB) void k_covis_bits(const int* __restrict__ obs_cam, const int* __restrict__ obs_pt,
                                                          const double* __restrict__ obs_depth, int n_obs, size_t nw,
                                                          unsigned long long* __restrict__ bits) {
    const size_t k = (size_t)blockIdx.x * COVIS_TPB + threadIdx.x;
    if (k >= (size_t)n_obs || !obs_admissible(obs_depth[k])) return;
    const unsigned pt = (unsigned)obs_pt[k];
    atomicOr(bits + (size_t)obs_cam[k] * nw + (pt >> 6), 1ull << (pt & 63u));
}

// grid (slices, camera tiles, camera tiles); the tiles above the diagonal leave at once, a tile below it writes its
// counts to both triangles.
__global__ __launch_bounds__(COVIS_TPB) void k_covis_count(const unsigned long long* __restrict__ bits, int n_cams,
                                                           size_t nw, int* __restrict__ W) {
    const int ta = blockIdx.y, tb = blockIdx.z;
    if (tb > ta) return;
    __shared__ unsigned long long pa[COVIS_TILE * COVIS_LDS_STRIDE];
    __shared__ unsigned long long pb[COVIS_TILE * COVIS_LDS_STRIDE];
    const size_t w0 = (size_t)blockIdx.x * COVIS_SLICE_WORDS;
    const int nwords = (int)(nw - w0 < (size_t)COVIS_SLICE_WORDS ? nw - w0 : (size_t)COVIS_SLICE_WORDS);
    // stage the two panels: consecutive threads read consecutive words of a row; rows past the last camera and
    // words past the row's end read as zero
    for (int e = threadIdx.x; e < COVIS_TILE * COVIS_SLICE_WORDS; e += COVIS_TPB) {
        const int r = e / COVIS_SLICE_WORDS, w = e % COVIS_SLICE_WORDS;
        const int ca = ta * COVIS_TILE + r, cb = tb * COVIS_TILE + r;
        const bool in = w < nwords;
        pa[r * COVIS_LDS_STRIDE + w] = (in && ca < n_cams) ? bits[(size_t)ca * nw + w0 + w] : 0ull;
        pb[r * COVIS_LDS_STRIDE + w] = (in && cb < n_cams) ? bits[(size_t)cb * nw + w0 + w] : 0ull;
    }
    __syncthreads();
    const int i = threadIdx.x / COVIS_TILE, j = threadIdx.x % COVIS_TILE;
    const unsigned long long* ra = pa + i * COVIS_LDS_STRIDE;
    const unsigned long long* rb = pb + j * COVIS_LDS_STRIDE;
    int cnt = 0;
    for (int w = 0; w < nwords; ++w) cnt += __popcll(ra[w] & rb[w]);
    const int a = ta * COVIS_TILE + i, b = tb * COVIS_TILE + j;
    if (cnt == 0 || a >= n_cams || b >= n_cams) return;
    atomicAdd(W + (size_t)a * n_cams + b, cnt);
    if (ta != tb) atomicAdd(W + (size_t)b * n_cams + a, cnt);
}

// span[0 * np + p] / [1 * np + p]: lowest / highest position of point p's active cameras under placement 0,
// [2 * np + p] / [3 * np + p] under placement 1 (initialised to INT_MAX-like / -1 by the launcher).
__global__ __launch_bounds__(COVIS_TPB) void k_covis_span(const int* __restrict__ obs_cam, const int* __restrict__ obs_pt,
                                                          const double* __restrict__ obs_depth, int n_obs, size_t np,
                                                          const int* __restrict__ pos0, const int* __restrict__ pos1,
                                                          int* __restrict__ span) {
    const size_t k = (size_t)blockIdx.x * COVIS_TPB + threadIdx.x;
    if (k >= (size_t)n_obs || !obs_admissible(obs_depth[k])) return;
    const int cam = obs_cam[k];
    const size_t p = (size_t)obs_pt[k];
    const int a0 = pos0[cam], a1 = pos1[cam];
    if (a0 >= 0) { atomicMin(span + p, a0); atomicMax(span + np + p, a0); }
    if (a1 >= 0) { atomicMin(span + 2 * np + p, a1); atomicMax(span + 3 * np + p, a1); }
}

__global__ __launch_bounds__(COVIS_TPB) void k_covis_wide(const int* __restrict__ span, size_t np, int tile_win,
                                                          int* __restrict__ wide) {
    __shared__ int cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * COVIS_TPB + threadIdx.x;
    if (p < np) {
        const int lo0 = span[p], hi0 = span[np + p], lo1 = span[2 * np + p], hi1 = span[3 * np + p];
        if (hi0 >= 0 && hi0 - lo0 + 1 > tile_win) atomicAdd(&cnt[0], 1);
        if (hi1 >= 0 && hi1 - lo1 + 1 > tile_win) atomicAdd(&cnt[1], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(wide + threadIdx.x, cnt[threadIdx.x]);
}

static unsigned covis_blocks(size_t n) { return (unsigned)((n + COVIS_TPB - 1) / COVIS_TPB); }

hipError_t launch_covis_bits(const int* obs_cam, const int* obs_pt, const double* obs_depth, int n_obs, int n_points,
                             unsigned long long* bits, hipStream_t s) {
    if (n_obs <= 0 || n_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_covis_bits, dim3(covis_blocks((size_t)n_obs)), dim3(COVIS_TPB), 0, s, obs_cam, obs_pt, obs_depth,
                       n_obs, covis_row_words(n_points), bits);
    return hipGetLastError();
}

hipError_t launch_covis_count(const unsigned long long* bits, int n_cams, int n_points, int* W, hipStream_t s) {
    const size_t nw = covis_row_words(n_points);
    if (n_cams <= 0 || nw == 0) return hipSuccess;
    const unsigned nt = (unsigned)((n_cams + COVIS_TILE - 1) / COVIS_TILE);
    const unsigned ns = (unsigned)((nw + COVIS_SLICE_WORDS - 1) / COVIS_SLICE_WORDS);
    if (nt > 65535u) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_covis_count, dim3(ns, nt, nt), dim3(COVIS_TPB), 0, s, bits, n_cams, nw, W);
    return hipGetLastError();
}

hipError_t launch_covis_span(const int* obs_cam, const int* obs_pt, const double* obs_depth, int n_obs, int n_points,
                             const int* pos0, const int* pos1, int tile_win, int* span, int* wide, hipStream_t s) {
    hipError_t e = hipMemsetAsync(wide, 0, 2 * sizeof(int), s);
    if (e != hipSuccess || n_obs <= 0 || n_points <= 0) return e;
    const size_t np = (size_t)n_points;
    // lowest positions start at 0x7f7f7f7f (above every position), highest at -1
    for (int h = 0; h < 4 && e == hipSuccess; ++h)
        e = hipMemsetAsync(span + h * np, (h & 1) ? 0xff : 0x7f, np * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_covis_span, dim3(covis_blocks((size_t)n_obs)), dim3(COVIS_TPB), 0, s, obs_cam, obs_pt, obs_depth,
                       n_obs, np, pos0, pos1, span);
    hipLaunchKernelGGL(k_covis_wide, dim3(covis_blocks(np)), dim3(COVIS_TPB), 0, s, span, np, tile_win, wide);
    return hipGetLastError();
}

}  // namespace miba
