// ba_local.hip — the local-window selection of ba_local_window on the device (gfx950).
//
// It works on the camera x point bit matrix of the admissible observations that k_covis_bits builds (ba_covis.hip: a
// camera's row packed into 64-bit words). The weight row is popcount(row a & row center) per camera, the local points
// P the OR of the local cameras' rows, the fixed cameras those with popcount(row a & P) > 0. A point's new index is
// its rank in P: the exclusive scan of P's word popcounts plus the popcount of the lower bits of its word. The kept
// observations (admissible, point in P) are compacted in the caller's order by an exclusive scan of their flags.
// Everything is integer and without atomics. The scans are three plain passes (workgroup-local scan, one workgroup
// over the workgroups' sums with a carry, the offsets added by the consumer): no workgroup waits for another inside
// a launch.
#include "ba_local.h"
#include "ba_obs.h"
#include "ba_scan.h"

namespace miba {

static_assert(LOCAL_TPB == SCAN_TPB, "block_excl (ba_scan.h) scans one workgroup of LOCAL_TPB threads");

__device__ __forceinline__ bool local_has(const unsigned long long* __restrict__ P, unsigned pt) {
    return (P[pt >> 6] >> (pt & 63u)) & 1ull;
}

// one workgroup per camera: consecutive threads read consecutive words of the row and of the mask
__global__ __launch_bounds__(LOCAL_TPB) void k_local_rows(const unsigned long long* __restrict__ bits,
                                                          const unsigned long long* __restrict__ mask, size_t nw,
                                                          int* __restrict__ cnt) {
    __shared__ int sh[LOCAL_TPB / 64];
    const unsigned long long* row = bits + (size_t)blockIdx.x * nw;
    int c = 0;
    for (size_t w = threadIdx.x; w < nw; w += LOCAL_TPB) c += __popcll(row[w] & mask[w]);
    int tot;
    (void)block_excl(c, sh, tot);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

// one thread per word of P: the selected rows are read word-coalesced, one row after the other
__global__ __launch_bounds__(LOCAL_TPB) void k_local_or(const unsigned long long* __restrict__ bits,
                                                        const int* __restrict__ sel, int n_sel, size_t nw,
                                                        unsigned long long* __restrict__ P, int* __restrict__ wcnt) {
    const size_t w = (size_t)blockIdx.x * LOCAL_TPB + threadIdx.x;
    if (w >= nw) return;
    unsigned long long acc = 0ull;
    for (int i = 0; i < n_sel; ++i) acc |= bits[(size_t)sel[i] * nw + w];
    P[w] = acc;
    wcnt[w] = __popcll(acc);
}

// scan, pass 1: out[i] = the exclusive prefix of in[] within the workgroup's LOCAL_TPB items, bsum[block] = their sum
__global__ __launch_bounds__(LOCAL_TPB) void k_local_scan_words(const int* __restrict__ in, size_t n,
                                                                int* __restrict__ out, int* __restrict__ bsum) {
    __shared__ int sh[LOCAL_TPB / 64];
    const size_t i = (size_t)blockIdx.x * LOCAL_TPB + threadIdx.x;
    const int v = i < n ? in[i] : 0;
    int tot;
    const int e = block_excl(v, sh, tot);
    if (i < n) out[i] = e;
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// the same over the observations' keep flags, formed on the fly
__global__ __launch_bounds__(LOCAL_TPB) void k_local_scan_keep(const int* __restrict__ obs_pt,
                                                               const double* __restrict__ obs_depth, size_t n,
                                                               const unsigned long long* __restrict__ P,
                                                               int* __restrict__ out, int* __restrict__ bsum) {
    __shared__ int sh[LOCAL_TPB / 64];
    const size_t k = (size_t)blockIdx.x * LOCAL_TPB + threadIdx.x;
    const int v = (k < n && obs_admissible(obs_depth[k]) && local_has(P, (unsigned)obs_pt[k])) ? 1 : 0;
    int tot;
    const int e = block_excl(v, sh, tot);
    if (k < n) out[k] = e;
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// scan, pass 2 (one workgroup): bsum[nb] becomes its exclusive scan, LOCAL_TPB sums at a time with a carry; the
// grand total goes to *total
__global__ __launch_bounds__(LOCAL_TPB) void k_local_scan_sums(int* __restrict__ bsum, int nb, int* __restrict__ total) {
    __shared__ int sh[LOCAL_TPB / 64];
    int carry = 0;
    for (int base = 0; base < nb; base += LOCAL_TPB) {
        const int j = base + threadIdx.x;
        const int v = j < nb ? bsum[j] : 0;
        int tot;
        const int e = block_excl(v, sh, tot);
        if (j < nb) bsum[j] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// one thread per point: its rank in P = the scanned popcounts of the words before its word + the set bits below it
__global__ __launch_bounds__(LOCAL_TPB) void k_local_points(const unsigned long long* __restrict__ P,
                                                            const int* __restrict__ wrank, const int* __restrict__ bsum,
                                                            int n_points, int* __restrict__ pt_new,
                                                            int* __restrict__ pt_index) {
    const size_t p = (size_t)blockIdx.x * LOCAL_TPB + threadIdx.x;
    if (p >= (size_t)n_points) return;
    const size_t w = p >> 6;
    const unsigned b = (unsigned)(p & 63u);
    const unsigned long long word = P[w];
    if (!((word >> b) & 1ull)) {
        pt_new[p] = -1;
        return;
    }
    const int r = bsum[w / LOCAL_TPB] + wrank[w] + __popcll(word & ((1ull << b) - 1ull));
    pt_new[p] = r;
    pt_index[r] = (int)p;
}

// scan, pass 3 and the scatter: a kept observation goes to the slot its scanned flag gives
__global__ __launch_bounds__(LOCAL_TPB) void k_local_scatter(const int* __restrict__ obs_cam, const int* __restrict__ obs_pt,
                                                             const double* __restrict__ obs_depth, size_t n,
                                                             const unsigned long long* __restrict__ P,
                                                             const int* __restrict__ cam_new, const int* __restrict__ pt_new,
                                                             const int* __restrict__ oscan, const int* __restrict__ bsum,
                                                             int* __restrict__ obs_index, int* __restrict__ sub_cam,
                                                             int* __restrict__ sub_pt) {
    const size_t k = (size_t)blockIdx.x * LOCAL_TPB + threadIdx.x;
    if (k >= n || !obs_admissible(obs_depth[k])) return;
    const int pt = obs_pt[k];
    if (!local_has(P, (unsigned)pt)) return;
    const int pos = bsum[blockIdx.x] + oscan[k];
    obs_index[pos] = (int)k;
    sub_cam[pos] = cam_new[obs_cam[k]];
    sub_pt[pos] = pt_new[pt];
}

hipError_t launch_local_rows(const unsigned long long* bits, const unsigned long long* mask, int n_cams, size_t nw,
                             int* cnt, hipStream_t s) {
    if (n_cams <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_local_rows, dim3((unsigned)n_cams), dim3(LOCAL_TPB), 0, s, bits, mask, nw, cnt);
    return hipGetLastError();
}

hipError_t launch_local_or(const unsigned long long* bits, const int* sel, int n_sel, size_t nw, unsigned long long* P,
                           int* wcnt, hipStream_t s) {
    if (nw == 0) return hipSuccess;
    hipLaunchKernelGGL(k_local_or, dim3((unsigned)local_scan_blocks(nw)), dim3(LOCAL_TPB), 0, s, bits, sel, n_sel, nw, P,
                       wcnt);
    return hipGetLastError();
}

hipError_t launch_local_points(const unsigned long long* P, const int* wcnt, int n_points, size_t nw, int* wrank,
                               int* bsum, int* pt_new, int* pt_index, int* total, hipStream_t s) {
    if (n_points <= 0 || nw == 0) return hipMemsetAsync(total, 0, sizeof(int), s);
    const int nb = local_scan_blocks(nw);
    hipLaunchKernelGGL(k_local_scan_words, dim3((unsigned)nb), dim3(LOCAL_TPB), 0, s, wcnt, nw, wrank, bsum);
    hipLaunchKernelGGL(k_local_scan_sums, dim3(1), dim3(LOCAL_TPB), 0, s, bsum, nb, total);
    hipLaunchKernelGGL(k_local_points, dim3((unsigned)local_scan_blocks((size_t)n_points)), dim3(LOCAL_TPB), 0, s, P,
                       wrank, bsum, n_points, pt_new, pt_index);
    return hipGetLastError();
}

hipError_t launch_local_obs(const int* obs_cam, const int* obs_pt, const double* obs_depth, int n_obs,
                            const unsigned long long* P, const int* cam_new, const int* pt_new, int* oscan, int* bsum,
                            int* obs_index, int* sub_cam, int* sub_pt, int* total, hipStream_t s) {
    if (n_obs <= 0) return hipMemsetAsync(total, 0, sizeof(int), s);
    const size_t n = (size_t)n_obs;
    const int nb = local_scan_blocks(n);
    hipLaunchKernelGGL(k_local_scan_keep, dim3((unsigned)nb), dim3(LOCAL_TPB), 0, s, obs_pt, obs_depth, n, P, oscan, bsum);
    hipLaunchKernelGGL(k_local_scan_sums, dim3(1), dim3(LOCAL_TPB), 0, s, bsum, nb, total);
    hipLaunchKernelGGL(k_local_scatter, dim3((unsigned)nb), dim3(LOCAL_TPB), 0, s, obs_cam, obs_pt, obs_depth, n, P,
                       cam_new, pt_new, oscan, bsum, obs_index, sub_cam, sub_pt);
    return hipGetLastError();
}

}  // namespace miba
