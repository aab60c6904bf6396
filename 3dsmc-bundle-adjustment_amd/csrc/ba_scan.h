// ba_scan.h — the block scan the integer passes share (ba_dplan.hip, ba_local.hip; device code, internal).
#pragma once
#include <hip/hip_runtime.h>

namespace miba {

static constexpr int SCAN_TPB = 256;  // threads of a scanning workgroup (four waves of 64)

// exclusive scan of one int per thread over the block (SCAN_TPB threads, all of them call); total = the block's sum;
// sh[SCAN_TPB / 64] is LDS scratch, free for reuse when the call returns
__device__ inline int block_excl(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < SCAN_TPB / 64; ++j) {
        const int s = sh[j];
        off += j < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + x - v;
}

}  // namespace miba
