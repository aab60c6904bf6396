// ba_top2.h — the running two smallest under a packed key, shared by ba_match.hip and ba_gmatch.hip (device code,
// internal). A key is distance << 32 | index: the unsigned order of the keys is the lexicographic order
// (distance, index), so the two smallest keys are the two nearest neighbours with the smaller index first among equal
// distances, whatever order the keys arrive in.
#pragma once
#include <hip/hip_runtime.h>

namespace miba {

// "no neighbour": larger than every key of a descriptor
static constexpr unsigned long long TOP2_NONE = ~0ull;

__device__ __forceinline__ unsigned long long top2_key(unsigned dist, unsigned index) {
    return (unsigned long long)dist << 32 | index;
}
__device__ __forceinline__ unsigned top2_dist(unsigned long long key) { return (unsigned)(key >> 32); }
__device__ __forceinline__ unsigned top2_index(unsigned long long key) { return (unsigned)key; }

// the running top-2 under the packed key: k0 < k1 always (the keys of one query are distinct by their index)
__device__ __forceinline__ void top2_push(unsigned long long key, unsigned long long& k0, unsigned long long& k1) {
    const unsigned long long hi = key > k0 ? key : k0;
    k0 = key < k0 ? key : k0;
    k1 = hi < k1 ? hi : k1;
}
__device__ __forceinline__ void top2_merge(unsigned long long b0, unsigned long long b1, unsigned long long& k0,
                                           unsigned long long& k1) {
    const unsigned long long hi = b0 > k0 ? b0 : k0, lo1 = b1 < k1 ? b1 : k1;
    k0 = b0 < k0 ? b0 : k0;
    k1 = hi < lo1 ? hi : lo1;
}

// the largest j in [0, n) with begin[j] <= x (begin is non-decreasing, begin[0] <= x < begin[n])
template <class T>
__device__ __forceinline__ int owner_of(const T* begin, int n, T x) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (begin[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace miba
