// ba_align_sample.h — ba_align's minimal samples (include/ba.h, "Hypotheses"): integer arithmetic on uint64 alone, one
// text for the kernels of ba_align.hip and for the host harness tests/cpp/align_sample_main.cpp, which holds it to
// tests/refalign.py's restatement in Python integers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_ALIGN_HD __host__ __device__ inline
#else
#define BA_ALIGN_HD inline
#endif

namespace miba {

// the splitmix64 finaliser
BA_ALIGN_HD uint64_t align_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// The three distinct indices in [0, n) of hypothesis h of pair j, n >= 3: uniform over the ordered triples. The draws
// take the high 32 bits of a mixed word times the count of indices left ((r >> 32) * m < 2^63 for m < 2^31), and the
// second and third are shifted past the indices already taken, in ascending order.
BA_ALIGN_HD void align_sample(uint64_t seed, uint32_t j, uint32_t h, uint32_t n, uint32_t idx[3]) {
    const uint64_t key = align_mix(seed ^ align_mix((uint64_t)j << 32 | h));
    const uint32_t d0 = (uint32_t)(((align_mix(key + 1) >> 32) * (uint64_t)n) >> 32);
    const uint32_t d1 = (uint32_t)(((align_mix(key + 2) >> 32) * (uint64_t)(n - 1)) >> 32);
    const uint32_t d2 = (uint32_t)(((align_mix(key + 3) >> 32) * (uint64_t)(n - 2)) >> 32);
    const uint32_t i0 = d0;
    const uint32_t i1 = d1 + (d1 >= i0 ? 1u : 0u);
    const uint32_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    uint32_t i2 = d2;
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
    idx[0] = i0; idx[1] = i1; idx[2] = i2;
}

}  // namespace miba
