// ba_obs.h — which observations count (internal; device and host-only translation units include it).
#pragma once

namespace miba {

// An observation takes part when its measured depth is positive: what the co-visibility bits, the local window's
// compaction and ba_localize's grouping all select by.
#ifdef __HIPCC__
__host__ __device__ __forceinline__
#else
inline
#endif
bool obs_admissible(double depth) { return depth > 1e-15; }

}  // namespace miba
