// ba_loc_group.h — the grouping of a window's observations by camera for ba_localize (ba_loc_group.cpp, host only,
// internal).
#pragma once
#include <cstdint>

namespace miba {

// A stable counting sort of the observations by camera. An observation is kept when it is admissible (depth > 1e-15)
// and its camera is selected (mask == nullptr: every camera; else mask[cam] != 0); the kept observations of camera c
// are idx[off[c] .. off[c + 1]), in the caller's order. off has n_cams + 1 entries, idx room for n_obs; the return
// value is the number kept (off[n_cams]). The indices must be in range (the caller checks them).
int32_t loc_group(int32_t n_cams, int32_t n_obs, const int32_t* obs_cam, const double* obs_depth, const uint8_t* mask,
                  int32_t* off, int32_t* idx);

}  // namespace miba
