// ba_loc_group.cpp — ba_loc_group.h: the observations of a window grouped by camera (host code only).
#include "ba_loc_group.h"

#include "ba_obs.h"

namespace miba {

int32_t loc_group(int32_t n_cams, int32_t n_obs, const int32_t* obs_cam, const double* obs_depth, const uint8_t* mask,
                  int32_t* off, int32_t* idx) {
    auto kept = [&](int32_t k) { return obs_admissible(obs_depth[k]) && (!mask || mask[obs_cam[k]]); };
    for (int32_t c = 0; c <= n_cams; ++c) off[c] = 0;
    for (int32_t k = 0; k < n_obs; ++k)
        if (kept(k)) ++off[obs_cam[k] + 1];
    for (int32_t c = 0; c < n_cams; ++c) off[c + 1] += off[c];
    // off[c] is camera c's next free slot while the observations are placed, and its begin again afterwards
    for (int32_t k = 0; k < n_obs; ++k)
        if (kept(k)) idx[off[obs_cam[k]]++] = k;
    for (int32_t c = n_cams; c > 0; --c) off[c] = off[c - 1];
    off[0] = 0;
    return off[n_cams];
}

}  // namespace miba
