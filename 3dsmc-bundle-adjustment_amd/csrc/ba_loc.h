// ba_loc.h — the launcher of ba_localize's kernel (ba_loc.hip, internal): the whole pose-only LM loop of one camera in
// one workgroup, a grid of independent cameras. No floating-point atomics and no coupling between workgroups: a
// camera's bits depend on its own observations alone.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_device.h"
#include "ba_kernels.h"

namespace miba {

// threads of a workgroup (B in the tests: observation counts 1, B - 1, B, B + 1, 4 B + 1 are its boundaries)
static constexpr int LOC_TPB = 256;
// per workgroup: stats[LOC_STAT] as ba_loc_request.cam_stats
static constexpr int LOC_STAT = 8;

struct LocArgs {
    double* cams;           // [n_cams * 7], the solved poses written in place
    const double* pts;      // [n_points * 3]
    const double* K;        // [4]
    const double2* uv;      // [n_obs] the caller's arrays, gathered through idx
    const double* depth;    // [n_obs]
    const int* obs_pt;      // [n_obs]
    const int* idx;         // the observations grouped by camera (ba_loc_group.h)
    const BlockRec* wg;     // [n_wg] one workgroup's camera each
    double* stats;          // [n_wg * LOC_STAT]
    double* log;            // [log_max_rows * LOG_W] of workgroup log_wg (log_wg < 0: none)
    int log_wg, log_max_rows;
    double initial_radius;
    int jacobi_scaling;
};

// c: the Huber parameters and the LM diagonal's clamp (sw_r, sw_d come from BlockRec); prm: the loop's thresholds
// (prm.progress is not used)
hipError_t launch_loc_lm(const LocArgs& a, const BaConsts& c, const LmParams& prm, int n_wg, hipStream_t s);

}  // namespace miba
