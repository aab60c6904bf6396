// ba_resid.h — launcher of the residual report kernels (ba_resid.hip, internal).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_kernels.h"

namespace miba {

// Internal width of a block's partial statistics: the six values of BA_RES_STAT_N, then what only the window
// totals need.
//   [0] admissible  [1] with a BA_RES_OUTLIER bit  [2] sum du^2 + dv^2  [3] max hypot(du, dv)  [4] sum (depth - z)^2
//   [5] sum obs_cost  [6] BA_RES_BEHIND  [7] BA_RES_REPROJ  [8] BA_RES_DEPTH  [9] BA_RES_HUBER_REPR
//   [10] BA_RES_HUBER_UNPR  [11] max |depth - z|
// Counts are kept as doubles (exact below 2^53). [2], [3], [4], [11] run over the projected observations only.
static constexpr int RES_PART_N = 12;
// totals: the RES_PART_N window values, then the IntrinsicsPrior cost
static constexpr int RES_TOTALS_N = 16;
static constexpr int RES_TOT_PRIOR = 12;

struct ResThresholds {
    double max_reproj;            // pixels
    double depth_abs, depth_rel;  // |depth - z| > depth_abs + depth_rel * depth
    int reproj_on, depth_on;
};

struct ResBufs {
    // point-major, one entry per admissible observation
    double* po_err;   // [n_adm * 4]
    double* po_cost;  // [n_adm]
    int* po_flags;    // [n_adm]
    // the caller's observation order (all three nullptr: not wanted)
    double* obs_err;  // [n_obs * 4]
    double* obs_cost; // [n_obs]
    int* obs_flags;   // [n_obs]
    double* point_stats;  // [n_points * 6], the caller's point order (nullptr: not wanted)
    double* seg_part;     // [n_seg * RES_PART_N]
    double* cam_stats;    // [n_cams * 6]
    double* totals;       // [RES_TOTALS_N]
};

// The whole report at the parameters a prepare left in slot 0 of P. Enqueues only; no launch has an empty grid.
hipError_t launch_resid(const DevProblem& P, const BaConsts& c, const PrepRaw& R, int n_points,
                        const ResThresholds& t, const ResBufs& b, hipStream_t s);

}  // namespace miba
