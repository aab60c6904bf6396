// ba_pts.h — the launcher of ba_refine_points' kernel (ba_pts.hip, internal): the whole structure-only LM loop of one
// point in one row of 16 lanes, four points per wave, a grid of independent points. No floating-point atomics, no LDS
// and no coupling between rows: a point's bits depend on its own observations alone.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_device.h"
#include "ba_kernels.h"

namespace miba {

// lanes of a point's group: one DPP row (the tests' boundaries: observation counts 1, 15, 16, 17, 2 * 16 + 1, ...
// and batches of 1, 3, 4, 5 (groups of a wave), 15, 16, 17 (groups of a workgroup) derive from it)
static constexpr int PTS_LANES = 16;
static constexpr int PTS_TPB = 256;
// points of a workgroup
static constexpr int PTS_PER_WG = PTS_TPB / PTS_LANES;
// per solved point: stats[PTS_STAT] as ba_pts_request.pt_stats
static constexpr int PTS_STAT = 8;

static_assert(PTS_LANES == 16, "dpp_row_sum sums a DPP row of 16 lanes");
static_assert(PTS_TPB % 64 == 0 && 64 % PTS_LANES == 0, "whole groups per wave, whole waves per workgroup");

struct PtsArgs {
    const double* pts;      // [n_points * 3]
    const double* cams;     // [n_cams * 7]
    const double* K;        // [4]
    const double2* uv;      // [n_obs] the caller's arrays, gathered through idx
    const double* depth;    // [n_obs]
    const int* obs_cam;     // [n_obs]
    const int* idx;         // the observations grouped by point (ba_loc_group.h)
    const BlockRec* rec;    // [n_rec] one row's point each
    int n_rec;
    double* xout;           // [n_rec * 3] the solved positions, in the records' order
    double* stats;          // [n_rec * PTS_STAT]
    double* log;            // [log_max_rows * LOG_W] of record log_rec (log_rec < 0: none)
    int log_rec, log_max_rows;
    double initial_radius;
    int jacobi_scaling;
};

inline int pts_workgroups(size_t n_rec) { return (int)((n_rec + PTS_PER_WG - 1) / PTS_PER_WG); }

// c: the Huber parameters and the LM diagonal's clamp (sw_r, sw_d come from BlockRec); prm: the loop's thresholds
// (prm.progress is not used)
hipError_t launch_pts_lm(const PtsArgs& a, const BaConsts& c, const LmParams& prm, hipStream_t s);

}  // namespace miba
