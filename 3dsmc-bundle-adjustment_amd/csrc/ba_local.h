// ba_local.h — launchers of the local-window selection kernels (ba_local.hip, internal). Integer only, no atomics:
// every result is a popcount, an OR or a scan with one fixed order, so the selection is bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace miba {

// threads of every workgroup here, and the items one workgroup scans (one per thread). A scan over n items takes
// ceil(n / LOCAL_TPB) workgroups, whose sums one workgroup scans LOCAL_TPB at a time with a carry: n > LOCAL_TPB
// is the scan's second workgroup, n > LOCAL_TPB^2 the carry's second round.
static constexpr int LOCAL_TPB = 256;

inline int local_scan_blocks(size_t n) { return (int)((n + LOCAL_TPB - 1) / LOCAL_TPB); }

// cnt[a] = popcount(row a & mask) for every camera a of the bit matrix bits[n_cams * nw]; mask[nw] is a row of the
// matrix (the weight row w: mask = row center) or the local points' set P (the fixed cameras: cnt > 0)
hipError_t launch_local_rows(const unsigned long long* bits, const unsigned long long* mask, int n_cams, size_t nw,
                             int* cnt, hipStream_t s);

// P[nw] = the OR of the rows of the n_sel cameras listed in sel; wcnt[nw] = popcount of each word of P
hipError_t launch_local_or(const unsigned long long* bits, const int* sel, int n_sel, size_t nw, unsigned long long* P,
                           int* wcnt, hipStream_t s);

// The points' ranks: the exclusive scan of wcnt[nw] (into wrank[nw], bsum[local_scan_blocks(nw)] scratch), then per
// point of P its rank among P's points: pt_new[n_points] (-1 outside P) and pt_index[rank] = point; total[0] = |P|.
hipError_t launch_local_points(const unsigned long long* P, const int* wcnt, int n_points, size_t nw, int* wrank,
                               int* bsum, int* pt_new, int* pt_index, int* total, hipStream_t s);

// The observations' stable compaction: keep = depth > 1e-15 and the point in P; the flags' exclusive scan
// (oscan[n_obs], bsum[local_scan_blocks(n_obs)] scratch) and the scatter: obs_index[pos] = k, sub_cam[pos] =
// cam_new[obs_cam[k]], sub_pt[pos] = pt_new[obs_pt[k]]; total[1] = observations kept.
hipError_t launch_local_obs(const int* obs_cam, const int* obs_pt, const double* obs_depth, int n_obs,
                            const unsigned long long* P, const int* cam_new, const int* pt_new, int* oscan, int* bsum,
                            int* obs_index, int* sub_cam, int* sub_pt, int* total, hipStream_t s);

}  // namespace miba
