// ba_gmatch.h — ba_guided_match's device side (ba_gmatch.hip, internal): the launches of a call.
//   k_gm_count     one thread per (distinct keypoint range, keypoint): the keypoint's cell (gm_cell_of, clamped into
//                  the border cells), an integer atomicAdd into the range's cell counts.
//   k_gm_offsets   one workgroup per range: the exclusive scan of its cell counts (ba_scan.h) into cell offsets; the
//                  counts are cleared for the scatter.
//   k_gm_scatter   the same threads as k_gm_count: the keypoint's index into its cell's list. The order inside a cell
//                  follows the atomics; no output depends on it (the neighbour key carries the keypoint index,
//                  n_in_window is a count).
//   k_gm_search    one row per lane, the landmark's descriptor in registers (NDW dwords, templated): obs_project,
//                  statuses 1 and 2, the cell rectangle of gm_cell_span, per keypoint of it the two gates, the
//                  descriptor distance (HAMMING xor + popcount, L2_U8 exact int32 by |a|^2 + |b|^2 - 2 a.b on the
//                  packed-byte dot product) and the running top-2 (ba_top2.h); then statuses 3 to 5 and, for a row
//                  that passed them, a 64-bit atomicMin of (d0, row in frame) into the one-to-one table.
//   k_gm_pick      one thread per row: status 6 from the table, status, the per-frame counts by integer atomics.
//   k_gm_begin     one workgroup: the exclusive scan of the frames' accepted counts, match_begin.
//   k_gm_compact   one workgroup per frame: the ordered scan over the frame's rows from match_begin[f], matches.
// Floating point for the projection and the two gates alone; integer atomics alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_gmatch_host.h"

namespace miba {

// rows of a workgroup of k_gm_search: one wave, so that the waves of a small call spread over the device
static constexpr int GMATCH_SEARCH_TPB = 64;

struct GmArgs {
    // the caller's problem on the device
    const double* kp_uv;          // [n_kp * 2]
    const uint8_t* kp_desc;       // [n_kp * desc_bytes], 16-byte aligned
    const double* kp_depth;       // [n_kp], or null: no depth gate
    const double* points;         // [n_points * 3]
    const uint8_t* pt_desc;       // [n_points * desc_bytes], 16-byte aligned
    const double* frame_pose;     // [n_frames * 7]
    const int* frame_range;       // [n_frames * 2]
    const int* cand_begin;        // [n_frames + 1]
    const int* cand_pt;           // [n_rows]
    // the host's layout (GmLayout)
    const int* frame_grid;        // [n_frames]
    const int* grid_range;        // [n_grids * 2]
    const int* grid_kp_begin;     // [n_grids + 1] first slot of a grid in cell_list
    const int* o2o_begin;         // [n_frames + 1] first slot of a frame entry in o2o
    double K[4];
    int width, height, n_frames, n_rows, n_grids, n_binned, kind, desc_bytes;
    int gw, gh, cells;            // the grid: cells across, down, gw * gh
    double inv_cell;              // 1.0 / cell side
    double radius, r2;            // r2 = radius * radius, rounded once
    double min_depth, depth_tol;  // depth_tol <= 0: no gate
    int one_to_one, max_distance;
    float ratio;                  // HAMMING's f32 test
    double ratio2;                // L2_U8's f64 test on the squares
    // work
    int* cell_count;              // [n_grids * cells], zero on entry
    int* cell_off;                // [n_grids * (cells + 1)] slots in cell_list
    int* cell_list;               // [n_binned] keypoint indices inside the range, by cell
    unsigned long long* o2o;      // [o2o slots], all ones on entry
    // out
    int* nn_kp;                   // [n_rows * 2]
    int* nn_dist;                 // [n_rows * 2]
    unsigned char* status;        // [n_rows]
    double* proj;                 // [n_rows * 3]
    int* n_in_window;             // [n_rows]
    int* counts;                  // [n_frames * GMATCH_COUNT], zero on entry
    int* matches;                 // [n_rows * 2] or null
    int* match_begin;             // [n_frames + 1]
};

hipError_t launch_gm_bin(const GmArgs& a, hipStream_t s);      // count, offsets, scatter
hipError_t launch_gm_search(const GmArgs& a, hipStream_t s);   // search, pick
hipError_t launch_gm_compact(const GmArgs& a, hipStream_t s);  // begin, compact (matches may be null)

}  // namespace miba
