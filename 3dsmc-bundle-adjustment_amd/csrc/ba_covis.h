// ba_covis.h — launchers of the co-visibility kernels (ba_covis.hip, internal). Integer only: bit sets, popcounts and
// integer atomics, so every result is bitwise reproducible whatever order the workgroups run in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ba_problem;  // include/ba.h

namespace miba {

// k_covis_count: one workgroup takes a COVIS_TILE x COVIS_TILE tile of camera pairs and COVIS_SLICE_WORDS 64-bit
// words (64 points each) of the two cameras' rows of the bit matrix
static constexpr int COVIS_TILE = 16;
static constexpr int COVIS_SLICE_WORDS = 128;

// 64-bit words of one camera's row of the bit matrix
inline size_t covis_row_words(int n_points) { return ((size_t)n_points + 63) / 64; }

// bits[n_cams * covis_row_words(n_points)] (zeroed by the caller): bit pt of camera cam's row set for every
// observation with depth > 1e-15. The indices must be in range (the caller checks them).
hipError_t launch_covis_bits(const int* obs_cam, const int* obs_pt, const double* obs_depth, int n_obs, int n_points,
                             unsigned long long* bits, hipStream_t s);

// W[n_cams * n_cams] (zeroed by the caller) += popcount(row a & row b), both triangles and the diagonal.
hipError_t launch_covis_count(const unsigned long long* bits, int n_cams, int n_points, int* W, hipStream_t s);

// Points whose active cameras span more than tile_win positions, under two placements of the cameras: pos[0] /
// pos[1][n_cams] give a camera's position among the active ones (-1: not active). span[4 * n_points] is scratch
// (lowest / highest position per point and placement), wide[2] receives the two counts.
hipError_t launch_covis_span(const int* obs_cam, const int* obs_pt, const double* obs_depth, int n_obs, int n_points,
                             const int* pos0, const int* pos1, int tile_win, int* span, int* wide, hipStream_t s);

// The bit matrix of a window on the device, for ba_covisibility and ba_local_window (ba_covis.cpp). The caller has
// sized B_COVIS_OBS to covis_obs_bytes and B_COVIS_BITS to covis_bits_bytes; the window's depths | camera indices |
// point indices are uploaded into the first, `start` is recorded (the caller's timed interval opens with the clear),
// the second is cleared and k_covis_bits run. A BA_* code; the HIP text is in the context's error.
struct Stage;
struct CovisBits { double* dep; int *cam, *pt; unsigned long long* bits; };
inline size_t covis_obs_bytes(size_t n_obs) { return 16 * (n_obs > 1 ? n_obs : 1); }
inline size_t covis_bits_bytes(size_t n_cams, size_t nw) { return 8 * (n_cams * nw > 1 ? n_cams * nw : 1); }
int32_t covis_upload_bits(const Stage& stg, const ba_problem* p, hipEvent_t start, CovisBits& b);

}  // namespace miba
