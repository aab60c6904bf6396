// ba_order.h — the camera ordering of a window from its co-visibility weights (ba_order.cpp, host only, internal).
#pragma once
#include <cstdint>
#include <vector>

namespace miba {

struct CamOrder {
    std::vector<int32_t> order;  // [n_cams]: order[k] = the camera placed k-th (the candidate, before acceptance)
    int n_active = 0;            // cameras with an admissible observation, the gauge camera apart
    int n_edges = 0;             // co-visible pairs of active cameras
    int n_components = 0;        // connected components of the active cameras' graph
    int band_before = 0;         // max a - fc[a] over the active cameras as given (ba_summary.camera_band)
    int band_after = 0;          // the same with the cameras placed as `order` says
};

// Reverse Cuthill-McKee over the active cameras of the n_cams x n_cams co-visibility weights W (row-major,
// symmetric; W[i][i] = points camera i sees): nodes are the cameras with W[i][i] > 0 and i != fixed_cam, an edge
// where W[i][j] > 0. Per component: start at the unvisited node of lowest (degree, index), breadth-first, each
// node's unvisited neighbours appended sorted by (degree, index), the component's list reversed; the components in
// the order they were started; then the gauge camera and the cameras without an admissible observation, in index
// order. Integer only, deterministic.
void covis_order(const int32_t* W, int n_cams, int fixed_cam, CamOrder& out);
// The same with a set of constant cameras (cam_const[n_cams], non-zero = constant; nullptr: none) treated as the gauge
// camera is: not nodes, placed after the active cameras in index order.
void covis_order(const int32_t* W, int n_cams, int fixed_cam, const uint8_t* cam_const, CamOrder& out);

// max a - fc[a] over the first n_active entries of `order`, fc[a] = the lowest position of a camera co-visible with
// the camera at position a.
int covis_band(const int32_t* W, int n_cams, const int32_t* order, int n_active);

}  // namespace miba
