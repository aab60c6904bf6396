// ba_gmatch_host.h — the host side of ba_guided_match that needs no device (internal): the verdict on the problem and
// the request, the binning grid's geometry, and the de-duplication of equal keypoint ranges. Plain C++ with no HIP
// include, so tests/cpp/gmatch_host_main.cpp exercises it as a stand-alone program under the host sanitizers.
// gm_cell_of / gm_cell_span are also what the kernels of ba_gmatch.hip bin and search with.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ba.h"

#ifdef __HIPCC__
#define GM_HD __host__ __device__ __forceinline__
#else
#define GM_HD inline
#endif

namespace miba {

// threads of a workgroup of every kernel of the stage (ba_scan.h's SCAN_TPB)
static constexpr int GMATCH_TPB = 256;
// per frame entry: counts[GMATCH_COUNT] as ba_gmatch_request.frame_counts
static constexpr int GMATCH_COUNT = 9;
// the smallest default cell
static constexpr int GMATCH_MIN_CELL = 8;
// cells, binned keypoints and one-to-one slots of a call: int32 indices on the device
static constexpr long long GMATCH_MAX_ITEMS = std::numeric_limits<int32_t>::max();
// frame entries of a call: one workgroup of GMATCH_TPB threads each in the compaction, 2^32 threads in a grid
static constexpr long long GMATCH_MAX_FRAMES = (1LL << 32) / GMATCH_TPB;

// The cell of a coordinate along an axis of n cells: floor(x / cell) clamped into [0, n - 1], as x * inv_cell with
// inv_cell = 1.0 / cell. Not a number and everything below the first cell go to cell 0, everything beyond the last
// to n - 1. Monotone in x: a product with a positive constant, floor and the clamp all are.
GM_HD int gm_cell_of(double x, double inv_cell, int n) {
    if (!(x > 0.0)) return 0;
    const double c = floor(x * inv_cell);
    return c >= (double)(n - 1) ? n - 1 : (int)c;
}

// The cells [lo, hi] along one axis that cover every keypoint coordinate k with |k - c| <= r under the window test's
// own rounding. The guard band g = (|c| + r) 2^-40 is a thousand times what the test's roundings can add (DESIGN
// §4.18); the exact test decides inside.
GM_HD void gm_cell_span(double c, double r, double inv_cell, int n, int& lo, int& hi) {
    const double g = (fabs(c) + r) * 0x1p-40;
    lo = gm_cell_of(c - r - g, inv_cell, n);
    hi = gm_cell_of(c + r + g, inv_cell, n);
}

// the default cell side: the smallest power of two >= radius, at least GMATCH_MIN_CELL
inline int gm_default_cell(double radius) {
    int c = GMATCH_MIN_CELL;
    while ((double)c < radius && c < (1 << 30)) c <<= 1;
    return c;
}

struct GmGrid {
    int cell = 0, gw = 0, gh = 0;  // the cell side in pixels, the cells across and down
    long long cells() const { return (long long)gw * gh; }
};
inline GmGrid gm_grid(int32_t width, int32_t height, int32_t cell_px, double radius) {
    GmGrid g;
    g.cell = cell_px > 0 ? cell_px : gm_default_cell(radius);
    g.gw = (int)(((long long)width + g.cell - 1) / g.cell);
    g.gh = (int)(((long long)height + g.cell - 1) / g.cell);
    return g;
}

// The distinct (begin, end) of the frame entries in the order of their first appearance: frame_grid[f] is the entry's
// grid, grid_range its two values, grid_kp_begin the grids' first slot in the binned keypoint lists (n_grids + 1),
// o2o_begin the entries' first slot in the one-to-one table (n_frames + 1; one slot per keypoint of the range).
struct GmLayout {
    std::vector<int32_t> frame_grid, grid_range;
    std::vector<long long> grid_kp_begin, o2o_begin;
    int n_grids() const { return (int)(grid_range.size() / 2); }
};
inline GmLayout gm_layout(const int32_t* frame_range, int32_t n_frames) {
    GmLayout L;
    L.frame_grid.resize((size_t)n_frames);
    L.grid_kp_begin.push_back(0);
    L.o2o_begin.assign((size_t)n_frames + 1, 0);
    std::map<std::pair<int32_t, int32_t>, int32_t> seen;
    for (int32_t f = 0; f < n_frames; ++f) {
        const int32_t b = frame_range[2 * (size_t)f], e = frame_range[2 * (size_t)f + 1];
        const auto it = seen.emplace(std::make_pair(b, e), (int32_t)seen.size());
        if (it.second) {
            L.grid_range.push_back(b);
            L.grid_range.push_back(e);
            L.grid_kp_begin.push_back(L.grid_kp_begin.back() + (e - b));
        }
        L.frame_grid[(size_t)f] = it.first->second;
        L.o2o_begin[(size_t)f + 1] = L.o2o_begin[(size_t)f] + (e - b);
    }
    return L;
}

// The stage's own refusals after the scaffold's four, in the order of include/ba.h. "" when the call may go on.
inline std::string gm_check(const ba_gmatch_problem* p, const ba_gmatch_request* req) {
    if (p->n_kp < 0 || p->n_points < 0 || p->n_frames < 0 || p->n_rows < 0) return "negative sizes";
    if (p->kind != BA_MATCH_HAMMING && p->kind != BA_MATCH_L2_U8)
        return "kind = " + std::to_string(p->kind) + " is neither BA_MATCH_HAMMING nor BA_MATCH_L2_U8";
    if (p->desc_bytes < 4 || p->desc_bytes > BA_MATCH_MAX_BYTES || p->desc_bytes % 4)
        return "desc_bytes = " + std::to_string(p->desc_bytes) + " is not a multiple of 4 in [4, " +
               std::to_string(BA_MATCH_MAX_BYTES) + "]";
    if (p->width < 1 || p->height < 1)
        return "width = " + std::to_string(p->width) + ", height = " + std::to_string(p->height) + ": both must be positive";
    if (!(req->radius > 0.0) || !std::isfinite(req->radius)) return "radius is not a finite positive number";
    if (p->n_frames && (!p->frame_pose || !p->frame_range || !p->cand_begin))
        return "null required buffer (frame_pose / frame_range / cand_begin)";  // (the two lists are read next)
    for (int32_t f = 0; f < p->n_frames; ++f) {
        const int32_t b = p->frame_range[2 * (size_t)f], e = p->frame_range[2 * (size_t)f + 1];
        if (b < 0 || e < b || e > p->n_kp)
            return "frame " + std::to_string(f) + ": the keypoint range [" + std::to_string(b) + ", " + std::to_string(e) +
                   ") is reversed or leaves [0, n_kp = " + std::to_string(p->n_kp) + ")";
    }
    if (p->n_frames) {
        if (p->cand_begin[0] != 0) return "cand_begin[0] = " + std::to_string(p->cand_begin[0]) + " is not 0";
        for (int32_t f = 0; f < p->n_frames; ++f)
            if (p->cand_begin[f + 1] < p->cand_begin[f]) return "cand_begin decreases at frame " + std::to_string(f);
    }
    const int32_t rows = p->n_frames ? p->cand_begin[p->n_frames] : 0;
    if (rows != p->n_rows)
        return "n_rows = " + std::to_string(p->n_rows) + " is not cand_begin[n_frames] (" + std::to_string(rows) + ")";
    if (rows && !p->cand_pt) return "null required buffer (cand_pt)";
    for (int32_t r = 0; r < rows; ++r)
        if (p->cand_pt[r] < 0 || p->cand_pt[r] >= p->n_points)
            return "cand_pt[" + std::to_string(r) + "] = " + std::to_string(p->cand_pt[r]) + " leaves [0, n_points = " +
                   std::to_string(p->n_points) + ")";
    if (p->n_kp && (!p->kp_uv || !p->kp_desc)) return "null required buffer (kp_uv / kp_desc)";
    if (rows && (!p->points || !p->pt_desc)) return "null required buffer (points / pt_desc)";
    if (rows && (!req->nn_kp || !req->nn_dist || !req->status)) return "null required buffer (nn_kp / nn_dist / status)";
    if (req->matches && !req->match_begin) return "null required buffer (match_begin with matches)";
    return "";
}

// The launch limits: the frame entries (asked before the layout is built over them), then, once the grid and the
// layout are known, the rest. "" when the call may go on.
inline std::string gm_frames_limit(const ba_gmatch_problem* p) {
    if (p->n_frames >= GMATCH_MAX_FRAMES)
        return "the grid of " + std::to_string(p->n_frames) + " frames x " + std::to_string(GMATCH_TPB) +
               " threads is above the launch limit of 2^32 threads";
    return "";
}
inline std::string gm_limits(const ba_gmatch_problem* p, const GmGrid& g, const GmLayout& L) {
    if (const std::string m = gm_frames_limit(p); !m.empty()) return m;
    // (gw, gh < 2^31: their product fits 64 bits; times n_grids it need not, so compare by division)
    const long long cells = g.cells();
    if (L.n_grids() && cells > GMATCH_MAX_ITEMS / L.n_grids())
        return "the grid of " + std::to_string(g.gw) + " x " + std::to_string(g.gh) + " cells x " + std::to_string(L.n_grids()) +
               " keypoint ranges is above the limit of 2^31 - 1 cells";
    if (L.grid_kp_begin.back() > GMATCH_MAX_ITEMS)
        return "the " + std::to_string(L.grid_kp_begin.back()) + " binned keypoints are above the limit of 2^31 - 1";
    if (L.o2o_begin.back() > GMATCH_MAX_ITEMS)
        return "the " + std::to_string(L.o2o_begin.back()) + " one-to-one slots are above the limit of 2^31 - 1";
    return "";
}

}  // namespace miba
