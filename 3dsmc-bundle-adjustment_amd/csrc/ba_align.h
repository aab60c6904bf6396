// ba_align.h — ba_align's device side (ba_align.hip, internal): the two launches of a call.
//   k_align_hyp   one workgroup per pair and block of ALIGN_TPB hypotheses, one hypothesis per lane: sample, fit on
//                 registers, score against the pair's correspondences staged through LDS in tiles of ALIGN_TILE
//                 (structure of arrays; every lane reads the same address, a broadcast). An integer count per lane,
//                 no reduction, no atomic.
//   k_align_pick  one workgroup per pair: the argmax with the smallest-h tie (an integer reduction), the winner's
//                 model recomputed, the refit rounds (fixed-shape tree sums over the inliers, the fit on one lane),
//                 the mask, the statistics and the pose.
// No floating-point atomics and no coupling between workgroups: a pair's bits depend on its own correspondences, the
// seed and its index alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace miba {

// hypotheses of a workgroup of k_align_hyp, threads of a workgroup of k_align_pick (the tests' hypothesis counts 1,
// 63, 64, 65, 255, 256, 257, 513 derive from it and from the wave's 64 lanes)
static constexpr int ALIGN_TPB = 256;
// correspondences of an LDS tile (the tests' pair sizes ALIGN_TILE - 1, ALIGN_TILE, ALIGN_TILE + 1, 2 ALIGN_TILE + 1
// derive from it): 6 arrays of ALIGN_TILE doubles, 12 KB
static constexpr int ALIGN_TILE = 256;
// per pair: stats[ALIGN_STAT] as ba_align_request.pair_stats ([7], k_needed, is the host's)
static constexpr int ALIGN_STAT = 8;

static_assert(ALIGN_TPB % 64 == 0 && ALIGN_TILE % 64 == 0, "whole waves");

struct AlignArgs {
    const int* pair_begin;  // [n_pairs + 1]
    const double* p1;       // [n_corr * 3]
    const double* p2;       // [n_corr * 3]
    int n_pairs, n_hyp, refit;
    unsigned long long seed;
    double thr2, min_cross2;  // the squares the comparisons are made on
    int* hyp_count;           // [n_pairs * n_hyp]
    double* poses;            // [n_pairs * 7]
    double* stats;            // [n_pairs * ALIGN_STAT]
    unsigned char* inlier;    // [n_corr]
};

inline int align_hyp_blocks(int n_hyp) { return (n_hyp + ALIGN_TPB - 1) / ALIGN_TPB; }

hipError_t launch_align_hyp(const AlignArgs& a, hipStream_t s);
hipError_t launch_align_pick(const AlignArgs& a, hipStream_t s);

}  // namespace miba
