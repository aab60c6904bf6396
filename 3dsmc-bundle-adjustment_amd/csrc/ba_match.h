// ba_match.h — ba_match's device side (ba_match.hip, internal): the launches of a call.
//   k_match_nn<KIND>  one workgroup per (pair, query tile of MATCH_QTILE, train slice): the slice's two smallest trains
//                     of every query of the tile under (distance, train index), as two packed keys
//                     distance << 32 | index, into the per-slice table. The slice's trains stream through an LDS tile
//                     of MATCH_TTILE descriptors.
//                       HAMMING  one wave, one query per lane with its descriptor in registers; every lane reads the
//                                same train dwords (a broadcast); xor + popcount per dword.
//                       L2_U8    four waves of MATCH_MFMA queries each: |a - b|^2 = |a'|^2 + |b'|^2 - 2 a'.b' with
//                                a' = a - 128 as i8, the dot products on mfma_i32_16x16x64_i8 (trains on the rows,
//                                queries on the columns, MATCH_KSTEP bytes per instruction), int32 norms.
//                     With cross_check the same kernel runs a second time with the roles swapped: the smallest query
//                     of every train is the first neighbour of the transposed problem (that launch stores the first
//                     key alone).
//   k_match_pick      one thread per row: the slices' keys merged (an integer min, order-free), the acceptance chain,
//                     nn_idx / nn_dist / accept, the per-pair counts by integer atomics.
//   k_match_begin     one workgroup: the exclusive scan of the pairs' accepted counts (ba_scan.h), match_begin.
//   k_match_compact   one workgroup per pair: the ordered scan over the pair's accept from match_begin[j], matches.
// Integer arithmetic and integer atomics alone; the two ratio tests are one f32 / f64 product and comparison per row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace miba {

// queries of a workgroup of k_match_nn (both kinds), trains of an LDS tile, rows / columns of an MFMA tile, bytes of a
// descriptor one MFMA consumes (tests/refmatch.py restates the four: its shapes derive from them)
static constexpr int MATCH_QTILE = 64;
static constexpr int MATCH_TTILE = 64;
static constexpr int MATCH_MFMA = 16;
static constexpr int MATCH_KSTEP = 64;
// threads of a workgroup: HAMMING one wave, L2_U8 MATCH_QTILE / MATCH_MFMA waves
static constexpr int MATCH_TPB_HAMMING = 64;
static constexpr int MATCH_TPB_L2 = 64 * (MATCH_QTILE / MATCH_MFMA);
// the most train slices the host chooses (MIBA_MATCH_SLICES is clamped to it)
static constexpr int MATCH_MAX_SLICES = 64;
// threads of a workgroup of k_match_pick, k_match_begin and k_match_compact (ba_scan.h's SCAN_TPB)
static constexpr int MATCH_SCAN_TPB = 256;
// per pair: counts[MATCH_COUNT] as ba_match_request.pair_counts
static constexpr int MATCH_COUNT = 7;
// "no neighbour": larger than every key of a descriptor
static constexpr unsigned long long MATCH_NONE = ~0ull;

static_assert(MATCH_QTILE == MATCH_TPB_HAMMING, "one query per lane");
static_assert(MATCH_TTILE % MATCH_MFMA == 0 && MATCH_TPB_L2 == 4 * MATCH_TTILE, "four staging threads per train");

struct MatchNnArgs {
    const uint8_t* query;         // the descriptors on the query side of this launch
    const uint8_t* train;         // and on the train side
    const int* range;             // [n_pairs * 4] q_begin, q_end, t_begin, t_end as the caller gave them
    int swap;                     // 1: the roles are swapped (the caller's trains are this launch's queries)
    const int* tile_begin;        // [n_pairs + 1] the pairs' first query tile of this launch
    const long long* row_begin;   // [n_pairs + 1] the pairs' first row of this launch
    int n_pairs, desc_bytes, n_slices;
    int keep;                     // keys stored per query and slice: 2, or 1 (the first neighbour alone)
    unsigned long long* top;      // [rows * n_slices * keep] out
};

struct MatchPickArgs {
    const int* range;             // [n_pairs * 4]
    const long long* row_begin;   // [n_pairs + 1]
    const long long* col_begin;   // [n_pairs + 1] the swapped launch's rows (cross_check)
    const unsigned long long* top;    // [n_rows * n_slices * 2]
    const unsigned long long* cross;  // [n_cols * n_slices] (cross_check): the swapped launch's first keys
    int n_pairs, n_slices, kind, cross_check, max_distance;
    long long n_rows;
    float ratio;                  // HAMMING's f32 test
    double ratio2;                // L2_U8's f64 test on the squares
    int* nn_idx;                  // [n_rows * 2]
    int* nn_dist;                 // [n_rows * 2]
    unsigned char* accept;        // [n_rows]
    int* counts;                  // [n_pairs * MATCH_COUNT], zero on entry
    int* matches;                 // [n_rows * 2]
    int* match_begin;             // [n_pairs + 1]
};

hipError_t launch_match_nn(int kind, const MatchNnArgs& a, int n_tiles, hipStream_t s);
hipError_t launch_match_pick(const MatchPickArgs& a, hipStream_t s);
hipError_t launch_match_begin(const MatchPickArgs& a, hipStream_t s);
hipError_t launch_match_compact(const MatchPickArgs& a, hipStream_t s);

}  // namespace miba
