// ba_match.cpp — ba_match of include/ba.h: batched 2-nearest-neighbour descriptor matching with the ratio test (the
// kernels of ba_match.hip: the slices' two nearest trains of every query, the merge with the acceptance chain, the
// ordered compaction). A stage beside the LM loop like ba_align: it works on device buffers of its own (B_MATCH_*), so
// nothing the plan or the LM loop reads is written. The host validates, lays the pairs out as query tiles, chooses the
// slice count, uploads, launches and reads back; there is no host round trip between the launches.
#include "ba_match.h"
#include "ba_stage.h"

#include <limits>

using namespace miba;

static_assert(MATCH_COUNT == BA_MATCH_COUNT_N, "the kernel writes the header's record width");
static_assert(BA_MATCH_MAX_BYTES % MATCH_KSTEP == 0, "the longest descriptor is whole k-steps");

namespace {

std::string range_text(int32_t j, const char* side, int32_t b, int32_t e, int32_t n) {
    return "pair " + std::to_string(j) + ": the " + side + " range [" + std::to_string(b) + ", " + std::to_string(e) +
           ") is reversed or leaves [0, n_" + side + " = " + std::to_string(n) + ")";
}

std::string match_check(ba_context* ctx, const ba_match_problem* p, const ba_match_request* req, const ba_match_info* info) {
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_MATCH)); !m.empty()) return m;
    if (p->n_query < 0 || p->n_train < 0 || p->n_pairs < 0 || p->n_rows < 0) return "negative sizes";
    if (p->kind != BA_MATCH_HAMMING && p->kind != BA_MATCH_L2_U8)
        return "kind = " + std::to_string(p->kind) + " is neither BA_MATCH_HAMMING nor BA_MATCH_L2_U8";
    if (p->desc_bytes < 4 || p->desc_bytes > BA_MATCH_MAX_BYTES || p->desc_bytes % 4)
        return "desc_bytes = " + std::to_string(p->desc_bytes) + " is not a multiple of 4 in [4, " +
               std::to_string(BA_MATCH_MAX_BYTES) + "]";
    if (p->n_pairs && !p->pair_range) return "null required buffer (pair_range)";  // (the ranges are read next)
    int64_t rows = 0, cols = 0;
    for (int32_t j = 0; j < p->n_pairs; ++j) {
        const int32_t* r = p->pair_range + 4 * (size_t)j;
        if (r[0] < 0 || r[1] < r[0] || r[1] > p->n_query) return range_text(j, "query", r[0], r[1], p->n_query);
        if (r[2] < 0 || r[3] < r[2] || r[3] > p->n_train) return range_text(j, "train", r[2], r[3], p->n_train);
        rows += r[1] - r[0];
        if (r[1] > r[0]) cols += r[3] - r[2];
    }
    if (rows != p->n_rows)
        return "n_rows = " + std::to_string(p->n_rows) + " is not the sum of the pairs' query counts (" + std::to_string(rows) + ")";
    if ((rows && !p->query) || (cols && !p->train)) return "null required buffer (query / train)";
    if (rows && (!req->nn_idx || !req->nn_dist)) return "null required buffer (nn_idx / nn_dist)";
    if (req->matches && !req->match_begin) return "null required buffer (match_begin with matches)";
    return "";
}

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" int32_t ba_match(ba_context* ctx, const ba_match_problem* p, const ba_match_request* req, ba_match_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_match", ctx->stream};
    if (const std::string m = match_check(ctx, p, req, info); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    const size_t np = (size_t)p->n_pairs, nr = (size_t)p->n_rows;
    const bool cross = req->cross_check != 0;
    const float ratio = req->ratio > 0.f ? req->ratio : 0.7f;

    // The pairs as query tiles, for the launch proper and for the swapped one (cross_check: the trains as queries).
    // [0] row_begin, [1] col_begin; tile_begin likewise.
    std::vector<long long> begin[2];
    std::vector<int> tile_begin[2];
    long long tiles[2] = {0, 0}, max_tt[2] = {0, 0};
    for (int o = 0; o < 2; ++o) {
        begin[o].assign(np + 1, 0);
        tile_begin[o].assign(np + 1, 0);
    }
    for (size_t j = 0; j < np; ++j) {
        const int32_t* r = p->pair_range + 4 * j;
        const long long n[2] = {r[1] - r[0], r[3] - r[2]};
        for (int o = 0; o < 2; ++o) {
            begin[o][j + 1] = begin[o][j] + n[o];
            tiles[o] += (n[o] + MATCH_QTILE - 1) / MATCH_QTILE;
            max_tt[o] = std::max(max_tt[o], (n[1 - o] + MATCH_TTILE - 1) / MATCH_TTILE);
            tile_begin[o][j + 1] = (int)std::min<long long>(tiles[o], std::numeric_limits<int32_t>::max());
        }
    }
    const size_t nc = (size_t)begin[1][np];

    // The slices: enough workgroups that one pair of a few hundred descriptors still spreads over the device, no more
    // than the longest train range has LDS tiles. Any count gives the same bits.
    const Settings st = read_settings();
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (!ctx->match_cus)
        HIPCHECK(ctx, hipDeviceGetAttribute(&ctx->match_cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const int cus = ctx->match_cus;
    long long slices = 1;
    if (st.match_slices > 0) {
        slices = std::min(st.match_slices, MATCH_MAX_SLICES);
    } else if (tiles[0]) {
        const long long want = (4LL * cus + tiles[0] - 1) / tiles[0];
        slices = std::max(1LL, std::min({want, max_tt[0], (long long)MATCH_MAX_SLICES}));
    }
    // The launch limit: a grid's threads (workgroups x threads of a workgroup) must stay below 2^32, which is 2^26
    // workgroups of HAMMING's one wave and 2^24 of L2_U8's four, far below 2^31 workgroups. k_match_compact's grid is
    // one workgroup of SCAN_TPB per pair.
    const long long tpb = p->kind == BA_MATCH_HAMMING ? MATCH_TPB_HAMMING : MATCH_TPB_L2;
    const long long grid_tiles = std::max(tiles[0], cross ? tiles[1] : 0);
    const long long launch_max = (long long)std::numeric_limits<uint32_t>::max();
    if (grid_tiles * slices * tpb > launch_max)
        return stg.invalid("the grid of " + std::to_string(grid_tiles) + " query tiles x " + std::to_string(slices) +
                           " train slices x " + std::to_string(tpb) + " threads is above the launch limit of 2^32 threads");
    if ((long long)np * MATCH_SCAN_TPB > launch_max)
        return stg.invalid("the grid of " + std::to_string(np) + " pairs x " + std::to_string(MATCH_SCAN_TPB) +
                           " threads is above the launch limit of 2^32 threads");

    ba_match_info full{};
    full.struct_size = (int32_t)sizeof(ba_match_info);
    full.n_pairs = p->n_pairs;
    full.n_rows = p->n_rows;
    full.kind = p->kind;
    float kernels_ms = 0.f;

    if (np) {
        HIPCHECK(ctx, stg.events(ctx->match_ev, 2));
        hipStream_t s = stg.s;
        const size_t db = (size_t)p->desc_bytes, S = (size_t)slices;
        // in: row_begin | col_begin (n_pairs + 1 each, 8 bytes), then pair_range (4 n_pairs) | the two tile_begin
        // (n_pairs + 1 each) ints, then the query and the train descriptors at 16-byte offsets
        const size_t o_range = 16 * (np + 1), o_tile = o_range + 16 * np, o_q = up16(o_tile + 8 * (np + 1));
        const size_t o_t = o_q + up16((size_t)p->n_query * db);
        const size_t in_bytes = o_t + up16((size_t)p->n_train * db);
        // top: the launch's table, the swapped launch's after it
        // (the swapped launch keeps the first neighbour alone: one key per train and slice)
        const size_t top_n = nr * S * 2, cross_n = cross ? nc * S : 0;
        // out: nn_idx | nn_dist | matches (2 n_rows each) | match_begin (n_pairs + 1) | counts ints, then accept
        const size_t out_i = 6 * nr + (np + 1) + MATCH_COUNT * np;
        if (int32_t rc = stg.ensure(B_MATCH_IN, in_bytes, "the descriptors' copy")) return rc;
        if (int32_t rc = stg.ensure(B_MATCH_TOP, 8 * (top_n + cross_n), "the slices' neighbour tables")) return rc;
        if (int32_t rc = stg.ensure(B_MATCH_OUT, 4 * out_i + nr, "the neighbours and the matches")) return rc;
        char* d_in = ctx->buf[B_MATCH_IN].as<char>();
        long long* d_row = reinterpret_cast<long long*>(d_in);
        long long* d_col = d_row + (np + 1);
        int* d_range = reinterpret_cast<int*>(d_in + o_range);
        int* d_tile = reinterpret_cast<int*>(d_in + o_tile);
        int* d_ctile = d_tile + (np + 1);
        uint8_t* d_q = reinterpret_cast<uint8_t*>(d_in + o_q);
        uint8_t* d_t = reinterpret_cast<uint8_t*>(d_in + o_t);
        unsigned long long* d_top = ctx->buf[B_MATCH_TOP].as<unsigned long long>();
        unsigned long long* d_cross = d_top + top_n;
        int* d_idx = ctx->buf[B_MATCH_OUT].as<int>();
        int* d_dist = d_idx + 2 * nr;
        int* d_matches = d_dist + 2 * nr;
        int* d_mbegin = d_matches + 2 * nr;
        int* d_counts = d_mbegin + (np + 1);
        unsigned char* d_accept = reinterpret_cast<unsigned char*>(d_counts + MATCH_COUNT * np);
        HIPCHECK(ctx, stg.h2d(d_row, begin[0].data(), 8 * (np + 1)));
        HIPCHECK(ctx, stg.h2d(d_col, begin[1].data(), 8 * (np + 1)));
        HIPCHECK(ctx, stg.h2d(d_range, p->pair_range, 16 * np));
        HIPCHECK(ctx, stg.h2d(d_tile, tile_begin[0].data(), 4 * (np + 1)));
        HIPCHECK(ctx, stg.h2d(d_ctile, tile_begin[1].data(), 4 * (np + 1)));
        if (p->query) HIPCHECK(ctx, stg.h2d(d_q, p->query, (size_t)p->n_query * db));
        if (p->train) HIPCHECK(ctx, stg.h2d(d_t, p->train, (size_t)p->n_train * db));
        HIPCHECK(ctx, hipMemsetAsync(d_counts, 0, 4 * MATCH_COUNT * np, s));

        MatchNnArgs a{};
        a.query = d_q; a.train = d_t; a.range = d_range; a.swap = 0;
        a.tile_begin = d_tile; a.row_begin = d_row;
        a.n_pairs = p->n_pairs; a.desc_bytes = p->desc_bytes; a.n_slices = (int)slices;
        a.top = d_top; a.keep = 2;
        MatchPickArgs k{};
        k.range = d_range; k.row_begin = d_row; k.col_begin = d_col; k.top = d_top; k.cross = d_cross;
        k.n_pairs = p->n_pairs; k.n_slices = (int)slices; k.kind = p->kind; k.cross_check = cross ? 1 : 0;
        k.max_distance = std::max(req->max_distance, 0);
        k.n_rows = (long long)nr;
        k.ratio = ratio; k.ratio2 = (double)ratio * (double)ratio;
        k.nn_idx = d_idx; k.nn_dist = d_dist; k.accept = d_accept; k.counts = d_counts;
        k.matches = req->matches ? d_matches : nullptr; k.match_begin = d_mbegin;
        const bool compact = req->matches || req->match_begin;
        HIPCHECK(ctx, hipEventRecord(ctx->match_ev[0], s));
        if (tiles[0]) HIPCHECK(ctx, launch_match_nn(p->kind, a, (int)tiles[0], s));
        if (cross && tiles[1] && nr) {
            // the transposed problem: the first neighbour of a train among the queries is the cross-check's winner
            MatchNnArgs c = a;
            c.query = d_t; c.train = d_q; c.swap = 1;
            c.tile_begin = d_ctile; c.row_begin = d_col; c.top = d_cross; c.keep = 1;
            HIPCHECK(ctx, launch_match_nn(p->kind, c, (int)tiles[1], s));
        }
        HIPCHECK(ctx, launch_match_pick(k, s));
        if (compact) {
            HIPCHECK(ctx, launch_match_begin(k, s));
            HIPCHECK(ctx, launch_match_compact(k, s));
        }
        HIPCHECK(ctx, hipEventRecord(ctx->match_ev[1], s));

        std::vector<int32_t> counts(MATCH_COUNT * np);
        HIPCHECK(ctx, stg.d2h(counts.data(), d_counts, 4 * MATCH_COUNT * np));
        HIPCHECK(ctx, stg.d2h(req->nn_idx, d_idx, 8 * nr));
        HIPCHECK(ctx, stg.d2h(req->nn_dist, d_dist, 8 * nr));
        if (req->accept) HIPCHECK(ctx, stg.d2h(req->accept, d_accept, nr));
        if (req->match_begin) HIPCHECK(ctx, stg.d2h(req->match_begin, d_mbegin, 4 * (np + 1)));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&kernels_ms, ctx->match_ev[0], ctx->match_ev[1]);
        long long n_matches = 0;
        for (size_t j = 0; j < np; ++j) n_matches += counts[MATCH_COUNT * j + 2];
        full.n_matches = (int32_t)n_matches;
        if (req->matches && n_matches) {  // (only the accepted rows' part of the list is defined)
            HIPCHECK(ctx, stg.d2h(req->matches, d_matches, 8 * (size_t)n_matches));
            HIPCHECK(ctx, hipStreamSynchronize(s));
        }
        if (req->pair_counts) std::memcpy(req->pair_counts, counts.data(), 4 * MATCH_COUNT * np);
    } else if (req->match_begin) {
        req->match_begin[0] = 0;
    }

    full.time_kernels_ms = kernels_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
