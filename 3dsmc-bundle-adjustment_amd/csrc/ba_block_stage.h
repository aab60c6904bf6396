// ba_block_stage.h — the host driver of a block LM stage (internal): what ba_localize (ba_loc.cpp) and
// ba_refine_points (ba_pts.cpp) do around their own launch. The entities (cameras / points) are the problems; the
// observations are grouped by entity (ba_loc_group.h), every selected entity with enough admissible observations gets
// a BlockRec, the window is copied into the stage's own three device buffers, and the kernels' 8-double statistics and
// one entity's iteration log come back.
#pragma once
#include <cmath>

#include "ba_loc_group.h"
#include "ba_stage.h"

namespace miba {

// the verdict on a request's log_* fields ("" when usable); `field` / `plural` keep each entry point's texts
inline std::string block_log_check(const char* field, int32_t log_id, int32_t n, const char* plural,
                                   int32_t log_max_rows, const double* log_rows) {
    if (log_id >= std::max(n, 1))  // (a zeroed request, log id 0, is legal on an empty window too)
        return std::string(field) + " = " + std::to_string(log_id) + " is out of range (" + std::to_string(n) + " " +
               plural + ")";
    if (log_id >= 0 && (log_max_rows < 0 || (log_max_rows > 0 && !log_rows)))
        return std::string(field) + " is set without a log_rows buffer";
    return "";
}

struct BlockStage {
    static constexpr int STAT = 8;  // LOC_STAT, PTS_STAT

    std::vector<int32_t> idx;     // the observations grouped by entity, the first n_kept entries
    std::vector<BlockRec> rec;    // the problems, in the entities' order
    std::vector<double> stats;    // [rec.size() * STAT], zero until fetch
    int32_t n_kept = 0, n_selected = 0;
    int log_rec = -1, log_max = 0;  // the record of the logged entity (-1: none) and the rows its log has room for
    // the in buffer: cams (7 nc) | pts (3 np) | K (4) | uv (2 no) | depth (no) doubles, then `other` (no) ints
    double *d_cams = nullptr, *d_pts = nullptr, *d_K = nullptr, *d_uv = nullptr, *d_dep = nullptr;
    int* d_other = nullptr;
    // the idx buffer: the records, then the grouped indices
    BlockRec* d_rec = nullptr;
    int* d_idx = nullptr;
    // the out buffer: stats (STAT n) | extra (extra_per_rec n) | log (LOG_W log_max) doubles
    double *d_stats = nullptr, *d_extra = nullptr, *d_log = nullptr;

    size_t n() const { return rec.size(); }

    // Group the observations by key (obs_cam / obs_pt) and make a record for every selected entity with min_n
    // admissible observations or more.
    void group(const ba_problem* p, int32_t n_ent, const int32_t* key, const uint8_t* mask, int32_t min_n,
               int32_t log_id, int32_t log_max_rows, double weight_unpr) {
        std::vector<int32_t> off((size_t)n_ent + 1, 0);
        idx.resize((size_t)p->n_obs);
        n_kept = loc_group(n_ent, p->n_obs, key, p->obs_depth, mask, off.data(), idx.data());
        for (int32_t e = 0; e < n_ent; ++e) {
            if (mask && !mask[e]) continue;
            ++n_selected;
            const int32_t cnt = off[e + 1] - off[e];
            if (cnt < min_n) continue;
            if (e == log_id) log_rec = (int)rec.size();
            const double N = (double)cnt;
            rec.push_back(BlockRec{e, off[e], off[e + 1], 0, std::sqrt(1.0 / N), std::sqrt(weight_unpr / N)});
        }
        log_max = log_rec >= 0 ? log_max_rows : 0;
        stats.assign(n() * STAT, 0.0);
    }

    // The three buffers at their sizes, the window's copy (`other`: the observations' index into the constant side)
    // and the records uploaded, the log cleared.
    int32_t upload(const Stage& stg, const ba_problem* p, BufId in, BufId ix, BufId out, const int32_t* other,
                   size_t extra_per_rec) {
        ba_context* ctx = stg.ctx;
        const size_t nc = (size_t)p->n_cams, np = (size_t)p->n_points, no = (size_t)p->n_obs;
        const size_t in_d = 7 * nc + 3 * np + 4 + 3 * no;
        const size_t in_bytes = 8 * (in_d + 1) + 4 * no, idx_bytes = sizeof(BlockRec) * n() + 4 * (size_t)n_kept;
        const size_t log_bytes = 8 * (size_t)LOG_W * (size_t)log_max;
        if (int32_t rc = stg.ensure(in, in_bytes, "the window's copy")) return rc;
        if (int32_t rc = stg.ensure(ix, idx_bytes, "the grouped observations")) return rc;
        if (int32_t rc = stg.ensure(out, 8 * (STAT + extra_per_rec) * n() + log_bytes, "the statistics")) return rc;
        d_cams = ctx->buf[in].as<double>();
        d_pts = d_cams + 7 * nc;
        d_K = d_pts + 3 * np;
        d_uv = d_K + 4;  // (an even count of doubles before it: 16-byte aligned for the double2 loads)
        if ((7 * nc + 3 * np) & 1) ++d_uv;
        d_dep = d_uv + 2 * no;
        d_other = reinterpret_cast<int*>(d_dep + no);
        d_rec = ctx->buf[ix].as<BlockRec>();
        d_idx = reinterpret_cast<int*>(d_rec + n());
        d_stats = ctx->buf[out].as<double>();
        d_extra = d_stats + STAT * n();
        d_log = d_extra + extra_per_rec * n();
        HIPCHECK(ctx, stg.h2d(d_cams, p->cams, 56 * nc));
        HIPCHECK(ctx, stg.h2d(d_pts, p->points, 24 * np));
        HIPCHECK(ctx, stg.h2d(d_K, p->intr, 32));
        HIPCHECK(ctx, stg.h2d(d_uv, p->obs_uv, 16 * no));
        HIPCHECK(ctx, stg.h2d(d_dep, p->obs_depth, 8 * no));
        HIPCHECK(ctx, stg.h2d(d_other, other, 4 * no));
        HIPCHECK(ctx, stg.h2d(d_rec, rec.data(), sizeof(BlockRec) * n()));
        HIPCHECK(ctx, stg.h2d(d_idx, idx.data(), 4 * (size_t)n_kept));
        if (log_max) HIPCHECK(ctx, hipMemsetAsync(d_log, 0, log_bytes, stg.s));
        return BA_OK;
    }

    // Behind the launch and the stage's own copy back: the statistics and the log fetched, the stream drained, the
    // kernel's time between ev[0] and ev[1] taken. *log_rows_out: the rows the logged entity's log has, of which the
    // first min(rows, log_max) are written to log_rows.
    int32_t fetch(const Stage& stg, hipEvent_t* ev, float* lm_ms, double* log_rows, int32_t* log_rows_out) {
        ba_context* ctx = stg.ctx;
        std::vector<double> log((size_t)LOG_W * (size_t)log_max);
        HIPCHECK(ctx, stg.d2h(stats.data(), d_stats, 8 * STAT * n()));
        HIPCHECK(ctx, stg.d2h(log.data(), d_log, 8 * log.size()));
        HIPCHECK(ctx, hipStreamSynchronize(stg.s));
        (void)hipEventElapsedTime(lm_ms, ev[0], ev[1]);
        if (log_rec >= 0) {
            // iterations + 1 rows; none when the evaluation at the given x failed (the loop never started)
            const double* st = &stats[STAT * (size_t)log_rec];
            *log_rows_out = (int)st[7] == MSG_EVAL_FAIL ? 0 : (int32_t)st[3] + 1;
            const size_t rows = (size_t)std::min(*log_rows_out, log_max);
            if (rows) std::memcpy(log_rows, log.data(), 8 * (size_t)LOG_W * rows);
        }
        return BA_OK;
    }

    // the caller's per-entity statistics: a solved entity's record, zeros with termination -1 for every other
    void scatter_stats(double* out, size_t n_ent) const {
        if (!out) return;
        for (size_t e = 0; e < n_ent; ++e) {
            double* st = out + STAT * e;
            for (int k = 0; k < STAT; ++k) st[k] = 0.0;
            st[6] = -1.0;
        }
        for (size_t g = 0; g < n(); ++g) std::memcpy(out + STAT * (size_t)rec[g].id, &stats[STAT * g], 8 * STAT);
    }

    // the counts of ba_loc_info / ba_pts_info
    template <class Info>
    void tally(Info& full) const {
        full.n_selected = n_selected;
        full.n_solved = (int32_t)n();
        for (size_t g = 0; g < n(); ++g) {
            const int term = (int)stats[STAT * g + 6];
            if (term == BA_CONVERGENCE) ++full.n_convergence;
            else if (term == BA_NO_CONVERGENCE) ++full.n_no_convergence;
            else ++full.n_failure;
            full.max_iterations = std::max(full.max_iterations, (int32_t)stats[STAT * g + 3]);
        }
    }
};

}  // namespace miba
