// ba_pts.cpp — ba_refine_points of include/ba.h: structure-only LM of the selected points against the window's
// constant cameras and intrinsics (the kernel of ba_pts.hip, one row of 16 lanes per point; the observations grouped
// by point on the host with ba_localize's counting sort, ba_loc_group.cpp).
// A stage beside the LM loop like ba_localize: it works on device buffers of its own (B_PTS_*), so nothing the plan
// or the LM loop reads is written.
#include "ba_pts.h"
#include "ba_loc_group.h"
#include "ba_stage.h"

#include <cmath>

using namespace miba;

static_assert(PTS_STAT == BA_PTS_STAT_N && LOG_W == BA_LOG_WIDTH, "the kernel writes the header's record widths");

namespace {

std::string pts_check(ba_context* ctx, const ba_problem* p, const ba_pts_request* req, const ba_pts_info* info) {
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_PTS)); !m.empty()) return m;
    if (const char* m = stage_validate_problem(p, STAGE_OBS | STAGE_PARAMS); *m) return m;
    if (req->log_pt >= std::max(p->n_points, 1))  // (a zeroed request, log_pt = 0, is legal on an empty window too)
        return "log_pt = " + std::to_string(req->log_pt) + " is out of range (" + std::to_string(p->n_points) + " points)";
    if (req->log_pt >= 0 && (req->log_max_rows < 0 || (req->log_max_rows > 0 && !req->log_rows)))
        return "log_pt is set without a log_rows buffer";
    return "";
}

}  // namespace

extern "C" int32_t ba_refine_points(ba_context* ctx, ba_problem* p, const ba_pts_request* req, ba_pts_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_refine_points", ctx->stream};
    if (const std::string m = pts_check(ctx, p, req, info); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    const size_t nc = (size_t)p->n_cams, np = (size_t)p->n_points, no = (size_t)p->n_obs;
    ba_pts_info full{};
    full.struct_size = (int32_t)sizeof(ba_pts_info);

    // the observations grouped by point, and one record per selected point with min_obs admissible ones or more
    std::vector<int32_t> off(np + 1, 0), idx(no);
    const int32_t n_kept = loc_group(p->n_points, p->n_obs, p->obs_pt, p->obs_depth, req->pt_mask, off.data(), idx.data());
    const int32_t min_obs = std::max(req->min_obs, 1);
    std::vector<PtsRec> rec;
    int log_rec = -1;
    for (int32_t q = 0; q < p->n_points; ++q) {
        if (req->pt_mask && !req->pt_mask[q]) continue;
        ++full.n_selected;
        const int32_t n = off[q + 1] - off[q];
        if (n < min_obs) continue;
        if (q == req->log_pt) log_rec = (int)rec.size();
        const double N = (double)n;
        rec.push_back(PtsRec{q, off[q], off[q + 1], 0, std::sqrt(1.0 / N), std::sqrt(ctx->opts.weight_unpr / N)});
    }
    const size_t nrec = rec.size();
    full.n_solved = (int32_t)nrec;
    const int log_max = log_rec >= 0 ? req->log_max_rows : 0;
    std::vector<double> stats(nrec * PTS_STAT, 0.0);
    float lm_ms = 0.f;

    if (nrec) {
        HIPCHECK(ctx, hipSetDevice(ctx->device));
        HIPCHECK(ctx, stg.events(ctx->pts_ev, 2));
        hipStream_t s = stg.s;
        // in: cams (7 nc) | pts (3 np) | K (4) | uv (2 no) | depth (no) doubles, then obs_cam (no) ints
        // idx: the points' records (PtsRec), then the grouped indices
        // out: stats (8 nrec) | the solved positions (3 nrec) | log (8 log_max) doubles
        const size_t in_d = 7 * nc + 3 * np + 4 + 3 * no;
        const size_t in_bytes = 8 * (in_d + 1) + 4 * no, idx_bytes = sizeof(PtsRec) * nrec + 4 * (size_t)n_kept;
        const size_t out_bytes = 8 * ((PTS_STAT + 3) * nrec + (size_t)LOG_W * (size_t)log_max);
        if (int32_t rc = stg.ensure(B_PTS_IN, in_bytes, "the window's copy")) return rc;
        if (int32_t rc = stg.ensure(B_PTS_IDX, idx_bytes, "the grouped observations")) return rc;
        if (int32_t rc = stg.ensure(B_PTS_OUT, out_bytes, "the statistics")) return rc;
        double* d_cams = ctx->buf[B_PTS_IN].as<double>();
        double* d_pts = d_cams + 7 * nc;
        double* d_K = d_pts + 3 * np;
        double* d_uv = d_K + 4;  // (an even count of doubles before it: 16-byte aligned for the double2 loads)
        if ((7 * nc + 3 * np) & 1) ++d_uv;
        double* d_dep = d_uv + 2 * no;
        int* d_cam = reinterpret_cast<int*>(d_dep + no);
        PtsRec* d_rec = ctx->buf[B_PTS_IDX].as<PtsRec>();
        int* d_idx = reinterpret_cast<int*>(d_rec + nrec);
        double* d_stats = ctx->buf[B_PTS_OUT].as<double>();
        double* d_x = d_stats + PTS_STAT * nrec;
        double* d_log = d_x + 3 * nrec;
        HIPCHECK(ctx, stg.h2d(d_cams, p->cams, 56 * nc));
        HIPCHECK(ctx, stg.h2d(d_pts, p->points, 24 * np));
        HIPCHECK(ctx, stg.h2d(d_K, p->intr, 32));
        HIPCHECK(ctx, stg.h2d(d_uv, p->obs_uv, 16 * no));
        HIPCHECK(ctx, stg.h2d(d_dep, p->obs_depth, 8 * no));
        HIPCHECK(ctx, stg.h2d(d_cam, p->obs_cam, 4 * no));
        HIPCHECK(ctx, stg.h2d(d_rec, rec.data(), sizeof(PtsRec) * nrec));
        HIPCHECK(ctx, stg.h2d(d_idx, idx.data(), 4 * (size_t)n_kept));
        if (log_max) HIPCHECK(ctx, hipMemsetAsync(d_log, 0, 8 * (size_t)LOG_W * (size_t)log_max, s));

        PtsArgs a{};
        a.pts = d_pts; a.cams = d_cams; a.K = d_K;
        a.uv = reinterpret_cast<const double2*>(d_uv);
        a.depth = d_dep; a.obs_cam = d_cam; a.idx = d_idx; a.rec = d_rec; a.n_rec = (int)nrec;
        a.xout = d_x; a.stats = d_stats; a.log = d_log; a.log_rec = log_rec; a.log_max_rows = log_max;
        a.initial_radius = ctx->opts.initial_trust_region_radius;
        a.jacobi_scaling = ctx->opts.jacobi_scaling;
        const ba_options& o = ctx->opts;
        BaConsts C{};
        C.a_r = o.hub_p_repr; C.b_r = o.hub_p_repr * o.hub_p_repr;
        C.a_d = o.hub_p_unpr; C.b_d = o.hub_p_unpr * o.hub_p_unpr;
        C.min_diag = o.min_lm_diagonal; C.max_diag = o.max_lm_diagonal;
        LmParams prm = lm_params(ctx);
        prm.progress = nullptr;
        HIPCHECK(ctx, hipEventRecord(ctx->pts_ev[0], s));
        HIPCHECK(ctx, launch_pts_lm(a, C, prm, s));
        HIPCHECK(ctx, hipEventRecord(ctx->pts_ev[1], s));

        // only the solved points come back, in the records' order, and only they are written into prob
        std::vector<double> x(3 * nrec);
        std::vector<double> log((size_t)LOG_W * (size_t)log_max);
        HIPCHECK(ctx, stg.d2h(x.data(), d_x, 24 * nrec));
        HIPCHECK(ctx, stg.d2h(stats.data(), d_stats, 8 * PTS_STAT * nrec));
        HIPCHECK(ctx, stg.d2h(log.data(), d_log, 8 * log.size()));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&lm_ms, ctx->pts_ev[0], ctx->pts_ev[1]);
        for (size_t g = 0; g < nrec; ++g) std::memcpy(p->points + 3 * (size_t)rec[g].pt, &x[3 * g], 24);
        if (log_rec >= 0) {
            // iterations + 1 rows; none when the evaluation at the given position failed (the loop never started)
            const double* st = &stats[PTS_STAT * (size_t)log_rec];
            full.log_rows = (int)st[7] == MSG_EVAL_FAIL ? 0 : (int32_t)st[3] + 1;
            const size_t rows = (size_t)std::min(full.log_rows, log_max);
            if (rows) std::memcpy(req->log_rows, log.data(), 8 * (size_t)LOG_W * rows);
        }
    }

    if (req->pt_stats) {
        for (size_t q = 0; q < np; ++q) {
            double* st = req->pt_stats + BA_PTS_STAT_N * q;
            for (int k = 0; k < BA_PTS_STAT_N; ++k) st[k] = 0.0;
            st[6] = -1.0;
        }
        for (size_t g = 0; g < nrec; ++g)
            std::memcpy(req->pt_stats + BA_PTS_STAT_N * (size_t)rec[g].pt, &stats[PTS_STAT * g], 8 * PTS_STAT);
    }
    for (size_t g = 0; g < nrec; ++g) {
        const int term = (int)stats[PTS_STAT * g + 6];
        if (term == BA_CONVERGENCE) ++full.n_convergence;
        else if (term == BA_NO_CONVERGENCE) ++full.n_no_convergence;
        else ++full.n_failure;
        full.max_iterations = std::max(full.max_iterations, (int32_t)stats[PTS_STAT * g + 3]);
    }
    full.time_lm_ms = lm_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
