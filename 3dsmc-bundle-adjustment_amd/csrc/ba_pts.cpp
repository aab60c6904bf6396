// ba_pts.cpp — ba_refine_points of include/ba.h: structure-only LM of the selected points against the window's
// constant cameras and intrinsics (the kernel of ba_pts.hip, one row of 16 lanes per point; the observations grouped
// by point on the host with ba_localize's counting sort, ba_loc_group.cpp; the driver of ba_block_stage.h).
// A stage beside the LM loop like ba_localize: it works on device buffers of its own (B_PTS_*), so nothing the plan
// or the LM loop reads is written.
#include "ba_pts.h"
#include "ba_block_stage.h"

using namespace miba;

static_assert(PTS_STAT == BA_PTS_STAT_N && PTS_STAT == BlockStage::STAT && LOG_W == BA_LOG_WIDTH,
              "the kernel writes the header's record widths");

namespace {

std::string pts_check(ba_context* ctx, const ba_problem* p, const ba_pts_request* req, const ba_pts_info* info) {
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_PTS)); !m.empty()) return m;
    if (const char* m = stage_validate_problem(p, STAGE_OBS | STAGE_PARAMS); *m) return m;
    return block_log_check("log_pt", req->log_pt, p->n_points, "points", req->log_max_rows, req->log_rows);
}

}  // namespace

extern "C" int32_t ba_refine_points(ba_context* ctx, ba_problem* p, const ba_pts_request* req, ba_pts_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_refine_points", ctx->stream};
    if (const std::string m = pts_check(ctx, p, req, info); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    ba_pts_info full{};
    full.struct_size = (int32_t)sizeof(ba_pts_info);

    // one record per selected point with min_obs admissible observations or more
    BlockStage B;
    B.group(p, p->n_points, p->obs_pt, req->pt_mask, std::max(req->min_obs, 1), req->log_pt, req->log_max_rows,
            ctx->opts.weight_unpr);
    const size_t nrec = B.n();
    float lm_ms = 0.f;

    if (nrec) {
        HIPCHECK(ctx, hipSetDevice(ctx->device));
        HIPCHECK(ctx, stg.events(ctx->pts_ev, 2));
        // (out: the solved positions, 3 per record, between the statistics and the log)
        if (int32_t rc = B.upload(stg, p, B_PTS_IN, B_PTS_IDX, B_PTS_OUT, p->obs_cam, 3)) return rc;

        PtsArgs a{};
        a.pts = B.d_pts; a.cams = B.d_cams; a.K = B.d_K;
        a.uv = reinterpret_cast<const double2*>(B.d_uv);
        a.depth = B.d_dep; a.obs_cam = B.d_other; a.idx = B.d_idx; a.rec = B.d_rec; a.n_rec = (int)nrec;
        a.xout = B.d_extra; a.stats = B.d_stats; a.log = B.d_log; a.log_rec = B.log_rec; a.log_max_rows = B.log_max;
        a.initial_radius = ctx->opts.initial_trust_region_radius;
        a.jacobi_scaling = ctx->opts.jacobi_scaling;
        BaConsts C{};
        cost_consts(ctx->opts, C);
        LmParams prm = lm_params(ctx);
        prm.progress = nullptr;
        HIPCHECK(ctx, hipEventRecord(ctx->pts_ev[0], stg.s));
        HIPCHECK(ctx, launch_pts_lm(a, C, prm, stg.s));
        HIPCHECK(ctx, hipEventRecord(ctx->pts_ev[1], stg.s));

        // only the solved points come back, in the records' order, and only they are written into prob
        std::vector<double> x(3 * nrec);
        HIPCHECK(ctx, stg.d2h(x.data(), B.d_extra, 24 * nrec));
        if (int32_t rc = B.fetch(stg, ctx->pts_ev, &lm_ms, req->log_rows, &full.log_rows)) return rc;
        for (size_t g = 0; g < nrec; ++g) std::memcpy(p->points + 3 * (size_t)B.rec[g].id, &x[3 * g], 24);
    }

    B.scatter_stats(req->pt_stats, (size_t)p->n_points);
    B.tally(full);
    full.time_lm_ms = lm_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
