// ba_loc.cpp — ba_localize of include/ba.h: pose-only LM of the selected cameras against the window's constant points
// and intrinsics (the kernel of ba_loc.hip, one workgroup per camera; the observations grouped by camera on the host,
// ba_loc_group.cpp; the driver of ba_block_stage.h).
// A stage beside the LM loop like ba_covisibility and ba_local_window: it works on device buffers of its own
// (B_LOC_*), so nothing the plan or the LM loop reads is written.
#include "ba_loc.h"
#include "ba_block_stage.h"

using namespace miba;

static_assert(LOC_STAT == BA_LOC_STAT_N && LOC_STAT == BlockStage::STAT && LOG_W == BA_LOG_WIDTH,
              "the kernel writes the header's record widths");

namespace {

std::string loc_check(ba_context* ctx, const ba_problem* p, const ba_loc_request* req, const ba_loc_info* info) {
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_LOC)); !m.empty()) return m;
    if (const char* m = stage_validate_problem(p, STAGE_OBS | STAGE_PARAMS); *m) return m;
    return block_log_check("log_cam", req->log_cam, p->n_cams, "cameras", req->log_max_rows, req->log_rows);
}

}  // namespace

extern "C" int32_t ba_localize(ba_context* ctx, ba_problem* p, const ba_loc_request* req, ba_loc_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_localize", ctx->stream};
    if (const std::string m = loc_check(ctx, p, req, info); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    const size_t nc = (size_t)p->n_cams;
    ba_loc_info full{};
    full.struct_size = (int32_t)sizeof(ba_loc_info);

    // one workgroup per selected camera that has any admissible observation
    BlockStage B;
    B.group(p, p->n_cams, p->obs_cam, req->cam_mask, 1, req->log_cam, req->log_max_rows, ctx->opts.weight_unpr);
    float lm_ms = 0.f;

    if (B.n()) {
        HIPCHECK(ctx, hipSetDevice(ctx->device));
        HIPCHECK(ctx, stg.events(ctx->loc_ev, 2));
        if (int32_t rc = B.upload(stg, p, B_LOC_IN, B_LOC_IDX, B_LOC_OUT, p->obs_pt, 0)) return rc;

        LocArgs a{};
        a.cams = B.d_cams; a.pts = B.d_pts; a.K = B.d_K;
        a.uv = reinterpret_cast<const double2*>(B.d_uv);
        a.depth = B.d_dep; a.obs_pt = B.d_other; a.idx = B.d_idx; a.wg = B.d_rec;
        a.stats = B.d_stats; a.log = B.d_log; a.log_wg = B.log_rec; a.log_max_rows = B.log_max;
        a.initial_radius = ctx->opts.initial_trust_region_radius;
        a.jacobi_scaling = ctx->opts.jacobi_scaling;
        BaConsts C{};
        cost_consts(ctx->opts, C);
        LmParams prm = lm_params(ctx);
        prm.progress = nullptr;
        HIPCHECK(ctx, hipEventRecord(ctx->loc_ev[0], stg.s));
        HIPCHECK(ctx, launch_loc_lm(a, C, prm, (int)B.n(), stg.s));
        HIPCHECK(ctx, hipEventRecord(ctx->loc_ev[1], stg.s));

        // the solved poses come back through a copy: only the workgroups' cameras are written into prob
        std::vector<double> cams(7 * nc);
        HIPCHECK(ctx, stg.d2h(cams.data(), B.d_cams, 56 * nc));
        if (int32_t rc = B.fetch(stg, ctx->loc_ev, &lm_ms, req->log_rows, &full.log_rows)) return rc;
        for (const BlockRec& r : B.rec) std::memcpy(p->cams + 7 * (size_t)r.id, &cams[7 * (size_t)r.id], 56);
    }

    B.scatter_stats(req->cam_stats, nc);
    B.tally(full);
    full.time_lm_ms = lm_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
