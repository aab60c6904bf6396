// ba_resid.cpp — ba_residuals of include/ba.h: the residual report of a window at its parameters (the counterpart
// of ceres::Problem::Evaluate). Prepares the window like the read-back entry points of ba_debug.cpp, runs the
// kernels of ba_resid.hip on the parameters the prepare left on the device and copies out what the request names.
// Nothing the LM loop reads is written: the report has buffers of its own and never touches the LM state.
#include <cmath>

#include "ba_resid.h"
#include "ba_stage.h"

using namespace miba;

extern "C" int32_t ba_residuals(ba_context* ctx, const ba_problem* p, const ba_res_request* req, ba_res_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_residuals", ctx->stream};
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_RES)); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = prepare(ctx, p)) return rc;
    ctx->err.clear();
    HIPCHECK(ctx, stg.events(ctx->res_ev, 2));
    const DevProblem& P = ctx->P;
    hipStream_t s = stg.s;
    const size_t no = (size_t)p->n_obs, np = (size_t)p->n_points, nc = (size_t)p->n_cams;
    const size_t na = (size_t)P.n_adm, nseg = (size_t)P.n_seg;
    const bool want_flags = req->obs_flags || req->obs_depth_culled;
    const bool per_obs = req->obs_err || req->obs_cost || want_flags;

    ResThresholds t{};
    t.max_reproj = req->max_reproj_px;
    t.reproj_on = req->max_reproj_px > 0 ? 1 : 0;
    t.depth_abs = std::max(req->max_depth_abs, 0.0);
    t.depth_rel = std::max(req->max_depth_rel, 0.0);
    t.depth_on = (req->max_depth_abs > 0 || req->max_depth_rel > 0) ? 1 : 0;

    // slot-order values | caller-order values | statistics (each part 8-byte aligned: doubles first)
    // (a failed allocation is BA_E_DEVICE with the HIP text here and in ba_covariance, not Stage::ensure's BA_E_NOMEM)
    HIPCHECK(ctx, ctx->buf[B_RES_PO].ensure(44 * std::max<size_t>(na, 1)));
    if (per_obs) HIPCHECK(ctx, ctx->buf[B_RES_OBS].ensure(44 * std::max<size_t>(no, 1)));
    const size_t n_stat = BA_RES_STAT_N * np + RES_PART_N * nseg + BA_RES_STAT_N * nc + RES_TOTALS_N;
    HIPCHECK(ctx, ctx->buf[B_RES_STAT].ensure(sizeof(double) * n_stat));
    ResBufs b{};
    b.po_err = ctx->buf[B_RES_PO].as<double>();
    b.po_cost = b.po_err + 4 * na;
    b.po_flags = reinterpret_cast<int*>(b.po_cost + na);
    if (per_obs) {
        b.obs_err = ctx->buf[B_RES_OBS].as<double>();
        b.obs_cost = b.obs_err + 4 * no;
        b.obs_flags = reinterpret_cast<int*>(b.obs_cost + no);
    }
    double* st = ctx->buf[B_RES_STAT].as<double>();
    b.point_stats = req->point_stats ? st : nullptr;
    b.seg_part = st + BA_RES_STAT_N * np;
    b.cam_stats = b.seg_part + RES_PART_N * nseg;
    b.totals = b.cam_stats + BA_RES_STAT_N * nc;

    HIPCHECK(ctx, hipEventRecord(ctx->res_ev[0], s));
    HIPCHECK(ctx, launch_resid(P, ctx->C, ctx->raw, p->n_points, t, b, s));
    HIPCHECK(ctx, hipEventRecord(ctx->res_ev[1], s));

    double tot[RES_TOTALS_N];
    std::vector<int32_t> flags_tmp;
    int32_t* flags_out = req->obs_flags;
    if (want_flags && !flags_out && no) { flags_tmp.resize(no); flags_out = flags_tmp.data(); }
    HIPCHECK(ctx, stg.d2h(tot, b.totals, sizeof(tot)));
    if (req->obs_err) HIPCHECK(ctx, stg.d2h(req->obs_err, b.obs_err, sizeof(double) * 4 * no));
    if (req->obs_cost) HIPCHECK(ctx, stg.d2h(req->obs_cost, b.obs_cost, sizeof(double) * no));
    if (flags_out) HIPCHECK(ctx, stg.d2h(flags_out, b.obs_flags, sizeof(int32_t) * no));
    if (req->cam_stats) HIPCHECK(ctx, stg.d2h(req->cam_stats, b.cam_stats, sizeof(double) * BA_RES_STAT_N * nc));
    if (req->point_stats) HIPCHECK(ctx, stg.d2h(req->point_stats, b.point_stats, sizeof(double) * BA_RES_STAT_N * np));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    if (req->obs_depth_culled)
        for (size_t k = 0; k < no; ++k)
            req->obs_depth_culled[k] = (flags_out[k] & BA_RES_OUTLIER) ? 0.0 : p->obs_depth[k];

    ba_res_info full{};
    full.struct_size = (int32_t)sizeof(ba_res_info);
    full.n_admissible = (int32_t)tot[0];
    full.n_outliers = (int32_t)tot[1];
    full.n_behind = (int32_t)tot[6];
    full.n_reproj = (int32_t)tot[7];
    full.n_depth = (int32_t)tot[8];
    full.n_huber_repr = (int32_t)tot[9];
    full.n_huber_unpr = (int32_t)tot[10];
    full.prior_cost = tot[RES_TOT_PRIOR];
    full.cost = tot[5] + tot[RES_TOT_PRIOR];
    const double n_proj = tot[0] - tot[6];
    full.rms_reproj_px = n_proj > 0 ? std::sqrt(tot[2] / n_proj) : 0.0;
    full.max_reproj_px = tot[3];
    full.rms_depth = n_proj > 0 ? std::sqrt(tot[4] / n_proj) : 0.0;
    full.max_depth = tot[11];
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->res_ev[0], ctx->res_ev[1]);
    full.time_eval_ms = ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    return BA_OK;
}
