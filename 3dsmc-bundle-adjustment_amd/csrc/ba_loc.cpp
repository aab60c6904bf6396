// ba_loc.cpp — ba_localize of include/ba.h: pose-only LM of the selected cameras against the window's constant points
// and intrinsics (the kernel of ba_loc.hip, one workgroup per camera; the observations grouped by camera on the host,
// ba_loc_group.cpp).
// A stage beside the LM loop like ba_covisibility and ba_local_window: it works on device buffers of its own
// (B_LOC_*), so nothing the plan or the LM loop reads is written.
#include "ba_loc.h"
#include "ba_loc_group.h"
#include "ba_stage.h"

#include <cmath>

using namespace miba;

static_assert(LOC_STAT == BA_LOC_STAT_N && LOG_W == BA_LOG_WIDTH, "the kernel writes the header's record widths");

namespace {

std::string loc_check(ba_context* ctx, const ba_problem* p, const ba_loc_request* req, const ba_loc_info* info) {
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_LOC)); !m.empty()) return m;
    if (const char* m = stage_validate_problem(p, STAGE_OBS | STAGE_PARAMS); *m) return m;
    if (req->log_cam >= std::max(p->n_cams, 1))  // (a zeroed request, log_cam = 0, is legal on an empty window too)
        return "log_cam = " + std::to_string(req->log_cam) + " is out of range (" + std::to_string(p->n_cams) + " cameras)";
    if (req->log_cam >= 0 && (req->log_max_rows < 0 || (req->log_max_rows > 0 && !req->log_rows)))
        return "log_cam is set without a log_rows buffer";
    return "";
}

}  // namespace

extern "C" int32_t ba_localize(ba_context* ctx, ba_problem* p, const ba_loc_request* req, ba_loc_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_localize", ctx->stream};
    if (const std::string m = loc_check(ctx, p, req, info); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    const size_t nc = (size_t)p->n_cams, np = (size_t)p->n_points, no = (size_t)p->n_obs;
    ba_loc_info full{};
    full.struct_size = (int32_t)sizeof(ba_loc_info);

    // the observations grouped by camera, and one workgroup per selected camera that has any
    std::vector<int32_t> off(nc + 1, 0), idx(no);
    const int32_t n_kept = loc_group(p->n_cams, p->n_obs, p->obs_cam, p->obs_depth, req->cam_mask, off.data(), idx.data());
    std::vector<LocCam> wg;
    int log_wg = -1;
    for (int32_t c = 0; c < p->n_cams; ++c) {
        if (req->cam_mask && !req->cam_mask[c]) continue;
        ++full.n_selected;
        const int32_t n = off[c + 1] - off[c];
        if (n <= 0) continue;
        if (c == req->log_cam) log_wg = (int)wg.size();
        const double N = (double)n;
        wg.push_back(LocCam{c, off[c], off[c + 1], 0, std::sqrt(1.0 / N), std::sqrt(ctx->opts.weight_unpr / N)});
    }
    const size_t nwg = wg.size();
    full.n_solved = (int32_t)nwg;
    const int log_max = log_wg >= 0 ? req->log_max_rows : 0;
    std::vector<double> stats(nwg * LOC_STAT, 0.0);
    float lm_ms = 0.f;

    if (nwg) {
        HIPCHECK(ctx, hipSetDevice(ctx->device));
        HIPCHECK(ctx, stg.events(ctx->loc_ev, 2));
        hipStream_t s = stg.s;
        // in: cams (7 nc) | pts (3 np) | K (4) | uv (2 no) | depth (no) doubles, then obs_pt (no) ints
        // idx: the workgroups' records (LocCam), then the grouped indices
        // out: stats (8 nwg) | log (8 log_max) doubles
        const size_t in_d = 7 * nc + 3 * np + 4 + 3 * no;
        const size_t in_bytes = 8 * (in_d + 1) + 4 * no, idx_bytes = sizeof(LocCam) * nwg + 4 * (size_t)n_kept;
        const size_t out_bytes = 8 * (LOC_STAT * nwg + (size_t)LOG_W * (size_t)log_max);
        if (int32_t rc = stg.ensure(B_LOC_IN, in_bytes, "the window's copy")) return rc;
        if (int32_t rc = stg.ensure(B_LOC_IDX, idx_bytes, "the grouped observations")) return rc;
        if (int32_t rc = stg.ensure(B_LOC_OUT, out_bytes, "the statistics")) return rc;
        double* d_cams = ctx->buf[B_LOC_IN].as<double>();
        double* d_pts = d_cams + 7 * nc;
        double* d_K = d_pts + 3 * np;
        double* d_uv = d_K + 4;  // (an even count of doubles before it: 16-byte aligned for the double2 loads)
        if ((7 * nc + 3 * np) & 1) ++d_uv;
        double* d_dep = d_uv + 2 * no;
        int* d_pt = reinterpret_cast<int*>(d_dep + no);
        LocCam* d_wg = ctx->buf[B_LOC_IDX].as<LocCam>();
        int* d_idx = reinterpret_cast<int*>(d_wg + nwg);
        double* d_stats = ctx->buf[B_LOC_OUT].as<double>();
        double* d_log = d_stats + LOC_STAT * nwg;
        HIPCHECK(ctx, stg.h2d(d_cams, p->cams, 56 * nc));
        HIPCHECK(ctx, stg.h2d(d_pts, p->points, 24 * np));
        HIPCHECK(ctx, stg.h2d(d_K, p->intr, 32));
        HIPCHECK(ctx, stg.h2d(d_uv, p->obs_uv, 16 * no));
        HIPCHECK(ctx, stg.h2d(d_dep, p->obs_depth, 8 * no));
        HIPCHECK(ctx, stg.h2d(d_pt, p->obs_pt, 4 * no));
        HIPCHECK(ctx, stg.h2d(d_wg, wg.data(), sizeof(LocCam) * nwg));
        HIPCHECK(ctx, stg.h2d(d_idx, idx.data(), 4 * (size_t)n_kept));
        if (log_max) HIPCHECK(ctx, hipMemsetAsync(d_log, 0, 8 * (size_t)LOG_W * (size_t)log_max, s));

        LocArgs a{};
        a.cams = d_cams; a.pts = d_pts; a.K = d_K;
        a.uv = reinterpret_cast<const double2*>(d_uv);
        a.depth = d_dep; a.obs_pt = d_pt; a.idx = d_idx; a.wg = d_wg;
        a.stats = d_stats; a.log = d_log; a.log_wg = log_wg; a.log_max_rows = log_max;
        a.initial_radius = ctx->opts.initial_trust_region_radius;
        a.jacobi_scaling = ctx->opts.jacobi_scaling;
        const ba_options& o = ctx->opts;
        BaConsts C{};
        C.a_r = o.hub_p_repr; C.b_r = o.hub_p_repr * o.hub_p_repr;
        C.a_d = o.hub_p_unpr; C.b_d = o.hub_p_unpr * o.hub_p_unpr;
        C.min_diag = o.min_lm_diagonal; C.max_diag = o.max_lm_diagonal;
        LmParams prm = lm_params(ctx);
        prm.progress = nullptr;
        HIPCHECK(ctx, hipEventRecord(ctx->loc_ev[0], s));
        HIPCHECK(ctx, launch_loc_lm(a, C, prm, (int)nwg, s));
        HIPCHECK(ctx, hipEventRecord(ctx->loc_ev[1], s));

        // the solved poses come back through a copy: only the workgroups' cameras are written into prob
        std::vector<double> cams(7 * nc);
        std::vector<double> log((size_t)LOG_W * (size_t)log_max);
        HIPCHECK(ctx, stg.d2h(cams.data(), d_cams, 56 * nc));
        HIPCHECK(ctx, stg.d2h(stats.data(), d_stats, 8 * LOC_STAT * nwg));
        HIPCHECK(ctx, stg.d2h(log.data(), d_log, 8 * log.size()));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&lm_ms, ctx->loc_ev[0], ctx->loc_ev[1]);
        for (size_t g = 0; g < nwg; ++g)
            std::memcpy(p->cams + 7 * (size_t)wg[g].cam, &cams[7 * (size_t)wg[g].cam], 56);
        if (log_wg >= 0) {
            // iterations + 1 rows; none when the evaluation at the given pose failed (the loop never started)
            const double* st = &stats[LOC_STAT * (size_t)log_wg];
            full.log_rows = (int)st[7] == MSG_EVAL_FAIL ? 0 : (int32_t)st[3] + 1;
            const size_t rows = (size_t)std::min(full.log_rows, log_max);
            if (rows) std::memcpy(req->log_rows, log.data(), 8 * (size_t)LOG_W * rows);
        }
    }

    if (req->cam_stats) {
        for (size_t c = 0; c < nc; ++c) {
            double* st = req->cam_stats + BA_LOC_STAT_N * c;
            for (int k = 0; k < BA_LOC_STAT_N; ++k) st[k] = 0.0;
            st[6] = -1.0;
        }
        for (size_t g = 0; g < nwg; ++g)
            std::memcpy(req->cam_stats + BA_LOC_STAT_N * (size_t)wg[g].cam, &stats[LOC_STAT * g], 8 * LOC_STAT);
    }
    for (size_t g = 0; g < nwg; ++g) {
        const int term = (int)stats[LOC_STAT * g + 6];
        if (term == BA_CONVERGENCE) ++full.n_convergence;
        else if (term == BA_NO_CONVERGENCE) ++full.n_no_convergence;
        else ++full.n_failure;
        full.max_iterations = std::max(full.max_iterations, (int32_t)stats[LOC_STAT * g + 3]);
    }
    full.time_lm_ms = lm_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
