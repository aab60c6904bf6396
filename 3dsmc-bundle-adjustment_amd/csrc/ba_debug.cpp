// ba_debug.cpp — the ba_debug_* entry points of include/ba.h: intermediate results of the prepared window read
// back for the tests (residuals and Jacobians, the reduced system, the camera sums, one LM step, the plan digest).
#include "ba_context.h"

using namespace miba;

// What the read-back entry points share: the window prepared, a fresh LM state at `radius` (<= 0: the options'
// initial radius) on the device, the linearisation at the window's parameters.
static int prepare_and_linearize(ba_context* ctx, const ba_problem* p, double radius) {
    if (int rc = prepare(ctx, p)) return rc;
    static thread_local LmState h_st;  // host staging (outlives the async copy)
    h_st = fresh_state(ctx->opts, radius > 0 ? radius : ctx->opts.initial_trust_region_radius);
    HIPCHECK(ctx, hipMemcpyAsync(ctx->W.st, &h_st, sizeof(LmState), hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, launch_linearize(ctx->P, ctx->C, 0, ctx->W, ctx->stream, nullptr));
    return BA_OK;
}

extern "C" int32_t ba_debug_linearize(ba_context* ctx, const ba_problem* p, double* cost, double* res, double* jcam,
                                      double* jpt, double* jint) {
    if (!ctx) return BA_E_INVALID;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = prepare_and_linearize(ctx, p, 0.0)) return rc;
    DevProblem& P = ctx->P;
    hipStream_t s = ctx->stream;
    const size_t na = P.n_adm;
    const size_t width[4] = {3, 18, 9, 8};  // residuals | camera, point, intrinsics Jacobians per observation
    double* out[4] = {res, jcam, jpt, jint};
    std::vector<double> host[4];
    for (int k = 0; k < 4; ++k) HIPCHECK(ctx, ctx->buf[B_DBG0 + k].ensure(sizeof(double) * width[k] * na));
    HIPCHECK(ctx, launch_debug_lin(P, ctx->C, ctx->W, ctx->buf[B_DBG0].as<double>(), ctx->buf[B_DBG1].as<double>(),
                                   ctx->buf[B_DBG2].as<double>(), ctx->buf[B_DBG3].as<double>(), s));
    double lin_h[LIN_N];
    for (int k = 0; k < 4; ++k) {
        host[k].resize(width[k] * na);
        HIPCHECK(ctx, hipMemcpyAsync(host[k].data(), ctx->buf[B_DBG0 + k].p, sizeof(double) * host[k].size(),
                                     hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(ctx, hipMemcpyAsync(lin_h, ctx->W.lin, sizeof(lin_h), hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    if (cost) *cost = lin_h[0];
    const size_t no = p->n_obs;
    for (int k = 0; k < 4; ++k)
        if (out[k]) std::memset(out[k], 0, sizeof(double) * width[k] * no);
    // original index -> point-major slot (the plan's po_dest, on the device for both plans)
    std::vector<int> pdest(no);
    if (no) HIPCHECK(ctx, hipMemcpy(pdest.data(), ctx->raw.po_dest, sizeof(int) * no, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < no; ++i) {
        if (pdest[i] < 0) continue;
        const size_t q = pdest[i];
        for (int k = 0; k < 4; ++k)
            if (out[k]) std::memcpy(out[k] + width[k] * i, &host[k][width[k] * q], sizeof(double) * width[k]);
    }
    return BA_OK;
}

extern "C" int32_t ba_debug_reduced_system(ba_context* ctx, const ba_problem* p, double radius, int32_t* n_out,
                                           double* S, double* rhs) {
    if (!ctx) return BA_E_INVALID;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (!S || !rhs) {  // the size only
        if (int rc = prepare(ctx, p)) return rc;
        if (n_out) *n_out = ctx->P.n;
        return BA_OK;
    }
    if (int rc = prepare_and_linearize(ctx, p, radius)) return rc;
    DevProblem& P = ctx->P;
    hipStream_t s = ctx->stream;
    if (n_out) *n_out = P.n;
    HIPCHECK(ctx, launch_scale(P, ctx->C, ctx->opts.jacobi_scaling, ctx->W, s, nullptr));
    HIPCHECK(ctx, launch_build(P, ctx->C, ctx->W, s, nullptr));
    std::vector<double> Sp((size_t)P.npad * P.npad);
    HIPCHECK(ctx, hipMemcpyAsync(Sp.data(), ctx->W.S, sizeof(double) * Sp.size(), hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(rhs, ctx->W.rhs, sizeof(double) * P.n, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    const int n = P.n;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = Sp[(size_t)i * P.npad + j];
            S[(size_t)i * n + j] = v;
            S[(size_t)j * n + i] = v;
        }
    return BA_OK;
}

extern "C" int32_t ba_debug_camera_sums(ba_context* ctx, const ba_problem* p, int32_t* nac, double* camdata,
                                        double* lin, int32_t* ac_cam) {
    if (!ctx) return BA_E_INVALID;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (!camdata || !lin) {  // the count only
        if (int rc = prepare(ctx, p)) return rc;
        if (nac) *nac = ctx->P.nac;
        return BA_OK;
    }
    if (int rc = prepare_and_linearize(ctx, p, 0.0)) return rc;
    DevProblem& P = ctx->P;
    hipStream_t s = ctx->stream;
    if (nac) *nac = P.nac;
    HIPCHECK(ctx, hipMemcpyAsync(camdata, ctx->W.camdata, sizeof(double) * CAMDATA * P.nac, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(lin, ctx->W.lin, sizeof(double) * LIN_N, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    if (ac_cam) std::copy(ctx->ac_cam.begin(), ctx->ac_cam.end(), ac_cam);
    return BA_OK;
}

extern "C" int32_t ba_debug_step(ba_context* ctx, const ba_problem* p, double radius, int32_t* nac, int32_t* ac_cam,
                                 double* delta_cam, double* delta_intr, double* delta_pts, double* log_row,
                                 int32_t* info) {
    if (!ctx) return BA_E_INVALID;
    if (!p || !nac || !ac_cam || !delta_cam || !delta_intr || !delta_pts || !log_row || !info) {
        ctx->err = "ba_debug_step: null argument";
        return BA_E_INVALID;
    }
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = apply_spin_limit(ctx)) return rc;
    if (int rc = prepare(ctx, p)) return rc;
    ctx->err.clear();
    DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    hipStream_t s = ctx->stream;
    static thread_local LmState h_st;
    h_st = fresh_state(ctx->opts, radius > 0 ? radius : ctx->opts.initial_trust_region_radius);
    const int base = h_st.cur;  // the slot of x; the step's candidate goes to the other one, whatever the decision
    const LmParams prm = lm_params(ctx);
    // iteration zero and the first LM iteration, as ba_solve_prepared enqueues them
    if (int rc = enqueue_reset(ctx, h_st, p->n_cams)) return rc;
    if (int rc = enqueue_iteration_zero(ctx)) return rc;
    int retried = 0;
    for (;;) {
        if (int rc = enqueue_iteration(ctx, prm)) return rc;
        HIPCHECK(ctx, hipMemcpyAsync(&h_st, W.st, sizeof(LmState), hipMemcpyDeviceToHost, s));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        flush_prof(ctx);
        // a resident-kernel hand-off timed out: the iteration again with the per-level launches (once: they
        // have no inter-workgroup waits)
        if (!(h_st.done && h_st.msg == MSG_TIMEOUT && h_st.termination < 0) || retried) break;
        if (int rc = bcr_timeout_retry(ctx, h_st)) return rc;
        retried = 1;
    }
    if (h_st.msg == MSG_TIMEOUT) {
        ctx->err = "ba_debug_step: the re-run iteration timed out again";
        return BA_E_INTERNAL;
    }
    const size_t np3 = 3 * (size_t)p->n_points;
    std::vector<double> dl((size_t)P.n), x0(np3), x1(np3);
    double lg[LOG_W] = {};
    int cf = 0;
    if (P.n) HIPCHECK(ctx, hipMemcpyAsync(dl.data(), W.delta, sizeof(double) * P.n, hipMemcpyDeviceToHost, s));
    if (np3) {
        const size_t off = 3 * (size_t)ctx->gather_off;
        HIPCHECK(ctx, hipMemcpyAsync(x0.data(), P.pts[base] + off, sizeof(double) * np3, hipMemcpyDeviceToHost, s));
        HIPCHECK(ctx, hipMemcpyAsync(x1.data(), P.pts[base ^ 1] + off, sizeof(double) * np3, hipMemcpyDeviceToHost, s));
    }
    if (h_st.iter >= 1) HIPCHECK(ctx, hipMemcpyAsync(lg, W.log + LOG_W, sizeof(lg), hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(&cf, W.chol_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    *nac = P.nac;
    std::copy(ctx->ac_cam.begin(), ctx->ac_cam.begin() + P.nac, ac_cam);
    std::copy(dl.begin(), dl.begin() + 6 * (size_t)P.nac, delta_cam);
    std::copy(dl.begin() + P.kb, dl.begin() + P.kb + 4, delta_intr);
    // (points without an admissible observation are never written: both slots hold the prepared value)
    for (size_t i = 0; i < np3; ++i) delta_pts[i] = x1[i] - x0[i];
    std::copy(lg, lg + LOG_W, log_row);
    const int32_t inf[BA_STEP_INFO_N] = {cf, retried, P.solver, P.cam_band, P.solver == 1 ? P.band_w : 0, h_st.iter, 0, 0};
    std::copy(inf, inf + BA_STEP_INFO_N, info);
    ctx->dbg_step_base = base;
    return BA_OK;
}

extern "C" int32_t ba_debug_step_state(ba_context* ctx, double* cams_x, double* cams_cand, double* intr_x,
                                       double* intr_cand, double* pts_x, double* pts_cand, double* scal, double* lin,
                                       double* log_rows, double* state) {
    if (!ctx) return BA_E_INVALID;
    if (!cams_x || !cams_cand || !intr_x || !intr_cand || !pts_x || !pts_cand || !scal || !lin || !log_rows || !state) {
        ctx->err = "ba_debug_step_state: null argument";
        return BA_E_INVALID;
    }
    if (!ctx->prepared || ctx->dbg_step_base < 0) {
        ctx->err = "ba_debug_step_state: no ba_debug_step on this context since the last prepare / solve";
        return BA_E_INVALID;
    }
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    hipStream_t s = ctx->stream;
    const int base = ctx->dbg_step_base;
    const size_t nc7 = 7 * (size_t)ctx->prep_nc, np3 = 3 * (size_t)ctx->prep_np, off = 3 * (size_t)ctx->gather_off;
    LmState st{};
    double sc[SC_N] = {};
    // copies only (pageable destinations: each returns once its data has arrived)
    if (nc7) {
        HIPCHECK(ctx, hipMemcpyAsync(cams_x, P.cams[base], sizeof(double) * nc7, hipMemcpyDeviceToHost, s));
        HIPCHECK(ctx, hipMemcpyAsync(cams_cand, P.cams[base ^ 1], sizeof(double) * nc7, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(ctx, hipMemcpyAsync(intr_x, P.K[base], sizeof(double) * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(intr_cand, P.K[base ^ 1], sizeof(double) * 4, hipMemcpyDeviceToHost, s));
    if (np3) {
        HIPCHECK(ctx, hipMemcpyAsync(pts_x, P.pts[base] + off, sizeof(double) * np3, hipMemcpyDeviceToHost, s));
        HIPCHECK(ctx, hipMemcpyAsync(pts_cand, P.pts[base ^ 1] + off, sizeof(double) * np3, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(ctx, hipMemcpyAsync(sc, W.scal, sizeof(sc), hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(lin, W.lin, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(log_rows, W.log, sizeof(double) * 2 * LOG_W, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(&st, W.st, sizeof(LmState), hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    const double scv[BA_STEP_SCAL_N] = {sc[SC_MCC], sc[SC_CAND], sc[SC_SN2], sc[SC_GMAX_PT], sc[SC_BAD], sc[SC_XN2], 0, 0};
    std::copy(scv, scv + BA_STEP_SCAL_N, scal);
    const double stv[BA_STEP_STATE_N] = {st.radius, st.decrease_factor, st.xnorm2, st.x_cost, st.final_cost,
                                         (double)st.cur, (double)st.termination, (double)st.msg,
                                         st.gmax_ci, st.initial_cost, (double)st.iter, (double)base};
    std::copy(stv, stv + BA_STEP_STATE_N, state);
    return BA_OK;
}

extern "C" int32_t ba_debug_plan_digest(ba_context* ctx, uint64_t* out, int32_t max_n) {
    if (!ctx || !ctx->prepared) return BA_E_INVALID;
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    const int n = (int)ctx->plan_parts.size();
    for (int k = 0; k < n && k < max_n; ++k) {
        const auto [off, len] = ctx->plan_parts[k];
        std::vector<int32_t> v(len);
        if (len)
            HIPCHECK(ctx, hipMemcpy(v.data(), ctx->buf[B_PLAN].as<int>() + off, sizeof(int32_t) * len,
                                    hipMemcpyDeviceToHost));
        uint64_t h = 1469598103934665603ull;
        for (int32_t x : v)
            for (int b = 0; b < 4; ++b) h = (h ^ ((uint32_t)x >> (8 * b) & 0xffu)) * 1099511628211ull;
        h = (h ^ (uint64_t)len) * 1099511628211ull;
        out[k] = h;
    }
    return n;
}
