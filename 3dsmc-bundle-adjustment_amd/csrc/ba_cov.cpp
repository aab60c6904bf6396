// ba_cov.cpp — ba_covariance of include/ba.h: the covariance of the estimate (kernels of ba_cov.hip over the reduced
// system the LM loop's own launches build).
// The reduced system is built as ba_debug_reduced_system builds it, with radius = +infinity: every damping site is
// clip(diag) / radius (camera / intrinsics blocks in env_tile and k_assemble, the points in point_tail), so S is the
// undamped Jacobi-scaled Schur complement. The dense inverse fills outside S's envelope and works in buffers of its
// own (ba_cov.hip); entries of W.S outside the envelope are zero here because every prepare() clears the whole of S
// and the build writes the envelope only.
#include <cmath>

#include "ba_cov.h"
#include "ba_stage.h"

using namespace miba;

extern "C" int32_t ba_covariance(ba_context* ctx, const ba_problem* p, const ba_cov_request* req, ba_cov_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_covariance", ctx->stream};
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_COV)); !m.empty()) return stg.invalid(m);
    const int npairs = req->n_pairs, nreq = req->n_points;
    if (npairs < 0 || nreq < 0) return stg.invalid("negative n_pairs / n_points");
    if (npairs > 0 && (!req->pair_a || !req->pair_b || !req->pair_cov)) return stg.invalid("null pair_a / pair_b / pair_cov");
    for (int k = 0; k < npairs; ++k)
        for (const int32_t v : {req->pair_a[k], req->pair_b[k]})
            if (v != BA_COV_INTR && (v < 0 || v >= p->n_cams))
                return stg.invalid("pair " + std::to_string(k) + ": camera index " + std::to_string(v) + " out of range");
    if (nreq > 0 && !req->point_cov) return stg.invalid("null point_cov");
    if (nreq > 0 && !req->point_idx && nreq != p->n_points)
        return stg.invalid("point_idx is NULL but n_points differs from the window's");
    if (req->point_idx)
        for (int k = 0; k < nreq; ++k)
            if (req->point_idx[k] < 0 || req->point_idx[k] >= p->n_points)
                return stg.invalid("point " + std::to_string(k) + ": index " + std::to_string(req->point_idx[k]) +
                                  " out of range");
    const double t0 = now_ms();
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = apply_spin_limit(ctx)) return rc;
    if (int rc = prepare(ctx, p)) return rc;
    ctx->err.clear();
    HIPCHECK(ctx, stg.events(ctx->cov_ev, 4));
    DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    hipStream_t s = stg.s;
    const int n = P.n, nblk = cov_nblk(n), ld = COV_B * nblk;
    const double rcond = req->min_reciprocal_condition_number > 0 ? req->min_reciprocal_condition_number : 1e-14;
    // the request in active indices
    std::vector<int> cam_ac(std::max(p->n_cams, 1), COV_PAIR_NAN), idx(2 * (size_t)npairs + nreq);
    for (int t = 0; t < P.nac; ++t) cam_ac[ctx->ac_cam[t]] = t;
    if (p->fixed_cam >= 0 && p->fixed_cam < p->n_cams) cam_ac[p->fixed_cam] = COV_PAIR_ZERO;
    if (ctx->cmask_any)  // a constant block like the gauge camera (prepare() has checked the mask's size)
        for (int i = 0; i < p->n_cams; ++i)
            if (ctx->cmask[i]) cam_ac[i] = COV_PAIR_ZERO;
    for (int k = 0; k < npairs; ++k) {
        idx[k] = req->pair_a[k] == BA_COV_INTR ? COV_PAIR_INTR : cam_ac[req->pair_a[k]];
        idx[npairs + k] = req->pair_b[k] == BA_COV_INTR ? COV_PAIR_INTR : cam_ac[req->pair_b[k]];
    }
    if (nreq > 0) {
        std::vector<int> pt_idx(P.n_ap), pt_ap(std::max(p->n_points, 1), -1);
        HIPCHECK(ctx, stg.d2h(pt_idx.data(), P.pt_idx, sizeof(int) * P.n_ap));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        for (int a = 0; a < P.n_ap; ++a) pt_ap[pt_idx[a]] = a;
        for (int k = 0; k < nreq; ++k) idx[2 * (size_t)npairs + k] = pt_ap[req->point_idx ? req->point_idx[k] : k];
    }
    const size_t mat = sizeof(double) * (size_t)ld * ld, nout = 36 * (size_t)npairs + 9 * (size_t)nreq;
    // (a failed allocation is BA_E_DEVICE with the HIP text here and in ba_residuals, not Stage::ensure's BA_E_NOMEM)
    HIPCHECK(ctx, ctx->buf[B_COV_A].ensure(mat));
    HIPCHECK(ctx, ctx->buf[B_COV_Z].ensure(mat));
    HIPCHECK(ctx, ctx->buf[B_COV_W].ensure(sizeof(double) * cov_wbuf_doubles(nreq > 0 ? P.n_adm : 0, nreq)));
    HIPCHECK(ctx, ctx->buf[B_COV_IDX].ensure(sizeof(CovStat) + sizeof(int) * idx.size()));
    HIPCHECK(ctx, ctx->buf[B_COV_OUT].ensure(sizeof(double) * nout));
    double* A = ctx->buf[B_COV_A].as<double>();
    double* Z = ctx->buf[B_COV_Z].as<double>();
    CovStat* stat = ctx->buf[B_COV_IDX].as<CovStat>();
    int* d_idx = reinterpret_cast<int*>(stat + 1);
    double* d_out = ctx->buf[B_COV_OUT].as<double>();
    if (!idx.empty()) HIPCHECK(ctx, hipMemcpy(d_idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice));
    // the undamped reduced system at the window's parameters (the hand-off words as launch_reset leaves them)
    static thread_local LmState h_st;
    h_st = fresh_state(ctx->opts, INFINITY);
    h_st.stop_next = 0;
    if (W.sw_cnt) HIPCHECK(ctx, hipMemsetAsync(W.sw_cnt, 0, sizeof(unsigned), s));
    W.sw_seq = 0;
    HIPCHECK(ctx, stg.h2d(W.st, &h_st, sizeof(LmState)));
    HIPCHECK(ctx, hipEventRecord(ctx->cov_ev[0], s));
    HIPCHECK(ctx, launch_linearize(P, ctx->C, 0, W, s, nullptr));
    HIPCHECK(ctx, launch_scale(P, ctx->C, ctx->opts.jacobi_scaling, W, s, nullptr));
    HIPCHECK(ctx, launch_build(P, ctx->C, W, s, nullptr));
    HIPCHECK(ctx, hipEventRecord(ctx->cov_ev[1], s));
    // blocked Cholesky with Z = L^-1 carried along, Z^T Z, unscale: about 3 launches per 64-column block
    HIPCHECK(ctx, launch_cov_copy(W.S, P.npad, n, A, ld, stat, s));
    HIPCHECK(ctx, hipMemsetAsync(Z, 0, mat, s));
    for (int k = 0; k < nblk; ++k) HIPCHECK(ctx, launch_cov_column(A, Z, ld, nblk, k, n, stat, s));
    HIPCHECK(ctx, launch_cov_finish(A, Z, ld, nblk, n, W.scale, P.kb, P.off_k, rcond, stat, s));
    HIPCHECK(ctx, launch_cov_pairs(Z, ld, P.kb, d_idx, d_idx + npairs, npairs, d_out, rcond, stat, s));
    HIPCHECK(ctx, hipEventRecord(ctx->cov_ev[2], s));
    HIPCHECK(ctx, launch_cov_points(P, ctx->C, W.st, Z, ld, d_idx + 2 * (size_t)npairs, nreq, ctx->buf[B_COV_W].as<double>(),
                                    d_out + 36 * (size_t)npairs, rcond, stat, s));
    HIPCHECK(ctx, hipEventRecord(ctx->cov_ev[3], s));
    // S and rhs as a prepare leaves them (the next solve's first assembly adds onto zeros)
    HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_S].p, 0, sizeof(double) * (size_t)P.npad * P.npad, s));
    HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_RHS].p, 0, sizeof(double) * P.npad, s));
    if (W.sw_cnt) HIPCHECK(ctx, hipMemsetAsync(W.sw_cnt, 0, sizeof(unsigned), s));
    W.sw_seq = 0;
    CovStat h_stat{};
    double lin_h[LIN_N];
    HIPCHECK(ctx, stg.d2h(&h_stat, stat, sizeof(CovStat)));
    HIPCHECK(ctx, stg.d2h(lin_h, W.lin, sizeof(lin_h)));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    const bool deficient = h_stat.flag != 0 || !(h_stat.pmin / h_stat.pmax >= rcond);
    const double nan = std::nan("");
    if (deficient) {
        if (npairs) std::fill(req->pair_cov, req->pair_cov + 36 * (size_t)npairs, nan);
        if (nreq) std::fill(req->point_cov, req->point_cov + 9 * (size_t)nreq, nan);
        if (req->full) std::fill(req->full, req->full + (size_t)n * n, nan);
    } else {
        HIPCHECK(ctx, stg.d2h(req->pair_cov, d_out, sizeof(double) * 36 * (size_t)npairs));
        HIPCHECK(ctx, stg.d2h(req->point_cov, d_out + 36 * (size_t)npairs, sizeof(double) * 9 * (size_t)nreq));
        if (req->full)
            HIPCHECK(ctx, hipMemcpy2DAsync(req->full, sizeof(double) * n, Z, sizeof(double) * ld, sizeof(double) * n, n,
                                           hipMemcpyDeviceToHost, s));
        HIPCHECK(ctx, hipStreamSynchronize(s));
    }
    ba_cov_info full{};
    full.struct_size = (int32_t)sizeof(ba_cov_info);
    full.status = deficient ? BA_COV_RANK_DEFICIENT : BA_COV_OK;
    full.n = n;
    full.nac = P.nac;
    full.pivot_min = h_stat.pmin;
    full.pivot_max = h_stat.pmax;
    full.cost = lin_h[0];
    const double dof = 3.0 * P.n_adm + 4.0 - (6.0 * P.nac + 3.0 * P.n_ap + 4.0);
    full.variance_factor = dof > 0 ? 2.0 * lin_h[0] / dof : 0.0;
    float ms[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], ctx->cov_ev[k], ctx->cov_ev[k + 1]);
    full.time_build_ms = ms[0];
    full.time_invert_ms = ms[1];
    full.time_points_ms = ms[2];
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    return BA_OK;
}
