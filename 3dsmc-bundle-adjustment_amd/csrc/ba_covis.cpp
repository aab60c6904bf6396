// ba_covis.cpp — ba_covisibility and ba_solve_ordered of include/ba.h: the keyframe co-visibility graph of a window
// (kernels of ba_covis.hip), the camera order that narrows its band (ba_order.cpp) and the solve in that order.
// ba_covisibility is a stage beside the LM loop: device buffers of its own, nothing the plan or the LM loop reads is
// written. ba_solve_ordered is ba_solve on a shadow problem the context keeps.
#include "ba_covis.h"
#include "ba_order.h"
#include "ba_stage.h"

using namespace miba;

int32_t miba::covis_upload_bits(const Stage& stg, const ba_problem* p, hipEvent_t start, CovisBits& b) {
    ba_context* ctx = stg.ctx;
    const size_t nc = (size_t)p->n_cams, no = (size_t)p->n_obs;
    b.dep = ctx->buf[B_COVIS_OBS].as<double>();
    b.cam = reinterpret_cast<int*>(b.dep + no);
    b.pt = b.cam + no;
    b.bits = ctx->buf[B_COVIS_BITS].as<unsigned long long>();
    HIPCHECK(ctx, stg.h2d(b.dep, p->obs_depth, sizeof(double) * no));
    HIPCHECK(ctx, stg.h2d(b.cam, p->obs_cam, sizeof(int32_t) * no));
    HIPCHECK(ctx, stg.h2d(b.pt, p->obs_pt, sizeof(int32_t) * no));
    HIPCHECK(ctx, hipEventRecord(start, stg.s));
    HIPCHECK(ctx, hipMemsetAsync(b.bits, 0, covis_bits_bytes(nc, covis_row_words(p->n_points)), stg.s));
    HIPCHECK(ctx, launch_covis_bits(b.cam, b.pt, b.dep, p->n_obs, p->n_points, b.bits, stg.s));
    return BA_OK;
}

namespace {

// a camera's position among the first n_active entries of `order` (-1: the gauge camera / no admissible observation)
void positions(const int32_t* order, int n_active, int n_cams, int32_t* pos) {
    std::fill(pos, pos + n_cams, -1);
    for (int k = 0; k < n_active; ++k) pos[order[k]] = k;
}

}  // namespace

extern "C" int32_t ba_covisibility(ba_context* ctx, const ba_problem* p, const ba_covis_request* req,
                                   ba_covis_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_covisibility", ctx->stream};
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_COVIS)); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    if (const char* m = stage_validate_problem(p, STAGE_OBS); *m) return stg.invalid(m);
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    HIPCHECK(ctx, stg.events(ctx->covis_ev, 2));
    hipStream_t s = stg.s;
    const size_t nc = (size_t)p->n_cams, np = (size_t)p->n_points, no = (size_t)p->n_obs;
    const size_t nw = covis_row_words(p->n_points);

    // depths | camera indices | point indices; the bit matrix; the weights; positions (2 nc) | spans (4 np) | counts (2)
    const size_t obs_bytes = covis_obs_bytes(no), bits_bytes = covis_bits_bytes(nc, nw);
    const size_t w_bytes = 4 * std::max<size_t>(nc * nc, 1), span_bytes = 4 * (2 * nc + 4 * np + 2);
    if (int32_t rc = stg.ensure(B_COVIS_OBS, obs_bytes, "the observation copies")) return rc;
    if (int32_t rc = stg.ensure(B_COVIS_BITS, bits_bytes, "the camera x point bit matrix")) return rc;
    if (int32_t rc = stg.ensure(B_COVIS_W, w_bytes, "the weights")) return rc;
    if (int32_t rc = stg.ensure(B_COVIS_SPAN, span_bytes, "the span scratch")) return rc;
    int* d_W = ctx->buf[B_COVIS_W].as<int>();
    int* d_pos0 = ctx->buf[B_COVIS_SPAN].as<int>();
    int* d_pos1 = d_pos0 + nc;
    int* d_span = d_pos1 + nc;
    int* d_wide = d_span + 4 * np;

    CovisBits cb{};
    if (int32_t rc = covis_upload_bits(stg, p, ctx->covis_ev[0], cb)) return rc;
    HIPCHECK(ctx, hipMemsetAsync(d_W, 0, w_bytes, s));
    HIPCHECK(ctx, launch_covis_count(cb.bits, p->n_cams, p->n_points, d_W, s));
    HIPCHECK(ctx, hipEventRecord(ctx->covis_ev[1], s));
    std::vector<int32_t> W_tmp;
    int32_t* W = req->weights;
    if (!W) { W_tmp.resize(std::max<size_t>(nc * nc, 1)); W = W_tmp.data(); }
    HIPCHECK(ctx, stg.d2h(W, d_W, sizeof(int32_t) * nc * nc));
    HIPCHECK(ctx, hipStreamSynchronize(s));

    // the candidate order on the host, then what it does to the points' spans on the device
    const double t_order = now_ms();
    CamOrder co;
    // the context's constant cameras count as the gauge camera does (a mask set for another n_cams: BA_E_INVALID, as
    // a prepare of this window would say)
    if (ctx->cmask_any && ctx->cmask.size() != nc)
        return stg.invalid("the window has " + std::to_string(p->n_cams) +
                           " cameras, the constant-camera mask was set for " + std::to_string(ctx->cmask.size()));
    const uint8_t* cam_const = ctx->cmask_any ? ctx->cmask.data() : nullptr;
    covis_order(W, p->n_cams, p->fixed_cam, cam_const, co);
    std::vector<int32_t> pos(2 * nc), given;
    for (int i = 0; i < p->n_cams; ++i)
        if (W[nc * i + i] > 0 && i != p->fixed_cam && !(cam_const && cam_const[i])) given.push_back(i);
    positions(given.data(), co.n_active, p->n_cams, pos.data());
    positions(co.order.data(), co.n_active, p->n_cams, pos.data() + nc);
    int32_t wide[2] = {0, 0};
    HIPCHECK(ctx, stg.h2d(d_pos0, pos.data(), sizeof(int32_t) * 2 * nc));
    HIPCHECK(ctx, launch_covis_span(cb.cam, cb.pt, cb.dep, p->n_obs, p->n_points, d_pos0, d_pos1, TILE_WIN, d_span, d_wide, s));
    HIPCHECK(ctx, stg.d2h(wide, d_wide, sizeof(wide)));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    const bool accept = co.band_after < co.band_before && wide[1] <= wide[0];
    if (req->order)
        for (int k = 0; k < p->n_cams; ++k) req->order[k] = accept ? co.order[k] : k;

    ba_covis_info full{};
    full.struct_size = (int32_t)sizeof(ba_covis_info);
    full.n_active = co.n_active;
    full.n_edges = co.n_edges;
    full.n_components = co.n_components;
    full.band_before = co.band_before;
    full.band_after = accept ? co.band_after : co.band_before;
    full.wide_before = wide[0];
    full.wide_after = accept ? wide[1] : wide[0];
    full.order_changed = accept ? 1 : 0;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->covis_ev[0], ctx->covis_ev[1]);
    full.time_count_ms = ms;
    full.time_order_ms = now_ms() - t_order;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}

extern "C" int32_t ba_solve_ordered(ba_context* ctx, ba_problem* p, const int32_t* order, ba_summary* sum) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_solve_ordered", ctx->stream};
    if (!p || !sum) return stg.invalid("null argument");
    // (its own checks: no request / info, and of the buffers only those the shadow problem is built from)
    if (ctx->W.comm.on() || ctx->comm_parked.on()) return stg.invalid(kStageShards);
    if (p->n_cams < 0 || p->n_points < 0 || p->n_obs < 0) return stg.invalid(kBadSizes);
    if ((p->n_cams && !p->cams) || (p->n_obs && !p->obs_cam)) return stg.invalid(kNullBuffer);
    const int nc = p->n_cams;
    ba_context::Ordered& sh = ctx->ordered;
    if (!order) {
        sh.order.assign((size_t)std::max(nc, 1), 0);
        ba_covis_request req;
        ba_covis_info info;
        BA_COVIS_REQUEST_INIT(req);
        BA_COVIS_INFO_INIT(info);
        req.order = sh.order.data();
        if (int32_t rc = ba_covisibility(ctx, p, &req, &info)) return rc;
        order = sh.order.data();
    }
    sh.inv.assign((size_t)nc, -1);
    for (int k = 0; k < nc; ++k) {
        const int32_t c = order[k];
        if (c < 0 || c >= nc) return stg.invalid("order[" + std::to_string(k) + "] = " + std::to_string(c) + " is out of range");
        if (sh.inv[c] >= 0) return stg.invalid("order repeats camera " + std::to_string(c) + ": not a permutation");
        sh.inv[c] = k;
    }
    sh.cams.resize((size_t)nc * 7);
    for (int k = 0; k < nc; ++k) std::memcpy(&sh.cams[(size_t)k * 7], p->cams + (size_t)order[k] * 7, 7 * sizeof(double));
    sh.obs_cam.resize((size_t)p->n_obs);
    for (int32_t k = 0; k < p->n_obs; ++k) {
        const int32_t c = p->obs_cam[k];
        if (c < 0 || c >= nc) return stg.invalid(kBadIndex);
        sh.obs_cam[k] = sh.inv[c];
    }
    ba_problem shadow = *p;
    shadow.cams = sh.cams.data();
    shadow.obs_cam = sh.obs_cam.data();
    if (p->fixed_cam >= 0 && p->fixed_cam < nc) shadow.fixed_cam = sh.inv[p->fixed_cam];
    // the shadow problem carries the constant cameras at their new positions; the caller's mask is back afterwards
    const std::vector<uint8_t> given_mask = ctx->cmask;
    if (ctx->cmask_any && ctx->cmask.size() == (size_t)nc)
        for (int k = 0; k < nc; ++k) ctx->cmask[k] = given_mask[order[k]];
    const int32_t rc = ba_solve(ctx, &shadow, sum);
    ctx->cmask = given_mask;
    if (rc != BA_OK) return rc;
    for (int k = 0; k < nc; ++k) std::memcpy(p->cams + (size_t)order[k] * 7, &sh.cams[(size_t)k * 7], 7 * sizeof(double));
    return BA_OK;
}
