// ba_covis.cpp — ba_covisibility and ba_solve_ordered of include/ba.h: the keyframe co-visibility graph of a window
// (kernels of ba_covis.hip), the camera order that narrows its band (ba_order.cpp) and the solve in that order.
// ba_covisibility is a stage beside the LM loop: device buffers of its own, nothing the plan or the LM loop reads is
// written. ba_solve_ordered is ba_solve on a shadow problem the context keeps.
#include "ba_context.h"
#include "ba_covis.h"
#include "ba_order.h"

using namespace miba;

namespace {

// ba_prepare's verdict on the sizes and buffers this call reads, then on every observation's indices (the kernels
// index with them unchecked).
const char* covis_validate(const ba_problem* p) {
    if (p->n_cams < 0 || p->n_points < 0 || p->n_obs < 0) return "invalid problem sizes";
    if (p->n_obs && (!p->obs_cam || !p->obs_pt || !p->obs_depth)) return "null problem buffer";
    for (int32_t k = 0; k < p->n_obs; ++k)
        if (p->obs_cam[k] < 0 || p->obs_cam[k] >= p->n_cams || p->obs_pt[k] < 0 || p->obs_pt[k] >= p->n_points)
            return "observation index out of range";
    return "";
}

// a camera's position among the first n_active entries of `order` (-1: the gauge camera / no admissible observation)
void positions(const int32_t* order, int n_active, int n_cams, int32_t* pos) {
    std::fill(pos, pos + n_cams, -1);
    for (int k = 0; k < n_active; ++k) pos[order[k]] = k;
}

}  // namespace

extern "C" int32_t ba_covisibility(ba_context* ctx, const ba_problem* p, const ba_covis_request* req,
                                   ba_covis_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    auto invalid = [&](const std::string& m) { ctx->err = "ba_covisibility: " + m; return (int32_t)BA_E_INVALID; };
    if (!p || !req || !info) return invalid("null argument");
    if (req->struct_size < BA_COVIS_REQUEST_MIN_SIZE)
        return invalid("request struct_size below BA_COVIS_REQUEST_MIN_SIZE (set it with BA_COVIS_REQUEST_INIT)");
    if (info->struct_size < BA_COVIS_INFO_MIN_SIZE)
        return invalid("info struct_size below BA_COVIS_INFO_MIN_SIZE (set it with BA_COVIS_INFO_INIT)");
    if (ctx->W.comm.on() || ctx->comm_parked.on())
        return invalid("contexts with landmark shards (ba_comm_init*) are not supported");
    const double t0 = now_ms();
    if (const char* m = covis_validate(p); *m) return invalid(m);
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    for (auto& e : ctx->covis_ev)
        if (!e) HIPCHECK(ctx, hipEventCreate(&e));
    hipStream_t s = ctx->stream;
    const size_t nc = (size_t)p->n_cams, np = (size_t)p->n_points, no = (size_t)p->n_obs;
    const size_t nw = covis_row_words(p->n_points);

    // depths | camera indices | point indices; the bit matrix; the weights; positions (2 nc) | spans (4 np) | counts (2)
    auto nomem = [&](const char* what, size_t bytes) {
        (void)hipGetLastError();
        ctx->err = std::string("ba_covisibility: cannot allocate ") + what + " (" + std::to_string(bytes) + " bytes)";
        return (int32_t)BA_E_NOMEM;
    };
    const size_t obs_bytes = 16 * std::max<size_t>(no, 1), bits_bytes = 8 * std::max<size_t>(nc * nw, 1);
    const size_t w_bytes = 4 * std::max<size_t>(nc * nc, 1), span_bytes = 4 * (2 * nc + 4 * np + 2);
    if (ctx->buf[B_COVIS_OBS].ensure(obs_bytes) != hipSuccess) return nomem("the observation copies", obs_bytes);
    if (ctx->buf[B_COVIS_BITS].ensure(bits_bytes) != hipSuccess) return nomem("the camera x point bit matrix", bits_bytes);
    if (ctx->buf[B_COVIS_W].ensure(w_bytes) != hipSuccess) return nomem("the weights", w_bytes);
    if (ctx->buf[B_COVIS_SPAN].ensure(span_bytes) != hipSuccess) return nomem("the span scratch", span_bytes);
    double* d_dep = ctx->buf[B_COVIS_OBS].as<double>();
    int* d_cam = reinterpret_cast<int*>(d_dep + no);
    int* d_pt = d_cam + no;
    unsigned long long* d_bits = ctx->buf[B_COVIS_BITS].as<unsigned long long>();
    int* d_W = ctx->buf[B_COVIS_W].as<int>();
    int* d_pos0 = ctx->buf[B_COVIS_SPAN].as<int>();
    int* d_pos1 = d_pos0 + nc;
    int* d_span = d_pos1 + nc;
    int* d_wide = d_span + 4 * np;

    auto h2d = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHECK(ctx, h2d(d_dep, p->obs_depth, sizeof(double) * no));
    HIPCHECK(ctx, h2d(d_cam, p->obs_cam, sizeof(int32_t) * no));
    HIPCHECK(ctx, h2d(d_pt, p->obs_pt, sizeof(int32_t) * no));
    HIPCHECK(ctx, hipEventRecord(ctx->covis_ev[0], s));
    HIPCHECK(ctx, hipMemsetAsync(d_bits, 0, bits_bytes, s));
    HIPCHECK(ctx, hipMemsetAsync(d_W, 0, w_bytes, s));
    HIPCHECK(ctx, launch_covis_bits(d_cam, d_pt, d_dep, p->n_obs, p->n_points, d_bits, s));
    HIPCHECK(ctx, launch_covis_count(d_bits, p->n_cams, p->n_points, d_W, s));
    HIPCHECK(ctx, hipEventRecord(ctx->covis_ev[1], s));
    std::vector<int32_t> W_tmp;
    int32_t* W = req->weights;
    if (!W) { W_tmp.resize(std::max<size_t>(nc * nc, 1)); W = W_tmp.data(); }
    if (nc) HIPCHECK(ctx, hipMemcpyAsync(W, d_W, sizeof(int32_t) * nc * nc, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));

    // the candidate order on the host, then what it does to the points' spans on the device
    const double t_order = now_ms();
    CamOrder co;
    // the context's constant cameras count as the gauge camera does (a mask set for another n_cams: BA_E_INVALID, as
    // a prepare of this window would say)
    if (ctx->cmask_any && ctx->cmask.size() != nc)
        return invalid("the window has " + std::to_string(p->n_cams) + " cameras, the constant-camera mask was set for " +
                       std::to_string(ctx->cmask.size()));
    const uint8_t* cam_const = ctx->cmask_any ? ctx->cmask.data() : nullptr;
    covis_order(W, p->n_cams, p->fixed_cam, cam_const, co);
    std::vector<int32_t> pos(2 * nc), given;
    for (int i = 0; i < p->n_cams; ++i)
        if (W[nc * i + i] > 0 && i != p->fixed_cam && !(cam_const && cam_const[i])) given.push_back(i);
    positions(given.data(), co.n_active, p->n_cams, pos.data());
    positions(co.order.data(), co.n_active, p->n_cams, pos.data() + nc);
    int32_t wide[2] = {0, 0};
    HIPCHECK(ctx, h2d(d_pos0, pos.data(), sizeof(int32_t) * 2 * nc));
    HIPCHECK(ctx, launch_covis_span(d_cam, d_pt, d_dep, p->n_obs, p->n_points, d_pos0, d_pos1, TILE_WIN, d_span, d_wide, s));
    HIPCHECK(ctx, hipMemcpyAsync(wide, d_wide, sizeof(wide), hipMemcpyDeviceToHost, s));
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
    const int32_t keep = info->struct_size;
    std::memcpy(info, &full, std::min<size_t>((size_t)keep, sizeof(full)));
    info->struct_size = keep;
    ctx->err.clear();
    return BA_OK;
}

extern "C" int32_t ba_solve_ordered(ba_context* ctx, ba_problem* p, const int32_t* order, ba_summary* sum) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    auto invalid = [&](const std::string& m) { ctx->err = "ba_solve_ordered: " + m; return (int32_t)BA_E_INVALID; };
    if (!p || !sum) return invalid("null argument");
    if (ctx->W.comm.on() || ctx->comm_parked.on())
        return invalid("contexts with landmark shards (ba_comm_init*) are not supported");
    if (p->n_cams < 0 || p->n_points < 0 || p->n_obs < 0) return invalid("invalid problem sizes");
    if ((p->n_cams && !p->cams) || (p->n_obs && !p->obs_cam)) return invalid("null problem buffer");
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
        if (c < 0 || c >= nc) return invalid("order[" + std::to_string(k) + "] = " + std::to_string(c) + " is out of range");
        if (sh.inv[c] >= 0) return invalid("order repeats camera " + std::to_string(c) + ": not a permutation");
        sh.inv[c] = k;
    }
    sh.cams.resize((size_t)nc * 7);
    for (int k = 0; k < nc; ++k) std::memcpy(&sh.cams[(size_t)k * 7], p->cams + (size_t)order[k] * 7, 7 * sizeof(double));
    sh.obs_cam.resize((size_t)p->n_obs);
    for (int32_t k = 0; k < p->n_obs; ++k) {
        const int32_t c = p->obs_cam[k];
        if (c < 0 || c >= nc) return invalid("observation index out of range");
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
