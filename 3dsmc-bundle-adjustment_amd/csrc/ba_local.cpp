// ba_local.cpp — ba_local_window and ba_solve_local of include/ba.h: the co-visibility-selected window around a
// camera of a map (kernels of ba_local.hip over ba_covis.hip's bit matrix; the sort of the weight row on the host, as
// ba_covisibility's Cuthill-McKee is) and the solve of that sub-window under its constant cameras.
// ba_local_window is a stage beside the LM loop, like ba_covisibility, whose observation and bit-matrix buffers it
// shares: nothing the plan or the LM loop reads is written. ba_solve_local is ba_solve on a shadow problem the
// context keeps.
#include "ba_covis.h"
#include "ba_local.h"
#include "ba_stage.h"

using namespace miba;

namespace {

// The selection into ctx->local (every list sized to what it holds) and `full`; the request's buffers are the caller's.
// (Its allocation failures read "ba_local_window: ..." under either entry point.)
int32_t local_select(ba_context* ctx, const ba_problem* p, int center, int min_weight, int max_local, ba_local_info& full) {
    const double t0 = now_ms();
    const Stage stg{ctx, "ba_local_window", ctx->stream};
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    HIPCHECK(ctx, stg.events(ctx->local_ev, 2));
    hipStream_t s = stg.s;
    hipEvent_t* ev = ctx->local_ev;
    const size_t nc = (size_t)p->n_cams, np = (size_t)p->n_points, no = (size_t)p->n_obs;
    const size_t nw = covis_row_words(p->n_points);
    ba_context::Local& out = ctx->local;
    if (min_weight <= 0) min_weight = 1;

    // work: P (nw words) | wcnt, wrank (nw) | cnt, sel, cam_new (nc) | pt_new (np) | oscan (no) | the scans' workgroup
    // sums | the two totals; out: pt_index (np) | obs_index, sub_cam, sub_pt (no)
    const size_t nbs = (size_t)std::max(local_scan_blocks(nw), local_scan_blocks(no)) + 1;
    const size_t work_bytes = 8 * nw + 4 * (2 * nw + 3 * nc + np + no + nbs + 2), out_bytes = 4 * (np + 3 * no + 1);
    if (int32_t rc = stg.ensure(B_COVIS_OBS, covis_obs_bytes(no), "the observation copies")) return rc;
    if (int32_t rc = stg.ensure(B_COVIS_BITS, covis_bits_bytes(nc, nw), "the camera x point bit matrix")) return rc;
    if (int32_t rc = stg.ensure(B_LOCAL_WORK, work_bytes, "the selection scratch")) return rc;
    if (int32_t rc = stg.ensure(B_LOCAL_OUT, out_bytes, "the selection outputs")) return rc;
    unsigned long long* d_P = ctx->buf[B_LOCAL_WORK].as<unsigned long long>();
    int* d_wcnt = reinterpret_cast<int*>(d_P + nw);
    int* d_wrank = d_wcnt + nw;
    int* d_cnt = d_wrank + nw;
    int* d_sel = d_cnt + nc;
    int* d_cam_new = d_sel + nc;
    int* d_pt_new = d_cam_new + nc;
    int* d_oscan = d_pt_new + np;
    int* d_bsum = d_oscan + no;
    int* d_total = d_bsum + nbs;
    int* d_pt_index = ctx->buf[B_LOCAL_OUT].as<int>();
    int* d_obs_index = d_pt_index + np;
    int* d_sub_cam = d_obs_index + no;
    int* d_sub_pt = d_sub_cam + no;

    float ms = 0.f, part = 0.f;
    // 1. the bit matrix and the weight row
    CovisBits cb{};
    if (int32_t rc = covis_upload_bits(stg, p, ev[0], cb)) return rc;
    HIPCHECK(ctx, launch_local_rows(cb.bits, cb.bits + (size_t)center * nw, p->n_cams, nw, d_cnt, s));
    HIPCHECK(ctx, hipEventRecord(ev[1], s));
    out.w.assign(nc, 0);
    HIPCHECK(ctx, stg.d2h(out.w.data(), d_cnt, sizeof(int32_t) * nc));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&part, ev[0], ev[1]);
    ms += part;

    // 2. the local cameras on the host: the sort of at most n_cams weights
    std::vector<int32_t> L{center};
    if (out.w[center] > 0) {
        std::vector<int32_t> cand;
        for (int a = 0; a < p->n_cams; ++a)
            if (a != center && out.w[a] >= min_weight) cand.push_back(a);
        if (max_local > 0 && 1 + cand.size() > (size_t)max_local) {
            std::sort(cand.begin(), cand.end(),
                      [&](int a, int b) { return out.w[a] != out.w[b] ? out.w[a] > out.w[b] : a < b; });
            cand.resize((size_t)max_local - 1);
        }
        L.insert(L.end(), cand.begin(), cand.end());
        std::sort(L.begin(), L.end());
    }
    std::vector<uint8_t> in_L(nc, 0);
    for (int a : L) in_L[a] = 1;
    out.cam_index.clear(); out.cam_constant.clear(); out.is_local.clear(); out.pt_index.clear();
    out.obs_index.clear(); out.obs_cam.clear(); out.obs_pt.clear();
    full = ba_local_info{};
    full.struct_size = (int32_t)sizeof(ba_local_info);
    full.n_local = (int32_t)L.size();
    if (out.w[center] == 0) {  // no admissible observation: L = {center}, everything else empty
        out.cam_index.push_back(center);
        out.cam_constant.push_back(0);
        out.is_local.push_back(1);
        full.sub_fixed_cam = 0;
        full.time_select_ms = ms;
        full.time_total_ms = now_ms() - t0;
        return BA_OK;
    }

    // 3. the local points and the cameras that see them
    std::vector<int32_t> cnt(nc, 0);
    HIPCHECK(ctx, stg.h2d(d_sel, L.data(), sizeof(int32_t) * L.size()));
    HIPCHECK(ctx, hipEventRecord(ev[0], s));
    HIPCHECK(ctx, launch_local_or(cb.bits, d_sel, (int)L.size(), nw, d_P, d_wcnt, s));
    HIPCHECK(ctx, launch_local_rows(cb.bits, d_P, p->n_cams, nw, d_cnt, s));
    HIPCHECK(ctx, hipEventRecord(ev[1], s));
    HIPCHECK(ctx, stg.d2h(cnt.data(), d_cnt, sizeof(int32_t) * nc));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&part, ev[0], ev[1]);
    ms += part;
    std::vector<int32_t> cam_new(nc, -1);
    const bool masked = ctx->cmask_any && ctx->cmask.size() == nc;
    bool any_const = false;
    for (int a = 0; a < p->n_cams; ++a) {
        if (!in_L[a] && cnt[a] <= 0) continue;
        const bool c = !in_L[a] || a == p->fixed_cam || (masked && ctx->cmask[a]);
        cam_new[a] = (int32_t)out.cam_index.size();
        out.cam_index.push_back(a);
        out.cam_constant.push_back(c ? 1 : 0);
        out.is_local.push_back(in_L[a]);
        any_const = any_const || c;
        if (!in_L[a]) ++full.n_fixed;
    }
    full.sub_fixed_cam = any_const ? -1 : cam_new[L[0]];

    // 4. the points' ranks and the observations' compaction
    int32_t total[2] = {0, 0};
    HIPCHECK(ctx, stg.h2d(d_cam_new, cam_new.data(), sizeof(int32_t) * nc));
    HIPCHECK(ctx, hipEventRecord(ev[0], s));
    HIPCHECK(ctx, launch_local_points(d_P, d_wcnt, p->n_points, nw, d_wrank, d_bsum, d_pt_new, d_pt_index, d_total, s));
    HIPCHECK(ctx, launch_local_obs(cb.cam, cb.pt, cb.dep, p->n_obs, d_P, d_cam_new, d_pt_new, d_oscan, d_bsum, d_obs_index,
                                   d_sub_cam, d_sub_pt, d_total + 1, s));
    HIPCHECK(ctx, hipEventRecord(ev[1], s));
    HIPCHECK(ctx, stg.d2h(total, d_total, sizeof(total)));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&part, ev[0], ev[1]);
    ms += part;
    if (total[0] < 0 || (size_t)total[0] > np || total[1] < 0 || (size_t)total[1] > no) {
        ctx->err = "ba_local_window: the selection's counts are out of range";
        return BA_E_INTERNAL;
    }
    out.pt_index.resize((size_t)total[0]);
    out.obs_index.resize((size_t)total[1]);
    out.obs_cam.resize((size_t)total[1]);
    out.obs_pt.resize((size_t)total[1]);
    HIPCHECK(ctx, stg.d2h(out.pt_index.data(), d_pt_index, sizeof(int32_t) * total[0]));
    HIPCHECK(ctx, stg.d2h(out.obs_index.data(), d_obs_index, sizeof(int32_t) * total[1]));
    HIPCHECK(ctx, stg.d2h(out.obs_cam.data(), d_sub_cam, sizeof(int32_t) * total[1]));
    HIPCHECK(ctx, stg.d2h(out.obs_pt.data(), d_sub_pt, sizeof(int32_t) * total[1]));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    full.n_points = total[0];
    full.n_obs = total[1];
    full.time_select_ms = ms;
    full.time_total_ms = now_ms() - t0;
    return BA_OK;
}

// the arguments' verdict shared by the two entry points ("" when they are usable)
std::string local_check(ba_context* ctx, const ba_problem* p, const ba_local_request* req, const ba_local_info* info) {
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_LOCAL)); !m.empty()) return m;
    if (const char* m = stage_validate_problem(p, STAGE_OBS); *m) return m;
    if (req->center < 0 || req->center >= p->n_cams)
        return "center = " + std::to_string(req->center) + " is out of range (" + std::to_string(p->n_cams) + " cameras)";
    return "";
}

// ctx->local and `full` into the caller's buffers
void local_publish(const ba_context* ctx, const ba_local_request* req, const ba_local_info& full, ba_local_info* info) {
    const ba_context::Local& o = ctx->local;
    auto put = [](auto* dst, const auto& v) {
        if (dst) std::copy(v.begin(), v.end(), dst);
    };
    put(req->w, o.w);
    put(req->cam_index, o.cam_index);
    put(req->cam_constant, o.cam_constant);
    put(req->pt_index, o.pt_index);
    put(req->obs_index, o.obs_index);
    put(req->sub_obs_cam, o.obs_cam);
    put(req->sub_obs_pt, o.obs_pt);
    put(req->cam_local, o.is_local);
    sized_copy_out(info, full);
}

}  // namespace

extern "C" int32_t ba_local_window(ba_context* ctx, const ba_problem* p, const ba_local_request* req,
                                   ba_local_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    if (const std::string m = local_check(ctx, p, req, info); !m.empty())
        return Stage{ctx, "ba_local_window", ctx->stream}.invalid(m);
    ba_local_info full{};
    if (int32_t rc = local_select(ctx, p, req->center, req->min_weight, req->max_local, full)) return rc;
    local_publish(ctx, req, full, info);
    ctx->err.clear();
    return BA_OK;
}

extern "C" int32_t ba_solve_local(ba_context* ctx, ba_problem* p, const ba_local_request* req, ba_local_info* info,
                                  ba_summary* sum) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_solve_local", ctx->stream};
    if (!sum) return stg.invalid("null argument");
    if (const std::string m = local_check(ctx, p, req, info); !m.empty()) return stg.invalid(m);
    // (the solve's own buffers come after the selection's checks, the center's included)
    if (stage_missing_buffer(p, STAGE_PARAMS)) return stg.invalid(kNullBuffer);
    ba_local_info full{};
    if (int32_t rc = local_select(ctx, p, req->center, req->min_weight, req->max_local, full)) return rc;
    local_publish(ctx, req, full, info);

    // the sub-window as a shadow problem: cameras, points and observation values gathered
    ba_context::Local& sh = ctx->local;
    const size_t snc = sh.cam_index.size(), snp = sh.pt_index.size(), sno = sh.obs_index.size();
    sh.cams.resize(7 * snc);
    sh.pts.resize(3 * snp);
    sh.uv.resize(2 * sno);
    sh.dep.resize(sno);
    for (size_t k = 0; k < snc; ++k) std::memcpy(&sh.cams[7 * k], p->cams + 7 * (size_t)sh.cam_index[k], 7 * sizeof(double));
    for (size_t k = 0; k < snp; ++k) std::memcpy(&sh.pts[3 * k], p->points + 3 * (size_t)sh.pt_index[k], 3 * sizeof(double));
    for (size_t k = 0; k < sno; ++k) {
        const size_t o = (size_t)sh.obs_index[k];
        sh.uv[2 * k] = p->obs_uv[2 * o];
        sh.uv[2 * k + 1] = p->obs_uv[2 * o + 1];
        sh.dep[k] = p->obs_depth[o];
    }
    double intr_copy[4];
    std::memcpy(intr_copy, p->intr, sizeof(intr_copy));
    ba_problem shadow{};
    shadow.n_cams = (int32_t)snc;
    shadow.n_points = (int32_t)snp;
    shadow.n_obs = (int32_t)sno;
    shadow.fixed_cam = full.sub_fixed_cam;
    shadow.cams = sh.cams.data();
    shadow.points = sh.pts.data();
    // an empty sub-window is not solved: its summary is that of the empty window, the caller's intrinsics stay
    shadow.intr = sno ? p->intr : intr_copy;
    shadow.intr_prior = p->intr_prior;
    shadow.obs_cam = sh.obs_cam.data();
    shadow.obs_pt = sh.obs_pt.data();
    shadow.obs_uv = sh.uv.data();
    shadow.obs_depth = sh.dep.data();
    // the sub-window's constant set for the solve, the caller's own back in force afterwards
    std::vector<uint8_t> given_mask = sh.cam_constant;
    bool given_any = false;
    for (uint8_t c : given_mask) given_any = given_any || c;
    std::swap(ctx->cmask, given_mask);
    std::swap(ctx->cmask_any, given_any);
    const int32_t rc = ba_solve(ctx, &shadow, sum);
    std::swap(ctx->cmask, given_mask);
    std::swap(ctx->cmask_any, given_any);
    if (rc != BA_OK || !sno) return rc;
    for (size_t k = 0; k < snc; ++k)
        if (sh.is_local[k] && !sh.cam_constant[k] && (int32_t)k != full.sub_fixed_cam)
            std::memcpy(p->cams + 7 * (size_t)sh.cam_index[k], &sh.cams[7 * k], 7 * sizeof(double));
    for (size_t k = 0; k < snp; ++k) std::memcpy(p->points + 3 * (size_t)sh.pt_index[k], &sh.pts[3 * k], 3 * sizeof(double));
    return BA_OK;
}
