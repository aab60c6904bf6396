// ba_align.cpp — ba_align of include/ba.h: batched RANSAC relative pose from 3D-3D correspondences (the kernels of
// ba_align.hip: every hypothesis's inlier count, then the pick, the refit rounds and the outputs of each pair).
// A stage beside the LM loop like ba_localize: it works on device buffers of its own (B_ALIGN_*), so nothing the plan
// or the LM loop reads is written. The host validates, uploads, launches twice, reads back and adds k_needed.
#include "ba_align.h"
#include "ba_stage.h"

#include <cmath>
#include <limits>

using namespace miba;

static_assert(ALIGN_STAT == BA_ALIGN_STAT_N, "the kernel writes the header's record width");
static_assert(BA_ALIGN_MAX_HYP % ALIGN_TPB == 0, "the cap is whole workgroups of hypotheses");

namespace {

std::string align_check(ba_context* ctx, const ba_align_problem* p, const ba_align_request* req, const ba_align_info* info) {
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_ALIGN)); !m.empty()) return m;
    if (p->n_pairs < 0 || p->n_corr < 0) return "negative sizes";
    if (!p->pair_begin) return "null required buffer (pair_begin)";
    if (p->pair_begin[0] < 0) return "pair_begin starts below 0";
    for (int32_t j = 0; j < p->n_pairs; ++j)
        if (p->pair_begin[j + 1] < p->pair_begin[j]) return "pair_begin decreases (pair " + std::to_string(j) + ")";
    if (p->pair_begin[p->n_pairs] != p->n_corr)
        return "pair_begin ends at " + std::to_string(p->pair_begin[p->n_pairs]) + ", not at n_corr = " + std::to_string(p->n_corr);
    if (p->n_corr && (!p->p1 || !p->p2)) return "null required buffer (p1 / p2)";
    if (p->n_pairs && !req->poses) return "null required buffer (poses)";
    if (req->n_hypotheses > BA_ALIGN_MAX_HYP)
        return "n_hypotheses = " + std::to_string(req->n_hypotheses) + " is above BA_ALIGN_MAX_HYP (" +
               std::to_string(BA_ALIGN_MAX_HYP) + ")";
    return "";
}

}  // namespace

extern "C" int32_t ba_align(ba_context* ctx, const ba_align_problem* p, const ba_align_request* req, ba_align_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_align", ctx->stream};
    if (const std::string m = align_check(ctx, p, req, info); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    const int nh = req->n_hypotheses > 0 ? req->n_hypotheses : 256;
    const double thr = req->threshold > 0.0 ? req->threshold : 0.1;
    const double min_cross = req->min_cross > 0.0 ? req->min_cross : 1e-6;
    const double prob = req->probability > 0.0 ? req->probability : 0.999;
    const size_t np = (size_t)p->n_pairs, ncr = (size_t)p->n_corr;
    if (np * (size_t)align_hyp_blocks(nh) > (size_t)std::numeric_limits<int32_t>::max())
        return stg.invalid("n_pairs x n_hypotheses is above the grid's limit of 2^31 workgroups of " +
                           std::to_string(ALIGN_TPB) + " hypotheses");
    ba_align_info full{};
    full.struct_size = (int32_t)sizeof(ba_align_info);
    full.n_pairs = p->n_pairs;
    full.n_hypotheses = nh;
    float kernels_ms = 0.f;

    if (np) {
        HIPCHECK(ctx, hipSetDevice(ctx->device));
        HIPCHECK(ctx, stg.events(ctx->align_ev, 2));
        hipStream_t s = stg.s;
        // in: p1 (3 n_corr) | p2 (3 n_corr) doubles, then pair_begin (n_pairs + 1) ints
        // out: poses (7 n_pairs) | stats (8 n_pairs) doubles, then hyp_count (n_pairs nh) ints, then the mask (n_corr)
        const size_t in_bytes = 8 * 6 * ncr + 4 * (np + 1);
        const size_t out_d = (7 + ALIGN_STAT) * np, n_cnt = np * (size_t)nh;
        const size_t out_bytes = 8 * out_d + 4 * n_cnt + ncr;
        if (int32_t rc = stg.ensure(B_ALIGN_IN, in_bytes, "the correspondences' copy")) return rc;
        if (int32_t rc = stg.ensure(B_ALIGN_OUT, out_bytes, "the hypotheses' counts")) return rc;
        double* d_p1 = ctx->buf[B_ALIGN_IN].as<double>();
        double* d_p2 = d_p1 + 3 * ncr;
        int* d_begin = reinterpret_cast<int*>(d_p2 + 3 * ncr);
        double* d_poses = ctx->buf[B_ALIGN_OUT].as<double>();
        double* d_stats = d_poses + 7 * np;
        int* d_cnt = reinterpret_cast<int*>(d_stats + ALIGN_STAT * np);
        unsigned char* d_mask = reinterpret_cast<unsigned char*>(d_cnt + n_cnt);
        HIPCHECK(ctx, stg.h2d(d_p1, p->p1, 24 * ncr));
        HIPCHECK(ctx, stg.h2d(d_p2, p->p2, 24 * ncr));
        HIPCHECK(ctx, stg.h2d(d_begin, p->pair_begin, 4 * (np + 1)));
        // (the correspondences before pair_begin[0] belong to no pair: their mask stays 0)
        if (ncr) HIPCHECK(ctx, hipMemsetAsync(d_mask, 0, ncr, s));

        AlignArgs a{};
        a.pair_begin = d_begin; a.p1 = d_p1; a.p2 = d_p2;
        a.n_pairs = p->n_pairs; a.n_hyp = nh; a.refit = std::max(req->refit, 0);
        a.seed = req->seed;
        a.thr2 = thr * thr; a.min_cross2 = min_cross * min_cross;
        a.hyp_count = d_cnt; a.poses = d_poses; a.stats = d_stats; a.inlier = d_mask;
        HIPCHECK(ctx, hipEventRecord(ctx->align_ev[0], s));
        HIPCHECK(ctx, launch_align_hyp(a, s));
        HIPCHECK(ctx, launch_align_pick(a, s));
        HIPCHECK(ctx, hipEventRecord(ctx->align_ev[1], s));

        std::vector<double> stats(ALIGN_STAT * np);
        HIPCHECK(ctx, stg.d2h(req->poses, d_poses, 56 * np));
        HIPCHECK(ctx, stg.d2h(stats.data(), d_stats, 8 * ALIGN_STAT * np));
        if (req->hyp_count) HIPCHECK(ctx, stg.d2h(req->hyp_count, d_cnt, 4 * n_cnt));
        if (req->inlier) HIPCHECK(ctx, stg.d2h(req->inlier, d_mask, ncr));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&kernels_ms, ctx->align_ev[0], ctx->align_ev[1]);

        for (size_t j = 0; j < np; ++j) {
            double* st = &stats[ALIGN_STAT * j];
            const int status = (int)st[0];
            if (status == BA_ALIGN_OK) {
                ++full.n_ok;
                // OpenGV's adaptive iteration count from the best sample's inlier share
                const double w = st[6] / st[1], w3 = w * w * w;
                st[7] = w3 <= 0.0 ? std::numeric_limits<double>::infinity()
                        : w3 >= 1.0 ? 0.0 : std::log(1.0 - prob) / std::log(1.0 - w3);
            } else if (status == BA_ALIGN_TOO_FEW) {
                ++full.n_too_few;
            } else {
                ++full.n_no_model;
            }
        }
        if (req->pair_stats) std::memcpy(req->pair_stats, stats.data(), 8 * ALIGN_STAT * np);
    }

    full.time_kernels_ms = kernels_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
