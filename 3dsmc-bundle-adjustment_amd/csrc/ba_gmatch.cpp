// ba_gmatch.cpp — ba_guided_match of include/ba.h: the descriptor search in a pixel window around projected landmarks
// (the kernels of ba_gmatch.hip: the binning of every distinct keypoint range, the search with the acceptance chain,
// the one-to-one pick, the ordered compaction). A stage beside the LM loop like ba_match: it works on device buffers
// of its own (B_GMATCH_*), so nothing the plan or the LM loop reads is written. The host validates and lays the call
// out (ba_gmatch_host.h), uploads, launches and reads back; there is no host round trip between the launches.
#include "ba_gmatch.h"
#include "ba_stage.h"

using namespace miba;

namespace {

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

std::vector<int> as_int(const std::vector<long long>& v) { return std::vector<int>(v.begin(), v.end()); }

}  // namespace

extern "C" int32_t ba_guided_match(ba_context* ctx, const ba_gmatch_problem* p, const ba_gmatch_request* req,
                                   ba_gmatch_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_guided_match", ctx->stream};
    if (const std::string m = stage_refusal(ctx, p, req, info, STAGE_SIZES(BA_GMATCH)); !m.empty()) return stg.invalid(m);
    if (const std::string m = gm_check(p, req); !m.empty()) return stg.invalid(m);
    if (const std::string m = gm_frames_limit(p); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    const GmGrid grid = gm_grid(p->width, p->height, req->cell_px, req->radius);
    const GmLayout lay = gm_layout(p->frame_range, p->n_frames);
    if (const std::string m = gm_limits(p, grid, lay); !m.empty()) return stg.invalid(m);

    const size_t nf = (size_t)p->n_frames, nr = (size_t)p->n_rows, nk = (size_t)p->n_kp, npt = (size_t)p->n_points;
    const size_t ng = (size_t)lay.n_grids(), cells = (size_t)grid.cells(), db = (size_t)p->desc_bytes;
    const bool one = req->one_to_one != 0;
    const bool gate = p->kp_depth && req->depth_tol > 0.0;
    const float ratio = req->ratio > 0.f ? req->ratio : 0.7f;

    ba_gmatch_info full{};
    full.struct_size = (int32_t)sizeof(ba_gmatch_info);
    full.n_frames = p->n_frames;
    full.n_rows = p->n_rows;
    full.kind = p->kind;
    full.n_grids = (int32_t)ng;
    full.cell_px = grid.cell;
    float kernels_ms = 0.f;

    if (nf) {
        HIPCHECK(ctx, hipSetDevice(ctx->device));
        HIPCHECK(ctx, stg.events(ctx->gmatch_ev, 2));
        hipStream_t s = stg.s;
        // a call without rows bins nothing: the counts' n_cand / n_kp and match_begin are all it writes
        const size_t n_binned = nr ? (size_t)lay.grid_kp_begin.back() : 0, n_slots = one && nr ? (size_t)lay.o2o_begin.back() : 0;
        // in: kp_uv | kp_depth | points | frame_pose (doubles), then frame_range | cand_begin | cand_pt | frame_grid |
        // grid_range | grid_kp_begin | o2o_begin (ints), then the two descriptor sets at 16-byte offsets
        const size_t o_dep = 16 * nk, o_pts = o_dep + (gate ? 8 * nk : 0), o_pose = o_pts + 24 * npt, o_int = o_pose + 56 * nf;
        const size_t n_int = 2 * nf + (nf + 1) + nr + nf + 2 * ng + (ng + 1) + (nf + 1);
        const size_t o_kd = up16(o_int + 4 * n_int), o_pd = o_kd + up16(nk * db), in_bytes = o_pd + up16(npt * db);
        // grid: cell_count | cell_off | cell_list (ints), then the one-to-one table
        const size_t o_off = 4 * ng * cells, o_list = o_off + 4 * ng * (cells + 1), o_o2o = up16(o_list + 4 * n_binned);
        // out: proj (doubles), then nn_kp | nn_dist | matches (2 n_rows each) | n_in_window | match_begin | counts
        // (ints), then status
        const size_t out_i = 7 * nr + (nf + 1) + GMATCH_COUNT * nf, o_outi = 24 * nr;
        if (int32_t rc = stg.ensure(B_GMATCH_IN, in_bytes, "the problem's copy")) return rc;
        if (int32_t rc = stg.ensure(B_GMATCH_GRID, o_o2o + 8 * n_slots, "the keypoint grids and the one-to-one table")) return rc;
        if (int32_t rc = stg.ensure(B_GMATCH_OUT, o_outi + 4 * out_i + nr, "the neighbours and the matches")) return rc;
        char* d_in = ctx->buf[B_GMATCH_IN].as<char>();
        char* d_grid = ctx->buf[B_GMATCH_GRID].as<char>();
        char* d_out = ctx->buf[B_GMATCH_OUT].as<char>();
        double* d_uv = reinterpret_cast<double*>(d_in);
        double* d_dep = reinterpret_cast<double*>(d_in + o_dep);
        double* d_pts = reinterpret_cast<double*>(d_in + o_pts);
        double* d_pose = reinterpret_cast<double*>(d_in + o_pose);
        int* d_range = reinterpret_cast<int*>(d_in + o_int);
        int* d_cbegin = d_range + 2 * nf;
        int* d_cpt = d_cbegin + (nf + 1);
        int* d_fgrid = d_cpt + nr;
        int* d_grange = d_fgrid + nf;
        int* d_gkb = d_grange + 2 * ng;
        int* d_o2ob = d_gkb + (ng + 1);
        uint8_t* d_kd = reinterpret_cast<uint8_t*>(d_in + o_kd);
        uint8_t* d_pd = reinterpret_cast<uint8_t*>(d_in + o_pd);

        const std::vector<int> gkb = as_int(lay.grid_kp_begin), o2ob = as_int(lay.o2o_begin);
        HIPCHECK(ctx, stg.h2d(d_uv, p->kp_uv, 16 * nk));
        if (gate) HIPCHECK(ctx, stg.h2d(d_dep, p->kp_depth, 8 * nk));
        if (nr) HIPCHECK(ctx, stg.h2d(d_pts, p->points, 24 * npt));
        HIPCHECK(ctx, stg.h2d(d_pose, p->frame_pose, 56 * nf));
        HIPCHECK(ctx, stg.h2d(d_range, p->frame_range, 8 * nf));
        HIPCHECK(ctx, stg.h2d(d_cbegin, p->cand_begin, 4 * (nf + 1)));
        HIPCHECK(ctx, stg.h2d(d_cpt, p->cand_pt, 4 * nr));
        HIPCHECK(ctx, stg.h2d(d_fgrid, lay.frame_grid.data(), 4 * nf));
        HIPCHECK(ctx, stg.h2d(d_grange, lay.grid_range.data(), 8 * ng));
        HIPCHECK(ctx, stg.h2d(d_gkb, gkb.data(), 4 * (ng + 1)));
        HIPCHECK(ctx, stg.h2d(d_o2ob, o2ob.data(), 4 * (nf + 1)));
        HIPCHECK(ctx, stg.h2d(d_kd, p->kp_desc, nk * db));
        if (nr) HIPCHECK(ctx, stg.h2d(d_pd, p->pt_desc, npt * db));

        GmArgs a{};
        a.kp_uv = d_uv; a.kp_desc = d_kd; a.kp_depth = gate ? d_dep : nullptr;
        a.points = d_pts; a.pt_desc = d_pd; a.frame_pose = d_pose;
        a.frame_range = d_range; a.cand_begin = d_cbegin; a.cand_pt = d_cpt;
        a.frame_grid = d_fgrid; a.grid_range = d_grange; a.grid_kp_begin = d_gkb; a.o2o_begin = d_o2ob;
        for (int i = 0; i < 4; ++i) a.K[i] = p->intr[i];
        a.width = p->width; a.height = p->height; a.n_frames = p->n_frames; a.n_rows = p->n_rows;
        a.n_grids = nr ? (int)ng : 0; a.n_binned = (int)n_binned; a.kind = p->kind; a.desc_bytes = p->desc_bytes;
        a.gw = grid.gw; a.gh = grid.gh; a.cells = (int)cells; a.inv_cell = 1.0 / (double)grid.cell;
        a.radius = req->radius; a.r2 = req->radius * req->radius;
        a.min_depth = req->min_depth > 0.0 ? req->min_depth : 1e-15;
        a.depth_tol = gate ? req->depth_tol : 0.0;
        a.one_to_one = one ? 1 : 0; a.max_distance = std::max(req->max_distance, 0);
        a.ratio = ratio; a.ratio2 = (double)ratio * (double)ratio;
        a.cell_count = reinterpret_cast<int*>(d_grid);
        a.cell_off = reinterpret_cast<int*>(d_grid + o_off);
        a.cell_list = reinterpret_cast<int*>(d_grid + o_list);
        a.o2o = reinterpret_cast<unsigned long long*>(d_grid + o_o2o);
        a.proj = reinterpret_cast<double*>(d_out);
        a.nn_kp = reinterpret_cast<int*>(d_out + o_outi);
        a.nn_dist = a.nn_kp + 2 * nr;
        int* d_matches = a.nn_dist + 2 * nr;
        a.n_in_window = d_matches + 2 * nr;
        a.match_begin = a.n_in_window + nr;
        a.counts = a.match_begin + (nf + 1);
        a.status = reinterpret_cast<unsigned char*>(a.counts + GMATCH_COUNT * nf);
        a.matches = req->matches ? d_matches : nullptr;

        HIPCHECK(ctx, hipMemsetAsync(a.counts, 0, 4 * GMATCH_COUNT * nf, s));
        if (nr) HIPCHECK(ctx, hipMemsetAsync(a.cell_count, 0, 4 * ng * cells, s));
        if (n_slots) HIPCHECK(ctx, hipMemsetAsync(a.o2o, 0xFF, 8 * n_slots, s));
        HIPCHECK(ctx, hipEventRecord(ctx->gmatch_ev[0], s));
        HIPCHECK(ctx, launch_gm_bin(a, s));
        HIPCHECK(ctx, launch_gm_search(a, s));
        if (req->matches || req->match_begin) HIPCHECK(ctx, launch_gm_compact(a, s));
        HIPCHECK(ctx, hipEventRecord(ctx->gmatch_ev[1], s));

        std::vector<int32_t> counts(GMATCH_COUNT * nf);
        HIPCHECK(ctx, stg.d2h(counts.data(), a.counts, 4 * GMATCH_COUNT * nf));
        HIPCHECK(ctx, stg.d2h(req->nn_kp, a.nn_kp, 8 * nr));
        HIPCHECK(ctx, stg.d2h(req->nn_dist, a.nn_dist, 8 * nr));
        HIPCHECK(ctx, stg.d2h(req->status, a.status, nr));
        if (req->proj) HIPCHECK(ctx, stg.d2h(req->proj, a.proj, 24 * nr));
        if (req->n_in_window) HIPCHECK(ctx, stg.d2h(req->n_in_window, a.n_in_window, 4 * nr));
        if (req->match_begin) HIPCHECK(ctx, stg.d2h(req->match_begin, a.match_begin, 4 * (nf + 1)));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&kernels_ms, ctx->gmatch_ev[0], ctx->gmatch_ev[1]);
        long long n_matches = 0;
        for (size_t f = 0; f < nf; ++f) n_matches += counts[GMATCH_COUNT * f + 2];
        full.n_matches = (int32_t)n_matches;
        if (req->matches && n_matches) {  // (only the accepted rows' part of the list is defined)
            HIPCHECK(ctx, stg.d2h(req->matches, d_matches, 8 * (size_t)n_matches));
            HIPCHECK(ctx, hipStreamSynchronize(s));
        }
        if (req->frame_counts) std::memcpy(req->frame_counts, counts.data(), 4 * GMATCH_COUNT * nf);
    } else if (req->match_begin) {
        req->match_begin[0] = 0;
    }

    full.time_kernels_ms = kernels_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
