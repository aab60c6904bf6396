// ba_pg.cpp — ba_pose_graph of include/ba.h: Levenberg-Marquardt over the poses of a pose graph (the kernels of
// ba_pg.hip, the reduced solve by launch_dense of ba_dense.hip).
// The host validates the graph, orders the active poses (reverse Cuthill-McKee, ba_order.cpp, on a 0 / 1 matrix of
// the active poses built from the edges), builds the incidence and pair lists and the block envelope, and then drives
// the loop: per LM iteration the kernels are enqueued and the device's decision (the LM state, 120 bytes) is read
// back once, so nothing of an iteration is enqueued after the loop has ended and a rejected step re-damps without
// a new linearisation.
// A stage beside the LM loop like ba_localize: device buffers of its own (B_PG_*), an LM state, Cholesky flag and
// DenseWork of its own, so nothing the plan or the LM loop reads is written.
#include "ba_pg.h"

#include <cmath>
#include <cstdio>

#include "ba_order.h"
#include "ba_stage.h"

using namespace miba;

static_assert(LOG_W == BA_LOG_WIDTH, "the decision writes the header's log rows");

namespace {

std::string pg_check(ba_context* ctx, const ba_pg_problem* g, const ba_pg_request* req, const ba_pg_info* info) {
    if (const std::string m = stage_refusal(ctx, g, req, info, STAGE_SIZES(BA_PG)); !m.empty()) return m;
    if (g->n_cams < 0 || g->n_edges < 0) return "negative graph sizes";
    if ((g->n_cams && !g->cams) || (g->n_edges && (!g->edge_a || !g->edge_b || !g->edge_meas))) return "null graph buffer";
    if (g->fixed_cam >= g->n_cams)
        return "fixed_cam = " + std::to_string(g->fixed_cam) + " is out of range (" + std::to_string(g->n_cams) + " poses)";
    for (int32_t k = 0; k < g->n_edges; ++k) {
        const int32_t a = g->edge_a[k], b = g->edge_b[k];
        if (a < 0 || a >= g->n_cams || b < 0 || b >= g->n_cams) return "edge index out of range (edge " + std::to_string(k) + ")";
        if (a == b) return "self edge (edge " + std::to_string(k) + " joins pose " + std::to_string(a) + " to itself)";
    }
    if (req->huber < 0.0 || !(req->huber == req->huber)) return "huber must be 0 or positive";
    if (req->log_max_rows < 0 || (req->log_max_rows > 0 && !req->log)) return "log_max_rows is set without a log buffer";
    return "";
}

bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

int roundup(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace

extern "C" int32_t ba_pose_graph(ba_context* ctx, ba_pg_problem* g, const ba_pg_request* req, ba_pg_info* info) {
    if (!ctx) { miba_set_error("null context"); return BA_E_INVALID; }
    const Stage stg{ctx, "ba_pose_graph", ctx->stream};
    if (const std::string m = pg_check(ctx, g, req, info); !m.empty()) return stg.invalid(m);
    const double t0 = now_ms();
    const int nc = g->n_cams, ne = g->n_edges;
    ba_pg_info full{};
    full.struct_size = (int32_t)sizeof(ba_pg_info);
    full.termination_type = BA_CONVERGENCE;

    // the active poses as given, and their positions among the unknowns in the order used
    std::vector<uint8_t> is_const((size_t)nc, 0);
    std::vector<int> given;  // active poses in index order
    std::vector<int> compact((size_t)nc, -1);
    for (int c = 0; c < nc; ++c) {
        is_const[c] = (g->is_constant && g->is_constant[c]) || c == g->fixed_cam;
        if (!is_const[c]) { compact[c] = (int)given.size(); given.push_back(c); }
    }
    const int na = (int)given.size();
    const int npad = roundup(std::max(6 * na, 1), 16);
    if (npad > BA_PG_MAX_NPAD)
        return stg.invalid("the graph has " + std::to_string(na) + " active poses: a reduced system of " +
                           std::to_string(6 * na) + " unknowns (padded " + std::to_string(npad) + ") is above the cap of " +
                           std::to_string(BA_PG_MAX_NPAD) + " (" + std::to_string(BA_PG_MAX_NPAD / 6) +
                           " active poses; the dense system would take " +
                           std::to_string((size_t)npad * npad * 8 / (1 << 20)) + " MB)");
    const double t_order = now_ms();
    CamOrder co;
    {
        std::vector<int32_t> W((size_t)na * na, 0);
        for (int i = 0; i < na; ++i) W[(size_t)i * na + i] = 1;
        for (int k = 0; k < ne; ++k) {
            const int a = compact[g->edge_a[k]], b = compact[g->edge_b[k]];
            if (a >= 0 && b >= 0) W[(size_t)a * na + b] = W[(size_t)b * na + a] = 1;
        }
        covis_order(W.data(), na, -1, co);
    }
    std::vector<int> cam_pos((size_t)nc, -1), pos_cam((size_t)na);
    for (int k = 0; k < na; ++k) {
        pos_cam[k] = given[co.order[k]];
        cam_pos[pos_cam[k]] = k;
    }
    if (req->cam_order) {
        int k = 0;
        for (; k < na; ++k) req->cam_order[k] = pos_cam[k];
        for (int c = 0; c < nc; ++c)
            if (is_const[c]) req->cam_order[k++] = c;
    }
    full.n_active = na;
    full.n_components = co.n_components;
    full.band_before = co.band_before;
    full.band_after = co.band_after;
    full.reduced_system_size = 6 * na;

    // incidence lists (the caller's edge order inside a pose), the coupled pairs (the caller's edge order inside a
    // pair; duplicate and reversed edges fall into one pair) and the envelope's first columns at 16 rows
    std::vector<int> inc_ptr((size_t)na + 1, 0);
    std::vector<PgInc> inc;
    struct PairKey { long long key; int edge, row_is_b; };
    std::vector<PairKey> pk;
    for (int k = 0; k < ne; ++k) {
        const int pa = cam_pos[g->edge_a[k]], pb = cam_pos[g->edge_b[k]];
        if (pa >= 0) ++inc_ptr[pa + 1];
        if (pb >= 0) ++inc_ptr[pb + 1];
        if (pa >= 0 || pb >= 0) ++full.n_edges_used;
        if (pa >= 0 && pb >= 0) {
            const int r = std::max(pa, pb), c = std::min(pa, pb);
            pk.push_back(PairKey{(long long)r * na + c, k, r == pb});
        }
    }
    for (int i = 0; i < na; ++i) inc_ptr[i + 1] += inc_ptr[i];
    inc.resize((size_t)inc_ptr[na]);
    {
        std::vector<int> fill(inc_ptr.begin(), inc_ptr.end() - 1);
        for (int k = 0; k < ne; ++k) {
            const int pa = cam_pos[g->edge_a[k]], pb = cam_pos[g->edge_b[k]];
            if (pa >= 0) inc[fill[pa]++] = PgInc{k, 0};
            if (pb >= 0) inc[fill[pb]++] = PgInc{k, 1};
        }
    }
    std::stable_sort(pk.begin(), pk.end(), [](const PairKey& x, const PairKey& y) { return x.key < y.key; });
    std::vector<int> pair_ptr{0};
    std::vector<int2> pair_rc;
    std::vector<PgPairEdge> pair_edge;
    std::vector<int> fcol((size_t)npad / 16);
    for (size_t r = 0; r < fcol.size(); ++r) fcol[r] = (int)r;
    auto cover = [&fcol](int row_pose, int col_pose) {
        for (int rb = 6 * row_pose / 16; rb <= (6 * row_pose + 5) / 16; ++rb) fcol[rb] = std::min(fcol[rb], 6 * col_pose / 16);
    };
    for (int i = 0; i < na; ++i) cover(i, i);
    for (size_t k = 0; k < pk.size(); ++k) {
        if (k == 0 || pk[k].key != pk[k - 1].key) {
            if (k) pair_ptr.push_back((int)k);
            const int r = (int)(pk[k].key / na), c = (int)(pk[k].key % na);
            pair_rc.push_back(make_int2(r, c));
            cover(r, c);
        }
        pair_edge.push_back(PgPairEdge{pk[k].edge, pk[k].row_is_b});
    }
    pair_ptr.push_back((int)pk.size());
    const int n_pairs = (int)pair_rc.size();
    DensePlan dp;
    dense_plan(fcol, npad, dp);
    full.time_order_ms = now_ms() - t_order;

    // non-finite input: the evaluation at the given poses fails (ba_localize's rule), decided before anything is
    // uploaded: BA_FAILURE, the poses kept, no log row
    const bool finite = all_finite(g->cams, 7 * (size_t)nc) && all_finite(g->edge_meas, 7 * (size_t)ne) &&
                        (!g->edge_weight || all_finite(g->edge_weight, 2 * (size_t)ne));
    LmState S = fresh_state(ctx->opts, ctx->opts.initial_trust_region_radius);
    float kernels_ms = 0.f, solve_ms = 0.f;
    std::vector<double> edge_cost;
    if (!finite) {
        S.done = 1; S.termination = BA_FAILURE; S.msg = MSG_EVAL_FAIL;
        S.initial_cost = S.final_cost = std::nan("");
        if (req->edge_cost)
            for (int k = 0; k < ne; ++k) req->edge_cost[k] = std::nan("");
    } else if (nc > 0) {
        HIPCHECK(ctx, hipSetDevice(ctx->device));
        HIPCHECK(ctx, stg.events(ctx->pg_ev, 4));
        hipStream_t s = stg.s;
        const int max_iter = std::max(ctx->opts.max_num_iterations, 0);
        const size_t snc = (size_t)nc, sne = (size_t)ne, sna = (size_t)na;
        // in: cams x 2 (7 nc each) | meas (7 ne) | weight (2 ne) doubles, then edge_a | edge_b ints
        const size_t in_d = 14 * snc + 9 * sne;
        if (int32_t rc = stg.ensure(B_PG_IN, 8 * in_d + 8 * sne, "the graph's copy")) return rc;
        double* d_cams0 = ctx->buf[B_PG_IN].as<double>();
        double* d_cams1 = d_cams0 + 7 * snc;
        double* d_meas = d_cams1 + 7 * snc;
        double* d_wgt = d_meas + 7 * sne;
        int* d_ea = reinterpret_cast<int*>(d_wgt + 2 * sne);
        int* d_eb = d_ea + sne;
        // idx: cam_pos | pos_cam | inc_ptr | pair_ptr | inc (2 ints each) | pair_rc (2) | pair_edge (2), all 8-byte
        // aligned by an even count of ints before the pairs
        std::vector<int> idx;
        auto put = [&idx](const void* p, size_t n_ints) {
            const size_t at = idx.size();
            idx.resize(at + n_ints + ((at + n_ints) & 1));
            if (n_ints) std::memcpy(idx.data() + at, p, 4 * n_ints);
            return at;
        };
        const size_t o_cp = put(cam_pos.data(), snc), o_pc = put(pos_cam.data(), sna);
        const size_t o_ip = put(inc_ptr.data(), inc_ptr.size()), o_pp = put(pair_ptr.data(), pair_ptr.size());
        const size_t o_in = put(inc.data(), 2 * inc.size()), o_rc = put(pair_rc.data(), 2 * pair_rc.size());
        const size_t o_pe = put(pair_edge.data(), 2 * pair_edge.size());
        if (int32_t rc = stg.ensure(B_PG_IDX, 4 * idx.size(), "the graph's structure")) return rc;
        // work: erec | prec | scale | delta | epart | ppart | rhs | edge costs | log doubles, then the LM state and flag
        const size_t n_log = (size_t)LOG_W * (size_t)(max_iter + 2);
        const size_t work_d = PG_EREC * sne + PG_PREC * sna + 12 * sna + PG_EPART * sne + PG_PPART * sna + (size_t)npad + sne + n_log;
        if (int32_t rc = stg.ensure(B_PG_WORK, 8 * work_d + sizeof(LmState) + 16, "the edge records")) return rc;
        if (int32_t rc = stg.ensure(B_PG_S, 8 * (size_t)npad * npad, "the dense normal equations")) return rc;
        // the blocked Cholesky's own workspace (setup_blocked's layout, in buffers of this stage)
        std::vector<int> h;
        const size_t o_bf = 0, o_rs = o_bf + dp.bfcol.size(), o_cpt = o_rs + dp.rowstart.size(), o_cr = o_cpt + dp.crptr.size();
        size_t o_bk = o_cr + dp.crows.size();
        o_bk += o_bk & 1;  // int2 alignment
        h.insert(h.end(), dp.bfcol.begin(), dp.bfcol.end());
        h.insert(h.end(), dp.rowstart.begin(), dp.rowstart.end());
        h.insert(h.end(), dp.crptr.begin(), dp.crptr.end());
        h.insert(h.end(), dp.crows.begin(), dp.crows.end());
        h.resize(o_bk, 0);
        h.insert(h.end(), dp.blk.begin(), dp.blk.end());
        if (int32_t rc = stg.ensure(B_PG_DENSE_IDX, 4 * h.size(), "the envelope's block lists")) return rc;
        if (int32_t rc = stg.ensure(B_PG_DENSE_A, 8 * (size_t)DENSE_BB * dp.n_env(), "the packed envelope")) return rc;
        if (int32_t rc = stg.ensure(B_PG_DENSE_Z, 8 * (size_t)DENSE_BB * dp.nblk, "the diagonal inverses")) return rc;
        if (int32_t rc = stg.ensure(B_PG_DENSE_B, 8 * (size_t)DENSE_B * dp.nblk, "the padded right-hand side")) return rc;
        DenseWork D;
        {
            const int* base = ctx->buf[B_PG_DENSE_IDX].as<int>();
            D.A = ctx->buf[B_PG_DENSE_A].as<double>();
            D.Zd = ctx->buf[B_PG_DENSE_Z].as<double>();
            D.bz = ctx->buf[B_PG_DENSE_B].as<double>();
            D.bfcol = base + o_bf; D.rowstart = base + o_rs; D.crptr = base + o_cpt; D.crows = base + o_cr;
            D.blk = reinterpret_cast<const int2*>(base + o_bk);
            D.nblk = dp.nblk; D.n_env = dp.n_env();
            D.h_crptr = dp.crptr.data();
        }

        PgArgs a{};
        a.cams[0] = d_cams0; a.cams[1] = d_cams1;
        a.edge_a = d_ea; a.edge_b = d_eb; a.meas = d_meas; a.weight = d_wgt;
        const int* d_idx = ctx->buf[B_PG_IDX].as<int>();
        a.cam_pos = d_idx + o_cp; a.pos_cam = d_idx + o_pc; a.inc_ptr = d_idx + o_ip; a.pair_ptr = d_idx + o_pp;
        a.inc = reinterpret_cast<const PgInc*>(d_idx + o_in);
        a.pair_rc = reinterpret_cast<const int2*>(d_idx + o_rc);
        a.pair_edge = reinterpret_cast<const PgPairEdge*>(d_idx + o_pe);
        a.n_cams = nc; a.n_edges = ne; a.n_active = na; a.n_pairs = n_pairs; a.npad = npad;
        a.huber_a = req->huber; a.huber_b = req->huber * req->huber;
        a.min_diag = ctx->opts.min_lm_diagonal; a.max_diag = ctx->opts.max_lm_diagonal;
        double* w = ctx->buf[B_PG_WORK].as<double>();
        a.erec = w; w += PG_EREC * sne;
        a.prec = w; w += PG_PREC * sna;
        a.scale = w; w += 6 * sna;
        a.delta = w; w += 6 * sna;
        a.epart = w; w += PG_EPART * sne;
        a.ppart = w; w += PG_PPART * sna;
        a.rhs = w; w += npad;
        double* d_ecost = w; w += sne;
        a.log = w; w += n_log;
        a.st = reinterpret_cast<LmState*>(w);
        a.chol_flag = reinterpret_cast<int*>(reinterpret_cast<char*>(w) + sizeof(LmState));
        a.S = ctx->buf[B_PG_S].as<double>();

        std::vector<double> ones;
        if (!g->edge_weight) ones.assign(2 * sne, 1.0);
        HIPCHECK(ctx, stg.h2d(d_cams0, g->cams, 56 * snc));
        HIPCHECK(ctx, stg.h2d(d_cams1, g->cams, 56 * snc));
        HIPCHECK(ctx, stg.h2d(d_meas, g->edge_meas, 56 * sne));
        HIPCHECK(ctx, stg.h2d(d_wgt, g->edge_weight ? g->edge_weight : ones.data(), 16 * sne));
        HIPCHECK(ctx, stg.h2d(d_ea, g->edge_a, 4 * sne));
        HIPCHECK(ctx, stg.h2d(d_eb, g->edge_b, 4 * sne));
        HIPCHECK(ctx, stg.h2d(ctx->buf[B_PG_IDX].p, idx.data(), 4 * idx.size()));
        HIPCHECK(ctx, stg.h2d(ctx->buf[B_PG_DENSE_IDX].p, h.data(), 4 * h.size()));
        // the structure is fixed over the call: S is cleared once, every iteration rewrites the same entries
        HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_PG_WORK].p, 0, 8 * work_d + sizeof(LmState) + 16, s));
        HIPCHECK(ctx, hipMemsetAsync(a.S, 0, 8 * (size_t)npad * npad, s));
        S.need_lin = 0;
        HIPCHECK(ctx, stg.h2d(a.st, &S, sizeof(LmState)));
        LmParams prm = lm_params(ctx);
        prm.progress = nullptr;
        Prof* pf = ctx->pf();
        auto read_state = [&]() -> hipError_t {
            if (hipError_t e = stg.d2h(&S, a.st, sizeof(LmState)); e != hipSuccess) return e;
            return hipStreamSynchronize(s);
        };

        // iteration 0, then one read of the decision per LM iteration
        HIPCHECK(ctx, launch_pg_linearize(a, 1, ctx->opts.jacobi_scaling, s));
        HIPCHECK(ctx, launch_pg_init(a, s));
        HIPCHECK(ctx, read_state());
        if (na == 0 || ne == 0) {  // nothing to solve: the costs are reported, nothing is written
            if (!S.done) { S.done = 1; S.termination = BA_CONVERGENCE; S.msg = MSG_NONE; }
        }
        for (int round = 0; !S.done && round < max_iter + 4; ++round) {
            HIPCHECK(ctx, hipEventRecord(ctx->pg_ev[0], s));
            if (S.need_lin) HIPCHECK(ctx, launch_pg_linearize(a, 0, ctx->opts.jacobi_scaling, s));
            const bool step = !S.stop_next;
            if (step) {
                HIPCHECK(ctx, launch_pg_assemble(a, s));
                HIPCHECK(ctx, hipEventRecord(ctx->pg_ev[2], s));
                HIPCHECK(ctx, launch_dense(a.st, a.S, npad, a.rhs, a.chol_flag, D, s, pf));
                HIPCHECK(ctx, hipEventRecord(ctx->pg_ev[3], s));
                HIPCHECK(ctx, launch_pg_step(a, s));
            }
            HIPCHECK(ctx, launch_pg_decide(a, prm, s));
            HIPCHECK(ctx, hipEventRecord(ctx->pg_ev[1], s));
            HIPCHECK(ctx, read_state());
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ctx->pg_ev[0], ctx->pg_ev[1]) == hipSuccess) kernels_ms += ms;
            if (step && hipEventElapsedTime(&ms, ctx->pg_ev[2], ctx->pg_ev[3]) == hipSuccess) solve_ms += ms;
            if (pf) flush_prof(ctx);
        }
        if (!S.done) {
            ctx->err = "ba_pose_graph: the LM loop did not end within its iteration limit";
            return BA_E_INTERNAL;
        }
        const bool failed_eval = S.msg == MSG_EVAL_FAIL;
        // the result: the poses of the accepted slot, only the active ones written back; the edges' costs there
        std::vector<double> cams(7 * snc);
        const int rows = failed_eval ? 0 : S.iter + 1;
        const size_t n_rows = (size_t)std::min(rows, (int)req->log_max_rows);
        std::vector<double> log((size_t)LOG_W * n_rows);
        if (req->edge_cost && ne) {
            edge_cost.resize(sne);
            HIPCHECK(ctx, launch_pg_edge_cost(a, d_ecost, s));
            HIPCHECK(ctx, stg.d2h(edge_cost.data(), d_ecost, 8 * sne));
        }
        HIPCHECK(ctx, stg.d2h(cams.data(), a.cams[S.cur], 56 * snc));
        HIPCHECK(ctx, stg.d2h(log.data(), a.log, 8 * log.size()));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        if (!failed_eval && S.iter > 0)
            for (int k = 0; k < na; ++k) std::memcpy(g->cams + 7 * (size_t)pos_cam[k], &cams[7 * (size_t)pos_cam[k]], 56);
        for (size_t r = 0; r < n_rows; ++r) {
            log[r * LOG_W + 7] = 0.0;
            std::memcpy(req->log + r * LOG_W, &log[r * LOG_W], 8 * LOG_W);
        }
        full.log_rows = rows;
        if (req->edge_cost && ne) std::memcpy(req->edge_cost, edge_cost.data(), 8 * sne);
    } else {
        S.done = 1; S.termination = BA_CONVERGENCE; S.msg = MSG_NONE;
    }

    full.iterations = S.iter;
    full.n_successful = S.n_succ;
    full.n_unsuccessful = S.n_unsucc;
    full.termination_type = S.termination;
    full.initial_cost = S.initial_cost;
    full.final_cost = S.final_cost;
    if (S.msg == MSG_NONE) std::snprintf(full.message, sizeof(full.message), "Nothing to optimise: the graph has no edge or no active pose.");
    else format_message(S, full.message, sizeof(full.message));
    full.time_kernels_ms = kernels_ms;
    full.time_solve_ms = solve_ms;
    full.time_total_ms = now_ms() - t0;
    sized_copy_out(info, full);
    ctx->err.clear();
    return BA_OK;
}
