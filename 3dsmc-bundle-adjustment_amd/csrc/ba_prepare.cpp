// ba_prepare.cpp — ba_prepare's host side: the window staged and uploaded, its plan built (host or device), the
// device structure allocated and wired, the reduced-system solver and the launch paths chosen; the plan cache.
//
// Problem preparation: admissibility (countConstraints :184-213, skip :265-268), active parameter blocks,
// point-major / camera-major orderings, envelope of S. prepare_core() runs the phases in a fixed order: with
// landmark shards the order of its collectives is a protocol (the verdict all-reduce before anything, then
// cam_seen / n_adm_all, then fc, then the final agreement).
#include <climits>
#include <cmath>
#include <cstdio>
#include <thread>

#include "ba_context.h"
#include "ba_dplan.h"

using namespace miba;

template <class T>
static hipError_t upload(ba_context* ctx, int id, const T* src, size_t n) {
    hipError_t e = ctx->buf[id].ensure(sizeof(T) * std::max<size_t>(n, 1));
    if (e != hipSuccess) return e;
    if (n) e = hipMemcpyAsync(ctx->buf[id].p, src, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream);
    return e;
}

// Host-side all-reduce of a small array across the landmark shards (prepare time).
template <class T>
static int host_allreduce(ba_context* ctx, T* v, size_t n, CommOp op) {
    if (!ctx->W.comm.on() || n == 0) return BA_OK;
    if (ctx->buf[B_PREP].ensure(sizeof(T) * n) != hipSuccess) { ctx->err = "prepare scratch allocation failed"; return BA_E_NOMEM; }
    T* d = ctx->buf[B_PREP].as<T>();
    hipStream_t s = ctx->stream;
    const CommType t = sizeof(T) == 8 ? COMM_F64 : COMM_I32;
    if (hipMemcpyAsync(d, v, sizeof(T) * n, hipMemcpyHostToDevice, s) != hipSuccess ||
        comm_allreduce(ctx->W.comm, d, d, n, t, op, s) != hipSuccess ||
        hipMemcpyAsync(v, d, sizeof(T) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        ctx->err = std::string("landmark-shard all-reduce failed: ") + comm_last_error();
        return BA_E_COMM;
    }
    return BA_OK;
}
static int host_allreduce_i32(ba_context* ctx, int* v, size_t n, CommOp op) { return host_allreduce(ctx, v, n, op); }

static int prepare_core(ba_context* ctx, const ba_problem* p, bool force_det);

// Landmark shards of a window too small to pay for the per-iteration exchange (admissible observations
// over all shards < ba_options.shard_min_obs): gather every shard onto every rank (SUM all-reduces of
// zero-padded slices, once per ba_prepare) and solve the whole window on each rank without collectives,
// in deterministic mode so that all ranks compute bitwise the same cameras; each rank keeps its slice.
// Returns 1 when the window was prepared gathered, 0 when it stays sharded, < 0 on error.
static int prepare_gathered(ba_context* ctx, const ba_problem* p) {
    Comm& comm = ctx->W.comm;
    const int R = comm.nranks, me = comm.rank;
    // agreement first (every rank reaches the same branch): local validity and admissible count
    int v[2] = {0, 0};
    bool ok = p && p->n_cams >= 0 && p->n_points >= 0 && p->n_obs >= 0 && p->intr && p->intr_prior &&
              (!p->n_cams || p->cams) && (!p->n_points || p->points) &&
              (!p->n_obs || (p->obs_cam && p->obs_pt && p->obs_uv && p->obs_depth));
    for (int k = 0; ok && k < p->n_obs; ++k) {
        if (p->obs_cam[k] < 0 || p->obs_cam[k] >= p->n_cams || p->obs_pt[k] < 0 || p->obs_pt[k] >= p->n_points) ok = false;
        else if (p->obs_depth[k] > 1e-15) ++v[1];
    }
    v[0] = ok ? 0 : 1;
    if (int rc = host_allreduce_i32(ctx, v, 2, COMM_SUM)) return rc;
    if (v[0] != 0 || v[1] >= ctx->opts.shard_min_obs) return 0;  // invalid (prepare_core reports it) or large
    std::vector<int> cnt(2 * (size_t)R, 0);
    cnt[2 * me] = p->n_points;
    cnt[2 * me + 1] = p->n_obs;
    if (int rc = host_allreduce_i32(ctx, cnt.data(), cnt.size(), COMM_SUM)) return rc;
    int np = 0, no = 0, poff = 0, ooff = 0;
    for (int r = 0; r < R; ++r) {
        if (r == me) { poff = np; ooff = no; }
        np += cnt[2 * r];
        no += cnt[2 * r + 1];
    }
    auto& g = ctx->gw;
    g.cams.assign(p->cams, p->cams + 7 * (size_t)p->n_cams);  // replicated on every rank
    std::memcpy(g.intr, p->intr, sizeof(g.intr));
    std::memcpy(g.prior, p->intr_prior, sizeof(g.prior));
    g.pts.assign(3 * (size_t)np, 0.0);
    g.uv.assign(2 * (size_t)no, 0.0);
    g.dep.assign(no, 0.0);
    g.oc.assign(no, 0);
    g.op.assign(no, 0);
    std::copy(p->points, p->points + 3 * (size_t)p->n_points, g.pts.begin() + 3 * (size_t)poff);
    std::copy(p->obs_uv, p->obs_uv + 2 * (size_t)p->n_obs, g.uv.begin() + 2 * (size_t)ooff);
    std::copy(p->obs_depth, p->obs_depth + p->n_obs, g.dep.begin() + ooff);
    std::copy(p->obs_cam, p->obs_cam + p->n_obs, g.oc.begin() + ooff);
    for (int k = 0; k < p->n_obs; ++k) g.op[ooff + k] = p->obs_pt[k] + poff;
    int rc = host_allreduce(ctx, g.pts.data(), g.pts.size(), COMM_SUM);
    if (!rc) rc = host_allreduce(ctx, g.uv.data(), g.uv.size(), COMM_SUM);
    if (!rc) rc = host_allreduce(ctx, g.dep.data(), g.dep.size(), COMM_SUM);
    if (!rc) rc = host_allreduce_i32(ctx, g.oc.data(), g.oc.size(), COMM_SUM);
    if (!rc) rc = host_allreduce_i32(ctx, g.op.data(), g.op.size(), COMM_SUM);
    if (rc) return rc;
    ba_problem full{};
    full.n_cams = p->n_cams;
    full.n_points = np;
    full.n_obs = no;
    full.fixed_cam = p->fixed_cam;
    full.cams = g.cams.data();
    full.points = g.pts.data();
    full.intr = g.intr;
    full.intr_prior = g.prior;
    full.obs_cam = g.oc.data();
    full.obs_pt = g.op.data();
    full.obs_uv = g.uv.data();
    full.obs_depth = g.dep.data();
    ctx->comm_parked = comm;  // no collective while this window is solved
    comm = Comm{};
    rc = prepare_core(ctx, &full, true);
    if (rc) return rc;
    ctx->gather_off = poff;
    ctx->dev_np = np;
    ctx->prep_nc = p->n_cams; ctx->prep_np = p->n_points; ctx->prep_no = p->n_obs;  // the caller's shard
    return 1;
}

// Landmark shards replicate the window's cameras, intrinsics, prior and gauge: every rank must pass the same
// values (each would otherwise solve a different window and still report success). FNV-1a over their bytes,
// MIN and MAX all-reduced: a mismatch anywhere gives every rank the same BA_E_INVALID.
static int shard_replicas_agree(ba_context* ctx, const ba_problem* p) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const void* d, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(d);
        for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 1099511628211ull;
    };
    const bool ok = p && p->n_cams >= 0 && (!p->n_cams || p->cams) && p->intr && p->intr_prior;
    if (ok) {
        mix(&p->n_cams, sizeof(p->n_cams));
        mix(&p->fixed_cam, sizeof(p->fixed_cam));
        mix(p->cams, sizeof(double) * 7 * (size_t)p->n_cams);
        mix(p->intr, sizeof(double) * 4);
        mix(p->intr_prior, sizeof(double) * 4);
    }
    int lo[2] = {(int)(unsigned)h, (int)(unsigned)(h >> 32)}, hi[2] = {lo[0], lo[1]};
    int rc = host_allreduce_i32(ctx, lo, 2, COMM_MIN);
    if (rc == BA_OK) rc = host_allreduce_i32(ctx, hi, 2, COMM_MAX);
    if (rc != BA_OK) return rc;
    if (lo[0] != hi[0] || lo[1] != hi[1]) {
        ctx->err = "landmark shards disagree on the window cameras / intrinsics / prior / fixed_cam (every rank must "
                   "pass the same replicated values)";
        return BA_E_INVALID;
    }
    return BA_OK;
}

int prepare(ba_context* ctx, const ba_problem* p) {
    ctx->dbg_step_base = -1;  // (every entry point that rewrites the device state prepares or resets first)
    if (ctx->comm_parked.on()) {  // the last window ran gathered: the communicator is back for this one
        ctx->W.comm = ctx->comm_parked;
        ctx->comm_parked = Comm{};
    }
    ctx->gather_off = 0;
    ctx->dev_np = p && p->n_points > 0 ? p->n_points : 0;
    if (ctx->W.comm.on() && ctx->cmask_any) {  // before any collective: every rank's own verdict
        ctx->err = "constant cameras (ba_set_constant_cameras) are not supported on contexts with landmark shards";
        return BA_E_INVALID;
    }
    if (ctx->W.comm.on())
        if (int rc = shard_replicas_agree(ctx, p)) return rc;
    if (ctx->W.comm.on() && ctx->opts.shard_min_obs > 0) {
        const int rc = prepare_gathered(ctx, p);
        if (rc != 0) return rc < 0 ? rc : BA_OK;
    }
    return prepare_core(ctx, p, false);
}

// k_bcr_split's hand-off state: the flags (epoch 0) and the flag-free buffers, which start empty (BCR_Y_EMPTY):
// y (Racc | Y, epoch parity), the published panels (Cf | X slots, two epochs) and the published X rows of the
// pull hand-off (bcr_reset_pull_slots: zeros instead when another BCR path runs). bcr_layout (ba_kernels.h) keeps
// the neighbours together.
int bcr_init_handoffs(ba_context* ctx) {
    const BcrWork& Bw = ctx->W.bcr;
    const size_t b64 = (size_t)64 * 64 * Bw.nblk, b8 = (size_t)64 * 8 * Bw.nblk;
    hipStream_t s = ctx->stream;
    HIPCHECK(ctx, hipMemsetAsync(Bw.flags, 0, sizeof(unsigned) * (16 + 6 * Bw.nblk), s));
    HIPCHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)Bw.Racc, BCR_Y_EMPTY_D32, 4 * b8, s));
    HIPCHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)Bw.Cf, BCR_Y_EMPTY_D32, 2 * (b64 + (size_t)64 * BCR_XW * Bw.nblk), s));
    HIPCHECK(ctx, bcr_reset_pull_slots(Bw, Bw.persist >= 2, s));
    ctx->bcr_launches = 0;
    return BA_OK;
}

// ---- staging. ctx->stage (pinned, kept by the context): the raw window is copied in by the host threads and
// DMA'd while the plan is built; the plan's index arrays follow in one DMA. Growing it for the plan keeps the raw
// region, which the plan cache compares the next window against.

// parallel memcpy (the host pool) of several arrays into a staging buffer
struct StageCopy { void* dst; const void* src; size_t bytes; };
static void stage_copy(const std::vector<StageCopy>& v) {
    size_t total = 0;
    for (const StageCopy& c : v) total += c.bytes;
    const int T = (int)std::max<size_t>(1, std::min<size_t>(4 * (size_t)host_threads(), total >> 18));
    host_parallel(T, [&](int t) {
        for (const StageCopy& c : v) {
            const size_t lo = c.bytes * t / T, hi = c.bytes * (t + 1) / T;
            if (hi > lo) std::memcpy(static_cast<char*>(c.dst) + lo, static_cast<const char*>(c.src) + lo, hi - lo);
        }
    });
}

static bool f32_exact(double v) { return (double)(float)v == v; }

// The pixels into the staging buffer (host pool), checking on the way that every admissible pixel and depth is
// exactly an f32 (the obs32 layout, DevProblem::obs32; plan_count's check for the device plan). Returns true when
// one is not.
static bool stage_values_f32check(double* dst_uv, double* dst_dep, const double* uv, const double* dep, size_t no) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>(4 * (size_t)host_threads(), no >> 12));
    std::vector<unsigned char> bad(T, 0);
    host_parallel(T, [&](int t) {
        const size_t lo = no * t / T, hi = no * (t + 1) / T;
        std::memcpy(dst_uv + 2 * lo, uv + 2 * lo, 16 * (hi - lo));
        std::memcpy(dst_dep + lo, dep + lo, 8 * (hi - lo));
        bool ok = true;
        for (size_t k = lo; k < hi; ++k)
            if (dep[k] > 1e-15) ok = ok && f32_exact(uv[2 * k]) && f32_exact(uv[2 * k + 1]) && f32_exact(dep[k]);
        bad[t] = ok ? 0 : 1;
    });
    for (int t = 0; t < T; ++t)
        if (bad[t]) return true;
    return false;
}

// The staging layout of the raw observations: obs_uv | obs_depth | obs_cam | obs_pt.
// (+ the admissibility bytes the device plan reads instead of the depths)
struct RawStage {
    double* uv; double* dep; int* cam; int* pt; unsigned char* adm;
    RawStage(const PinnedBuf& sg, size_t no)
        : uv(sg.as<double>()), dep(uv + 2 * no), cam(reinterpret_cast<int*>(dep + no)), pt(cam + no),
          adm(reinterpret_cast<unsigned char*>(pt + no)) {}
};
static size_t raw_stage_bytes(size_t no) { return no * (16 + 8 + 4 + 4 + 1); }

// Before the raw window is staged: the last prepare's value DMA no longer reads the staging buffer (a prepare
// that failed after it), the buffer takes the window, the device's raw arrays exist.
static int raw_stage_begin(ba_context* ctx, int no, bool with_adm) {
    if (ctx->uv_pending) {
        HIPCHECK(ctx, hipEventSynchronize(ctx->ev_uv));
        ctx->uv_pending = false;
    }
    HIPCHECK(ctx, ctx->stage.ensure(raw_stage_bytes((size_t)no)));
    HIPCHECK(ctx, ctx->buf[B_RAW_UV].ensure(16 * (size_t)no));
    HIPCHECK(ctx, ctx->buf[B_RAW_DEP].ensure(8 * (size_t)no));
    HIPCHECK(ctx, ctx->buf[B_RAW_CAM].ensure(4 * (size_t)no));
    HIPCHECK(ctx, ctx->buf[B_RAW_PT].ensure(4 * (size_t)no));
    if (with_adm) HIPCHECK(ctx, ctx->buf[B_RAW_ADM].ensure((size_t)no));
    return BA_OK;
}

// The host plan's upload: the raw observations -> pinned staging -> HBM, in flight while the host builds the plan.
static int stage_raw(ba_context* ctx, const ba_problem* p, int no_) {
    if (no_ <= 0) return BA_OK;
    const size_t no = (size_t)no_;
    hipStream_t s = ctx->stream;
    if (int rc = raw_stage_begin(ctx, no_, false)) return rc;
    RawStage rs(ctx->stage, no);
    stage_copy({{rs.uv, p->obs_uv, 16 * no}, {rs.dep, p->obs_depth, 8 * no}, {rs.cam, p->obs_cam, 4 * no},
                {rs.pt, p->obs_pt, 4 * no}});
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_UV].p, rs.uv, 16 * no, hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_DEP].p, rs.dep, 8 * no, hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_CAM].p, rs.cam, 4 * no, hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_PT].p, rs.pt, 4 * no, hipMemcpyHostToDevice, s));
    return BA_OK;
}

// The device plan's inputs into the staging buffer (host pool): the indices and one admissibility byte per
// observation (depth > 1e-15, countConstraints / the skip at OptimizationUtils.cpp:265-268).
static void stage_indices_adm(const RawStage& rs, const ba_problem* p, size_t no) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>(4 * (size_t)host_threads(), no >> 15));
    host_parallel(T, [&](int t) {
        const size_t lo = no * t / T, hi = no * (t + 1) / T;
        std::memcpy(rs.cam + lo, p->obs_cam + lo, 4 * (hi - lo));
        std::memcpy(rs.pt + lo, p->obs_pt + lo, 4 * (hi - lo));
        for (size_t k = lo; k < hi; ++k) rs.adm[k] = p->obs_depth[k] > 1e-15 ? 1 : 0;
    });
}

// The window's parameters (cameras, points, intrinsics, prior) -> pinned staging -> HBM slot 0, then copied on the
// device into the candidate and initial slots (k_reset starts every solve from the initial ones).
static int upload_params(ba_context* ctx, const ba_problem* p, hipStream_t s) {
    const size_t nc = p->n_cams, np = p->n_points;
    HIPCHECK(ctx, ctx->pstage.ensure(56 * nc + 24 * np + 64));
    double* hc = ctx->pstage.as<double>();
    double* hp = hc + 7 * nc;
    double* hk = hp + 3 * np;
    std::vector<StageCopy> cp = {{hk, p->intr, 32}, {hk + 4, p->intr_prior, 32}};
    if (nc) cp.push_back({hc, p->cams, 56 * nc});
    if (np) cp.push_back({hp, p->points, 24 * np});
    stage_copy(cp);
    const int slots[3][3] = {{B_CAMS0, B_CAMS1, B_CAMS_INIT}, {B_PTS0, B_PTS1, B_PTS_INIT}, {B_K0, B_K1, B_K_INIT}};
    const size_t len[3] = {56 * nc, 24 * np, 32};
    const double* src[3] = {hc, hp, hk};
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) HIPCHECK(ctx, ctx->buf[slots[a][b]].ensure(std::max<size_t>(len[a], 8)));
        if (!len[a]) continue;
        HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[slots[a][0]].p, src[a], len[a], hipMemcpyHostToDevice, s));
        for (int b = 1; b < 3; ++b)
            HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[slots[a][b]].p, ctx->buf[slots[a][0]].p, len[a], hipMemcpyDeviceToDevice, s));
    }
    HIPCHECK(ctx, ctx->buf[B_PRIOR].ensure(32));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_PRIOR].p, hk + 4, 32, hipMemcpyHostToDevice, s));
    return BA_OK;
}

// The band tail's flag-free partial slots (PART_TAIL, ba_kernels.h) start empty: the BCR_Y_EMPTY pattern in every
// double (its two 32-bit halves are equal, so one 32-bit fill)
static hipError_t empty_tail_slots(double* part, int stride, hipStream_t s) {
    static_assert((BCR_Y_EMPTY >> 32) == (BCR_Y_EMPTY & 0xffffffffull), "a 32-bit fill writes the pattern");
    return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(part + (size_t)PART_TAIL * stride), (int)BCR_Y_EMPTY_D32,
                             2 * 5 * (size_t)stride, s);
}

// ba_prepare_info.bcr_path of the reduced-solve path (include/ba.h)
static int bcr_path_id(const BcrWork& Bw) { return Bw.band ? 5 : Bw.dense1 ? 4 : Bw.persist; }

// The block cyclic reduction's workspace: zeroed (the upper tiles of UL / UR are never written and must read as
// zero), the resident path probed (bcr_persist_ok; MIBA_BCR overrides), the hand-off state initialised. Every
// full prepare probes again, also after a hand-off timeout moved the last window to the per-level launches
// (ba_prepare_info.bcr_path reports the path).
static int bcr_setup(ba_context* ctx) {
    BcrWork& Bw = ctx->W.bcr;
    const Settings& st = ctx->st;
    HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_BCR].p, 0, ctx->buf[B_BCR].cap, ctx->stream));
    Bw.persist = bcr_persist_ok(Bw.nblk);
    Bw.dense1 = bcr_dense1_ok(Bw.nblk, ctx->P.kb, st.bcr_set, st.bcr_dense1);
    Bw.band = bcr_band_ok(ctx->P.nac, ctx->P.cam_band, ctx->P.kb, ctx->tail_possible, st.bcr_set, st.bcr_band);
    if (st.bcr == 0) Bw.persist = 0;
    else if (st.bcr == 1 && Bw.persist >= 2) Bw.persist = 1;
    else if (st.bcr == 2 && Bw.persist == 3) Bw.persist = 2;  // "split3" or unset: default
    Bw.xmap = bcr_xmap_ok(Bw.nblk, Bw.persist, st.bcr_xmap);
    ctx->bcr_fallback = false;
    return bcr_init_handoffs(ctx);
}

// The cost constants of the window (weights, Huber scales, LM diagonal bounds) from the context's options and N.
// Every prepare sets them, the plan-cache reuse path included: ba_set_options may change a weight or a Huber
// scale between two solves of one window structure.
static void set_consts(ba_context* ctx) {
    const ba_options& o = ctx->opts;
    BaConsts& C = ctx->C;
    // all shards' admissible observations (N = 0: no observation block exists, so the 1/N weights are unused
    // and the window reduces to the IntrinsicsPrior block, :236-241)
    const double N = (double)std::max(ctx->n_adm_all, 1);
    C.sw_r = std::sqrt(1.0 / N);             // ReprojectionConstraint weight 1/N (:280)
    C.sw_d = std::sqrt(o.weight_unpr / N);   // DepthPrior WEIGHT_UNPR/N (:290)
    C.sw_k = std::sqrt(o.weight_intrinsics); // IntrinsicsPrior (:238)
    cost_consts(o, C);
}

// The device state every prepare leaves behind, full or reused: S, rhs and the partial slots cleared, the tail
// slots empty. (Each path enqueues it where it always did: the full prepare early, so that the clears run while
// the host wires the window; the reuse path behind the parameter upload.)
static int clear_solve_state(ba_context* ctx, int npad, int part_stride) {
    hipStream_t s = ctx->stream;
    HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_S].p, 0, sizeof(double) * (size_t)npad * npad, s));
    HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_RHS].p, 0, sizeof(double) * npad, s));
    HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_PART].p, 0, sizeof(double) * PART_NSLOTS * part_stride, s));
    HIPCHECK(ctx, empty_tail_slots(ctx->buf[B_PART].as<double>(), part_stride, s));
    return BA_OK;
}

// The host state every prepare leaves behind, full or reused, behind clear_solve_state: the BCR workspace set up
// again after a hand-off timeout, the launch paths the full prepare chose (a timeout cleared them for the rest of
// that solve: the next one takes them again, ADVICE r4: no sticky fallback), the cost constants, the paths
// reported, the window marked prepared.
static int finish_prepare(ba_context* ctx, int nc, int np, int no) {
    const DevProblem& P = ctx->P;
    if (P.solver == 2 && ctx->bcr_fallback)
        if (int rc = bcr_setup(ctx)) return rc;
    ctx->W.sw = ctx->sw_full;
    ctx->W.tail = ctx->tail_full;
    ctx->W.bsfin = ctx->bsfin_full;
    set_consts(ctx);
    ctx->pinfo.bcr_path = P.solver == 2 ? bcr_path_id(ctx->W.bcr) : -1;
    ctx->pinfo.lin_path = ctx->W.sw;
    ctx->pinfo.tail = ctx->W.tail;
    ctx->pinfo.bsfin = ctx->W.bsfin;
    ctx->prepared = true;
    ctx->prep_nc = nc; ctx->prep_np = np; ctx->prep_no = no;
    return BA_OK;
}

// Plan cache: the window has the structure of the last full prepare (sizes, gauge, deterministic option and layout
// settings in the key; obs_cam, obs_pt and the admissibility mask compared here, on the host threads, against the
// staged copy of that window) -> only the parameters, and the observation values that changed, are uploaded.
// An admissible value that is no longer an exact f32 on an obs32 plan also forces a rebuild.
// Returns 1 when the plan was reused, 0 when the window needs a full prepare, < 0 on error.
static int prepare_reuse(ba_context* ctx, const ba_problem* p, double tp0) {
    const int no = p->n_obs;
    RawStage rs(ctx->stage, (size_t)no);
    const bool o32 = ctx->key.obs32 != 0;
    const int T = (int)std::max<long long>(1, std::min<long long>(4LL * host_threads(), (long long)no >> 15));
    std::vector<unsigned char> changed(T, 0), vals(T, 0);
    host_parallel(T, [&](int t) {
        const size_t lo = (size_t)no * t / T, hi = (size_t)no * (t + 1) / T, n = hi - lo;
        if (!n) return;
        if (std::memcmp(rs.cam + lo, p->obs_cam + lo, 4 * n) || std::memcmp(rs.pt + lo, p->obs_pt + lo, 4 * n)) {
            changed[t] = 1;
            return;
        }
        if (std::memcmp(rs.dep + lo, p->obs_depth + lo, 8 * n)) {
            for (size_t k = lo; k < hi; ++k) {
                const double nd = p->obs_depth[k];
                const bool adm = nd > 1e-15;
                if (adm != (rs.dep[k] > 1e-15) || (adm && o32 && !f32_exact(nd))) { changed[t] = 1; return; }
            }
            std::memcpy(rs.dep + lo, p->obs_depth + lo, 8 * n);
            vals[t] = 1;
        }
        if (std::memcmp(rs.uv + 2 * lo, p->obs_uv + 2 * lo, 16 * n)) {
            if (o32)
                for (size_t k = lo; k < hi; ++k)
                    if (p->obs_depth[k] > 1e-15 && !(f32_exact(p->obs_uv[2 * k]) && f32_exact(p->obs_uv[2 * k + 1]))) {
                        changed[t] = 1;
                        return;
                    }
            std::memcpy(rs.uv + 2 * lo, p->obs_uv + 2 * lo, 16 * n);
            vals[t] = 1;
        }
    });
    ctx->pinfo.compare_ms = now_ms() - tp0;
    for (int t = 0; t < T; ++t)
        if (changed[t]) return 0;
    const double tu = now_ms();
    hipStream_t s = ctx->stream;
    bool any_vals = false;
    for (int t = 0; t < T; ++t) any_vals = any_vals || vals[t];
    if (any_vals) {  // new pixel / depth values on the same structure: re-gather the observation layouts
        HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_UV].p, rs.uv, 16 * (size_t)no, hipMemcpyHostToDevice, s));
        HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_DEP].p, rs.dep, 8 * (size_t)no, hipMemcpyHostToDevice, s));
        HIPCHECK(ctx, launch_prep_gather(ctx->P, ctx->raw, s));
    }
    if (int rc = upload_params(ctx, p, s)) return rc;
    if (int rc = clear_solve_state(ctx, ctx->P.npad, ctx->P.part_stride)) return rc;
    if (int rc = finish_prepare(ctx, p->n_cams, p->n_points, p->n_obs)) return rc;
    ctx->pinfo.plan_reused = 1;
    ctx->pinfo.obs_uploaded = any_vals ? 1 : 0;
    ctx->pinfo.upload_ms = now_ms() - tu;
    return 1;
}

// The plan's tiling / chunking parameters (n_adm: this shard's admissible observations).
static PlanParams plan_params(int n_adm, const Settings& st) {
    PlanParams pp;
    pp.tile_win = TILE_WIN;
    pp.chunk_pts = CHUNK_PTS;
    pp.chunk_obs = CHUNK_OBS;
    pp.tile_slots = schur_tile_slots();
    if (st.tile_pts) pp.tile_pts_env = st.tile_pts;
    pp.bs_pts = BS_PTS;
    pp.bs_obs = BS_OBS;
    // sub-segment size: ~6.5 observations per thread on large windows (C4 rocprof, fused linearisation:
    // 34.2 us at 1700 vs 36.1 at 1024, 42.7 at 512, 34.7 at 2500); MIBA_SUBSEG overrides (tuning)
    // and 256 on windows of a few thousand observations (C1's camera side in its Schur launch: shorter per-thread
    // chains, with the half-chunk tiles -2.4 % per LM iteration; neutral at C3's 8k, which keeps 1024)
    pp.subseg = n_adm >= 200000 ? SUBSEG_OBS_LARGE : n_adm < 4096 ? SUBSEG_OBS_SMALL : SUBSEG_OBS;
    if (st.subseg) pp.subseg = st.subseg;
    return pp;
}

// MIBA_DEVICE_PLAN: 0 = the host plan; 1 = the device plan whenever the window fits it; unset = the device plan on
// windows of >= DPLAN_MIN_OBS observations (prepare, host vs device plan: C1, 1.6k observations, 0.15 vs 0.21 ms;
// C3, 8k, 0.26 vs 0.23-0.37; C2, 50k, 0.87 vs 0.31-0.34; C4, 1M, 2.8 vs 1.3-1.5)
static constexpr int DPLAN_MIN_OBS = 16384;
// windows from which a helper thread builds the host side of the plan while the values are staged (below, the
// thread costs more than the overlap saves)
static constexpr int DPLAN_HELPER_OBS = 262144;
static bool want_dplan(const Settings& st, int nc, int np, int no) {
    if (st.device_plan == 0) return false;
    if (!dplan_fits(no, np, nc)) return false;
    return st.device_plan == 1 || no >= DPLAN_MIN_OBS;
}

// The window a full prepare is building: its sizes and what the phases hand on to each other.
struct Win {
    const ba_problem* p = nullptr;
    int nc = 0, np = 0, no = 0;  // (zeros while the problem is invalid)
    bool shard = false;          // landmark shards: collectives in the prepare and in every LM iteration
    bool want_det = false;       // ba_options.deterministic, or a gathered window
    bool det = false;            // ... and the window has Schur tiles: per-tile slabs (stage_and_upload_plan_arrays)
    bool dplan = false;          // the device plan builds this window
    bool dplan_built = false;    // ... and its helper thread has built the host side already
    bool notf32 = false;         // device plan: an admissible pixel / depth is no exact f32
    bool params_up = false;      // the parameters are uploaded (the device plan's prepare)
    int n_adm_all = 0;           // admissible observations over all shards
    int n_seg = 0, n_env = 0, n_bs_chunks = 0, nblk_pt = 0, part_stride = 0;  // alloc_work_buffers
    double tp0 = 0, tp_raw = 0;
};

// The device plan's prepare: the indices and admissibility bytes staged and DMA'd first; the plan's passes
// enqueued behind them (the last one writes the summary into mapped host memory, no DMA engine involved); the
// depths, pixels (obs32 checked on the way) and parameters staged meanwhile and DMA'd on the copy stream; then one
// wait for the passes. w.dplan = false afterwards: a point list longer than the device sort takes, or a scan that
// did not settle (the host plan builds the window instead; the staged upload stands).
static int run_dplan(ba_context* ctx, Win& w) {
    const ba_problem* p = w.p;
    const int nc = w.nc, np = w.np, no = w.no;
    hipStream_t s = ctx->stream;
    w.dplan_built = false;
    const bool times = ctx->st.plan_times;  // diagnostic: host phases of the device plan
    double tm = now_ms();
    auto mark = [&](const char* what) {
        if (!times) return;
        const double t = now_ms();
        std::fprintf(stderr, "dplan %s %.3f ms\n", what, t - tm);
        tm = t;
    };
    if (int rc = raw_stage_begin(ctx, no, true)) return rc;
    RawStage rs(ctx->stage, (size_t)no);
    mark("buffers");
    stage_indices_adm(rs, p, (size_t)no);
    mark("stage_indices");
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_CAM].p, rs.cam, 4 * (size_t)no, hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_PT].p, rs.pt, 4 * (size_t)no, hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_ADM].p, rs.adm, (size_t)no, hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipEventRecord(ctx->ev_idx, s));
    const size_t nsum = dplan_sum_ints(nc, np);
    HIPCHECK(ctx, ctx->buf[B_DP_SCRATCH].ensure(4 * dplan_scratch_ints(no, np, nc)));
    HIPCHECK(ctx, ctx->buf[B_DP_PO_DEST].ensure(4 * (size_t)no));
    HIPCHECK(ctx, ctx->buf[B_DP_CO_DEST].ensure(4 * (size_t)no));
    HIPCHECK(ctx, ctx->buf[B_DP_CAM_AC].ensure(4 * (size_t)nc));
    HIPCHECK(ctx, ctx->buf[B_DP_PT_IDX].ensure(4 * (size_t)np));
    HIPCHECK(ctx, ctx->buf[B_DP_OVF].ensure(4 * (size_t)no));
    HIPCHECK(ctx, ctx->buf[B_DP_SUM].ensure(4 * nsum));
    HIPCHECK(ctx, ctx->rsum.ensure(4 * nsum));
    DPlanArgs a{};
    a.cam = ctx->buf[B_RAW_CAM].as<int>();
    a.pt = ctx->buf[B_RAW_PT].as<int>();
    a.adm = ctx->buf[B_RAW_ADM].as<unsigned char>();
    a.no = no; a.np = np; a.nc = nc; a.fixed_cam = p->fixed_cam;
    a.tile_win = TILE_WIN; a.chunk_obs = CHUNK_OBS;
    a.po_dest = ctx->buf[B_DP_PO_DEST].as<int>();
    a.co_dest = ctx->buf[B_DP_CO_DEST].as<int>();
    a.cam_ac = ctx->buf[B_DP_CAM_AC].as<int>();
    a.pt_idx = ctx->buf[B_DP_PT_IDX].as<int>();
    a.ovf_obs = ctx->buf[B_DP_OVF].as<int>();
    a.sum = ctx->buf[B_DP_SUM].as<int>();
    a.sum_host = static_cast<int*>(ctx->rsum.dev);
    a.scratch = ctx->buf[B_DP_SCRATCH].as<int>();
    if (ctx->cmask_any) {  // prepare_core has checked its size against nc
        HIPCHECK(ctx, ctx->buf[B_DP_CONST].ensure((size_t)nc));
        HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_DP_CONST].p, ctx->cmask.data(), (size_t)nc, hipMemcpyHostToDevice, s));
        a.cam_const = ctx->buf[B_DP_CONST].as<unsigned char>();
    }
    const uint8_t* cam_const = ctx->cmask_any ? ctx->cmask.data() : nullptr;
    HIPCHECK(ctx, dplan_enqueue(a, s));
    mark("enqueue");
    // a helper thread waits for the passes and builds the host side of the plan (tiles, chunks, segments) from the
    // summary while this thread stages the values and parameters
    hipError_t helper_err = hipSuccess;
    const int* sm = ctx->rsum.as<int>();
    auto build_host_side = [&]() {
        helper_err = hipStreamSynchronize(s);
        if (helper_err == hipSuccess && sm[DP_TOOLONG] == 0 && sm[DP_BAD] == INT_MAX) {
            plan_from_device(sm, nc, np, p->fixed_cam, plan_params(sm[DP_NADM], ctx->st), ctx->plan, cam_const);
            w.dplan_built = true;
        }
    };
    std::thread helper;
    if (no >= DPLAN_HELPER_OBS) helper = std::thread(build_host_side);
    struct Join {
        std::thread& t;
        ~Join() { if (t.joinable()) t.join(); }
    } join{helper};
    // host work while the passes run: the values (behind the index DMA on the copy stream) and the parameters
    hipStream_t cs = ctx->copy_stream;
    HIPCHECK(ctx, hipStreamWaitEvent(cs, ctx->ev_idx, 0));
    // the values in pieces, each DMA'd while the next is staged (the copies and the DMA share the host's memory
    // bandwidth: same-box A/B, prepare ms at 1 / 2 / 4 / 8 pieces: C4 1.28-1.59 / 1.29-1.37 / 1.26-1.28 /
    // 1.36-1.42, C5 7.44 / 5.10 / 5.78 / 6.33); MIBA_VALUE_CHUNKS overrides
    const int nchunk = ctx->st.value_chunks ? ctx->st.value_chunks : no >= (1 << 19) ? 2 : 1;
    w.notf32 = false;
    for (int c = 0; c < nchunk; ++c) {
        const size_t lo = (size_t)no * c / nchunk, n = (size_t)no * (c + 1) / nchunk - lo;
        if (!n) continue;
        w.notf32 = stage_values_f32check(rs.uv + 2 * lo, rs.dep + lo, p->obs_uv + 2 * lo, p->obs_depth + lo, n) || w.notf32;
        HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_DEP].as<double>() + lo, rs.dep + lo, 8 * n, hipMemcpyHostToDevice,
                                     cs));
        HIPCHECK(ctx, hipMemcpyAsync(ctx->buf[B_RAW_UV].as<double>() + 2 * lo, rs.uv + 2 * lo, 16 * n,
                                     hipMemcpyHostToDevice, cs));
    }
    mark("stage_values");
    if (int rc = upload_params(ctx, p, cs)) return rc;
    HIPCHECK(ctx, hipEventRecord(ctx->ev_uv, cs));
    ctx->uv_pending = true;
    mark("params");
    if (helper.joinable()) helper.join();
    else build_host_side();
    HIPCHECK(ctx, helper_err);
    mark("helper");
    w.dplan = sm[DP_TOOLONG] == 0;
    w.params_up = true;
    return BA_OK;
}

// The arrays of B_PLAN, in upload order (ctx->plan_parts; ba_debug_plan_digest digests them in this order)
enum PlanPart { PO_DEST, CO_DEST, CAM_AC, PT_PTR, PT_IDX, SEG_PTR, SEG_CAM, SEG_AC, AC_SEG, AC_CAM, FCOL, TILE_CHUNK,
                TILE_BASE, TILE_SPAN, CHUNK_AP, BS_CHUNK, OVF_OBS, RPTR, ROWS, ENV_TILE, TRANGE };
static int* plan_part(const ba_context* ctx, int k) {
    return ctx->buf[B_PLAN].as<int>() + ctx->plan_parts[k].first;
}

// The plan's index arrays in one staged DMA (each array 256-byte aligned in B_PLAN; device plan: po_dest, co_dest,
// pt_idx and ovf_obs are copied on the device into their slots), then the parameters unless they are up already.
static int stage_and_upload_plan_arrays(ba_context* ctx, Win& w) {
    const Plan& pl = ctx->plan;
    hipStream_t s = ctx->stream;
    const int nc = w.nc, no = w.no, nac = pl.nac, nb = pl.nb, n_ap = pl.n_ap();
    w.det = w.want_det && !pl.tile_base.empty();
    std::vector<int> trange;  // deterministic mode: each active camera's Schur tile range
    if (w.det) {
        trange.assign(2 * (size_t)std::max(nac, 1), 0);
        const int nt = (int)pl.tile_base.size();
        for (int a = 0, lo = 0, hi = 0; a < nac; ++a) {
            while (lo < nt && pl.tile_base[lo] < a - (TILE_WIN - 1)) ++lo;
            while (hi < nt && pl.tile_base[hi] <= a) ++hi;
            trange[2 * a] = lo;
            trange[2 * a + 1] = std::max(lo, hi);
        }
    }
    struct Part { const int* src; size_t n; size_t off; const int* dev; };
    auto dv = [&](int id) -> const int* { return pl.dev ? ctx->buf[id].as<int>() : nullptr; };
    std::vector<Part> parts = {
        {pl.po_dest.data(), (size_t)no, 0, dv(B_DP_PO_DEST)}, {pl.co_dest.data(), (size_t)no, 0, dv(B_DP_CO_DEST)},
        {pl.cam_ac.data(), (size_t)nc, 0, nullptr},
        {pl.pt_ptr.data(), (size_t)n_ap + 1, 0, nullptr}, {pl.pt_idx.data(), (size_t)n_ap, 0, dv(B_DP_PT_IDX)},
        {pl.seg_ptr.data(), pl.seg_ptr.size(), 0}, {pl.seg_cam.data(), pl.seg_cam.size(), 0},
        {pl.seg_ac.data(), pl.seg_ac.size(), 0}, {pl.ac_seg.data(), pl.ac_seg.size(), 0},
        {pl.ac_cam.data(), (size_t)nac, 0}, {pl.fcol.data(), (size_t)nb, 0},
        {pl.tile_chunk.data(), pl.tile_chunk.size(), 0}, {pl.tile_base.data(), pl.tile_base.size(), 0},
        {pl.tile_span.data(), pl.tile_span.size(), 0}, {pl.chunk_ap.data(), pl.chunk_ap.size(), 0},
        {pl.bs_chunk.data(), pl.bs_chunk.size(), 0}, {pl.ovf_obs.data(), (size_t)pl.n_ovf(), 0, dv(B_DP_OVF)},
        {pl.rptr.data(), (size_t)nb + 1, 0}, {pl.rows.data(), pl.rows.size(), 0},
        {pl.env_tile.data(), pl.env_tile.size(), 0}, {trange.data(), trange.size(), 0}};
    size_t plan_ints = 0;
    for (Part& q : parts) {
        q.off = plan_ints;
        plan_ints += (q.n + 63) / 64 * 64 + 64;
    }
    const size_t raw_bytes = raw_stage_bytes((size_t)no);
    const size_t raw_off = (raw_bytes + 255) / 256 * 256;  // after the raw region, which may still be in flight
    if (ctx->stage.cap < raw_off + 4 * plan_ints) {
        // growing frees the buffer the raw DMAs read: the index DMA on `stream`, the device plan's pixel /
        // depth DMA on the copy stream
        HIPCHECK(ctx, hipStreamSynchronize(s));
        if (ctx->uv_pending) HIPCHECK(ctx, hipEventSynchronize(ctx->ev_uv));
        HIPCHECK(ctx, ctx->stage.ensure(raw_off + 4 * plan_ints, raw_bytes));
    }
    int* sp = reinterpret_cast<int*>(ctx->stage.as<char>() + raw_off);
    std::vector<StageCopy> cp;
    for (const Part& q : parts)
        if (q.n && !q.dev) cp.push_back({sp + q.off, q.src, 4 * q.n});
    stage_copy(cp);
    HIPCHECK(ctx, ctx->buf[B_PLAN].ensure(4 * plan_ints));
    int* dp = ctx->buf[B_PLAN].as<int>();
    // device plan: from the first host part on (po_dest / co_dest lead and come device-to-device)
    const size_t lo = pl.dev ? parts[CAM_AC].off : 0;
    HIPCHECK(ctx, hipMemcpyAsync(dp + lo, sp + lo, 4 * (plan_ints - lo), hipMemcpyHostToDevice, s));
    ctx->plan_parts.clear();
    for (const Part& q : parts) {
        ctx->plan_parts.emplace_back(q.off, q.n);
        if (q.n && q.dev) HIPCHECK(ctx, hipMemcpyAsync(dp + q.off, q.dev, 4 * q.n, hipMemcpyDeviceToDevice, s));
    }
    if (!w.params_up)
        if (int rc = upload_params(ctx, w.p, s)) return rc;
    return BA_OK;
}

// Sizes every buffer of DevProblem / DevWork for this window; the shard exchange buffers start as zeros, S, rhs and
// the partial slots cleared.
static int alloc_work_buffers(ba_context* ctx, Win& w) {
    const Plan& pl = ctx->plan;
    hipStream_t s = ctx->stream;
    const int n_adm = pl.n_adm, n_ap = pl.n_ap(), nac = pl.nac, npad = pl.npad;
    const int n_seg = w.n_seg = (int)pl.seg_cam.size();
    const int n_env = w.n_env = (int)pl.env_tile.size() / 2;
    const int n_bs_chunks = w.n_bs_chunks = (int)pl.bs_chunk.size() - 1;
    // the observation layouts, gathered on the device from the raw window and the plan's orderings
    // ... in ONE layout: the 16-byte records on obs32 windows, the f64 arrays otherwise (the index arrays always)
    const size_t na = std::max<size_t>(n_adm, 1);
    HIPCHECK(ctx, ctx->buf[B_PO_AC].ensure(4 * na));
    HIPCHECK(ctx, ctx->buf[B_PO_AP].ensure(4 * na));
    HIPCHECK(ctx, ctx->buf[B_PO_PT].ensure(4 * na));
    if (pl.obs32) {
        HIPCHECK(ctx, ctx->buf[B_PO_REC].ensure(16 * na));
        HIPCHECK(ctx, ctx->buf[B_CO_REC].ensure(16 * na));
    } else {
        HIPCHECK(ctx, ctx->buf[B_PO_CAM].ensure(4 * na));
        HIPCHECK(ctx, ctx->buf[B_PO_UV].ensure(16 * na));
        HIPCHECK(ctx, ctx->buf[B_PO_DEP].ensure(8 * na));
        HIPCHECK(ctx, ctx->buf[B_CO_PT].ensure(4 * na));
        HIPCHECK(ctx, ctx->buf[B_CO_UV].ensure(16 * na));
        HIPCHECK(ctx, ctx->buf[B_CO_DEP].ensure(8 * na));
    }
    ctx->ac_cam = pl.ac_cam;
    ctx->pt_idx = pl.pt_idx;
    w.nblk_pt = pp_blocks(n_ap, PP_LANES_MAX);  // part slots sized for the widest lane grouping
    // (+ the small-window launch's per-tile and non-tiled point partials, §3 of DESIGN)
    w.part_stride = std::max({w.nblk_pt, (nac + 1 + 255) / 256, n_bs_chunks, (nac + BCR_CAMS - 1) / BCR_CAMS,
                              (int)pl.tile_base.size() + pp_blocks(n_ap - pl.n_tiled, PP_LANES_MAX), 1});
    const size_t camdata_bytes = sizeof(double) * ((size_t)CAMDATA * std::max(nac, 1) + 16);
    HIPCHECK(ctx, ctx->buf[B_CAMDATA].ensure(camdata_bytes));
    // landmark sharding: pack buffers of the envelope tiles of S, exchange scalars
    if (w.shard) {
        // envelope tiles + rhs (+ the camera and intrinsics sums of the folded exchange)
        const size_t ne = (size_t)n_env * 256 + (size_t)npad + (size_t)nac * CAMDATA + SEGINTR + 1;
        HIPCHECK(ctx, ctx->buf[B_CAMDATA_LOC].ensure(camdata_bytes));
        HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_CAMDATA_LOC].p, 0, camdata_bytes, s));
        HIPCHECK(ctx, ctx->buf[B_ENV_LOC].ensure(sizeof(double) * ne));
        const size_t nred = RED_X + 4 + 2 * (size_t)ctx->W.comm.nranks;
        HIPCHECK(ctx, ctx->buf[B_RED].ensure(sizeof(double) * nred));
        HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_RED].p, 0, sizeof(double) * nred, s));
    }
    HIPCHECK(ctx, ctx->buf[B_SEGINTR].ensure(sizeof(double) * SEGINTR * std::max(n_seg, 1)));
    HIPCHECK(ctx, ctx->buf[B_CAMPART].ensure(sizeof(double) * CAMDATA * std::max(n_seg, 1)));
    HIPCHECK(ctx, ctx->buf[B_LIN].ensure(sizeof(double) * LIN_N));
    HIPCHECK(ctx, ctx->buf[B_SCALE].ensure(sizeof(double) * (6 * nac + 3 * (size_t)n_ap + 4)));
    HIPCHECK(ctx, ctx->buf[B_CNP].ensure(sizeof(double) * 3 * std::max(n_ap, 1)));
    HIPCHECK(ctx, ctx->buf[B_PDATA].ensure(sizeof(double) * PDATA * std::max(n_ap, 1)));
    HIPCHECK(ctx, ctx->buf[B_S].ensure(sizeof(double) * (size_t)npad * npad));
    HIPCHECK(ctx, ctx->buf[B_RHS].ensure(sizeof(double) * npad));
    HIPCHECK(ctx, ctx->buf[B_DELTA].ensure(sizeof(double) * npad));
    HIPCHECK(ctx, ctx->buf[B_PART].ensure(sizeof(double) * PART_NSLOTS * w.part_stride));
    HIPCHECK(ctx, ctx->buf[B_SCAL].ensure(sizeof(double) * SC_N));
    HIPCHECK(ctx, ctx->buf[B_FLAG].ensure(sizeof(int) * 8));
    HIPCHECK(ctx, ctx->buf[B_STATE].ensure(sizeof(LmState)));
    HIPCHECK(ctx, ctx->buf[B_LOG].ensure(sizeof(double) * LOG_W * (std::max(ctx->opts.max_num_iterations, 0) + 2)));
    return clear_solve_state(ctx, npad, w.part_stride);
}

// DevProblem's pointers and sizes, then the observation layouts gathered on the device.
static int wire_problem(ba_context* ctx, const Win& w) {
    const Plan& pl = ctx->plan;
    hipStream_t s = ctx->stream;
    DevProblem& P = ctx->P;
    auto dptr = [&](int k) { return plan_part(ctx, k); };
    const int nac = pl.nac, n_ap = pl.n_ap();
    P.cams[0] = ctx->buf[B_CAMS0].as<double>(); P.cams[1] = ctx->buf[B_CAMS1].as<double>();
    P.pts[0] = ctx->buf[B_PTS0].as<double>(); P.pts[1] = ctx->buf[B_PTS1].as<double>();
    P.K[0] = ctx->buf[B_K0].as<double>(); P.K[1] = ctx->buf[B_K1].as<double>();
    P.prior = ctx->buf[B_PRIOR].as<double>();
    const bool f64l = !pl.obs32;  // the f64 layout (else nullptr: no kernel of an obs32 window reads it)
    P.po_cam = f64l ? ctx->buf[B_PO_CAM].as<int>() : nullptr; P.po_ac = ctx->buf[B_PO_AC].as<int>();
    P.po_uv = f64l ? ctx->buf[B_PO_UV].as<double2>() : nullptr;
    P.po_depth = f64l ? ctx->buf[B_PO_DEP].as<double>() : nullptr;
    P.po_ap = ctx->buf[B_PO_AP].as<int>(); P.po_pt = ctx->buf[B_PO_PT].as<int>();
    P.pt_ptr = dptr(PT_PTR);
    P.pt_idx = dptr(PT_IDX);
    P.co_pt = f64l ? ctx->buf[B_CO_PT].as<int>() : nullptr;
    P.co_uv = f64l ? ctx->buf[B_CO_UV].as<double2>() : nullptr;
    P.co_depth = f64l ? ctx->buf[B_CO_DEP].as<double>() : nullptr;
    P.obs32 = pl.obs32 ? 1 : 0;
    P.po_rec = pl.obs32 ? ctx->buf[B_PO_REC].as<float4>() : nullptr;
    P.co_rec = pl.obs32 ? ctx->buf[B_CO_REC].as<float4>() : nullptr;
    P.seg_ptr = dptr(SEG_PTR); P.seg_cam = dptr(SEG_CAM);
    P.seg_ac = dptr(SEG_AC); P.ac_cam = dptr(AC_CAM);
    P.ac_seg = reinterpret_cast<const int2*>(dptr(AC_SEG));
    P.tile_chunk = dptr(TILE_CHUNK); P.tile_base = dptr(TILE_BASE);
    P.tile_span = dptr(TILE_SPAN); P.chunk_ap = dptr(CHUNK_AP);
    P.ovf_obs = dptr(OVF_OBS);
    P.bs_chunk = dptr(BS_CHUNK);
    P.n_bs_chunks = w.n_bs_chunks;
    P.n_tiles = (int)pl.tile_base.size(); P.n_ovf_obs = pl.n_ovf();
    P.n_tiled_pts = pl.n_tiled;
    ctx->n_tiles = P.n_tiles; ctx->n_ovf_obs = P.n_ovf_obs; ctx->n_tiled_pts = pl.n_tiled;
    P.n_seg = w.n_seg; P.n_ap = n_ap; P.n_adm = pl.n_adm; P.nac = nac; P.n_cams = w.nc;
    P.n = pl.n; P.npad = pl.npad; P.kb = 6 * nac;
    P.off_pt = 6 * nac; P.off_k = 6 * nac + 3 * n_ap;
    P.part_stride = w.part_stride;
    P.rank = ctx->W.comm.rank;
    P.nranks = ctx->W.comm.nranks;
    P.xcd_map = ctx->st.xcd_map ? 1 : 0;
    PrepRaw R;
    R.cam = ctx->buf[B_RAW_CAM].as<int>();
    R.pt = ctx->buf[B_RAW_PT].as<int>();
    R.uv = ctx->buf[B_RAW_UV].as<double2>();
    R.depth = ctx->buf[B_RAW_DEP].as<double>();
    R.cam_ac = dptr(CAM_AC);
    R.po_dest = dptr(PO_DEST);
    R.co_dest = dptr(CO_DEST);
    R.n_obs = w.no;
    ctx->raw = R;
    if (ctx->uv_pending) {  // the device plan's pixel DMA (copy stream)
        HIPCHECK(ctx, hipStreamWaitEvent(s, ctx->ev_uv, 0));
        ctx->uv_pending = false;
    }
    HIPCHECK(ctx, launch_prep_gather(P, R, s));
    return BA_OK;
}

// Reduced-system solver: block cyclic reduction when the camera band fits a 64-dof block (a window of
// <= 10 active cameras is one block: the root alone, its factorization on the split kernel's look-ahead
// pivot chain — C1 4.9 ms per solve against 5.6 with the band Cholesky); else the banded LDS Cholesky;
// else the dense envelope kernel.
static void choose_solver(ba_context* ctx) {
    const Plan& pl = ctx->plan;
    const Settings& st = ctx->st;
    DevProblem& P = ctx->P;
    const int nb = pl.nb, band_w = pl.band_w, cam_band = pl.cam_band;
    P.band_w = (nb >= 2 && nb <= 2048 && band_w <= 6) ? std::max(band_w, 1) : 0;
    P.cam_band = cam_band;
    const int bcr_nblk = (pl.nac + BCR_CAMS - 1) / BCR_CAMS;
    const bool bcr_fits = cam_band < BCR_CAMS && bcr_nblk >= 1;
    P.solver = bcr_fits ? 2 : (P.band_w > 0 ? 1 : 0);
    // wide windows (no narrow band: global BA, loop closures): from npad >= BLOCKED_MIN_NPAD the blocked
    // multi-workgroup Cholesky (ba_dense.hip) instead of the one-workgroup envelope kernel
    const long long bmin = st.blocked_min_set ? st.blocked_min : BLOCKED_MIN_NPAD;
    if (P.solver == 0 && pl.npad >= bmin) P.solver = 3;
    if (st.solver == 0 || st.solver == 3) P.solver = st.solver;
    else if (st.solver == 1 && P.band_w > 0) P.solver = 1;
    else if (st.solver == 2 && bcr_fits) P.solver = 2;
    if (st.dense_chol) P.solver = 0;
}

// The BCR workspace laid out (bcr_layout), the elimination tree's shape, the path probed (bcr_setup).
static int setup_bcr(ba_context* ctx) {
    const int nblk = (ctx->P.nac + BCR_CAMS - 1) / BCR_CAMS;
    HIPCHECK(ctx, ctx->buf[B_BCR].ensure(bcr_bytes(nblk)));
    BcrWork& Bw = ctx->W.bcr;
    Bw.nblk = nblk;
    Bw.levels = 0;
    while ((1 << Bw.levels) < nblk) ++Bw.levels;
    // balanced elimination tree for the split kernels: K = floor(log2 nblk), v = i + 2^K - nblk/2,
    // so [voff, voff + nblk) holds one multiple of 2^K (the root, block nblk/2) and none of 2^(K+1)
    Bw.vlevels = 0;
    while ((2 << Bw.vlevels) <= nblk) ++Bw.vlevels;
    Bw.voff = (1 << Bw.vlevels) - nblk / 2;
    Bw.vroot = nblk / 2;
    const char* base = ctx->buf[B_BCR].as<char>();
    if (bcr_layout(Bw, ctx->buf[B_BCR].as<double>(), nblk) != base + bcr_bytes(nblk)) {
        ctx->err = "BCR workspace layout does not match bcr_bytes";
        return BA_E_INTERNAL;
    }
    return bcr_setup(ctx);
}

// The blocked Cholesky's envelope at 64-block granularity: its index buffer (one upload) and work matrices.
static int setup_blocked(ba_context* ctx) {
    DensePlan& dp = ctx->dplan;
    dense_plan(ctx->plan.fcol, ctx->plan.npad, dp);
    std::vector<int>& h = ctx->dplan_idx;
    h.clear();
    const size_t o_bf = 0, o_rs = o_bf + dp.bfcol.size(), o_cp = o_rs + dp.rowstart.size(),
                 o_cr = o_cp + dp.crptr.size();
    size_t o_bk = o_cr + dp.crows.size();
    o_bk += o_bk & 1;  // int2 alignment
    h.insert(h.end(), dp.bfcol.begin(), dp.bfcol.end());
    h.insert(h.end(), dp.rowstart.begin(), dp.rowstart.end());
    h.insert(h.end(), dp.crptr.begin(), dp.crptr.end());
    h.insert(h.end(), dp.crows.begin(), dp.crows.end());
    h.resize(o_bk, 0);
    h.insert(h.end(), dp.blk.begin(), dp.blk.end());
    HIPCHECK(ctx, upload(ctx, B_DENSE_IDX, h.data(), h.size()));
    HIPCHECK(ctx, ctx->buf[B_DENSE_A].ensure(sizeof(double) * DENSE_BB * (size_t)dp.n_env()));
    HIPCHECK(ctx, ctx->buf[B_DENSE_Z].ensure(sizeof(double) * DENSE_BB * (size_t)dp.nblk));
    HIPCHECK(ctx, ctx->buf[B_DENSE_B].ensure(sizeof(double) * DENSE_B * (size_t)dp.nblk));
    DenseWork& D = ctx->W.dense;
    const int* base = ctx->buf[B_DENSE_IDX].as<int>();
    D.A = ctx->buf[B_DENSE_A].as<double>();
    D.Zd = ctx->buf[B_DENSE_Z].as<double>();
    D.bz = ctx->buf[B_DENSE_B].as<double>();
    D.bfcol = base + o_bf; D.rowstart = base + o_rs; D.crptr = base + o_cp; D.crows = base + o_cr;
    D.blk = reinterpret_cast<const int2*>(base + o_bk);
    D.nblk = dp.nblk; D.n_env = dp.n_env();
    D.h_crptr = dp.crptr.data();
    return BA_OK;
}

// DevWork's pointers; deterministic mode: the Schur tiles write per-tile slabs, summed in tile order per element
// of S.
static int wire_work(ba_context* ctx, const Win& w) {
    DevWork& W = ctx->W;
    auto dptr = [&](int k) { return plan_part(ctx, k); };
    W.camdata = ctx->buf[B_CAMDATA].as<double>(); W.seg_intr = ctx->buf[B_SEGINTR].as<double>();
    W.camdata_loc = w.shard ? ctx->buf[B_CAMDATA_LOC].as<double>() : W.camdata;
    W.camdata_part = ctx->buf[B_CAMPART].as<double>();
    W.env_tile = reinterpret_cast<const int2*>(dptr(ENV_TILE));
    W.n_env = w.n_env;
    W.env_loc = w.shard ? ctx->buf[B_ENV_LOC].as<double>() : nullptr;
    W.red = w.shard ? ctx->buf[B_RED].as<double>() : nullptr;
    W.lin = ctx->buf[B_LIN].as<double>(); W.scale = ctx->buf[B_SCALE].as<double>();
    W.cnp = ctx->buf[B_CNP].as<double>(); W.pdata = ctx->buf[B_PDATA].as<double>();
    W.S = ctx->buf[B_S].as<double>(); W.rhs = ctx->buf[B_RHS].as<double>();
    W.delta = ctx->buf[B_DELTA].as<double>(); W.part = ctx->buf[B_PART].as<double>();
    W.scal = ctx->buf[B_SCAL].as<double>(); W.chol_flag = ctx->buf[B_FLAG].as<int>();
    W.fcol = dptr(FCOL); W.rptr = dptr(RPTR); W.rows = dptr(ROWS);
    W.st = ctx->buf[B_STATE].as<LmState>(); W.log = ctx->buf[B_LOG].as<double>();
    W.det_tbuf = nullptr;
    W.det_trange = nullptr;
    if (w.det) {
        HIPCHECK(ctx, ctx->buf[B_DET_TBUF].ensure(sizeof(double) * SCH_TBUF * (size_t)ctx->P.n_tiles));
        W.det_tbuf = ctx->buf[B_DET_TBUF].as<double>();
        W.det_trange = reinterpret_cast<const int2*>(dptr(TRANGE));
    }
    return BA_OK;
}

// The window's LM loop can take the band tail launch: known before bcr_setup, which picks the band solve for a
// one-block window only then.
static bool tail_possible(const ba_context* ctx, const Win& w) {
    return !w.shard && !w.det && ctx->P.n_ap > 0 && w.n_seg > 0 && ctx->st.fused && ctx->st.tail &&
           w.n_bs_chunks + 2 <= 128;
}

// The launch paths of the LM loop: fused linearisation, band tail, fused back-substitution + decision, the
// small-window Schur launch, the point side in the Schur tiles; their hand-off words start as zeros.
static int choose_launch_paths(ba_context* ctx, const Win& w) {
    const Settings& st = ctx->st;
    const DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    hipStream_t s = ctx->stream;
    const bool shard = w.shard;
    const int n_ap = P.n_ap, n_seg = P.n_seg, nac = P.nac;
    // fused LM-loop linearisation (k_lin_point + envelope tiles in k_schur_tile, S / rhs zeroed by the previous
    // iteration): the unsharded default-mode path with points and camera segments
    // landmark shards: the same choice on every rank (it fixes the collective sequence), so only uniform inputs
    W.fused = (shard ? (!ctx->opts.deterministic && st.fused)
                     : (!W.det_tbuf && n_ap > 0 && n_seg > 0 && st.fused)) ? 1 : 0;
    // the band solve's tail (back-substitution chunks + decision) in its launch: unsharded default-mode band
    // windows whose tail fits one resident round; MIBA_TAIL=0 keeps the separate launches
    W.tail = (P.solver == 2 && W.bcr.band && W.fused && !shard && !W.det_tbuf && band_tail_blocks(P, W.bcr.band) > 0 &&
              st.tail) ? 1 : 0;
    // larger windows, opt-in (MIBA_BSFIN=1): the back-substitution chunks and the decision in one launch
    // (k_backsub_final). Measured slower at C4 (4035-4070 vs 4154-4195 LM it/s, same box: the chunks'
    // drained agent-scope partial stores and the decision workgroup's agent-scope loads cost more than the
    // k_final launch they save) and even at C2, so k_backsub_chunk + k_final stay the default
    W.bsfin = (!W.tail && W.fused && !shard && !W.det_tbuf && n_ap > 0 && P.n_bs_chunks > 0 && st.bsfin) ? 1 : 0;
    W.tail_flags = reinterpret_cast<unsigned*>(ctx->buf[B_FLAG].as<int>() + 4);
    // the band tail's y hand-off: two npad-double buffers by launch parity (flag-free, emptied by launch_reset)
    W.tail_y = nullptr;
    if (W.tail) {
        HIPCHECK(ctx, ctx->buf[B_TAIL_Y].ensure(sizeof(double) * 2 * (size_t)P.npad));
        W.tail_y = ctx->buf[B_TAIL_Y].as<double>();
    }
    W.tail_seq = 0;
    HIPCHECK(ctx, hipMemsetAsync(W.tail_flags, 0, 3 * sizeof(unsigned), s));
    // small windows: the point side inside the Schur tiles, the camera side and the non-tiled points as
    // extra workgroups of the Schur launch (no k_lin_point in the LM loop) when the whole launch is one
    // resident round (its envelope tiles wait for its camera side): one-block windows (<= BCR_CAMS active
    // cameras) and the band tail's windows. The camera side hands
    // its sums to the envelope tiles without a release fence (round 5): C3 with the tail launch 58.8-58.9 us
    // per LM iteration against 62.1-62.3 with k_lin_point (same box); round 4's fenced hand-off measured
    // 3 us slower than k_lin_point there. MIBA_SW=0: off; 2: every window that fits
    const int n_sw = P.n_tiles + 1 + n_seg + pp_blocks(n_ap - P.n_tiled_pts, 1) + w.n_env;
    const bool sw_fit = W.fused && !shard && P.n_tiles > 0 && n_sw <= 256;
    W.sw = (sw_fit && (nac <= BCR_CAMS || W.tail) && st.sw != 0) ? 1 : 0;
    if (st.sw == 2) W.sw = sw_fit ? 1 : 0;  // A/B
    // larger windows, opt-in (MIBA_FPL=1): the tiled points' point side in the Schur tiles. k_lin_point
    // 48 -> 25 us at C4 but the tiles 76 -> 133 us (their per-chunk point reduction and tail run on one
    // wave between two barriers, and the registers spill), 4140 -> 3650 LM it/s
    W.fpl = (W.fused && !shard && !W.det_tbuf && P.n_tiles > 0 && !W.sw && st.fpl) ? 1 : 0;
    W.sw_cnt = reinterpret_cast<unsigned*>(ctx->buf[B_FLAG].as<int>() + 2);
    W.sw_seq = 0;
    HIPCHECK(ctx, hipMemsetAsync(W.sw_cnt, 0, sizeof(unsigned), s));
    ctx->sw_full = W.sw;
    ctx->tail_full = W.tail;
    ctx->bsfin_full = W.bsfin;
    return BA_OK;
}

// Algorithmic (compulsory) traffic and work per launch, DESIGN.md §Roofline: each input byte read once, each
// output byte written once. kb / kf: ba_kernel_stat's bytes_per_launch / flops_per_launch, per kernel id.
static void fill_kernel_model(const Plan& pl, const DensePlan& dp, const BcrWork& Bw, const DevProblem& P, int n_env,
                              double* kb, double* kf) {
    const int nb = pl.nb, npad = P.npad;
    const double A = P.n_adm, Pn = P.n_ap, Cn = P.nac, Sg = P.n_seg;
    double env = 0;  // envelope tiles of the reduced system
    for (int k = 0; k < nb; ++k) env += (double)(pl.rptr[k + 1] - pl.rptr[k]) + 1.0;
    const double env_bytes = env * 16 * 16 * 8;
    // observation record per sweep: obs32 {u, v, depth, index} 16 B; f64 arrays: index 4 + pixel 16 + depth 8
    const double rec = P.obs32 ? 16.0 : 28.0;
    kb[K_CAM_SIDE] = A * rec + Pn * 24 + (Cn + 1) * 56 + 32 + Sg * (CAMDATA + SEGINTR) * 8;
    kb[K_CAM_REDUCE] = Sg * CAMDATA * 8 + Cn * CAMDATA * 8;
    kf[K_CAM_SIDE] = A * 420;
    kb[K_LIN_FINALIZE] = Sg * SEGINTR * 8 + Cn * (56 + 48) + LIN_N * 8;
    kb[K_POINT_COLNORM] = A * rec + Pn * (8 + 24 + 24);
    kb[K_SCALE] = (6 * Cn + 3 * Pn + 4) * 16;
    kb[K_MEMSET_S] = (double)n_env * 256 * 8;
    kb[K_ASSEMBLE] = Cn * CAMDATA * 8 + Cn * 36 * 8 + Cn * 24 * 8;
    kb[K_POINT_PREP] = A * rec + Pn * (8 + 24 + 24) + Pn * PDATA * 8;
    kf[K_POINT_PREP] = A * 300 + Pn * 200;
    kb[K_SCHUR_TILE] = A * (rec + 12) + Pn * (PDATA * 8 + 24 + 24 + 8) + env_bytes + npad * 8.0;
    kf[K_SCHUR_TILE] = A * 350 + Pn * 13300;
    kb[K_OBS_PAIRS] = P.n_ovf_obs * 40.0;
    kb[K_CHOL] = 2 * env_bytes + 3 * npad * 8.0;
    kf[K_CHOL] = 0;
    for (int k = 0; k < nb; ++k) {
        const double r = pl.rptr[k + 1] - pl.rptr[k];
        kf[K_CHOL] += (r * (r + 1) / 2) * 2.0 * 16 * 16 * 16 + r * 16 * 16 * 16 + 16 * 16 * 16 / 3.0;
    }
    if (P.solver == 3) {
        // blocked Cholesky: per launch = the solve's total / its launches. A 64^3 block product is
        // 2 * 64^3 flops and moves three blocks; the diagonal block is factored and inverted (2 * 64^3 / 3)
        const double blk = 64.0 * 64 * 8, f3 = 2.0 * 64 * 64 * 64;
        double n_pan = 0, n_tr = 0, n_lp = 0;
        for (int k = 0; k < dp.nblk; ++k) {
            const double r = dp.crptr[k + 1] - dp.crptr[k];
            n_pan += r;
            n_tr += r * (r + 1) / 2;
            n_lp += r > 0 ? 1 : 0;
        }
        n_lp = std::max(n_lp, 1.0);
        kb[K_DENSE_COPY] = 2.0 * dp.n_env() * blk + 2.0 * npad * 8;
        kb[K_DENSE_DIAG] = 2 * blk + 2 * 64 * 8.0; kf[K_DENSE_DIAG] = f3 / 3 + 64.0 * 64;
        kb[K_DENSE_PANEL] = n_pan * 3 * blk / n_lp; kf[K_DENSE_PANEL] = n_pan * f3 / n_lp;
        kb[K_DENSE_TRAIL] = (n_tr * 4 + n_pan) * blk / n_lp; kf[K_DENSE_TRAIL] = (n_tr * f3 + n_pan * 2 * 64 * 64) / n_lp;
        kb[K_DENSE_BACK] = (n_pan + dp.nblk) * blk / dp.nblk; kf[K_DENSE_BACK] = (n_pan + dp.nblk) * 2.0 * 64 * 64 / dp.nblk;
    }
    if (P.solver == 2) {
        // block cyclic reduction: per eliminated 64-dof block, Cholesky 64^3/3 + forward solve of
        // 136 columns 64^2*136 (elim); 44 16x16x64 contribution tiles (contrib); per launch =
        // solve total / launches per solve. Bytes: the blocks each kernel must read / write.
        const int nblk = Bw.nblk, L = Bw.levels;
        const double blk = 64.0 * 64 * 8, xblk = 64.0 * 136 * 8;
        double e_fl = 64.0 * 64 * 64 / 3 + 2.0 * 64 * 64 * 8, e_by = 3 * blk + 2 * 64 * 8 * 8;  // root
        double c_fl = 0, c_by = 0, b_by = 0;
        for (int m = 0; m < L; ++m) {
            const int s_ = 1 << m, nel = (nblk - s_ + 2 * s_ - 1) / (2 * s_);
            e_fl += nel * (64.0 * 64 * 64 / 3 + 64.0 * 64 * 136 * 2);
            e_by += nel * (5 * blk + blk + xblk);
            c_fl += nel * 44.0 * 16 * 16 * 64 * 2;
            c_by += nel * (xblk + 3 * blk + 2 * 64 * 8 * 8);
            b_by += nel * (blk + xblk + 3 * 64 * 8 * 8);
        }
        kf[K_BCR_ELIM] = e_fl / (L + 1); kb[K_BCR_ELIM] = e_by / (L + 1);
        kf[K_BCR_CONTRIB] = c_fl / std::max(L, 1); kb[K_BCR_CONTRIB] = c_by / std::max(L, 1);
        kf[K_BCR_BACK] = nblk * 2.0 * 64 * 64 * 8 * 2 / std::max(L, 1); kb[K_BCR_BACK] = b_by / std::max(L, 1);
        kb[K_BCR_BORDER] = nblk * (32.0 + 64 * 8) * 8;
        // persistent kernel = the whole elimination + contributions + back-substitution in one
        // launch; bytes: S blocks read once (D, level-0 couplings, border rows, rhs), the
        // contributions written once and read by the two neighbours, y written / read twice.
        // (k_bcr_split hands the eliminated blocks' X rows over instead — XL, XR, x written once and
        // read once by the survivors — which the per-launch model below counts.)
        double p_by = nblk * (blk + 4 * 64 * 8.0 + 64 * 8 * 8.0), n_el = 0;
        for (int m = 0; m < L; ++m) {
            const int s_ = 1 << m, nel = (nblk - s_ + 2 * s_ - 1) / (2 * s_);
            n_el += nel;
            if (m == 0) p_by += nel * 2 * blk;
        }
        p_by += (Bw.persist >= 2 ? n_el * 2 * (2 * blk + 64 * 8 * 8.0) : n_el * 3 * (3 * blk + 2 * 64 * 8 * 8.0)) +
                nblk * 3 * 64 * 8 * 8.0;
        kf[K_BCR_PERSIST] = e_fl + c_fl + kf[K_BCR_BACK] * std::max(L, 1);
        kb[K_BCR_PERSIST] = p_by;
    }
    kb[K_UPDATE_CAMS] = Cn * (56 * 2 + 48 * 3) + 4 * 8 * 4;
    kb[K_BACKSUB_EVAL] = A * (rec + 8) + Pn * (8 + 24 * 2 + 24 + PDATA * 8) + npad * 16.0;  // obs records read once
    kf[K_BACKSUB_EVAL] = A * 450;
    kb[K_FINAL] = (double)PART_NSLOTS * P.part_stride * 8;
    kb[K_LIN_POINT] = kb[K_CAM_SIDE] + kb[K_POINT_PREP];  // the whole linearisation pass of an accepted step
    kf[K_LIN_POINT] = kf[K_CAM_SIDE] + kf[K_POINT_PREP];
}

// The uploads and the device structure of a planned window, phase by phase (the stream sees them in this order).
static int build_device_structure(ba_context* ctx, Win& w) {
    const double tp_plan = now_ms();
    double ftm = tp_plan;
    auto fmark = [&](const char* what) {  // diagnostic: host phases
        if (!ctx->st.plan_times) return;
        const double t = now_ms();
        std::fprintf(stderr, "finish %s %.3f ms\n", what, t - ftm);
        ftm = t;
    };
    if (int rc = stage_and_upload_plan_arrays(ctx, w)) return rc;
    fmark("stage_plan");
    if (int rc = alloc_work_buffers(ctx, w)) return rc;
    if (int rc = wire_problem(ctx, w)) return rc;
    fmark("allocs_gather");
    choose_solver(ctx);
    ctx->tail_possible = tail_possible(ctx, w);
    if (ctx->P.solver == 2)
        if (int rc = setup_bcr(ctx)) return rc;
    if (ctx->P.solver == 3)
        if (int rc = setup_blocked(ctx)) return rc;
    fmark("solver_setup");
    if (int rc = wire_work(ctx, w)) return rc;
    if (int rc = choose_launch_paths(ctx, w)) return rc;
    ctx->n_adm_all = w.n_adm_all;
    ctx->nblk_pt = w.nblk_pt;
    fill_kernel_model(ctx->plan, ctx->dplan, ctx->W.bcr, ctx->P, w.n_env, ctx->k_bytes, ctx->k_flops);
    fmark("work_accounting");
    if (int rc = finish_prepare(ctx, w.nc, w.np, w.no)) return rc;
    if (ctx->st.prep_times)  // diagnostic: host phases of ba_prepare (the device work is still in flight)
        std::fprintf(stderr, "prepare: raw staging %.3f ms, plan %.3f ms, plan staging + enqueue %.3f ms (%d host threads)\n",
                     w.tp_raw - w.tp0, tp_plan - w.tp_raw, now_ms() - tp_plan, host_threads());
    ctx->pinfo.plan_ms = tp_plan - w.tp_raw;
    ctx->pinfo.upload_ms = (w.tp_raw - w.tp0) + (now_ms() - tp_plan);
    ctx->pinfo.obs_uploaded = 1;
    return BA_OK;
}

// A rank-local verdict on the problem's sizes and buffers ("" when they are usable).
static const char* validate(const ba_problem* p) {
    if (!p || p->n_cams < 0 || p->n_points < 0 || p->n_obs < 0) return "invalid problem sizes";
    if ((p->n_cams && !p->cams) || (p->n_points && !p->points) || !p->intr || !p->intr_prior ||
        (p->n_obs && (!p->obs_cam || !p->obs_pt || !p->obs_uv || !p->obs_depth)))
        return "null problem buffer";
    return "";
}

// Stage 1 of the plan: admissibility and the per-camera counts, from the device plan's summary or on the host.
static void count_window(ba_context* ctx, const Win& w, const PlanInput& in) {
    Plan& pl = ctx->plan;
    if (!w.dplan) return plan_count(in, pl);
    const int* sm = ctx->rsum.as<int>();
    pl.err = sm[DP_BAD] != INT_MAX ? "observation index out of range" : "";
    pl.n_adm = sm[DP_NADM];
    pl.obs32 = in.obs_uv != nullptr && !w.notf32;
    pl.cam_cnt.assign(sm + DP_HDR, sm + DP_HDR + w.nc);
}

// With landmark shards every rank must reach the same verdict before any further collective (a rank that bailed
// out alone would leave the others waiting): a rank-local failure (an invalid problem, 1; a staging / allocation
// error, 2) is all-reduced, with n_cams, before anything else. bad: this rank's verdict so far.
static int agree_on_verdict(ba_context* ctx, const Win& w, int bad, std::string local_err) {
    if (!w.shard) {
        if (!bad) return BA_OK;
        ctx->err = local_err;
        return BA_E_INVALID;
    }
    int verdict[3] = {bad, w.nc, -w.nc};  // [0] error code (max), [1] n_cams (min), [2] -n_cams (min)
    int local_rc = BA_OK;
    if (!verdict[0] && (local_rc = stage_raw(ctx, w.p, w.no)) != BA_OK) { local_err = ctx->err; verdict[0] = 2; }
    int rc = host_allreduce_i32(ctx, verdict, 1, COMM_MAX);
    if (rc == BA_OK) rc = host_allreduce_i32(ctx, verdict + 1, 2, COMM_MIN);
    if (rc != BA_OK) return rc;
    if (!verdict[0] && verdict[1] != -verdict[2]) { local_err = "landmark shards disagree on n_cams"; verdict[0] = 1; }
    if (!verdict[0]) return BA_OK;
    ctx->err = local_err.empty() ? (verdict[0] >= 2 ? "another landmark shard failed to stage its observations"
                                                     : "another landmark shard rejected its problem")
                                 : local_err;
    return local_rc != BA_OK ? local_rc : (verdict[0] >= 2 ? BA_E_DEVICE : BA_E_INVALID);
}

// Stages 2 and 3 of the plan. Active cameras (Ceres removes unused blocks; the gauge block is constant, :299): a
// camera is active when any shard observes it; N (the 1/N weights, :280/:290) counts every shard; the envelope /
// band of the summed S is the union over the shards.
static int order_and_envelope(ba_context* ctx, Win& w, const PlanInput& in) {
    Plan& pl = ctx->plan;
    std::vector<int> cam_seen(w.nc);
    for (int i = 0; i < w.nc; ++i) cam_seen[i] = pl.cam_cnt[i] > 0;
    w.n_adm_all = pl.n_adm;
    if (w.shard) {
        int rc = host_allreduce_i32(ctx, cam_seen.data(), w.nc, COMM_MAX);
        if (rc == BA_OK) rc = host_allreduce_i32(ctx, &w.n_adm_all, 1, COMM_SUM);
        if (rc != BA_OK) return rc;
    }
    const PlanParams pp = plan_params(pl.n_adm, ctx->st);
    if (w.dplan) {
        if (!w.dplan_built) plan_from_device(ctx->rsum.as<int>(), w.nc, w.np, in.fixed_cam, pp, pl, in.cam_const);
    } else {
        plan_order(in, cam_seen, pp, pl);
    }
    if (w.shard)
        if (int rc = host_allreduce_i32(ctx, pl.fc.data(), pl.nac, COMM_MIN)) return rc;
    plan_envelope(pl);
    return BA_OK;
}

static int prepare_core(ba_context* ctx, const ba_problem* p, bool force_det) {
    Win w;
    w.tp0 = now_ms();
    w.shard = ctx->W.comm.on();
    w.want_det = ctx->opts.deterministic || force_det;
    ctx->pinfo = ba_prepare_info{};
    ctx->pinfo.host_threads = host_threads();
    ctx->pinfo.bcr_path = -1;
    ctx->st = read_settings();
    ctx->plan.times = ctx->st.plan_times;
    std::string local_err = validate(p);
    int bad = local_err.empty() ? 0 : 1;
    // the constant cameras (ba_set_constant_cameras) belong to one n_cams (landmark shards: refused in prepare())
    if (!bad && !ctx->cmask.empty()) {
        if ((size_t)p->n_cams != ctx->cmask.size()) {
            ctx->err = "the window has " + std::to_string(p->n_cams) + " cameras, the constant-camera mask was set for " +
                       std::to_string(ctx->cmask.size()) + " (ba_set_constant_cameras)";
            return BA_E_INVALID;
        }
    }
    if (!bad) { w.p = p; w.nc = p->n_cams; w.np = p->n_points; w.no = p->n_obs; }
    // plan cache: a window with the last full prepare's structure reuses its plan (unsharded contexts)
    ba_context::PlanKey key{};
    key.nc = w.nc; key.np = w.np; key.no = w.no;
    key.fixed_cam = bad ? -1 : p->fixed_cam;
    key.det = w.want_det ? 1 : 0;
    key.env = ctx->st.key;
    if (!bad && ctx->cmask_any) key.cmask = ctx->cmask;
    if (!bad && !w.shard && !force_det && !ctx->opts.rebuild_plan && ctx->plan_ok && key == ctx->key) {
        const int r = prepare_reuse(ctx, p, w.tp0);
        if (r != 0) {
            ctx->pinfo.total_ms = now_ms() - w.tp0;
            return r < 0 ? r : BA_OK;
        }
    }
    ctx->plan_ok = false;
    ctx->prepared = false;
    // the device plan (unsharded windows that fit it) stages and uploads the window itself (run_dplan); the host
    // plan's raw upload is in flight while the plan is built (landmark shards: after the local count, its errors
    // into the verdict)
    w.dplan = !w.shard && !bad && want_dplan(ctx->st, w.nc, w.np, w.no);
    if (!w.shard && !bad && !w.dplan)
        if (int rc = stage_raw(ctx, p, w.no)) return rc;
    w.tp_raw = now_ms();
    PlanInput in;
    in.nc = w.nc; in.np = w.np; in.no = w.no;
    in.fixed_cam = bad ? -1 : p->fixed_cam;
    if (!bad && ctx->cmask_any) in.cam_const = ctx->cmask.data();
    if (!bad) { in.obs_cam = p->obs_cam; in.obs_pt = p->obs_pt; in.obs_depth = p->obs_depth; }
    // obs32 records when every admissible pixel / depth is an f32 (the reference's are); MIBA_OBS32=0: f64 arrays
    if (!bad && ctx->st.obs32) in.obs_uv = p->obs_uv;
    // the device plan: its passes run behind the index / depth upload, the parameters are staged meanwhile, one
    // read-back (the window's values are valid: a malformed window fails below, before any of them is used)
    if (w.dplan)
        if (int rc = run_dplan(ctx, w)) return rc;
    ctx->pinfo.plan_device = w.dplan ? 1 : 0;
    count_window(ctx, w, in);
    if (!bad && !ctx->plan.err.empty()) { local_err = ctx->plan.err; bad = 1; }
    if (int rc = agree_on_verdict(ctx, w, bad, local_err)) return rc;
    if (int rc = order_and_envelope(ctx, w, in)) return rc;
    // the uploads and the device structure: every collective of the prepare is behind us, so a landmark shard that
    // fails here (allocation, staging, launch) says so in one more agreement all-reduce instead of leaving the
    // other ranks to wait in the first LM iteration's collectives
    int rc = build_device_structure(ctx, w);
    if (w.shard) {
        int failed = rc != BA_OK ? 1 : 0;
        const std::string my_err = ctx->err;
        const int rc2 = host_allreduce_i32(ctx, &failed, 1, COMM_MAX);
        if (rc == BA_OK && rc2 != BA_OK) rc = rc2;
        else if (rc == BA_OK && failed) {
            ctx->err = "another landmark shard failed its prepare (device allocation / upload)";
            rc = BA_E_DEVICE;
        } else if (rc != BA_OK) ctx->err = my_err;
        if (rc != BA_OK) ctx->prepared = false;
        return rc;
    }
    if (rc != BA_OK) return rc;
    // plan cache (unsharded, not gathered): this window's structure is the context's from now on
    ctx->key = key;
    ctx->key.obs32 = ctx->plan.obs32 ? 1 : 0;
    ctx->plan_ok = !force_det;
    ctx->pinfo.total_ms = now_ms() - w.tp0;
    return BA_OK;
}
