// ba_solver.cpp — libmiba host side: the C-ABI core of include/ba.h and the LM loop (ba_prepare's phases are in
// ba_prepare.cpp, the ba_debug_* entry points in ba_debug.cpp, the stages beside the LM loop in files of their own,
// the context they share in ba_context.h).
//
// ba_solve() replaces `ceres::Solve(globalProblem.options, &problem, &summary)`
// at the reference's src/OptimizationUtils.cpp:300 for the problem assembled at
// :236-299. The trust-region control flow below restates Ceres 2.0's
// TrustRegionMinimizer::Minimize with LevenbergMarquardtStrategy;
// every numeric pass over observations / points / the reduced camera system runs
// on the GPU (ba_kernels.hip). Per iteration the host reads back 8 scalars.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>

#include "ba_stage.h"

using namespace miba;

void flush_prof(ba_context* ctx) {
    Prof& P = ctx->prof;
    for (int i = 0; i < P.n; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, P.ev[2 * i], P.ev[2 * i + 1]) == hipSuccess) {
            ctx->k_ms[P.id[i]] += ms;
            ctx->k_launches[P.id[i]] += 1;
        }
    }
    P.n = 0;
}

static thread_local std::string g_err;

void miba_set_error(const std::string& msg) { g_err = msg; }

extern "C" {

int32_t ba_api_version(void) { return BA_API_VERSION; }

const char* ba_build_info(void) {
    return "libmiba " __DATE__ " gfx950 f64; kernels: cam_side/point_prep/obs_pairs(atomic)/chol(env,mfma_f64_16x16x4)/"
           "backsub_eval";
}

void ba_default_options(ba_options* o) {
    std::memset(o, 0, sizeof(*o));
    o->hub_p_repr = 1e-3;         // BundleAdjustmentConfig.h:47
    o->hub_p_unpr = 1e-3;         // :50
    o->weight_intrinsics = 1e-6;  // :48
    o->weight_unpr = 10.0;        // :49
    o->max_num_iterations = 75;   // :64
    o->minimizer_progress_to_stdout = 1;  // :63
    o->eta = 1e-6;                // :65
    o->initial_trust_region_radius = 1e4;  // Ceres 2.0 defaults below
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->max_num_consecutive_invalid_steps = 5;
    o->jacobi_scaling = 1;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->device = -1;
    o->deterministic = 0;
    o->shard_min_obs = 262144;
    o->small_window = 0;          // ignored (the single-workgroup small-window kernel was removed)
}

ba_context* ba_create(const ba_options* opts) {
    ba_context* ctx = new ba_context();
    if (opts) ctx->opts = *opts; else ba_default_options(&ctx->opts);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_err = std::string("no HIP device available: ") + hipGetErrorString(e);
        delete ctx;
        return nullptr;
    }
    if (ctx->opts.device >= 0) {
        if (ctx->opts.device >= ndev) {
            g_err = "device ordinal out of range";
            delete ctx;
            return nullptr;
        }
        ctx->device = ctx->opts.device;
        e = hipSetDevice(ctx->device);
    } else {
        e = hipGetDevice(&ctx->device);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreate(&ctx->ev[i]);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_idx, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_uv, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->hprog, PROG_BYTES, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&ctx->dprog, ctx->hprog, 0);
    if (ctx->opts.profile_kernels) {
        for (int i = 0; i < 2 * Prof::MAXP && e == hipSuccess; ++i) e = hipEventCreate(&ctx->prof.ev[i]);
        ctx->prof_events = (e == hipSuccess);
        ctx->prof.on = 1;
        ctx->prof.mask = (unsigned)ctx->opts.profile_mask;
    }
    if (e != hipSuccess) {
        g_err = std::string("HIP init failed: ") + hipGetErrorString(e);
        delete ctx;
        return nullptr;
    }
    return ctx;
}

void ba_destroy(ba_context* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    // a prepare that returned early (e.g. BA_E_INVALID) may have left value copies queued on the copy stream:
    // they read the staging buffer and write device buffers released below
    if (ctx->copy_stream) hipStreamSynchronize(ctx->copy_stream);
    comm_destroy(ctx->W.comm);
    comm_destroy(ctx->comm_parked);
    for (auto& b : ctx->buf) b.release();
    for (auto& e : ctx->ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->cov_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->res_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->covis_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->local_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->loc_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->pts_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->pg_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->align_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->match_ev)
        if (e) hipEventDestroy(e);
    for (auto& e : ctx->gmatch_ev)
        if (e) hipEventDestroy(e);
    if (ctx->prof_events)
        for (int i = 0; i < 2 * Prof::MAXP; ++i) hipEventDestroy(ctx->prof.ev[i]);
    if (ctx->hprog) hipHostFree(ctx->hprog);
    for (PinnedBuf* b : {&ctx->hres, &ctx->stage, &ctx->pstage, &ctx->rsum}) b->release();
    if (ctx->copy_stream) {
        hipStreamSynchronize(ctx->copy_stream);
        hipStreamDestroy(ctx->copy_stream);
    }
    if (ctx->ev_idx) hipEventDestroy(ctx->ev_idx);
    if (ctx->ev_uv) hipEventDestroy(ctx->ev_uv);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* ba_last_error(const ba_context* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int32_t ba_comm_unique_id(uint8_t id[BA_COMM_ID_BYTES]) {
    if (!id) { g_err = "null id buffer"; return BA_E_INVALID; }
    if (comm_unique_id(id, BA_COMM_ID_BYTES) != 0) {
        g_err = comm_last_error();
        return BA_E_COMM;
    }
    return BA_OK;
}

int32_t ba_comm_init(ba_context* ctx, int32_t nranks, int32_t rank, const uint8_t id[BA_COMM_ID_BYTES]) {
    if (!ctx || !id) return BA_E_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return BA_E_DEVICE; }
    comm_destroy(ctx->comm_parked);
    if (comm_init(ctx->W.comm, nranks, rank, id) != 0) {
        ctx->err = comm_last_error();
        return nranks < 1 || rank < 0 || rank >= nranks ? BA_E_INVALID : BA_E_COMM;
    }
    ctx->prepared = false;  // the next solve re-prepares with the shard-global structure
    return BA_OK;
}

int32_t ba_comm_init_host(ba_context* ctx, int32_t nranks, int32_t rank, ba_allreduce_fn fn, void* user) {
    if (!ctx) return BA_E_INVALID;
    comm_destroy(ctx->comm_parked);
    if (comm_init_host(ctx->W.comm, nranks, rank, fn, user) != 0) {
        ctx->err = comm_last_error();
        return BA_E_INVALID;
    }
    ctx->prepared = false;  // the next solve re-prepares with the shard-global structure
    return BA_OK;
}

int32_t ba_iteration_log(const ba_context* ctx, double* rows, int32_t max_rows) {
    if (!ctx || ctx->last_iter < 0 || !ctx->W.log) return 0;
    const int n = ctx->last_iter + 1;
    if (rows && max_rows > 0) {
        const int m = std::min(n, (int)max_rows);
        if (hipSetDevice(ctx->device) != hipSuccess ||
            hipMemcpy(rows, ctx->W.log, sizeof(double) * LOG_W * m, hipMemcpyDeviceToHost) != hipSuccess)
            return 0;
        for (int i = 0; i < m; ++i) rows[(size_t)i * LOG_W + 7] = 0.0;
    }
    return n;
}

int32_t ba_set_options(ba_context* ctx, const ba_options* opts) {
    if (!ctx || !opts) return BA_E_INVALID;
    if (opts->device >= 0 && opts->device != ctx->device) {
        ctx->err = "ba_set_options cannot move a context to another device";
        return BA_E_INVALID;
    }
    const int dev = ctx->device;
    ctx->opts = *opts;
    ctx->opts.device = dev;
    if (ctx->opts.profile_kernels && !ctx->prof_events) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 * Prof::MAXP && e == hipSuccess; ++i) e = hipEventCreate(&ctx->prof.ev[i]);
        if (e != hipSuccess) { ctx->err = "event creation failed"; return BA_E_DEVICE; }
        ctx->prof_events = true;
    }
    ctx->prof.on = ctx->opts.profile_kernels ? 1 : 0;
    ctx->prof.mask = (unsigned)ctx->opts.profile_mask;
    return BA_OK;
}

int32_t ba_set_constant_cameras(ba_context* ctx, const uint8_t* is_constant, int32_t n_cams) {
    if (!ctx) { g_err = "null context"; return BA_E_INVALID; }
    if (n_cams < 0) { ctx->err = "ba_set_constant_cameras: negative n_cams"; return BA_E_INVALID; }
    ctx->cmask.clear();
    ctx->cmask_any = false;
    if (is_constant)
        for (int32_t i = 0; i < n_cams; ++i) {
            ctx->cmask.push_back(is_constant[i] ? 1 : 0);
            ctx->cmask_any = ctx->cmask_any || is_constant[i];
        }
    return BA_OK;
}

}  // extern "C"

// Fresh LM state (Ceres IterationZero): radius = initial_trust_region_radius.
LmState fresh_state(const ba_options& o, double radius) {
    LmState st{};
    st.radius = radius;
    st.decrease_factor = 2.0;
    st.n_succ = 1;  // iteration 0 counts as successful (Ceres convention)
    st.step_ok = 1;
    st.termination = -1;
    st.stop_next = o.max_num_iterations <= 0;
    return st;
}

void format_message(const LmState& S, char* out, size_t n) {
    switch (S.msg) {
        case MSG_MAX_ITER: std::snprintf(out, n, "Maximum number of iterations reached. Number of iterations: %d.", (int)S.msg_a); break;
        case MSG_GRAD_TOL: std::snprintf(out, n, "Gradient tolerance reached. Gradient max norm: %e <= %e", S.msg_a, S.msg_b); break;
        case MSG_MIN_RADIUS: std::snprintf(out, n, "Minimum trust region radius reached. Trust region radius: %e <= %e", S.msg_a, S.msg_b); break;
        case MSG_PARAM_TOL: std::snprintf(out, n, "Parameter tolerance reached. Relative step_norm: %e <= %e.", S.msg_a, S.msg_b); break;
        case MSG_FUNC_TOL: std::snprintf(out, n, "Function tolerance reached. |cost_change|/cost: %e <= %e", S.msg_a, S.msg_b); break;
        case MSG_INVALID: std::snprintf(out, n, "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps: %d", (int)S.msg_a); break;
        case MSG_EVAL_FAIL: std::snprintf(out, n, "Residual and Jacobian evaluation failed."); break;
        case MSG_TIMEOUT: std::snprintf(out, n, "Reduced camera solve failed: an inter-workgroup hand-off of the resident BCR kernel timed out."); break;
        default: std::snprintf(out, n, "unknown"); break;
    }
}

static void print_header() {
    std::printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  ls_iter  iter_time  total_time\n");
}
static void print_row(int it, double cost, double dc, double g, double st, double rho, double rad, double ti, double tt) {
    std::printf("% 4d % 3.6e % 3.2e % 3.2e % 3.2e % 3.2e % 3.2e % 4d % 3.2e % 3.2e\n", it, cost, dc, g, st, rho, rad, 0,
                ti * 1e-3, tt * 1e-3);
    std::fflush(stdout);
}

// The spin bound is a per-device global of the BCR module: remembered per device, set under the context's
// device (the caller has made it current), serialised across contexts / threads.
int apply_spin_limit(ba_context* ctx) {
    static std::mutex mu;
    static std::vector<unsigned> applied;  // per device; 0 = not yet set
    // tests: force the hand-off timeout path of the resident BCR kernels and of the small-window launch's wait
    const char* e = std::getenv("MIBA_BCR_SPIN_LIMIT");
    unsigned want = e ? (unsigned)std::strtoul(e, nullptr, 10) : (1u << 22);
    if (want == 0) want = 1;
    const unsigned want_sw = e ? want : (1u << 20);
    std::lock_guard<std::mutex> lock(mu);
    if ((int)applied.size() <= ctx->device) applied.resize(ctx->device + 1, 0u);
    if (applied[ctx->device] != want) {
        HIPCHECK(ctx, bcr_set_spin_limit(want));
        HIPCHECK(ctx, sw_set_spin_limit(want_sw));
        HIPCHECK(ctx, tail_set_spin_limit(want_sw));
        applied[ctx->device] = want;
    }
    return BA_OK;
}

// A hand-off of the resident BCR kernel timed out (its workgroups were not all co-resident: another context
// or process held CUs). The decision stopped the device loop without a termination and without counting the
// iteration (x, radius and the trust-region state untouched): from now on this context runs the per-level
// launches (no inter-workgroup waits), and the host re-enqueues the iteration. The in-flight iterations behind
// the decision were no-ops. S / rhs are cleared here for the re-run's assembly.
int bcr_timeout_retry(ba_context* ctx, LmState& S) {
    hipStream_t s = ctx->stream;
    HIPCHECK(ctx, hipStreamSynchronize(s));
    BcrWork& Bw = ctx->W.bcr;
    Bw.persist = 0;
    Bw.dense1 = 0;  // (k_bcr_dense1 waits only inside its workgroup: a forced spin bound can still time it out)
    ctx->W.sw = 0;  // the small-window Schur launch's envelope tiles wait for its camera side
    ctx->W.tail = 0;  // the band tail's chunks and decision wait for the solve / the chunks
    ctx->W.bsfin = 0;  // the back-substitution launch's decision workgroup waits for its chunks
    ctx->bcr_fallback = true;
    if (Bw.flags) HIPCHECK(ctx, hipMemsetAsync(Bw.flags, 0, sizeof(unsigned) * (16 + 6 * Bw.nblk), s));
    HIPCHECK(ctx, bcr_reset_pull_slots(Bw, false, s));
    // S and rhs as after a prepare: a band-tail chunk whose own wait also timed out may have zeroed S / rhs while
    // the solve workgroup had not yet run, and the solve may then have written y into rhs behind the zeroing
    // (ADVICE r5); the re-run's assembly must start from zeros
    {
        const DevProblem& P = ctx->P;
        HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_S].p, 0, sizeof(double) * (size_t)P.npad * P.npad, s));
        HIPCHECK(ctx, hipMemsetAsync(ctx->buf[B_RHS].p, 0, sizeof(double) * P.npad, s));
    }
    S.done = 0;
    S.termination = -1;
    S.msg = MSG_NONE;
    static thread_local LmState h_retry;
    h_retry = S;
    HIPCHECK(ctx, hipMemcpyAsync(ctx->W.st, &h_retry, sizeof(LmState), hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    if (ctx->hprog) __atomic_store_n(ctx->hprog, (unsigned)S.n_decide, __ATOMIC_RELEASE);
    ++ctx->bcr_retries;
    return BA_OK;
}

extern "C" int32_t ba_prepare(ba_context* ctx, const ba_problem* p) {
    if (!ctx) { g_err = "null context"; return BA_E_INVALID; }
    miba_maybe_dump_window(p, &ctx->opts);
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = apply_spin_limit(ctx)) return rc;
    const double t0 = now_ms();
    int rc = prepare(ctx, p);
    if (rc) return rc;
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pinfo.total_ms = now_ms() - t0;  // device work included
    return BA_OK;
}

extern "C" int32_t ba_last_prepare(const ba_context* ctx, ba_prepare_info* info) {
    if (!ctx || !info) return BA_E_INVALID;
    if (!sized_out_ok(info, BA_PREPARE_INFO_MIN_SIZE)) {
        g_err = "ba_last_prepare: info->struct_size below BA_PREPARE_INFO_MIN_SIZE (set it with BA_PREPARE_INFO_INIT)";
        return BA_E_INVALID;
    }
    sized_copy_out(info, ctx->pinfo);
    return BA_OK;
}

// ---- the enqueue code of an LM solve on the prepared window, shared by ba_solve_prepared and ba_debug_step
LmParams lm_params(const ba_context* ctx) {
    const ba_options& o = ctx->opts;
    LmParams prm{};
    prm.min_relative_decrease = o.min_relative_decrease;
    prm.max_radius = o.max_trust_region_radius;
    prm.min_radius = o.min_trust_region_radius;
    prm.function_tolerance = o.function_tolerance;
    prm.gradient_tolerance = o.gradient_tolerance;
    prm.parameter_tolerance = o.parameter_tolerance;
    prm.max_iter = std::max(o.max_num_iterations, 0);
    prm.max_invalid = o.max_num_consecutive_invalid_steps;
    prm.progress = ctx->dprog;
    return prm;
}

// The solve's start: the iteration log, then x and the candidate slots from the parameters of the last
// ba_prepare() (device-to-device) and the fresh state st0.
int enqueue_reset(ba_context* ctx, const LmState& st0, int n_cams) {
    DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    ctx->dbg_step_base = -1;
    const int max_iter = std::max(ctx->opts.max_num_iterations, 0);
    HIPCHECK(ctx, ctx->buf[B_LOG].ensure(sizeof(double) * LOG_W * (max_iter + 2)));
    W.log = ctx->buf[B_LOG].as<double>();
    // (a terminal row's gradient entry and every row's last entry are never written by the decision: they read
    // as zero, not as whatever the allocation held)
    HIPCHECK(ctx, hipMemsetAsync(W.log, 0, sizeof(double) * LOG_W * (max_iter + 2), ctx->stream));
    // the split BCR kernel's flags hold 4 * epoch + panel (one epoch per launch): re-initialise the hand-off
    // state long before 4 * epoch wraps (2^30 launches) on a context that re-solves one prepared window forever
    if (P.solver == 2 && ctx->bcr_launches > (1ull << 28))
        if (int rc = bcr_init_handoffs(ctx)) return rc;
    HIPCHECK(ctx, launch_reset(P, W, st0, ctx->buf[B_CAMS_INIT].as<double>(), ctx->buf[B_PTS_INIT].as<double>(),
                               ctx->buf[B_K_INIT].as<double>(), n_cams, ctx->dev_np, ctx->stream));
    return BA_OK;
}

// IterationZero: cost, gradient, column norms -> Jacobi scale, |x|.
// (fused path: S and rhs, the atomic targets of the first assembly (later ones are zeroed in-loop), were
// zeroed by k_reset)
int enqueue_iteration_zero(ba_context* ctx) {
    DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    hipStream_t s = ctx->stream;
    Prof* pf = ctx->pf();
    if (ctx->hprog) __atomic_store_n(ctx->hprog, 0u, __ATOMIC_RELEASE);
    HIPCHECK(ctx, launch_linearize(P, ctx->C, 0, W, s, pf));
    HIPCHECK(ctx, launch_scale(P, ctx->C, ctx->opts.jacobi_scaling, W, s, pf));
    HIPCHECK(ctx, launch_init_state(P, W, ctx->hprog ? ctx->dprog : nullptr, s, pf));
    return BA_OK;
}

// One LM iteration: a fixed launch sequence with device-side decisions.
int enqueue_iteration(ba_context* ctx, const LmParams& prm) {
    DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    hipStream_t s = ctx->stream;
    Prof* pf = ctx->pf();
    HIPCHECK(ctx, launch_linearize(P, ctx->C, 1, W, s, pf));
    HIPCHECK(ctx, launch_build(P, ctx->C, W, s, pf));
    HIPCHECK(ctx, launch_factor(P, ctx->C, W, s, pf));
    HIPCHECK(ctx, launch_update(P, ctx->C, prm, W, s, pf));
    if (P.solver == 2 && W.bcr.persist >= 2) ++ctx->bcr_launches;
    return BA_OK;
}

static int32_t solve_prepared(ba_context* ctx, ba_problem* p, ba_summary* sum, double t0);

// the LM loop into a full-size summary, copied out at the caller's size
static int32_t solve_prepared_out(ba_context* ctx, ba_problem* p, ba_summary* out, double t0) {
    ba_summary full{};
    const int32_t rc = solve_prepared(ctx, p, &full, t0);
    full.struct_size = (int32_t)sizeof(ba_summary);
    sized_copy_out(out, full);
    return rc;
}

static const char* const kSummarySizeErr =
    "ba_summary.struct_size below BA_SUMMARY_MIN_SIZE (set it with BA_SUMMARY_INIT)";

extern "C" int32_t ba_solve(ba_context* ctx, ba_problem* p, ba_summary* sum) {
    if (!ctx) { g_err = "null context"; return BA_E_INVALID; }
    if (!sum) { ctx->err = "null summary"; return BA_E_INVALID; }
    if (!sized_out_ok(sum, BA_SUMMARY_MIN_SIZE)) { ctx->err = kSummarySizeErr; return BA_E_INVALID; }
    miba_maybe_dump_window(p, &ctx->opts);
    const double t0 = now_ms();
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = apply_spin_limit(ctx)) return rc;
    int rc = prepare(ctx, p);
    if (rc) return rc;
    return solve_prepared_out(ctx, p, sum, t0);
}

extern "C" int32_t ba_solve_prepared(ba_context* ctx, ba_problem* p, ba_summary* sum) {
    if (!ctx) { g_err = "null context"; return BA_E_INVALID; }
    if (!sum || !p) { ctx->err = "null argument"; return BA_E_INVALID; }
    if (!sized_out_ok(sum, BA_SUMMARY_MIN_SIZE)) { ctx->err = kSummarySizeErr; return BA_E_INVALID; }
    if (!ctx->prepared || p->n_cams != ctx->prep_nc || p->n_points != ctx->prep_np || p->n_obs != ctx->prep_no) {
        ctx->err = "ba_solve_prepared: problem does not match the last ba_prepare()";
        return BA_E_INVALID;
    }
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    return solve_prepared_out(ctx, p, sum, now_ms());
}

static int32_t solve_prepared(ba_context* ctx, ba_problem* p, ba_summary* sum, double t0) {
    std::memset(sum, 0, sizeof(*sum));
    ctx->err.clear();  // ba_last_error() describes this solve from here on
    const ba_options& o = ctx->opts;
    Prof* pf = ctx->pf();
    DevProblem& P = ctx->P;
    DevWork& W = ctx->W;
    hipStream_t s = ctx->stream;
    const int max_iter = std::max(o.max_num_iterations, 0);
    static thread_local LmState h_state;  // host staging (outlives the async copies)
    h_state = fresh_state(o, o.initial_trust_region_radius);
    if (int rc = enqueue_reset(ctx, h_state, p->n_cams)) return rc;
    sum->num_obs_admissible = ctx->n_adm_all;
    sum->num_active_cams = P.nac;
    sum->num_active_points = P.n_ap;
    sum->reduced_system_size = P.n;
    sum->linear_solver = P.solver;
    sum->camera_band = P.cam_band;
    const double tl0 = now_ms();
    sum->time_setup_ms = tl0 - t0;
    double kms0[K_COUNT];
    std::memcpy(kms0, ctx->k_ms, sizeof(kms0));

    const LmParams prm = lm_params(ctx);
    if (int rc = enqueue_iteration_zero(ctx)) return rc;
    // LM iterations: fixed launch sequence, device-side decisions; the host follows the device.
    // Iterations enqueued after the termination are no-ops (their kernels exit at once).
    int launched = 0;
    int batch = 2;
    // (profiled: the blocked Cholesky's launches of one batch fit the event pool)
    const int batch_cap = P.solver == 3 ? std::max(1, std::min(8, Prof::MAXP / (4 * W.dense.nblk + 16))) : 8;
    batch = std::min(batch, batch_cap);
    int retries = 0;  // decisions that re-ran an iteration after a BCR hand-off timeout (not LM iterations)
    LmState& S = h_state;
    const bool shard = W.comm.on();
    auto launch_iter = [&]() -> int {
        if (int rc = enqueue_iteration(ctx, prm)) return rc;
        ++launched;
        return BA_OK;
    };
    // at most max_iter + 1 iterations can run (max_iter steps, then the terminal re-linearisation of the
    // stop_next iteration), plus one per re-run iteration
    auto launch_cap = [&]() { return max_iter + 1 + retries; };
    auto is_retry = [](const LmState& st) { return st.done && st.msg == MSG_TIMEOUT && st.termination < 0; };
    if (!pf && ctx->hprog) {
        // Unprofiled: keep LM_AHEAD iterations in flight and follow the device through the host-mapped
        // progress word (n_decide | done << 31, written by every decision and by a failed initial
        // evaluation) instead of synchronising the stream per batch: the GPU never waits for the host.
        // When no launch is allowed and the word has not moved for 2 ms, the host also checks that the stream
        // still runs: an idle or failed stream without a published decision (a device fault) ends the polling
        // instead of spinning. (Not sooner: a hipStreamQuery on a busy stream enqueues a marker behind the
        // last launch, which cost ~5.5 us between k_final and the next iteration's first kernel when it was
        // issued every 256 spins.)
        constexpr int LM_AHEAD = 2;
        volatile unsigned* hp = ctx->hprog;
        for (;;) {
            unsigned w = 0, w_seen = ~0u;
            auto t_seen = std::chrono::steady_clock::now();
            for (;;) {
                w = __atomic_load_n(hp, __ATOMIC_ACQUIRE);
                if (w >> 31) break;
                const auto t_now = std::chrono::steady_clock::now();
                if (w != w_seen) { w_seen = w; t_seen = t_now; }
                // no look-ahead launch past the last iteration that can run
                if (launched - (int)(w & 0x7fffffffu) < LM_AHEAD && launched < launch_cap()) {
                    if (int rc = launch_iter()) return rc;
                } else if (t_now - t_seen > std::chrono::milliseconds(2)) {
                    t_seen = t_now;
                    const hipError_t q = hipStreamQuery(s);
                    if (q == hipSuccess) {  // idle: re-read the word once (it is written before the kernel ends)
                        w = __atomic_load_n(hp, __ATOMIC_ACQUIRE);
                        break;
                    }
                    if (q != hipErrorNotReady) HIPCHECK(ctx, q);
                    std::this_thread::yield();
                } else {
                    std::this_thread::yield();
                }
            }
            // Landmark shards: every iteration issues collectives, so every rank must enqueue the same number
            // of iterations. The decisions are identical on all ranks; the host has enqueued between d and
            // d + LM_AHEAD - 1 iterations when it sees the terminating (or re-run) decision d: pad to
            // d + LM_AHEAD - 1.
            if (shard && (w >> 31)) {
                const int target = std::min((int)(w & 0x7fffffffu) + LM_AHEAD - 1, launch_cap());
                while (launched < target)
                    if (int rc = launch_iter()) return rc;
            }
            if (w >> 31) {  // the terminal state was stored to the host-mapped block before the done bit
                std::memcpy(&S, reinterpret_cast<const char*>(ctx->hprog) + PROG_STATE_OFF, sizeof(LmState));
            } else {
                HIPCHECK(ctx, hipMemcpyAsync(&S, W.st, sizeof(LmState), hipMemcpyDeviceToHost, s));
                HIPCHECK(ctx, hipStreamSynchronize(s));
            }
            if (!is_retry(S)) break;
            if (int rc = bcr_timeout_retry(ctx, S)) return rc;
            ++retries;
            launched = S.n_decide;  // every enqueued iteration has run (the ones behind the decision as no-ops)
        }
    }
    // profiled (HIP events around every launch) or no host-mapped word: batches of iterations, one
    // stream synchronisation per batch (the same batch sizes on every landmark shard)
    for (; !S.done;) {
        for (int i = 0; i < batch && launched <= launch_cap(); ++i)
            if (int rc = launch_iter()) return rc;
        HIPCHECK(ctx, hipMemcpyAsync(&S, W.st, sizeof(LmState), hipMemcpyDeviceToHost, s));
        HIPCHECK(ctx, hipStreamSynchronize(s));
        flush_prof(ctx);
        if (is_retry(S)) {
            if (int rc = bcr_timeout_retry(ctx, S)) return rc;
            ++retries;
            launched = S.n_decide;
            continue;
        }
        if (S.done || launched > launch_cap()) break;
        batch = std::min(batch * 2, batch_cap);
    }
    if (!S.done || S.msg == MSG_TIMEOUT) {  // cannot happen (max_iter bounds the loop; timeouts are re-run)
        ctx->err = "LM loop did not terminate";
        return BA_E_INTERNAL;
    }
    sum->initial_cost = S.initial_cost;
    sum->final_cost = S.final_cost;
    sum->num_successful_steps = S.n_succ;
    sum->num_unsuccessful_steps = S.n_unsucc;
    sum->num_iterations = S.iter;
    sum->termination_type = S.termination;
    ctx->last_iter = S.iter;
    format_message(S, sum->message, sizeof(sum->message));
    if (o.minimizer_progress_to_stdout) {
        std::vector<double> lg((size_t)LOG_W * (S.iter + 1));
        HIPCHECK(ctx, hipMemcpy(lg.data(), W.log, sizeof(double) * lg.size(), hipMemcpyDeviceToHost));
        print_header();
        for (int it = 0; it <= S.iter; ++it) {
            const double* r = &lg[(size_t)it * LOG_W];
            print_row(it, r[0], r[1], r[2], r[3], r[4], r[5], 0.0, 0.0);
        }
    }
    // copy the best (= last accepted) parameters back in place: cameras + intrinsics by DMA into pinned
    // staging (no host-side staging round trip per copy), the points straight into the caller's buffer
    const int cur = S.cur;
    const size_t ncd = 7 * (size_t)p->n_cams;
    HIPCHECK(ctx, ctx->hres.ensure(sizeof(double) * (ncd + 4)));
    double* hres = ctx->hres.as<double>();
    if (ncd) HIPCHECK(ctx, hipMemcpyAsync(hres, P.cams[cur], sizeof(double) * ncd, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(hres + ncd, P.K[cur], sizeof(double) * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(p->points, P.pts[cur] + 3 * (size_t)ctx->gather_off, sizeof(double) * 3 * (size_t)p->n_points,
                                 hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipStreamSynchronize(s));
    if (ncd) std::memcpy(p->cams, hres, sizeof(double) * ncd);
    std::memcpy(p->intr, hres + ncd, sizeof(double) * 4);
    const double t1 = now_ms();
    sum->time_lm_ms = t1 - tl0;
    sum->time_total_ms = t1 - t0;
    if (retries)  // informational (rc stays BA_OK): ba_last_error() says why the context left the resident kernel
        ctx->err = std::to_string(retries) + " LM iteration(s) re-run with the per-level BCR launches after an "
                   "inter-workgroup hand-off of the resident BCR kernel timed out; the context keeps the per-level "
                   "launches from now on.";
    auto dk = [&](int k) { return ctx->k_ms[k] - kms0[k]; };
    sum->time_linearize_ms = dk(K_CAM_SIDE) + dk(K_LIN_FINALIZE) + dk(K_POINT_COLNORM) + dk(K_SCALE);
    sum->time_schur_ms = dk(K_MEMSET_S) + dk(K_ASSEMBLE) + dk(K_POINT_PREP) + dk(K_SCHUR_TILE) + dk(K_OBS_PAIRS);
    sum->time_factor_ms = dk(K_CHOL) + dk(K_BCR_ELIM) + dk(K_BCR_CONTRIB) + dk(K_BCR_BACK) + dk(K_BCR_BORDER) +
                          dk(K_DENSE_COPY) + dk(K_DENSE_DIAG) + dk(K_DENSE_PANEL) + dk(K_DENSE_TRAIL) + dk(K_DENSE_BACK);
    sum->time_update_ms = dk(K_UPDATE_CAMS) + dk(K_BACKSUB_EVAL) + dk(K_FINAL) + dk(K_DECIDE);
    return BA_OK;
}

extern "C" int32_t ba_kernel_stats(const ba_context* ctx, ba_kernel_stat* out, int32_t max_n) {
    if (!ctx || !out) return 0;
    int n = 0;
    for (int k = 0; k < K_COUNT && n < max_n; ++k, ++n) {
        std::memset(&out[n], 0, sizeof(ba_kernel_stat));
        // the resident BCR id times whichever resident kernel the window runs: name it after that kernel
        const char* nm = (k == K_BCR_PERSIST && ctx->W.bcr.band) ? "bcr_band"
                         : (k == K_BCR_PERSIST && ctx->W.bcr.dense1) ? "bcr_dense1"
                         : (k == K_BCR_PERSIST && ctx->W.bcr.persist >= 2) ? "bcr_split" : kKernelNames[k];
        std::snprintf(out[n].name, sizeof(out[n].name), "%s", nm);
        out[n].launches = ctx->k_launches[k];
        out[n].total_ms = ctx->k_ms[k];
        out[n].bytes_per_launch = ctx->k_bytes[k];
        out[n].flops_per_launch = ctx->k_flops[k];
    }
    return n;
}

extern "C" void ba_reset_kernel_stats(ba_context* ctx) {
    if (!ctx) return;
    for (int k = 0; k < K_COUNT; ++k) { ctx->k_launches[k] = 0; ctx->k_ms[k] = 0; }
}

