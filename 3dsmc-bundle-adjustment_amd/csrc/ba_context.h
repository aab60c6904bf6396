// ba_context.h — the libmiba context and what its host translation units share (internal).
//
// ba_solver.cpp: the C-ABI core and the LM loop; ba_prepare.cpp: ba_prepare's phases (staging, plan, device
// structure, plan cache); ba_debug.cpp: the ba_debug_* entry points. The stages beside the LM loop, one file each on
// the scaffold of ba_stage.h: ba_cov.cpp (ba_covariance), ba_resid.cpp (ba_residuals), ba_covis.cpp (ba_covisibility,
// ba_solve_ordered), ba_local.cpp (ba_local_window, ba_solve_local), ba_loc.cpp (ba_localize), ba_pts.cpp (ba_refine_points),
// ba_pg.cpp (ba_pose_graph), ba_align.cpp (ba_align), ba_match.cpp (ba_match), ba_gmatch.cpp (ba_guided_match).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ba.h"
#include "ba_host.h"
#include "ba_kernels.h"
#include "ba_plan.h"
#include "ba_settings.h"

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(bytes, 256);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// Pinned host memory, grown on demand (an eighth of slack, at least min_cap bytes) and kept by the context.
// Growing keeps the first `keep` bytes; a mapped buffer is host-coherent and `dev` its device address. The caller
// makes sure that no DMA still reads the buffer before it asks for more than `cap`.
struct PinnedBuf {
    size_t min_cap = 0;
    bool mapped = false;
    void* p = nullptr;
    void* dev = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes, size_t keep = 0) {
        if (cap >= bytes) return hipSuccess;
        if (!keep) release();
        const size_t want = std::max(bytes + bytes / 8, min_cap);
        void* nb = nullptr;
        hipError_t e = hipHostMalloc(&nb, want, mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (p) std::memcpy(nb, p, std::min(keep, cap));
        release();
        p = nb;
        cap = want;
        return mapped ? hipHostGetDevicePointer(&dev, p, 0) : hipSuccess;
    }
    void release() {
        if (p) hipHostFree(p);
        p = dev = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

enum BufId {
    B_CAMS0, B_CAMS1, B_PTS0, B_PTS1, B_K0, B_K1, B_PRIOR,
    B_PO_CAM, B_PO_AC, B_PO_UV, B_PO_DEP, B_PO_AP, B_PO_PT,
    B_CO_PT, B_CO_UV, B_CO_DEP, B_RAW_CAM, B_RAW_PT, B_RAW_UV, B_RAW_DEP, B_PLAN,
    B_CAMDATA, B_SEGINTR, B_LIN, B_SCALE, B_CNP, B_PDATA, B_S, B_RHS, B_DELTA, B_PART, B_SCAL, B_FLAG,
    B_BCR, B_CAMDATA_LOC, B_ENV_LOC, B_RED, B_PREP, B_CAMPART, B_STATE, B_LOG, B_CAMS_INIT, B_PTS_INIT, B_K_INIT,
    B_DBG0, B_DBG1, B_DBG2, B_DBG3, B_DET_TBUF, B_PO_REC, B_CO_REC,
    B_RAW_ADM, B_DP_SCRATCH, B_DP_PO_DEST, B_DP_CO_DEST, B_DP_CAM_AC, B_DP_PT_IDX, B_DP_OVF, B_DP_SUM, B_TAIL_Y,
    // ba_covariance (allocated on its first call): the two dense work matrices, the points' W_o scratch, the
    // request's index lists + the status word, and the outputs
    B_COV_A, B_COV_Z, B_COV_W, B_COV_IDX, B_COV_OUT,
    // the blocked multi-workgroup Cholesky (BA_LS_BLOCKED): packed envelope blocks, diagonal inverses, padded rhs
    // and the block lists
    B_DENSE_A, B_DENSE_Z, B_DENSE_B, B_DENSE_IDX,
    // ba_residuals (allocated on its first call): the per-observation values in point-major slot order and in the
    // caller's order (errors | cost | flags each), the block statistics with their partials and the totals
    B_RES_PO, B_RES_OBS, B_RES_STAT,
    // ba_covisibility (allocated on its first call): its own copy of the observation indices and depths, the
    // camera x point bit matrix, the weights, and the cameras' positions with the points' spans and the two counts
    B_COVIS_OBS, B_COVIS_BITS, B_COVIS_W, B_COVIS_SPAN,
    // the constant cameras' mask for the device plan (ba_set_constant_cameras)
    B_DP_CONST,
    // ba_local_window (allocated on its first call): the integer scratch of the selection and its outputs
    B_LOCAL_WORK, B_LOCAL_OUT,
    // ba_localize (allocated on its first call): its own copy of the window (poses, points, intrinsics, observation
    // values), the grouped observation indices with the workgroups' records, and the statistics and log it writes
    B_LOC_IN, B_LOC_IDX, B_LOC_OUT,
    // ba_refine_points (allocated on its first call): its own copy of the window, the observation indices grouped by
    // point with the points' records, and the statistics, solved positions and log it writes
    B_PTS_IN, B_PTS_IDX, B_PTS_OUT,
    // ba_pose_graph (allocated on its first call): the graph's copy (poses twice, measurements, weights, endpoints),
    // the host-built structure (positions, incidence and pair lists), the records / partials / LM state / log, the
    // dense S, and the blocked Cholesky's own packed envelope, diagonal inverses, padded rhs and block lists
    B_PG_IN, B_PG_IDX, B_PG_WORK, B_PG_S, B_PG_DENSE_A, B_PG_DENSE_Z, B_PG_DENSE_B, B_PG_DENSE_IDX,
    // ba_align (allocated on its first call): its own copy of the correspondences with the pairs' offsets, and what it
    // writes (poses, statistics, the hypotheses' counts, the inlier mask)
    B_ALIGN_IN, B_ALIGN_OUT,
    // ba_match (allocated on its first call): its own copy of the descriptors with the pairs' ranges and offsets, the
    // slices' neighbour tables (the swapped launch's beside them), and what it writes
    B_MATCH_IN, B_MATCH_TOP, B_MATCH_OUT,
    // ba_guided_match (allocated on its first call): its own copy of the keypoints, landmarks, frames and candidates
    // with the host's layout, the binned keypoint grids with the one-to-one table, and what it writes
    B_GMATCH_IN, B_GMATCH_GRID, B_GMATCH_OUT,
    B_COUNT
};

struct ba_context {
    ba_options opts;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t cov_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // ba_covariance's own phase events (first call)
    hipEvent_t res_ev[2] = {nullptr, nullptr};  // ba_residuals' events around its kernels (first call)
    hipEvent_t covis_ev[2] = {nullptr, nullptr};  // ba_covisibility's events around its count kernels (first call)
    unsigned* hprog = nullptr;  // host-mapped LM progress word (LmParams::progress)
    unsigned* dprog = nullptr;  // its device address
    PinnedBuf hres;             // staging of the solved cameras + intrinsics (async device-to-host copies)
    DevBuf buf[B_COUNT];
    std::string err;
    // host-side structure of the last prepared problem (ba_plan.h; plan.po_orig: point-major admissible obs ->
    // original obs index)
    miba::Plan plan;
    std::vector<int> pt_idx, ac_cam;
    miba::DensePlan dplan;       // BA_LS_BLOCKED: the envelope at 64-block granularity, kept with the plan
    std::vector<int> dplan_idx;  // its device index buffer's host image (outlives the upload)
    PinnedBuf stage{1 << 20};    // staging of ba_prepare's uploads: [raw observations | plan index arrays]
    PinnedBuf pstage{1 << 16};   // staging of the parameter uploads (cameras | points | intrinsics | prior)
    hipStream_t copy_stream = nullptr;  // the device plan's pixel DMA, beside the plan passes on `stream`
    hipEvent_t ev_idx = nullptr, ev_uv = nullptr;  // indices / depths DMA'd; pixels DMA'd
    bool uv_pending = false;  // the pixel DMA of the last prepare has not been waited for on `stream`
    PinnedBuf rsum{256, true};  // the device plan's summary (ba_plan.h), mapped: the last pass writes it
    std::vector<std::pair<size_t, size_t>> plan_parts;  // (offset, ints) of each array in B_PLAN (PlanPart order)
    // plan cache (ba_options.rebuild_plan = 0): the structure key of the last full prepare; while plan_ok the
    // staging buffer's raw region holds that window's observations (the reuse check compares against it) and
    // `raw` the device gather inputs (B_RAW_* + the plan's orderings in B_PLAN)
    struct PlanKey {
        int nc = -1, np = -1, no = -1, fixed_cam = 0, det = 0, obs32 = 0;
        unsigned long long env = 0;  // Settings::key
        std::vector<uint8_t> cmask;  // the constant cameras in force (empty: none)
        bool operator==(const PlanKey& o) const {
            return nc == o.nc && np == o.np && no == o.no && fixed_cam == o.fixed_cam && det == o.det &&
                   env == o.env && cmask == o.cmask;
        }
    } key;
    // ba_set_constant_cameras: [n_cams] 0 / 1 as given (empty: none set); cmask_any: it has a member
    std::vector<uint8_t> cmask;
    bool cmask_any = false;
    bool plan_ok = false;
    miba::Settings st;  // the MIBA_* settings of the prepare under way (read at its start; the key's env part)
    miba::PrepRaw raw{};
    ba_prepare_info pinfo{};
    miba::DevProblem P{};
    miba::DevWork W{};
    miba::BaConsts C{};
    int nblk_pt = 0;
    bool prepared = false;
    int n_tiles = 0, n_ovf_obs = 0, n_tiled_pts = 0;
    int n_adm_all = 0;  // admissible observations over all landmark shards
    int sw_full = 0;    // DevWork::sw as the last full prepare chose it (a timeout re-run clears W.sw)
    int tail_full = 0;  // DevWork::tail likewise
    int bsfin_full = 0;  // DevWork::bsfin likewise
    bool tail_possible = false;  // the window's LM loop can take the band tail launch (set before bcr_setup)
    int prep_nc = -1, prep_np = -1, prep_no = -1;
    int last_iter = -1;        // iterations of the last solve (ba_iteration_log rows - 1)
    int dbg_step_base = -1;    // ba_debug_step's slot of x while the device still holds what that step left behind
    // shard_min_obs: a window below the threshold is gathered onto every rank and solved there alone; the
    // communicator is parked meanwhile (restored by the next prepare), the rank's points are the slice
    // [gather_off, gather_off + its n_points) of the gathered window
    miba::Comm comm_parked;
    int gather_off = 0;
    int dev_np = 0;  // points on the device (the gathered window's when gathered)
    struct Gathered {
        std::vector<double> cams, pts, uv, dep;
        std::vector<int> oc, op;
        double intr[4], prior[4];
    } gw;
    // ba_solve_ordered's shadow problem: the cameras as placed, the observations' camera indices remapped, and the
    // order it computes itself (order == NULL)
    struct Ordered {
        std::vector<double> cams;
        std::vector<int32_t> obs_cam, inv, order;
    } ordered;
    // ba_solve_local's shadow problem (the sub-window of the last call) and the selection's host outputs
    struct Local {
        std::vector<double> cams, pts, uv, dep;
        std::vector<int32_t> w, cam_index, pt_index, obs_index, obs_cam, obs_pt;
        std::vector<uint8_t> cam_constant, is_local;  // per sub-window camera: constant; a member of L
    } local;
    hipEvent_t local_ev[2] = {nullptr, nullptr};  // ba_local_window's events around its kernels (first call)
    hipEvent_t loc_ev[2] = {nullptr, nullptr};    // ba_localize's events around its kernel (first call)
    hipEvent_t pts_ev[2] = {nullptr, nullptr};    // ba_refine_points' events around its kernel (first call)
    hipEvent_t pg_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // ba_pose_graph's: an iteration, its reduced solve
    hipEvent_t align_ev[2] = {nullptr, nullptr};  // ba_align's events around its two kernels (first call)
    hipEvent_t match_ev[2] = {nullptr, nullptr};  // ba_match's events around its kernels (first call)
    hipEvent_t gmatch_ev[2] = {nullptr, nullptr};  // ba_guided_match's events around its kernels (first call)
    int match_cus = 0;  // the device's compute units, for ba_match's slice count (asked once, at its first call)
    bool bcr_fallback = false;  // a resident BCR kernel timed out: per-level launches from then on
    unsigned long long bcr_launches = 0;  // split-kernel launches since the BCR workspace was initialised
    int bcr_retries = 0;        // iterations re-run with the per-level launches after a hand-off timeout
    // per-kernel profiling
    miba::Prof prof;
    bool prof_events = false;
    int k_launches[miba::K_COUNT] = {0};
    double k_ms[miba::K_COUNT] = {0};
    double k_bytes[miba::K_COUNT] = {0};
    double k_flops[miba::K_COUNT] = {0};
    miba::Prof* pf() { return opts.profile_kernels ? &prof : nullptr; }
};

#define HIPCHECK(ctx, x)                                                                  \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            (ctx)->err = std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x; \
            return BA_E_DEVICE;                                                           \
        }                                                                                 \
    } while (0)

// The cost constants that come from the options alone: the Huber scales and the LM diagonal's clamp. (The weights
// sw_r / sw_d / sw_k depend on whose observations are counted: the window's in ba_prepare, a camera's or a point's own
// in ba_localize / ba_refine_points.)
inline void cost_consts(const ba_options& o, miba::BaConsts& C) {
    C.a_r = o.hub_p_repr; C.b_r = o.hub_p_repr * o.hub_p_repr;
    C.a_d = o.hub_p_unpr; C.b_d = o.hub_p_unpr * o.hub_p_unpr;
    C.min_diag = o.min_lm_diagonal; C.max_diag = o.max_lm_diagonal;
}

// ---- ba_prepare.cpp
// Uploads the window and builds (or reuses) its plan and device structure; the device work is left in flight.
int prepare(ba_context* ctx, const ba_problem* p);
// k_bcr_split's hand-off state as a prepare leaves it (also after 2^28 launches on one prepared window)
int bcr_init_handoffs(ba_context* ctx);

// ---- ba_solver.cpp: the enqueue code of an LM solve on the prepared window (ba_solve_prepared, ba_debug_step)
void flush_prof(ba_context* ctx);
int apply_spin_limit(ba_context* ctx);
miba::LmState fresh_state(const ba_options& o, double radius);
miba::LmParams lm_params(const ba_context* ctx);
// the termination text of a finished LM state (ba_summary.message)
void format_message(const miba::LmState& S, char* out, size_t n);
int enqueue_reset(ba_context* ctx, const miba::LmState& st0, int n_cams);
int enqueue_iteration_zero(ba_context* ctx);
int enqueue_iteration(ba_context* ctx, const miba::LmParams& prm);
int bcr_timeout_retry(ba_context* ctx, miba::LmState& S);
