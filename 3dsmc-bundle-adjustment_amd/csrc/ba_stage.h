// ba_stage.h — the host scaffold of a stage beside the LM loop (internal): what ba_covariance, ba_residuals,
// ba_covisibility, ba_local_window / ba_solve_local, ba_localize, ba_refine_points, ba_pose_graph, ba_align, ba_match and
// ba_guided_match do
// before and after their own work. The sized out-structs, the common refusals in their fixed order, the verdict on the
// problem's sizes / buffers / indices, and the per-call helper (error texts under the entry point's name, device
// buffers, copies, events). (ba_localize and ba_refine_points share more than this: ba_block_stage.h.)
#pragma once
#include "ba_context.h"

// Sized out-structs (BA_API_VERSION 2): the caller's struct_size says how many bytes its struct has; write no more
// than that, keep its struct_size, and refuse a size below the version's minimum.
template <class T>
inline bool sized_out_ok(const T* out, int32_t min_size) {
    return out && out->struct_size >= min_size;
}
template <class T>
inline void sized_copy_out(T* out, const T& full) {
    const size_t n = std::min<size_t>((size_t)out->struct_size, sizeof(T));
    const int32_t keep = out->struct_size;
    std::memcpy(out, &full, n);
    out->struct_size = keep;
}

namespace miba {

// (also ba_solve_ordered's, which has no request / info to check before it)
constexpr const char* kStageShards = "contexts with landmark shards (ba_comm_init*) are not supported";
// ba_prepare's three verdicts on a problem, for the entry points that never prepare or check before they do
constexpr const char* kBadSizes = "invalid problem sizes";
constexpr const char* kNullBuffer = "null problem buffer";
constexpr const char* kBadIndex = "observation index out of range";

// The refusals every stage opens with, in this order: null argument, request struct_size, info struct_size, landmark
// shards. req_macro / info_macro are the stems of the header's macros (BA_COV_REQUEST -> BA_COV_REQUEST_MIN_SIZE,
// BA_COV_REQUEST_INIT); STAGE_SIZES(BA_COV) gives the four arguments. "" when the call may go on.
#define STAGE_SIZES(stem) stem##_REQUEST_MIN_SIZE, stem##_INFO_MIN_SIZE, #stem "_REQUEST", #stem "_INFO"
template <class Prob, class Req, class Info>
inline std::string stage_refusal(const ba_context* ctx, const Prob* p, const Req* req, const Info* info,
                                 int32_t req_min, int32_t info_min, const char* req_macro, const char* info_macro) {
    if (!p || !req || !info) return "null argument";
    auto below = [](const char* what, const char* macro) {
        return std::string(what) + " struct_size below " + macro + "_MIN_SIZE (set it with " + macro + "_INIT)";
    };
    if (req->struct_size < req_min) return below("request", req_macro);
    if (!sized_out_ok(info, info_min)) return below("info", info_macro);
    if (ctx->W.comm.on() || ctx->comm_parked.on()) return kStageShards;
    return "";
}

// Which of the problem's buffers a stage reads: the observations' camera / point indices and depths; the parameters
// (cameras, points, intrinsics and their prior) with the observations' pixels.
enum : unsigned { STAGE_OBS = 1u, STAGE_PARAMS = 2u };

inline bool stage_missing_buffer(const ba_problem* p, unsigned needs) {
    if ((needs & STAGE_PARAMS) && ((p->n_cams && !p->cams) || (p->n_points && !p->points) || !p->intr || !p->intr_prior ||
                                   (p->n_obs && !p->obs_uv)))
        return true;
    return (needs & STAGE_OBS) && p->n_obs && (!p->obs_cam || !p->obs_pt || !p->obs_depth);
}

// ba_prepare's verdict on the sizes and the buffers the stage reads, then on every observation's indices (the kernels
// index with them unchecked). "" when the problem is usable.
inline const char* stage_validate_problem(const ba_problem* p, unsigned needs) {
    if (p->n_cams < 0 || p->n_points < 0 || p->n_obs < 0) return kBadSizes;
    if (stage_missing_buffer(p, needs)) return kNullBuffer;
    for (int32_t k = 0; k < p->n_obs; ++k)
        if (p->obs_cam[k] < 0 || p->obs_cam[k] >= p->n_cams || p->obs_pt[k] < 0 || p->obs_pt[k] >= p->n_points)
            return kBadIndex;
    return "";
}

// One call of a stage: the context, the entry point's name (the prefix of its error texts) and the stream.
struct Stage {
    ba_context* ctx;
    const char* name;
    hipStream_t s;

    int32_t invalid(const std::string& msg) const {
        ctx->err = std::string(name) + ": " + msg;
        return BA_E_INVALID;
    }
    // a device buffer of the context at `bytes` or more, or BA_E_NOMEM with the size in the text
    int32_t ensure(BufId id, size_t bytes, const char* what) const {
        if (ctx->buf[id].ensure(bytes) == hipSuccess) return BA_OK;
        (void)hipGetLastError();
        ctx->err = std::string(name) + ": cannot allocate " + what + " (" + std::to_string(bytes) + " bytes)";
        return BA_E_NOMEM;
    }
    // copies on the stage's stream; a zero-length copy (an empty window, a NULL source) is not issued
    hipError_t h2d(void* dst, const void* src, size_t bytes) const {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    }
    hipError_t d2h(void* dst, const void* src, size_t bytes) const {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    }
    // the stage's own events, created by its first call on the context
    hipError_t events(hipEvent_t* ev, int n) const {
        for (int i = 0; i < n; ++i)
            if (!ev[i])
                if (hipError_t e = hipEventCreate(&ev[i]); e != hipSuccess) return e;
        return hipSuccess;
    }
};

}  // namespace miba
