// ba_pg.h — ba_pose_graph's device side (ba_pg.hip, internal): the records the host builds and the launchers of the
// kernels of one LM iteration. The reduced solve between them is launch_dense (ba_dense.h), unchanged.
// (The kernels here have no ids in the Prof table: tests/golden/prepare_golden.json pins ba_kernel_stats at its 30
// entries. Under profile_kernels the reduced solve's launches are recorded under their own ids as ever.)
#pragma once
#include <hip/hip_runtime.h>

#include "ba_kernels.h"

namespace miba {

// Per-edge linearisation record, written by k_pg_lin at the poses of slot `cur`:
//   [0, 21)  J_a^T J_a upper-packed (i <= j: q = 6 i - i (i - 1) / 2 + (j - i))   [21, 42)  J_b^T J_b likewise
//   [42, 78) J_a^T J_b row-major (row: a's dof)   [78, 84) J_a^T f   [84, 90) J_b^T f   [90] the edge's cost
//   [91]     1 when the evaluation is not finite
static constexpr int PG_EREC = 92;
// Per-active-pose gather record (position order): H_ii upper-packed (21) | g_i (6) | gradient max-norm of the pose
static constexpr int PG_PREC = 28;
// per-edge / per-pose step partials: edges (candidate cost, model cost change, bad), poses (|step|^2, |x_cand|^2, bad)
static constexpr int PG_EPART = 3, PG_PPART = 3;
static constexpr int PG_TPB = 256;

// one incident edge of a pose: the edge and whether the pose is its b end
struct PgInc { int edge, is_b; };
// one edge of an off-diagonal block: the edge and whether the block's row pose is its b end (the block is then the
// transpose of the record's J_a^T J_b)
struct PgPairEdge { int edge, row_is_b; };

struct PgArgs {
    // the graph (device copies)
    double* cams[2];          // [7 n_cams] x and candidate (ping-pong on LmState::cur); constant poses equal in both
    const int* edge_a;        // [n_edges]
    const int* edge_b;
    const double* meas;       // [7 n_edges]
    const double* weight;     // [2 n_edges] (filled with 1 when the caller gave none)
    const int* cam_pos;       // [n_cams]: position of an active pose among the unknowns, -1 for a constant one
    const int* pos_cam;       // [n_active]
    const int* inc_ptr;       // [n_active + 1] CSR of a pose's incident edges, the caller's edge order inside a pose
    const PgInc* inc;
    const int* pair_ptr;      // [n_pairs + 1] CSR of the coupled unordered pairs of active poses
    const int2* pair_rc;      // [n_pairs] (row position, column position), row > column
    const PgPairEdge* pair_edge;
    int n_cams, n_edges, n_active, n_pairs, npad;
    double huber_a, huber_b;  // a and b = a^2; a = 0: the trivial loss
    double min_diag, max_diag;
    // work
    double* erec;   // [PG_EREC n_edges]
    double* prec;   // [PG_PREC n_active]
    double* scale;  // [6 n_active]
    double* delta;  // [6 n_active]
    double* epart;  // [PG_EPART n_edges]
    double* ppart;  // [PG_PPART n_active]
    double* S;      // [npad^2]
    double* rhs;    // [npad]: s g in, y out
    int* chol_flag;
    LmState* st;
    double* log;    // [(max_iter + 2) LOG_W]
};

// the residual record at slot st->cur (first: also the Jacobi scaling, iteration 0), then the poses' gather
hipError_t launch_pg_linearize(const PgArgs& a, int first, int jacobi, hipStream_t s);
// the iteration-0 state: costs, gradient norm, |x|^2, log row 0 (one workgroup)
hipError_t launch_pg_init(const PgArgs& a, hipStream_t s);
// S (lower triangle, scaled and damped at the state's radius) and rhs from the gather records
hipError_t launch_pg_assemble(const PgArgs& a, hipStream_t s);
// the candidate poses from y, the candidate's cost and the model cost change per edge
hipError_t launch_pg_step(const PgArgs& a, hipStream_t s);
// the fixed-order reductions and the trust-region decision (one workgroup, one deciding thread)
hipError_t launch_pg_decide(const PgArgs& a, const LmParams& prm, hipStream_t s);
// every edge's cost at slot st->cur into out[n_edges]
hipError_t launch_pg_edge_cost(const PgArgs& a, double* out, hipStream_t s);

}  // namespace miba
