// ba_pg.hip — ba_pose_graph's kernels (ba_pg.h): one LM iteration of a pose graph is
//
//   k_pg_lin       one thread per edge: residual, the two 6x6 Jacobians, the Huber corrector, and from them the
//                  edge's products J_a^T J_a, J_b^T J_b, J_a^T J_b, J_a^T f, J_b^T f and cost (the edge record)
//   k_pg_gather    one thread per active pose: H_ii and g_i as the sum of the pose's incident edge records in the
//                  caller's edge order (a host-built CSR), the pose's gradient max-norm, at iteration 0 the scaling
//   k_pg_assemble  six threads per active pose / per coupled pair: the scaled, damped diagonal block and s g; the
//                  off-diagonal block as the sum over the pair's edges in the caller's order, written once into the
//                  lower triangle of S; unit diagonal on the pad
//   launch_dense   (ba_dense.hip) y from S and s g
//   k_pg_step      one thread per active pose: delta = -s y, the candidate T exp(delta), |step|^2, |x_cand|^2
//   k_pg_cand      one thread per edge: the candidate's cost and the edge's share of the model cost change
//   k_pg_decide    one workgroup: the fixed-order sums of the per-edge / per-pose values (thread t takes t, t + 256,
//                  ..., then the DPP wave sum and the waves in order), one thread decides (lm_decide_local)
//
// A rejected step re-damps: only k_pg_assemble onwards run again. No floating-point atomics anywhere: every value of
// S, every sum and every partial has one writer and one order, so a call is bitwise reproducible.
// The residual is rounded by one sequence of operations (pg_residual, contraction off) shared by the linearisation
// and the candidate evaluation: the cost of an accepted candidate is bitwise the cost its linearisation reports.
#include "ba_pg.h"

#include "ba_common.h"

namespace miba {

namespace {

constexpr int PG_NW = PG_TPB / 64;
constexpr int E_HAA = 0, E_HBB = 21, E_HAB = 42, E_GA = 78, E_GB = 84, E_COST = 90, E_BAD = 91;
constexpr int P_G = 21, P_GMAX = 27;

__host__ __device__ constexpr int hq(int i, int j) { return 6 * i - (i * (i - 1)) / 2 + (j - i); }  // i <= j
// the structure of the Jacobians: J_a = [ -A I, * ; 0, * ], J_b = [ *, 0 ; 0, * ] in 3x3 blocks
__host__ __device__ constexpr bool nz_a(int row, int c) { return row < 3 ? (c >= 3 || row == c) : c >= 3; }
__host__ __device__ constexpr bool nz_b(int row, int c) { return (row < 3) == (c < 3); }

struct PgRes {
    double r[6];   // [w_t (t^ - t_meas) ; w_r 2 vec(dq)], not robustified
    double th[3];  // t^
    double dq[4];  // dq (x y z w), on the hemisphere w >= 0
    double Rh[9];  // R_a^T R_b, row-major
    double s;      // |r|^2
};

// The residual of edge (a, b) in one fixed sequence of operations.
__device__ __forceinline__ void pg_residual(const double* __restrict__ xa, const double* __restrict__ xb,
                                            const double* __restrict__ z, double wt, double wr, PgRes& o) {
#pragma clang fp contract(off)
    double Ra[9], Rb[9];
    quat_R(xa, Ra);
    quat_R(xb, Rb);
    const double d0 = xb[4] - xa[4], d1 = xb[5] - xa[5], d2 = xb[6] - xa[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.th[i] = __builtin_fma(Ra[6 + i], d2, __builtin_fma(Ra[3 + i], d1, Ra[i] * d0));
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o.Rh[3 * i + j] = __builtin_fma(Ra[6 + i], Rb[6 + j], __builtin_fma(Ra[3 + i], Rb[3 + j], Ra[i] * Rb[j]));
    }
    // q^ = conj(q_a) q_b
    const double ax = -xa[0], ay = -xa[1], az = -xa[2], aw = xa[3];
    const double bx = xb[0], by = xb[1], bz = xb[2], bw = xb[3];
    const double hw = ((aw * bw - ax * bx) - ay * by) - az * bz;
    const double hx = ((aw * bx + ax * bw) + ay * bz) - az * by;
    const double hy = ((aw * by - ax * bz) + ay * bw) + az * bx;
    const double hz = ((aw * bz + ax * by) - ay * bx) + az * bw;
    // dq = q_meas conj(q^)
    const double mx = z[0], my = z[1], mz = z[2], mw = z[3];
    const double cx = -hx, cy = -hy, cz = -hz, cw = hw;
    double ew = ((mw * cw - mx * cx) - my * cy) - mz * cz;
    double ex = ((mw * cx + mx * cw) + my * cz) - mz * cy;
    double ey = ((mw * cy - mx * cz) + my * cw) + mz * cx;
    double ez = ((mw * cz + mx * cy) - my * cx) + mz * cw;
    if (ew < 0.0) { ew = -ew; ex = -ex; ey = -ey; ez = -ez; }
    o.dq[0] = ex; o.dq[1] = ey; o.dq[2] = ez; o.dq[3] = ew;
    o.r[0] = wt * (o.th[0] - z[4]);
    o.r[1] = wt * (o.th[1] - z[5]);
    o.r[2] = wt * (o.th[2] - z[6]);
    o.r[3] = wr * (2.0 * ex);
    o.r[4] = wr * (2.0 * ey);
    o.r[5] = wr * (2.0 * ez);
    double s = o.r[0] * o.r[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) s = __builtin_fma(o.r[k], o.r[k], s);
    o.s = s;
}

// rho(s) and sqrt(rho'(s)) of the edge's loss (a = 0: trivial)
__device__ __forceinline__ void pg_loss(const PgArgs& a, double s, double& rho0, double& sq) {
    rho0 = s;
    sq = 1.0;
    if (a.huber_a > 0.0) huber(s, a.huber_a, a.huber_b, rho0, sq);
}

__device__ __forceinline__ void load7(const double* __restrict__ p, double x[7]) {
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = p[j];
}

// ---------------------------------------------------------------- linearisation
__global__ __launch_bounds__(PG_TPB) void k_pg_lin(PgArgs a) {
    const int e = blockIdx.x * PG_TPB + threadIdx.x;
    if (e >= a.n_edges) return;
    const int cur = a.st->cur;
    const int ca = a.edge_a[e], cb = a.edge_b[e];
    double xa[7], xb[7], z[7];
    load7(a.cams[cur] + 7 * (size_t)ca, xa);
    load7(a.cams[cur] + 7 * (size_t)cb, xb);
    load7(a.meas + 7 * (size_t)e, z);
    const double wt = a.weight[2 * e], wr = a.weight[2 * e + 1];
    PgRes R;
    pg_residual(xa, xb, z, wt, wr, R);
    double rho0, sq;
    pg_loss(a, R.s, rho0, sq);
    double* E = a.erec + (size_t)e * PG_EREC;
    const double cost = 0.5 * rho0;
    E[E_COST] = cost;
    E[E_BAD] = isfinite(cost) ? 0.0 : 1.0;
    double f[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = sq * R.r[k];
    // J_a = sq [ -w_t I, w_t [t^]x ; 0, w_r M ],  J_b = sq [ w_t R^, 0 ; 0, -w_r M R^ ],  M = dq.w I + [dq.v]x
    const double At = sq * wt, Ar = sq * wr;
    const double tx = R.th[0], ty = R.th[1], tz = R.th[2];
    const double vx = R.dq[0], vy = R.dq[1], vz = R.dq[2], vw = R.dq[3];
    const double M[9] = {vw, -vz, vy, vz, vw, -vx, -vy, vx, vw};
    const double Tx[9] = {0.0, -tz, ty, tz, 0.0, -tx, -ty, tx, 0.0};
    // the non-zero 3x3 blocks: Ja = [ -At I, Jat ; 0, Jar ], Jb = [ Jbt, 0 ; 0, Jbr ]
    double Jat[9], Jar[9], Jbt[9], Jbr[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Jat[3 * i + j] = At * Tx[3 * i + j];
            Jar[3 * i + j] = Ar * M[3 * i + j];
            Jbt[3 * i + j] = At * R.Rh[3 * i + j];
            Jbr[3 * i + j] = -Ar * (M[3 * i] * R.Rh[j] + M[3 * i + 1] * R.Rh[3 + j] + M[3 * i + 2] * R.Rh[6 + j]);
        }
    __builtin_amdgcn_sched_barrier(0);
    // entry (row, c) of J_a / J_b (translation rows 0..2, rotation rows 3..5); the structural zeros (nz_a / nz_b)
    // are left out of every product at compile time
    auto ja = [&](int row, int c) -> double {
        if (row < 3) return c < 3 ? -At : Jat[3 * row + (c - 3)];
        return Jar[3 * (row - 3) + (c - 3)];
    };
    auto jb = [&](int row, int c) -> double {
        if (row < 3) return Jbt[3 * row + c];
        return Jbr[3 * (row - 3) + (c - 3)];
    };
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double haa = 0.0, hbb = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                if (nz_a(r, i) && nz_a(r, j)) haa += ja(r, i) * ja(r, j);
                if (nz_b(r, i) && nz_b(r, j)) hbb += jb(r, i) * jb(r, j);
            }
            E[E_HAA + hq(i, j)] = haa;
            E[E_HBB + hq(i, j)] = hbb;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double hab = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
                if (nz_a(r, i) && nz_b(r, j)) hab += ja(r, i) * jb(r, j);
            E[E_HAB + 6 * i + j] = hab;
        }
        double ga = 0.0, gb = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (nz_a(r, i)) ga += ja(r, i) * f[r];
            if (nz_b(r, i)) gb += jb(r, i) * f[r];
        }
        E[E_GA + i] = ga;
        E[E_GB + i] = gb;
    }
}

__global__ __launch_bounds__(PG_TPB) void k_pg_gather(PgArgs a, int first, int jacobi) {
    const int i = blockIdx.x * PG_TPB + threadIdx.x;
    if (i >= a.n_active) return;
    double acc[27];
#pragma unroll
    for (int q = 0; q < 27; ++q) acc[q] = 0.0;
    for (int t = a.inc_ptr[i]; t < a.inc_ptr[i + 1]; ++t) {
        const PgInc in = a.inc[t];
        const double* E = a.erec + (size_t)in.edge * PG_EREC;
        const double* H = E + (in.is_b ? E_HBB : E_HAA);
        const double* g = E + (in.is_b ? E_GB : E_GA);
#pragma unroll
        for (int q = 0; q < 21; ++q) acc[q] += H[q];
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[P_G + k] += g[k];
    }
    double* P = a.prec + (size_t)i * PG_PREC;
#pragma unroll
    for (int q = 0; q < 27; ++q) P[q] = acc[q];
    // the pose's part of the gradient max-norm |x - Plus(x, -g)|_inf
    double x[7], ng[6], tp[7];
    load7(a.cams[a.st->cur] + 7 * (size_t)a.pos_cam[i], x);
#pragma unroll
    for (int k = 0; k < 6; ++k) ng[k] = -acc[P_G + k];
    se3_plus(x, ng, tp);
    double gm = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) gm = fmax(gm, fabs(x[j] - tp[j]));
    P[P_GMAX] = gm;
    if (first)
#pragma unroll
        for (int k = 0; k < 6; ++k) a.scale[6 * i + k] = jacobi ? 1.0 / (1.0 + sqrt(acc[hq(k, k)])) : 1.0;
}

// ---------------------------------------------------------------- the fixed-order sums of the one deciding workgroup
// thread t takes the entries t, t + PG_TPB, ... of a strided array, then the block sum (DPP inside a wave, the waves
// in order); out[] valid for every thread afterwards
template <int NV>
__device__ __forceinline__ void pg_sum(const double* __restrict__ base, int n, int stride, const int (&off)[NV],
                                       double* lds, double* out) {
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += PG_TPB)
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += base[(size_t)i * stride + off[k]];
    block_sum_nw<PG_NW, NV>(acc, lds, out);
}
__device__ __forceinline__ double pg_max(const double* __restrict__ base, int n, int stride, int off, double* lds) {
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += PG_TPB) m = fmax(m, base[(size_t)i * stride + off]);
    return block_max_nw<PG_NW>(m, lds);
}

__global__ __launch_bounds__(PG_TPB) void k_pg_init(PgArgs a) {
    __shared__ double lds[PG_NW * 4];
    __shared__ double out[4];
    const int lin_off[2] = {E_COST, E_BAD};
    pg_sum<2>(a.erec, a.n_edges, PG_EREC, lin_off, lds, out);
    const double cost = out[0], bad = out[1];
    __syncthreads();
    const double gmax = pg_max(a.prec, a.n_active, PG_PREC, P_GMAX, lds);
    double xn[1] = {0.0};
    const double* x = a.cams[0];
    for (int i = threadIdx.x; i < a.n_active; i += PG_TPB) {
        const double* p = x + 7 * (size_t)a.pos_cam[i];
#pragma unroll
        for (int j = 0; j < 7; ++j) xn[0] += p[j] * p[j];
    }
    block_sum_nw<PG_NW, 1>(xn, lds, out);
    if (threadIdx.x != 0) return;
    LmState S = *a.st;
    S.need_lin = 0;
    S.xnorm2 = out[0];
    S.gmax_ci = gmax;
    if (bad > 0.0 || !isfinite(cost)) {  // "Residual and Jacobian evaluation failed."
        S.x_cost = S.initial_cost = S.final_cost = __builtin_nan("");
        S.done = 1; S.termination = 2; S.msg = MSG_EVAL_FAIL;
    } else {
        S.x_cost = S.initial_cost = S.final_cost = cost;
        double* r = a.log;
        r[0] = cost; r[1] = 0.0; r[2] = gmax; r[3] = 0.0; r[4] = 0.0; r[5] = S.radius; r[6] = 1.0; r[7] = 0.0;
    }
    *a.st = S;
}

// ---------------------------------------------------------------- assembly
__global__ __launch_bounds__(PG_TPB) void k_pg_assemble(PgArgs a) {
    if (skip_step(a.st)) return;
    const int t = blockIdx.x * PG_TPB + threadIdx.x;
    const int n_items = a.n_active + a.n_pairs;
    const int item = t / 6, u = t - 6 * item;
    const size_t ld = (size_t)a.npad;
    if (item >= n_items) {  // the pad: unit diagonal, zero right-hand side
        const int r = 6 * a.n_active + (t - 6 * n_items);
        if (r < a.npad) {
            a.S[(size_t)r * ld + r] = 1.0;
            a.rhs[r] = 0.0;
        }
        return;
    }
    if (item < a.n_active) {
        const int i = item;
        const double radius = a.st->radius;
        const double* P = a.prec + (size_t)i * PG_PREC;
        const double su = a.scale[6 * i + u];
        double* row = a.S + (size_t)(6 * i + u) * ld + 6 * i;
        for (int v = 0; v <= u; ++v) {
            double h = su * P[hq(v, u)] * a.scale[6 * i + v];
            if (v == u) h = h + fmin(fmax(h, a.min_diag), a.max_diag) / radius;
            row[v] = h;
        }
        a.rhs[6 * i + u] = su * P[P_G + u];
        return;
    }
    const int p = item - a.n_active;
    const int2 rc = a.pair_rc[p];
    const double su = a.scale[6 * rc.x + u];
    double* row = a.S + (size_t)(6 * rc.x + u) * ld + 6 * rc.y;
    const int k0 = a.pair_ptr[p], k1 = a.pair_ptr[p + 1];
    for (int v = 0; v < 6; ++v) {
        double h = 0.0;
        for (int k = k0; k < k1; ++k) {
            const PgPairEdge pe = a.pair_edge[k];
            h += a.erec[(size_t)pe.edge * PG_EREC + E_HAB + (pe.row_is_b ? 6 * v + u : 6 * u + v)];
        }
        row[v] = su * h * a.scale[6 * rc.y + v];
    }
}

// ---------------------------------------------------------------- step
__global__ __launch_bounds__(PG_TPB) void k_pg_step(PgArgs a) {
    if (skip_step(a.st) || (*a.chol_flag & FLAG_NOT_PD)) return;
    const int i = blockIdx.x * PG_TPB + threadIdx.x;
    if (i >= a.n_active) return;
    const int cur = a.st->cur, c = a.pos_cam[i];
    double x[7], d[6], tp[7];
    load7(a.cams[cur] + 7 * (size_t)c, x);
    bool zero = true, bad = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        d[k] = -a.rhs[6 * i + k] * a.scale[6 * i + k];
        a.delta[6 * i + k] = d[k];
        zero = zero && d[k] == 0.0;
        bad = bad || !isfinite(d[k]);
    }
    se3_plus(x, d, tp);
    double sn2 = 0.0, xn2 = 0.0;
    double* xc = a.cams[cur ^ 1] + 7 * (size_t)c;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        // a zero step leaves the pose as it is, bitwise (the retraction would renormalise the quaternion)
        const double v = zero ? x[j] : tp[j];
        xc[j] = v;
        const double df = x[j] - v;
        sn2 += df * df;
        xn2 += v * v;
    }
    double* P = a.ppart + (size_t)i * PG_PPART;
    P[0] = sn2; P[1] = xn2; P[2] = bad ? 1.0 : 0.0;
}

// delta of a pose (zero for a constant one)
__device__ __forceinline__ void pg_delta(const PgArgs& a, int cam, double d[6]) {
    const int pos = a.cam_pos[cam];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = pos >= 0 ? a.delta[6 * pos + k] : 0.0;
}

__global__ __launch_bounds__(PG_TPB) void k_pg_cand(PgArgs a) {
    if (skip_step(a.st) || (*a.chol_flag & FLAG_NOT_PD)) return;
    const int e = blockIdx.x * PG_TPB + threadIdx.x;
    if (e >= a.n_edges) return;
    const int nxt = a.st->cur ^ 1;
    const int ca = a.edge_a[e], cb = a.edge_b[e];
    double xa[7], xb[7], z[7];
    load7(a.cams[nxt] + 7 * (size_t)ca, xa);
    load7(a.cams[nxt] + 7 * (size_t)cb, xb);
    load7(a.meas + 7 * (size_t)e, z);
    PgRes R;
    pg_residual(xa, xb, z, a.weight[2 * e], a.weight[2 * e + 1], R);
    double rho0, sq;
    pg_loss(a, R.s, rho0, sq);
    const double cost = 0.5 * rho0;
    // the edge's share of -(delta^T g + delta^T H delta / 2), from its record at x
    const double* E = a.erec + (size_t)e * PG_EREC;
    double da[6], db[6];
    pg_delta(a, ca, da);
    pg_delta(a, cb, db);
    double dg = 0.0, dHd = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double ha = 0.0, hb = 0.0, hab = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            ha += E[E_HAA + (i <= j ? hq(i, j) : hq(j, i))] * da[j];
            hb += E[E_HBB + (i <= j ? hq(i, j) : hq(j, i))] * db[j];
            hab += E[E_HAB + 6 * i + j] * db[j];
        }
        dHd += da[i] * ha + db[i] * hb + 2.0 * (da[i] * hab);
        dg += da[i] * E[E_GA + i] + db[i] * E[E_GB + i];
    }
    double* P = a.epart + (size_t)e * PG_EPART;
    P[0] = cost;
    P[1] = -(dg + 0.5 * dHd);
    P[2] = isfinite(cost) ? 0.0 : 1.0;
}

// ---------------------------------------------------------------- decision
__global__ __launch_bounds__(PG_TPB) void k_pg_decide(PgArgs a, LmParams prm) {
    __shared__ double lds[PG_NW * 4];
    __shared__ double es[4], ps[4], ls[4];
    const int e_off[3] = {0, 1, 2};
    pg_sum<3>(a.epart, a.n_edges, PG_EPART, e_off, lds, es);
    pg_sum<3>(a.ppart, a.n_active, PG_PPART, e_off, lds, ps);
    const int lin_off[2] = {E_COST, E_BAD};
    pg_sum<2>(a.erec, a.n_edges, PG_EREC, lin_off, lds, ls);
    const double gmax = pg_max(a.prec, a.n_active, PG_PREC, P_GMAX, lds);
    if (threadIdx.x != 0) return;
    LmState S = *a.st;
    if (S.done) return;
    const int flag = *a.chol_flag;
    *a.chol_flag = 0;
    double scal[SC_N];
    scal[SC_MCC] = es[1];
    scal[SC_CAND] = es[0];
    scal[SC_SN2] = ps[0];
    scal[SC_GMAX_PT] = 0.0;
    // a pivot that is not positive or a step that is not finite: a linear-solver failure; a candidate that does
    // not evaluate: the worst cost
    scal[SC_BAD] = ((flag & FLAG_NOT_PD) || ps[2] > 0.0) ? 2.0 : (es[2] > 0.0 ? 1.0 : 0.0);
    scal[SC_XN2] = ps[1];
    scal[6] = scal[7] = 0.0;
    const double lin0 = ls[1] > 0.0 ? __builtin_nan("") : ls[0];
    lm_decide_local(S, prm, lin0, gmax, scal, a.log);
    S.n_decide += 1;
    S.stop_next = !S.done && S.iter >= prm.max_iter;
    *a.st = S;
}

__global__ __launch_bounds__(PG_TPB) void k_pg_edge_cost(PgArgs a, double* __restrict__ out) {
    const int e = blockIdx.x * PG_TPB + threadIdx.x;
    if (e >= a.n_edges) return;
    const int cur = a.st->cur;
    double xa[7], xb[7], z[7];
    load7(a.cams[cur] + 7 * (size_t)a.edge_a[e], xa);
    load7(a.cams[cur] + 7 * (size_t)a.edge_b[e], xb);
    load7(a.meas + 7 * (size_t)e, z);
    PgRes R;
    pg_residual(xa, xb, z, a.weight[2 * e], a.weight[2 * e + 1], R);
    double rho0, sq;
    pg_loss(a, R.s, rho0, sq);
    out[e] = 0.5 * rho0;
}

inline unsigned blocks(int n) { return (unsigned)((n + PG_TPB - 1) / PG_TPB); }

#define PGL(...)                                 \
    do {                                         \
        hipLaunchKernelGGL(__VA_ARGS__);         \
        const hipError_t e_ = hipGetLastError(); \
        if (e_ != hipSuccess) return e_;         \
    } while (0)

}  // namespace

hipError_t launch_pg_linearize(const PgArgs& a, int first, int jacobi, hipStream_t s) {
    if (a.n_edges > 0) PGL(k_pg_lin, dim3(blocks(a.n_edges)), dim3(PG_TPB), 0, s, a);
    if (a.n_active > 0) PGL(k_pg_gather, dim3(blocks(a.n_active)), dim3(PG_TPB), 0, s, a, first, jacobi);
    return hipSuccess;
}

hipError_t launch_pg_init(const PgArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_pg_init, dim3(1), dim3(PG_TPB), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pg_assemble(const PgArgs& a, hipStream_t s) {
    const int threads = 6 * (a.n_active + a.n_pairs) + (a.npad - 6 * a.n_active);
    PGL(k_pg_assemble, dim3(blocks(threads)), dim3(PG_TPB), 0, s, a);
    return hipSuccess;
}

hipError_t launch_pg_step(const PgArgs& a, hipStream_t s) {
    PGL(k_pg_step, dim3(blocks(a.n_active)), dim3(PG_TPB), 0, s, a);
    if (a.n_edges > 0) PGL(k_pg_cand, dim3(blocks(a.n_edges)), dim3(PG_TPB), 0, s, a);
    return hipSuccess;
}

hipError_t launch_pg_decide(const PgArgs& a, const LmParams& prm, hipStream_t s) {
    PGL(k_pg_decide, dim3(1), dim3(PG_TPB), 0, s, a, prm);
    return hipSuccess;
}

hipError_t launch_pg_edge_cost(const PgArgs& a, double* out, hipStream_t s) {
    if (a.n_edges <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pg_edge_cost, dim3(blocks(a.n_edges)), dim3(PG_TPB), 0, s, a, out);
    return hipGetLastError();
}

}  // namespace miba
