// ba_align_fit.h — ba_align's model of a set of correspondences (include/ba.h, "Hypotheses"): the degeneracy test of a
// sample, Arun's fit by Horn's quaternion form with a fixed number of cyclic Jacobi sweeps, and the squared distance of
// a correspondence to a model. One text for both kernels of ba_align.hip (so the winner's model recomputed by
// k_align_pick is bitwise the one k_align_hyp scored) and for the host harness tests/cpp/align_sample_main.cpp.
// Everything is plain IEEE f64 with no contraction left to the compiler: the fit multiplies and adds separately, the
// distance states its fused multiply-adds itself, so tests/refalign.py's align64 can restate the fit operation by
// operation.
#pragma once
#include <cmath>

#include "ba_align_sample.h"

#define BA_ALIGN_FN BA_ALIGN_HD __attribute__((always_inline))
#if defined(__clang__)
#define BA_ALIGN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BA_ALIGN_NO_CONTRACT
#endif

namespace miba {

static constexpr int ALIGN_SWEEPS = 6;  // BA_ALIGN_SWEEPS: five leave 5e-21 of the diagonal off it on every test case

// p1 ~ R p2 + t, R row-major; q the unit quaternion of R as (x, y, z, w), w >= 0
struct AlignModel {
    double R[9];
    double t[3];
    double q[4];
};

BA_ALIGN_FN bool align_finite(double x) { return x - x == 0.0; }

// |(b - a) x (c - a)|^2
BA_ALIGN_FN double align_cross2(const double a[3], const double b[3], const double c[3]) {
    BA_ALIGN_NO_CONTRACT
    const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
    const double v0 = c[0] - a[0], v1 = c[1] - a[1], v2 = c[2] - a[2];
    const double x = u1 * v2 - u2 * v1, y = u2 * v0 - u0 * v2, z = u0 * v1 - u1 * v0;
    return (x * x + y * y) + z * z;
}

// one Jacobi rotation that clears A[P][Q] of the symmetric A, accumulated into the eigenvector matrix V
template <int P, int Q>
BA_ALIGN_FN void align_jacobi_rot(double (&A)[4][4], double (&V)[4][4]) {
    BA_ALIGN_NO_CONTRACT
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
    A[P][P] = A[P][P] - tt * apq;
    A[Q][Q] = A[Q][Q] + tt * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// R (det +1) maximising tr(R H) for H = sum (p2 - c2)(p1 - c1)^T (row-major: H[3 i + k] = sum a_i b_k, a of cloud 2,
// b of cloud 1), and t = c1 - R c2. Horn's N with the quaternion as (w, x, y, z); the eigenvector of the largest
// diagonal entry after the sweeps (the first among equals), normalised, w >= 0.
BA_ALIGN_FN void align_fit_H(const double H[9], const double c1[3], const double c2[3], AlignModel& m) {
    BA_ALIGN_NO_CONTRACT
    const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz;
    A[1][1] = (Sxx - Syy) - Szz;
    A[2][2] = (Syy - Sxx) - Szz;
    A[3][3] = (Szz - Sxx) - Syy;
    A[0][1] = A[1][0] = Syz - Szy;
    A[0][2] = A[2][0] = Szx - Sxz;
    A[0][3] = A[3][0] = Sxy - Syx;
    A[1][2] = A[2][1] = Sxy + Syx;
    A[1][3] = A[3][1] = Szx + Sxz;
    A[2][3] = A[3][2] = Syz + Szy;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ALIGN_SWEEPS; ++sweep) {
        align_jacobi_rot<0, 1>(A, V);
        align_jacobi_rot<0, 2>(A, V);
        align_jacobi_rot<0, 3>(A, V);
        align_jacobi_rot<1, 2>(A, V);
        align_jacobi_rot<1, 3>(A, V);
        align_jacobi_rot<2, 3>(A, V);
    }
    int k = 0;
    double best = A[0][0];
    if (A[1][1] > best) { best = A[1][1]; k = 1; }
    if (A[2][2] > best) { best = A[2][2]; k = 2; }
    if (A[3][3] > best) { best = A[3][3]; k = 3; }
    double q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = k == 0 ? V[r][0] : k == 1 ? V[r][1] : k == 2 ? V[r][2] : V[r][3];
    const double nrm = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double sg = q[0] < 0.0 ? -1.0 : 1.0;
    const double w = sg * q[0] / nrm, x = sg * q[1] / nrm, y = sg * q[2] / nrm, z = sg * q[3] / nrm;
    m.q[0] = x; m.q[1] = y; m.q[2] = z; m.q[3] = w;
    m.R[0] = 1.0 - 2.0 * (y * y + z * z);
    m.R[1] = 2.0 * (x * y - z * w);
    m.R[2] = 2.0 * (x * z + y * w);
    m.R[3] = 2.0 * (x * y + z * w);
    m.R[4] = 1.0 - 2.0 * (x * x + z * z);
    m.R[5] = 2.0 * (y * z - x * w);
    m.R[6] = 2.0 * (x * z - y * w);
    m.R[7] = 2.0 * (y * z + x * w);
    m.R[8] = 1.0 - 2.0 * (x * x + y * y);
    m.t[0] = c1[0] - ((m.R[0] * c2[0] + m.R[1] * c2[1]) + m.R[2] * c2[2]);
    m.t[1] = c1[1] - ((m.R[3] * c2[0] + m.R[4] * c2[1]) + m.R[5] * c2[2]);
    m.t[2] = c1[2] - ((m.R[6] * c2[0] + m.R[7] * c2[1]) + m.R[8] * c2[2]);
}

// The model of a minimal sample: a[i] / b[i] the i-th sample point in cloud 1 / cloud 2. False for a degenerate
// sample (a cross product at or below min_cross in either cloud, a coordinate that is not finite).
BA_ALIGN_FN bool align_fit3(const double a[3][3], const double b[3][3], double min_cross2, AlignModel& m) {
    BA_ALIGN_NO_CONTRACT
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) fin = fin && align_finite(a[i][k]) && align_finite(b[i][k]);
    if (!fin) return false;
    if (!(align_cross2(a[0], a[1], a[2]) > min_cross2) || !(align_cross2(b[0], b[1], b[2]) > min_cross2)) return false;
    double c1[3], c2[3], H[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c1[k] = ((a[0][k] + a[1][k]) + a[2][k]) / 3.0;
        c2[k] = ((b[0][k] + b[1][k]) + b[2][k]) / 3.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            H[3 * i + k] = ((b[0][i] - c2[i]) * (a[0][k] - c1[k]) + (b[1][i] - c2[i]) * (a[1][k] - c1[k])) +
                           (b[2][i] - c2[i]) * (a[2][k] - c1[k]);
    align_fit_H(H, c1, c2, m);
    return true;
}

BA_ALIGN_FN bool align_model_finite(const AlignModel& m) {
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && align_finite(m.R[i]);
    return fin && align_finite(m.t[0]) && align_finite(m.t[1]) && align_finite(m.t[2]);
}

// |p1 - (R p2 + t)|^2 with the fused multiply-adds stated: 15 operations. NaN or +inf for a correspondence with a
// coordinate that is not finite, which no threshold admits.
BA_ALIGN_FN double align_dist2(const AlignModel& m, double x1, double y1, double z1, double x2, double y2, double z2) {
    const double ex = x1 - fma(m.R[0], x2, fma(m.R[1], y2, fma(m.R[2], z2, m.t[0])));
    const double ey = y1 - fma(m.R[3], x2, fma(m.R[4], y2, fma(m.R[5], z2, m.t[1])));
    const double ez = z1 - fma(m.R[6], x2, fma(m.R[7], y2, fma(m.R[8], z2, m.t[2])));
    return fma(ex, ex, fma(ey, ey, ez * ez));
}

}  // namespace miba
