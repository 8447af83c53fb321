// The arithmetic of PnPsolver (reference src/PnPsolver.cc; Tracking::Relocalization runs it at src/Tracking.cc:2004-2030): the constructor's per-correspondence values
// (:67-110), SetRansacParameters (:121-157), the control flow of iterate (:165-258), Refine (:260-305), CheckInliers (:308-339) and EPnP (:375-950).  No HIP in here:
// csrc/pnp.hip compiles this text for the device and tests/sim/pnp_sim.cpp for the host with a plain compiler, both without contraction (-ffp-contract=off), so that the two
// produce the same bits.  Only + - * / and sqrt are used on the device.
//
// Reference-owned arithmetic is restated operation for operation with its types and evaluation order: CheckInliers (the double sums are narrowed to float Xc, Yc, invZc;
// ue / ve are double; distX / distY and error2 are float; fu fv uc vc are doubles made from the frame's floats), choose_control_points' sums, the barycentric
// coordinates (1.0f - a[1] - a[2] - a[3]), fill_M, compute_L_6x10 (2.0f * dot), compute_rho, the sign rules of find_betas_approx_1 / 2 / 3, gauss_newton (five steps),
// qr_solve literally (its first loop never looks at the last row; its singular exit leaves x as it was -- the reference never initialises x, here it starts as zeros),
// compute_ccs / compute_pcs / solve_for_sign / estimate_R_and_t (the det < 0 flip) / reprojection_error, and N = 1, 2, 3 by strict <.
// What the reference leaves to OpenCV is decision D17:
//   mult     cvMulTransposed(A, dst, 1) = A^T A: every entry is the sum over A's rows in row order, starting from +0.0, each product in double.
//   symsvd   cvSVD of the symmetric 3 x 3 and 12 x 12 (CV_SVD_U_T): cyclic Jacobi in double, PNP_SWEEPS sweeps over (p, q), p < q, in row-major order, D15's rotation.
//            Singular value = |diagonal entry|; descending, the lower column first among exactly equal ones; the vector is the Jacobi column as the rotations left it
//            (the product starts from I; no sign normalisation).
//   svd      cvSVD of ABt, cvInvert(.., CV_SVD) and cvSolve(.., CV_SVD): one-sided (Hestenes) Jacobi on the columns of A, PNP_SWEEPS sweeps over the same (p, q) order, the
//            rotation of D15 with app = a_p.a_p, aqq = a_q.a_q, apq = a_p.a_q (dot products over the rows in order); it leaves A' = U S and V.  s2_k = a'_k.a'_k, s_k = sqrt.
//            A column is kept when s_k > 2 DBL_EPSILON (s_0 + s_1 + ..), the truncation rule of OpenCV's back substitution.  Sums over k run in column order over kept columns:
//            pinv[r][c] = sum_k (V[r][k] * A'[c][k]) / s2_k;      x[r] = sum_k V[r][k] * ((sum_i A'[i][k] * b[i]) / s2_k).
//            For ABt: u_k = a'_k / s_k, but the column with the smallest s_k (the highest k among equals) is the cross product of the other two in cyclic order, negated
//            when it points against a'_k: a rank-2 ABt still gets an orthonormal U, and det(U V^T) < 0 reaches the reference's flip.  R = sum_k u_k v_k^T in column order.
//   table    SetRansacParameters' log / pow / ceil are libm's, evaluated on the host (ransac_params below is host code) for every N the kernel can meet.
// For a minimal set of four points M is 8 x 12 and MtM has a null space of dimension >= 4: the basis of it that symsvd returns is D17's, not the reference's; only the pose
// that the four betas recover from it is comparable.
//
// The draw: DUtils::Random::RandomInt is rand(); here draw_set<4> of ransac_draw.h.  A set with an index outside [0, N) or past the caller's sets is walked, never
// qualifies (count -1, a zero pose).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "ransac_draw.h"

namespace sslam {
namespace pnp {

using sslam::draw_set;      // :188-201 for one iteration over n >= 4 correspondences: set is an int[4]

constexpr int PNP_SWEEPS = 10;      // D17: two more than JACOBI_SWEEPS gives the 9 x 9 of D15: the 12 x 12 has 66 pairs and, for a minimal set, a four-fold cluster at zero.  A count of its own, not tuned
constexpr int WS_DOUBLES = 78 + 144;      // the upper triangle of the symmetric 12 x 12 and its eigenvectors; everything smaller is laid over them
// offsets into the working storage once the 12 x 12 is solved: the four null vectors (12 each), rho, L_6x10, and the area of the small solvers
constexpr int WS_NULL = 0, WS_RHO = 48, WS_L = 78, WS_S = 138;

struct Cam { double fu, fv, uc, vc; };
struct Row { float X[3], u, v, maxErr; };      // mvP3Dw, mvP2D, mvMaxError of one correspondence.  24 bytes
struct Pose { double R[9], t[3]; };            // mRi (row-major), mti
struct Trace { int N, flags; double rep[3], betas[3][4]; };      // the chosen N, what the solve reached (REACH_*), rep_errors[1 .. 3], Betas[1 .. 3] after gauss_newton
// branches a solve went through, for the tests: the flip of :618, the sign change of :638, the negative b4[0] of :683, a singular value of CC at or below D17's threshold
constexpr int REACH_DET = 1, REACH_PCS = 2, REACH_B4 = 4, REACH_CC = 8;

RANSAC_FN float max_error(float sigma2, float th2) { return sigma2 * th2; }      // :156

// :314-337 for one correspondence
RANSAC_FN bool check_row(const Pose& P, const Cam& K, const Row& r) {
    const float Xc = (float)(P.R[0] * r.X[0] + P.R[1] * r.X[1] + P.R[2] * r.X[2] + P.t[0]);
    const float Yc = (float)(P.R[3] * r.X[0] + P.R[4] * r.X[1] + P.R[5] * r.X[2] + P.t[1]);
    const float invZc = (float)(1 / (P.R[6] * r.X[0] + P.R[7] * r.X[1] + P.R[8] * r.X[2] + P.t[2]));
    const double ue = K.uc + K.fu * Xc * invZc;
    const double ve = K.vc + K.fv * Yc * invZc;
    const float distX = (float)(r.u - ue);
    const float distY = (float)(r.v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < r.maxErr;
}

RANSAC_FN int sym_index(int n, int i, int j) {      // upper triangle of an n-wide symmetric matrix, any order of (i, j)
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo * n - lo * (lo - 1) / 2 + (hi - lo);
}
RANSAC_FN void jacobi_cs(double app, double aqq, double apq, double& c, double& s, double& t) {      // D15's rotation
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    t = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    c = 1.0 / __builtin_sqrt(t * t + 1.0);
    s = t * c;
}

// D17 symsvd: the symmetric N x N in w[0 ..) (upper triangle, sym_index), eigenvector columns to w[78 + i * N + j].  Fixed trip counts: NaNs pass through and end
template <int N, class W>
RANSAC_FN void jacobi_sym(W& w) {
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) w.at(78 + i * N + j) = i == j ? 1.0 : 0.0;
    RANSAC_NOUNROLL
    for (int sweep = 0; sweep < PNP_SWEEPS; ++sweep) {
        RANSAC_NOUNROLL
        for (int p = 0; p < N - 1; ++p) {
            RANSAC_NOUNROLL
            for (int q = p + 1; q < N; ++q) {
                const int ipq = sym_index(N, p, q), ipp = sym_index(N, p, p), iqq = sym_index(N, q, q);
                const double apq = w.at(ipq);
                if (apq == 0.0) continue;
                const double app = w.at(ipp), aqq = w.at(iqq);
                double c, s, t;
                jacobi_cs(app, aqq, apq, c, s, t);
                RANSAC_NOUNROLL
                for (int k = 0; k < N; ++k) {
                    if (k != p && k != q) {
                        const int ikp = sym_index(N, k, p), ikq = sym_index(N, k, q);
                        const double akp = w.at(ikp), akq = w.at(ikq);
                        w.at(ikp) = c * akp - s * akq;
                        w.at(ikq) = s * akp + c * akq;
                    }
                    const double vkp = w.at(78 + k * N + p), vkq = w.at(78 + k * N + q);
                    w.at(78 + k * N + p) = c * vkp - s * vkq;
                    w.at(78 + k * N + q) = s * vkp + c * vkq;
                }
                w.at(ipp) = app - t * apq;
                w.at(iqq) = aqq + t * apq;
                w.at(ipq) = 0.0;
            }
        }
    }
}
// the position of column i in D17's order of the singular values: how many columns come before it
template <int N, class W>
RANSAC_FN int sym_rank(W& w, int i) {
    const double di = __builtin_fabs(w.at(sym_index(N, i, i)));
    int r = 0;
    RANSAC_NOUNROLL
    for (int j = 0; j < N; ++j) {
        const double dj = __builtin_fabs(w.at(sym_index(N, j, j)));
        if (dj > di || (dj == di && j < i)) ++r;
    }
    return r;
}

// D17 svd: A (NR x NC, row-major) at w[WS_S ..), V (NC x NC) behind it
template <int NR, int NC, class W> RANSAC_FN double& os_a(W& w, int r, int c) { return w.at(WS_S + r * NC + c); }
template <int NR, int NC, class W> RANSAC_FN double& os_v(W& w, int r, int c) { return w.at(WS_S + NR * NC + r * NC + c); }
template <int NR, int NC, class W>
RANSAC_FN void jacobi_onesided(W& w) {
    for (int i = 0; i < NC; ++i) for (int j = 0; j < NC; ++j) os_v<NR, NC>(w, i, j) = i == j ? 1.0 : 0.0;
    RANSAC_NOUNROLL
    for (int sweep = 0; sweep < PNP_SWEEPS; ++sweep) {
        RANSAC_NOUNROLL
        for (int p = 0; p < NC - 1; ++p) {
            RANSAC_NOUNROLL
            for (int q = p + 1; q < NC; ++q) {
                double app = 0.0, aqq = 0.0, apq = 0.0;
                RANSAC_NOUNROLL
                for (int r = 0; r < NR; ++r) {
                    const double x = os_a<NR, NC>(w, r, p), y = os_a<NR, NC>(w, r, q);
                    app += x * x; aqq += y * y; apq += x * y;
                }
                if (apq == 0.0) continue;
                double c, s, t;
                jacobi_cs(app, aqq, apq, c, s, t);
                RANSAC_NOUNROLL
                for (int r = 0; r < NR; ++r) {
                    const double x = os_a<NR, NC>(w, r, p), y = os_a<NR, NC>(w, r, q);
                    os_a<NR, NC>(w, r, p) = c * x - s * y;
                    os_a<NR, NC>(w, r, q) = s * x + c * y;
                }
                RANSAC_NOUNROLL
                for (int r = 0; r < NC; ++r) {
                    const double x = os_v<NR, NC>(w, r, p), y = os_v<NR, NC>(w, r, q);
                    os_v<NR, NC>(w, r, p) = c * x - s * y;
                    os_v<NR, NC>(w, r, q) = s * x + c * y;
                }
            }
        }
    }
}
template <int NR, int NC, class W>
RANSAC_FN double os_s2(W& w, int k) {
    double s2 = 0.0;
    RANSAC_NOUNROLL
    for (int r = 0; r < NR; ++r) { const double x = os_a<NR, NC>(w, r, k); s2 += x * x; }
    return s2;
}
template <int NR, int NC, class W>
RANSAC_FN double os_threshold(W& w) {
    double sum = 0.0;
    RANSAC_NOUNROLL
    for (int k = 0; k < NC; ++k) sum += __builtin_sqrt(os_s2<NR, NC>(w, k));
    return 2.0 * 2.220446049250313e-16 * sum;
}
// cvSolve(A, b, x, CV_SVD): A is in place at os_a, b = rho at w[WS_RHO ..)
template <int NC, class W>
RANSAC_FN void solve_svd(W& w, double (&x)[NC]) {
    jacobi_onesided<6, NC>(w);
    const double thr = os_threshold<6, NC>(w);
    RANSAC_UNROLL
    for (int r = 0; r < NC; ++r) x[r] = 0.0;
    RANSAC_NOUNROLL
    for (int k = 0; k < NC; ++k) {
        const double s2 = os_s2<6, NC>(w, k);
        if (!(__builtin_sqrt(s2) > thr)) continue;
        double proj = 0.0;
        RANSAC_NOUNROLL
        for (int i = 0; i < 6; ++i) proj += os_a<6, NC>(w, i, k) * w.at(WS_RHO + i);
        proj = proj / s2;
        RANSAC_UNROLL
        for (int r = 0; r < NC; ++r) x[r] += os_v<6, NC>(w, r, k) * proj;
    }
}

// D17 svd of a general 3 x 3 at w[WS_S ..) (row-major): U and V (row-major, column k = vector k) with the weakest column of U made orthogonal to the other two
template <class W>
RANSAC_FN void svd3_uv(W& w, double (&U)[9], double (&V)[9]) {
    jacobi_onesided<3, 3>(w);
    double s[3];
    RANSAC_UNROLL
    for (int k = 0; k < 3; ++k) s[k] = __builtin_sqrt(os_s2<3, 3>(w, k));
    RANSAC_UNROLL
    for (int r = 0; r < 3; ++r) {
        RANSAC_UNROLL
        for (int k = 0; k < 3; ++k) { U[r * 3 + k] = os_a<3, 3>(w, r, k) / s[k]; V[r * 3 + k] = os_v<3, 3>(w, r, k); }
    }
    const int weak = (s[2] <= s[0] && s[2] <= s[1]) ? 2 : (s[1] <= s[0] ? 1 : 0);
    RANSAC_UNROLL
    for (int k = 0; k < 3; ++k) if (k == weak) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        double c[3] = {U[3 + i] * U[6 + j] - U[6 + i] * U[3 + j], U[6 + i] * U[j] - U[i] * U[6 + j], U[i] * U[3 + j] - U[3 + i] * U[j]};
        const double along = c[0] * os_a<3, 3>(w, 0, k) + c[1] * os_a<3, 3>(w, 1, k) + c[2] * os_a<3, 3>(w, 2, k);
        if (along < 0.0) { c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2]; }
        U[k] = c[0]; U[3 + k] = c[1]; U[6 + k] = c[2];
    }
}
// D17 svd, cvInvert(.., CV_SVD) of the 3 x 3 at w[WS_S ..): the pseudo-inverse (row-major); returns whether a column was dropped
template <class W>
RANSAC_FN bool pinv3(W& w, double (&ci)[9]) {
    jacobi_onesided<3, 3>(w);
    const double thr = os_threshold<3, 3>(w);
    bool dropped = false;
    RANSAC_UNROLL
    for (int k = 0; k < 9; ++k) ci[k] = 0.0;
    RANSAC_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double s2 = os_s2<3, 3>(w, k);
        if (__builtin_sqrt(s2) > thr) {
            RANSAC_UNROLL
            for (int r = 0; r < 3; ++r) {
                RANSAC_UNROLL
                for (int c = 0; c < 3; ++c) ci[r * 3 + c] += (os_v<3, 3>(w, r, k) * os_a<3, 3>(w, c, k)) / s2;
            }
        } else {
            dropped = true;
        }
    }
    return dropped;
}

// :423-432 for one point
RANSAC_FN void alphas_of(const double ci[9], const double c0[3], const double pw[3], double a[4]) {
    RANSAC_UNROLL
    for (int j = 0; j < 3; ++j) a[1 + j] = ci[3 * j] * (pw[0] - c0[0]) + ci[3 * j + 1] * (pw[1] - c0[1]) + ci[3 * j + 2] * (pw[2] - c0[2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
}
RANSAC_FN void pw_of(const Row& r, double pw[3]) { pw[0] = r.X[0]; pw[1] = r.X[1]; pw[2] = r.X[2]; }      // add_correspondence, :363-373
RANSAC_FN double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
RANSAC_FN double dist2(const double* a, const double* b) { return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]); }

// qr_solve (:860-950) on the 6 x 4 A at w[WS_S ..), b behind it, then A1, A2, X
constexpr int QR_B = WS_S + 24, QR_A1 = QR_B + 6, QR_A2 = QR_A1 + 4, QR_X = QR_A2 + 4;
template <class W>
RANSAC_FN void qr_solve(W& w) {
    const int nr = 6, nc = 4;
    int kk = WS_S;
    RANSAC_NOUNROLL
    for (int k = 0; k < nc; ++k) {
        int ik = kk;
        double eta = __builtin_fabs(w.at(ik));
        RANSAC_NOUNROLL
        for (int i = k + 1; i < nr; ++i) {
            const double elt = __builtin_fabs(w.at(ik));
            if (eta < elt) eta = elt;
            ik += nc;
        }
        if (eta == 0) {
            w.at(QR_A1 + k) = 0.0; w.at(QR_A2 + k) = 0.0;
            return;
        }
        ik = kk;
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        RANSAC_NOUNROLL
        for (int i = k; i < nr; ++i) {
            const double e = w.at(ik) * inv_eta;
            w.at(ik) = e;
            sum += e * e;
            ik += nc;
        }
        double sigma = __builtin_sqrt(sum);
        if (w.at(kk) < 0) sigma = -sigma;
        const double akk = w.at(kk) + sigma;
        w.at(kk) = akk;
        const double a1 = sigma * akk;
        w.at(QR_A1 + k) = a1;
        w.at(QR_A2 + k) = -eta * sigma;
        RANSAC_NOUNROLL
        for (int j = k + 1; j < nc; ++j) {
            ik = kk;
            double sm = 0;
            RANSAC_NOUNROLL
            for (int i = k; i < nr; ++i) { sm += w.at(ik) * w.at(ik + j - k); ik += nc; }
            const double tau = sm / a1;
            ik = kk;
            RANSAC_NOUNROLL
            for (int i = k; i < nr; ++i) { w.at(ik + j - k) -= tau * w.at(ik); ik += nc; }
        }
        kk += nc + 1;
    }
    // b <- Qt b
    int jj = WS_S;
    RANSAC_NOUNROLL
    for (int j = 0; j < nc; ++j) {
        int ij = jj;
        double tau = 0;
        RANSAC_NOUNROLL
        for (int i = j; i < nr; ++i) { tau += w.at(ij) * w.at(QR_B + i); ij += nc; }
        tau /= w.at(QR_A1 + j);
        ij = jj;
        RANSAC_NOUNROLL
        for (int i = j; i < nr; ++i) { w.at(QR_B + i) -= tau * w.at(ij); ij += nc; }
        jj += nc + 1;
    }
    // X = R-1 b
    w.at(QR_X + nc - 1) = w.at(QR_B + nc - 1) / w.at(QR_A2 + nc - 1);
    RANSAC_NOUNROLL
    for (int i = nc - 2; i >= 0; --i) {
        int ij = WS_S + i * nc + (i + 1);
        double sum = 0;
        RANSAC_NOUNROLL
        for (int j = i + 1; j < nc; ++j) { sum += w.at(ij) * w.at(QR_X + j); ++ij; }
        w.at(QR_X + i) = (w.at(QR_B + i) - sum) / w.at(QR_A2 + i);
    }
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838)
template <class W>
RANSAC_FN void gauss_newton(W& w, double (&betas)[4]) {
    RANSAC_UNROLL
    for (int i = 0; i < 4; ++i) w.at(QR_X + i) = 0.0;
    RANSAC_NOUNROLL
    for (int k = 0; k < 5; ++k) {
        RANSAC_NOUNROLL
        for (int i = 0; i < 6; ++i) {
            double L[10];
            RANSAC_UNROLL
            for (int c = 0; c < 10; ++c) L[c] = w.at(WS_L + i * 10 + c);
            w.at(WS_S + i * 4 + 0) = 2 * L[0] * betas[0] + L[1] * betas[1] + L[3] * betas[2] + L[6] * betas[3];
            w.at(WS_S + i * 4 + 1) = L[1] * betas[0] + 2 * L[2] * betas[1] + L[4] * betas[2] + L[7] * betas[3];
            w.at(WS_S + i * 4 + 2) = L[3] * betas[0] + L[4] * betas[1] + 2 * L[5] * betas[2] + L[8] * betas[3];
            w.at(WS_S + i * 4 + 3) = L[6] * betas[0] + L[7] * betas[1] + L[8] * betas[2] + 2 * L[9] * betas[3];
            w.at(QR_B + i) = w.at(WS_RHO + i) -
                (L[0] * betas[0] * betas[0] + L[1] * betas[0] * betas[1] + L[2] * betas[1] * betas[1] + L[3] * betas[0] * betas[2] + L[4] * betas[1] * betas[2] +
                 L[5] * betas[2] * betas[2] + L[6] * betas[0] * betas[3] + L[7] * betas[1] * betas[3] + L[8] * betas[2] * betas[3] + L[9] * betas[3] * betas[3]);
        }
        qr_solve(w);
        RANSAC_UNROLL
        for (int i = 0; i < 4; ++i) betas[i] += w.at(QR_X + i);
    }
}

// L_6x10 columns `cols` into the solver's A
template <int NC, class W>
RANSAC_FN void fill_L(W& w, const int (&cols)[NC]) {
    RANSAC_NOUNROLL
    for (int i = 0; i < 6; ++i) {
        RANSAC_UNROLL
        for (int c = 0; c < NC; ++c) os_a<6, NC>(w, i, c) = w.at(WS_L + i * 10 + cols[c]);
    }
}
template <class W>
RANSAC_FN void find_betas_approx_1(W& w, double (&betas)[4], int& flags) {      // :667-694
    const int cols[4] = {0, 1, 3, 6};
    double b4[4];
    fill_L<4>(w, cols);
    solve_svd<4>(w, b4);
    if (b4[0] < 0) {
        flags |= REACH_B4;
        betas[0] = __builtin_sqrt(-b4[0]);
        betas[1] = -b4[1] / betas[0];
        betas[2] = -b4[2] / betas[0];
        betas[3] = -b4[3] / betas[0];
    } else {
        betas[0] = __builtin_sqrt(b4[0]);
        betas[1] = b4[1] / betas[0];
        betas[2] = b4[2] / betas[0];
        betas[3] = b4[3] / betas[0];
    }
}
template <class W>
RANSAC_FN void find_betas_approx_2(W& w, double (&betas)[4]) {      // :699-726
    const int cols[3] = {0, 1, 2};
    double b3[3];
    fill_L<3>(w, cols);
    solve_svd<3>(w, b3);
    if (b3[0] < 0) {
        betas[0] = __builtin_sqrt(-b3[0]);
        betas[1] = (b3[2] < 0) ? __builtin_sqrt(-b3[2]) : 0.0;
    } else {
        betas[0] = __builtin_sqrt(b3[0]);
        betas[1] = (b3[2] > 0) ? __builtin_sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) betas[0] = -betas[0];
    betas[2] = 0.0;
    betas[3] = 0.0;
}
template <class W>
RANSAC_FN void find_betas_approx_3(W& w, double (&betas)[4]) {      // :731-758
    const int cols[5] = {0, 1, 2, 3, 4};
    double b5[5];
    fill_L<5>(w, cols);
    solve_svd<5>(w, b5);
    if (b5[0] < 0) {
        betas[0] = __builtin_sqrt(-b5[0]);
        betas[1] = (b5[2] < 0) ? __builtin_sqrt(-b5[2]) : 0.0;
    } else {
        betas[0] = __builtin_sqrt(b5[0]);
        betas[1] = (b5[2] > 0) ? __builtin_sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) betas[0] = -betas[0];
    betas[2] = b5[3] / betas[0];
    betas[3] = 0.0;
}

// what the passes over the points need of choose_control_points and compute_barycentric_coordinates
struct Basis { double cws[4][3], ci[9]; };

// compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error.  pws / alphas / pcs are recomputed per point from the rows
template <class Pts, class W>
RANSAC_FN double compute_R_and_t(const Pts& pts, const Cam& K, const Basis& B, W& w, const double (&betas)[4], double (&R)[9], double (&t)[3], int& flags) {
    const int n = pts.n;
    double ccs[4][3];
    RANSAC_UNROLL
    for (int i = 0; i < 4; ++i) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0f;
    RANSAC_UNROLL
    for (int i = 0; i < 4; ++i) {
        RANSAC_UNROLL
        for (int j = 0; j < 4; ++j) {
            RANSAC_UNROLL
            for (int k = 0; k < 3; ++k) ccs[j][k] += betas[i] * w.at(WS_NULL + i * 12 + 3 * j + k);
        }
    }
    auto pc_of = [&](const Row& r, double pw[3], double pc[3]) {
        double a[4];
        pw_of(r, pw);
        alphas_of(B.ci, B.cws[0], pw, a);
        RANSAC_UNROLL
        for (int j = 0; j < 3; ++j) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
    };
    {   // solve_for_sign (:636-649): the negated ccs give exactly the negated pcs
        double pw[3], pc[3];
        pc_of(pts.first(), pw, pc);
        if (pc[2] < 0.0) {
            flags |= REACH_PCS;
            RANSAC_UNROLL
            for (int i = 0; i < 4; ++i) {
                RANSAC_UNROLL
                for (int j = 0; j < 3; ++j) ccs[i][j] = -ccs[i][j];
            }
        }
    }
    // estimate_R_and_t (:569-627)
    double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};
    pts.each([&](const Row& r) {
        double pw[3], pc[3];
        pc_of(r, pw, pc);
        RANSAC_UNROLL
        for (int j = 0; j < 3; ++j) { pc0[j] += pc[j]; pw0[j] += pw[j]; }
    });
    RANSAC_UNROLL
    for (int j = 0; j < 3; ++j) { pc0[j] /= n; pw0[j] /= n; }
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    pts.each([&](const Row& r) {
        double pw[3], pc[3];
        pc_of(r, pw, pc);
        RANSAC_UNROLL
        for (int j = 0; j < 3; ++j) {
            abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
            abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
            abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
        }
    });
    // D17 svd of ABt
    RANSAC_UNROLL
    for (int k = 0; k < 9; ++k) w.at(WS_S + k) = abt[k];
    double U[9], V[9];
    svd3_uv(w, U, V);
    RANSAC_UNROLL
    for (int i = 0; i < 3; ++i) {
        RANSAC_UNROLL
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = dot3(U + 3 * i, V + 3 * j);
    }
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; flags |= REACH_DET; }
    t[0] = pc0[0] - dot3(R, pw0);
    t[1] = pc0[1] - dot3(R + 3, pw0);
    t[2] = pc0[2] - dot3(R + 6, pw0);
    // reprojection_error (:550-567)
    double sum2 = 0.0;
    pts.each([&](const Row& r) {
        double pw[3];
        pw_of(r, pw);
        const double Xc = dot3(R, pw) + t[0];
        const double Yc = dot3(R + 3, pw) + t[1];
        const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
        const double ue = K.uc + K.fu * Xc * inv_Zc;
        const double ve = K.vc + K.fv * Yc * inv_Zc;
        const double u = r.u, v = r.v;
        sum2 += __builtin_sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    });
    return sum2 / n;
}

// compute_pose (:477-525) over pts: pts.n points, pts.each(f) calls f(row) in list order, pts.first() is the first row.  w: WS_DOUBLES doubles behind w.at(k)
template <class Pts, class W>
RANSAC_FN void compute_pose(const Pts& pts, const Cam& K, W& w, Pose& out, Trace& tr) {
    const int n = pts.n;
    Basis B;
    tr.flags = 0;
    // choose_control_points (:375-409)
    B.cws[0][0] = B.cws[0][1] = B.cws[0][2] = 0;
    pts.each([&](const Row& r) {
        double pw[3];
        pw_of(r, pw);
        RANSAC_UNROLL
        for (int j = 0; j < 3; ++j) B.cws[0][j] += pw[j];
    });
    RANSAC_UNROLL
    for (int j = 0; j < 3; ++j) B.cws[0][j] /= n;
    {
        double m[6] = {0, 0, 0, 0, 0, 0};      // D17 mult: PW0^T PW0, (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        pts.each([&](const Row& r) {
            double pw[3];
            pw_of(r, pw);
            const double d0 = pw[0] - B.cws[0][0], d1 = pw[1] - B.cws[0][1], d2 = pw[2] - B.cws[0][2];
            m[0] += d0 * d0; m[1] += d0 * d1; m[2] += d0 * d2; m[3] += d1 * d1; m[4] += d1 * d2; m[5] += d2 * d2;
        });
        RANSAC_UNROLL
        for (int k = 0; k < 6; ++k) w.at(k) = m[k];
        jacobi_sym<3>(w);
        int col[3] = {0, 0, 0};
        RANSAC_UNROLL
        for (int i = 0; i < 3; ++i) {
            const int r = sym_rank<3>(w, i);
            if (r == 0) col[0] = i;
            if (r == 1) col[1] = i;
            if (r == 2) col[2] = i;
        }
        RANSAC_UNROLL
        for (int i = 1; i < 4; ++i) {
            const int c = col[i - 1];
            const double k = __builtin_sqrt(__builtin_fabs(w.at(sym_index(3, c, c))) / n);
            RANSAC_UNROLL
            for (int j = 0; j < 3; ++j) B.cws[i][j] = B.cws[0][j] + k * w.at(78 + j * 3 + c);
        }
    }
    // compute_barycentric_coordinates (:411-421): D17 svd, the pseudo-inverse of CC
    {
        RANSAC_UNROLL
        for (int i = 0; i < 3; ++i) {
            RANSAC_UNROLL
            for (int j = 1; j < 4; ++j) os_a<3, 3>(w, i, j - 1) = B.cws[j][i] - B.cws[0][i];
        }
        if (pinv3(w, B.ci)) tr.flags |= REACH_CC;
    }
    // fill_M (:436-451) and D17 mult: MtM, rows 2i and 2i + 1 parked behind the triangle
    for (int k = 0; k < 78; ++k) w.at(k) = 0.0;
    pts.each([&](const Row& r) {
        double pw[3], a[4];
        pw_of(r, pw);
        alphas_of(B.ci, B.cws[0], pw, a);
        const double u = r.u, v = r.v;
        RANSAC_UNROLL
        for (int i = 0; i < 4; ++i) {
            w.at(78 + 3 * i) = a[i] * K.fu;
            w.at(78 + 3 * i + 1) = 0.0;
            w.at(78 + 3 * i + 2) = a[i] * (K.uc - u);
            w.at(90 + 3 * i) = 0.0;
            w.at(90 + 3 * i + 1) = a[i] * K.fv;
            w.at(90 + 3 * i + 2) = a[i] * (K.vc - v);
        }
        int idx = 0;
        RANSAC_NOUNROLL
        for (int i = 0; i < 12; ++i) {
            const double m1 = w.at(78 + i), m2 = w.at(90 + i);
            RANSAC_NOUNROLL
            for (int j = i; j < 12; ++j, ++idx) {
                double acc = w.at(idx);
                acc += m1 * w.at(78 + j);
                acc += m2 * w.at(90 + j);
                w.at(idx) = acc;
            }
        }
    });
    jacobi_sym<12>(w);
    {   // ut rows 11, 10, 9, 8: the four smallest singular values, the smallest first
        int col[4] = {0, 0, 0, 0};
        RANSAC_NOUNROLL
        for (int i = 0; i < 12; ++i) {
            const int r = sym_rank<12>(w, i);
            if (r == 11) col[0] = i;
            if (r == 10) col[1] = i;
            if (r == 9) col[2] = i;
            if (r == 8) col[3] = i;
        }
        RANSAC_UNROLL
        for (int m = 0; m < 4; ++m) {
            RANSAC_NOUNROLL
            for (int k = 0; k < 12; ++k) w.at(WS_NULL + m * 12 + k) = w.at(78 + k * 12 + col[m]);
        }
    }
    // compute_L_6x10 (:760-800)
    {
        int a = 0, b = 1;
        RANSAC_NOUNROLL
        for (int j = 0; j < 6; ++j) {
            double dv[4][3];
            RANSAC_UNROLL
            for (int i = 0; i < 4; ++i) {
                RANSAC_UNROLL
                for (int c = 0; c < 3; ++c) dv[i][c] = w.at(WS_NULL + i * 12 + 3 * a + c) - w.at(WS_NULL + i * 12 + 3 * b + c);
            }
            b++;
            if (b > 3) { a++; b = a + 1; }
            const int row = WS_L + 10 * j;
            w.at(row + 0) = dot3(dv[0], dv[0]);
            w.at(row + 1) = 2.0f * dot3(dv[0], dv[1]);
            w.at(row + 2) = dot3(dv[1], dv[1]);
            w.at(row + 3) = 2.0f * dot3(dv[0], dv[2]);
            w.at(row + 4) = 2.0f * dot3(dv[1], dv[2]);
            w.at(row + 5) = dot3(dv[2], dv[2]);
            w.at(row + 6) = 2.0f * dot3(dv[0], dv[3]);
            w.at(row + 7) = 2.0f * dot3(dv[1], dv[3]);
            w.at(row + 8) = 2.0f * dot3(dv[2], dv[3]);
            w.at(row + 9) = dot3(dv[3], dv[3]);
        }
    }
    // compute_rho (:802-810)
    w.at(WS_RHO + 0) = dist2(B.cws[0], B.cws[1]);
    w.at(WS_RHO + 1) = dist2(B.cws[0], B.cws[2]);
    w.at(WS_RHO + 2) = dist2(B.cws[0], B.cws[3]);
    w.at(WS_RHO + 3) = dist2(B.cws[1], B.cws[2]);
    w.at(WS_RHO + 4) = dist2(B.cws[1], B.cws[3]);
    w.at(WS_RHO + 5) = dist2(B.cws[2], B.cws[3]);

    double betas[4], R[9], t[3];
    find_betas_approx_1(w, betas, tr.flags);
    gauss_newton(w, betas);
    tr.rep[0] = compute_R_and_t(pts, K, B, w, betas, out.R, out.t, tr.flags);
    RANSAC_UNROLL
    for (int i = 0; i < 4; ++i) tr.betas[0][i] = betas[i];
    tr.N = 1;
    double best = tr.rep[0];

    find_betas_approx_2(w, betas);
    gauss_newton(w, betas);
    tr.rep[1] = compute_R_and_t(pts, K, B, w, betas, R, t, tr.flags);
    RANSAC_UNROLL
    for (int i = 0; i < 4; ++i) tr.betas[1][i] = betas[i];
    if (tr.rep[1] < best) {
        tr.N = 2; best = tr.rep[1];
        RANSAC_UNROLL
        for (int k = 0; k < 9; ++k) out.R[k] = R[k];
        RANSAC_UNROLL
        for (int k = 0; k < 3; ++k) out.t[k] = t[k];
    }

    find_betas_approx_3(w, betas);
    gauss_newton(w, betas);
    tr.rep[2] = compute_R_and_t(pts, K, B, w, betas, R, t, tr.flags);
    RANSAC_UNROLL
    for (int i = 0; i < 4; ++i) tr.betas[2][i] = betas[i];
    if (tr.rep[2] < best) {
        tr.N = 3;
        RANSAC_UNROLL
        for (int k = 0; k < 9; ++k) out.R[k] = R[k];
        RANSAC_UNROLL
        for (int k = 0; k < 3; ++k) out.t[k] = t[k];
    }
}

// the four points of a minimal set (:191-201)
struct SetPts {
    Row r[4];
    int n;
    template <class F> RANSAC_FN void each(F f) const { f(r[0]); f(r[1]); f(r[2]); f(r[3]); }
    RANSAC_FN Row first() const { return r[0]; }
};
// the rows whose bit is set in mask (64 rows a word), in list order: Refine's correspondences (:262-281)
template <class Rows, class Mask>
struct MaskedPts {
    Rows rows; Mask mask; int total, n;
    template <class F> RANSAC_FN void each(F f) const {
        RANSAC_NOUNROLL
        for (int w0 = 0; w0 < total; w0 += 64) {
            unsigned long long m = mask(w0 >> 6);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                f(rows(w0 + b));
            }
        }
    }
    RANSAC_FN Row first() const {
        for (int w0 = 0; w0 < total; w0 += 64) {
            const unsigned long long m = mask(w0 >> 6);
            if (m) return rows(w0 + __builtin_ctzll(m));
        }
        return Row{{0.f, 0.f, 0.f}, 0.f, 0.f, 0.f};
    }
};

RANSAC_FN void zero_pose(Pose& h) {
    for (int k = 0; k < 9; ++k) h.R[k] = 0.0;
    for (int k = 0; k < 3; ++k) h.t[k] = 0.0;
}
RANSAC_FN void zero_trace(Trace& tr) {
    tr.N = 0; tr.flags = 0;
    for (int k = 0; k < 3; ++k) { tr.rep[k] = 0.0; for (int i = 0; i < 4; ++i) tr.betas[k][i] = 0.0; }
}

// One iteration of :186-207 up to and including CheckInliers.  rows(i) = correspondence i of mvKeyPointIndices' order, n of them; set: four indices into it, valid = all in
// [0, n).  Returns mnInliersi; -1 with a zero pose for an invalid set.  mark(i, bIn) receives mvbInliersi
template <class Rows, class W, class Mark>
RANSAC_FN int hypothesis(const Rows& rows, int n, const Cam& K, const int set[4], bool valid, W& w, Pose& h, Trace& tr, Mark mark) {
    if (!valid) {
        zero_pose(h);
        zero_trace(tr);
        return -1;
    }
    SetPts P;
    P.n = 4;
    P.r[0] = rows(set[0]); P.r[1] = rows(set[1]); P.r[2] = rows(set[2]); P.r[3] = rows(set[3]);
    compute_pose(P, K, w, h, tr);
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const bool in = check_row(h, K, rows(i));
        mark(i, in);
        if (in) ++count;
    }
    return count;
}

// :129-152 for N correspondences, host only (libm): the adjusted mRansacMinInliers and mRansacMaxIts.  N below its own min_inliers: {that value, 0} -- iterate returns at
// :173 and (float)minInliers / N at N = 0 is never evaluated.  Where ceil's value is no int smaller than maxIterations the reference's conversion is undefined;
// mRansacMaxIts is maxIterations then, which is what every defined value that large gives.
inline void ransac_params(double probability, int minInliers, int maxIterations, float epsilon, int N, int32_t& minOut, int32_t& itsOut) {
    int nMinInliers = (int)(N * epsilon);
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < 4) nMinInliers = 4;
    minOut = nMinInliers;
    if (N < nMinInliers) { itsOut = 0; return; }
    if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
    if (nMinInliers == N) { itsOut = 1; return; }      // max(1, min(1, maxIterations))
    const double d = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
    if (!(d >= 0.0 && d < (double)maxIterations)) { itsOut = maxIterations > 1 ? maxIterations : 1; return; }
    const int nIterations = (int)d;
    const int m = nIterations < maxIterations ? nIterations : maxIterations;
    itsOut = m > 1 ? m : 1;
}

}  // namespace pnp
}  // namespace sslam
