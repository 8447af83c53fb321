// The arithmetic of the second half of Initializer::Initialize (reference src/Initializer.cc:143-152): ReconstructF (:500-608) with DecomposeE (:964-984), ReconstructH
// (:611-781, the eight hypotheses of Faugeras), CheckRT (:833-961), Triangulate (:987-1000), LineTriangulate (:1003-1055), ReconstructLine (:1059-1171) and vector_mad
// (include/auxiliar.h:91-106).  No HIP in here: csrc/reconstruct.hip compiles this text for the device and tests/sim/reconstruct_sim.cpp for the host with a plain compiler,
// both without contraction (-ffp-contract=off), so that the two produce the same bits.  Only + - * / and sqrt in double and + - * / in float are used (a float sqrt is the
// double one rounded once more, which is the correctly rounded float sqrt); acos is restated below from the same operations.
//
// Reference-owned arithmetic is restated operation for operation with its types: the double comparisons nGood > 0.7 * maxGood, secondBestGood < 0.75 * bestGood and
// bestGood > 0.9 * N, static_cast<int>(0.9 * N), min(50, size - 1), im1Endy with fx (:1129), the line row that is not finite (error 0, zero endpoints, stays true and takes
// part in both MADs), ReconstructF trying only the FIRST hypothesis whose nGood equals maxGood.  What the reference leaves to OpenCV, Eigen or libm is decision D18:
//   svd3     cv::SVD::compute of a 3 x 3 (E of DecomposeE, A of ReconstructH): D17's one-sided Jacobi (pnp_math.h: svd3_uv, on the float entries widened to double), columns
//            ordered by descending singular value, the lower Jacobi column first among exactly equal ones; U, w and Vt are rounded once to float.
//   svd4     cv::SVD::compute of the 4 x 4 of Triangulate / LineTriangulate, of which only vt.row(3) is used: D15's solver (two_view_math.h: jacobi_smallest on A^T A, which is
//            accumulated in double from the float entries row after row), the eigenvector rounded once to float.
//   gemm     every float matrix product, 3 x 3 or not: D15's (each element accumulated in double from +0.0 in k order, rounded once); A * B * C is (A * B) * C; R * x + t is
//            the product rounded, then a float addition.  cv::determinant and Mat::inv of a 3 x 3: D15's cofactor forms in double.
//   scale    s * A, A / s, A *= s and x * A.row(): every element (float)((double)a * alpha) with alpha = s or 1.0 / s in double; -A negates.
//   norm     cv::norm and Mat::dot on CV_32F: products and the running sum in double, element order; norm is the double sqrt of that sum.  Eigen's Vector2d::norm():
//            sqrt(e0 * e0 + e1 * e1) in double.
//   acos     acos(float) at :955 is libm's acosf: here acos_f, the rational approximation of fdlibm's e_acos.c evaluated in double on the widened float and rounded once.
//   order    vCosParallax[min(50, size - 1)] and the medians of vector_mad are order statistics: kth_key selects by value on order-preserving integer keys.  A NaN makes the
//            reference's std::sort undefined; the keys order every NaN last (behind +inf).  -0.0f orders before +0.0f; acos of both is the same float.
#pragma once
#include <cstdint>
#include "pnp_math.h"
#include "two_view_math.h"

#define RC_FN RANSAC_FN
#define RC_UNROLL RANSAC_UNROLL

namespace sslam {
namespace rc {

constexpr int WS4_DOUBLES = 10 + 16;      // svd4: the upper triangle of the symmetric 4 x 4 and its eigenvectors (two_view_math.h's layout with LD = 4)
constexpr int WS3_DOUBLES = 18;           // svd3: A and V of pnp_math.h's one-sided Jacobi; W3::at(k) is addressed with k in [pnp::WS_S, pnp::WS_S + 18)
// CheckRT's exits for one match (:874, :885, :904, :911, :923, :934, :943)
constexpr int STAGE_NOT_INLIER = 0, STAGE_NOT_FINITE = 1, STAGE_Z1 = 2, STAGE_Z2 = 3, STAGE_ERR1 = 4, STAGE_ERR2 = 5, STAGE_GOOD = 6;
constexpr int REASON_OK = 0, REASON_SKIPPED = 1, REASON_NOT_SEPARATED = 2, REASON_NO_WINNER = 3, REASON_PARALLAX = 4;

struct Cam { float fx, fy, cx, cy; };                    // mK
struct Hyp { float R[9], t[3], P2[12], O2[3]; };         // one motion hypothesis: R, t, and CheckRT's P2 = K [R | t] (:860-864) and O2 = -R^T t (:867)

RC_FN void cam_matrix(const Cam& c, float K[9]) { K[0] = c.fx; K[1] = 0.f; K[2] = c.cx; K[3] = 0.f; K[4] = c.fy; K[5] = c.cy; K[6] = 0.f; K[7] = 0.f; K[8] = 1.f; }
RC_FN bool finite_f(float x) { return __builtin_fabsf(x) <= 3.4028234663852886e38f; }
RC_FN float sqrt_f(float x) { return (float)__builtin_sqrt((double)x); }

// D18 gemm: C (R x C) = A (R x K) * B (K x C), row-major
template <int R, int K, int C>
RC_FN void gemm(const float* A, const float* B, float* out) {
    RC_UNROLL
    for (int i = 0; i < R; ++i) {
        RC_UNROLL
        for (int j = 0; j < C; ++j) {
            double acc = 0.0;
            RC_UNROLL
            for (int k = 0; k < K; ++k) acc += (double)A[i * K + k] * (double)B[k * C + j];
            out[i * C + j] = (float)acc;
        }
    }
}
RC_FN double det3(const float m[9]) {      // D15's determinant (two_view_math.h: inv3)
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    return m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6) + m2 * (m3 * m7 - m4 * m6);
}
RC_FN double norm3(const float v[3]) { double s = 0.0; RC_UNROLL for (int i = 0; i < 3; ++i) s += (double)v[i] * (double)v[i]; return __builtin_sqrt(s); }
RC_FN float scale_f(float a, double alpha) { return (float)((double)a * alpha); }

// D18 acos: fdlibm's e_acos.c in double on a float argument, rounded once
RC_FN double acos_poly(double z) {
    const double p = z * (1.66666666666666657415e-01 + z * (-3.25565818622400915405e-01 + z * (2.01212532134862925881e-01 + z * (-4.00555345006794114027e-02 +
                     z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
    const double q = 1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)));
    return p / q;
}
RC_FN float acos_f(float xf) {
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const double x = (double)xf, ax = x < 0.0 ? -x : x;
    if (!(ax < 1.0)) {
        if (x == 1.0) return 0.f;
        if (x == -1.0) return (float)(pi + 2.0 * pio2_lo);
        return (float)((x - x) / (x - x));      // NaN
    }
    if (ax < 0.5) {
        if (ax < 6.938893903907228e-18) return (float)(pio2_hi + pio2_lo);      // 2^-57
        const double r = acos_poly(x * x);
        return (float)(pio2_hi - (x - (pio2_lo - x * r)));
    }
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5, s = __builtin_sqrt(z), r = acos_poly(z), w = r * s - pio2_lo;
        return (float)(pi - 2.0 * (s + w));
    }
    const double z = (1.0 - x) * 0.5, s = __builtin_sqrt(z);
    uint64_t u;
    __builtin_memcpy(&u, &s, 8);
    u &= 0xffffffff00000000ull;
    double df;
    __builtin_memcpy(&df, &u, 8);
    const double c = (z - df * df) / (s + df), r = acos_poly(z), w = r * s + c;
    return (float)(2.0 * (df + w));
}
// :955
RC_FN float parallax_of(float cosv) { return (float)((double)(acos_f(cosv) * 180.f) / 3.1415926535897932384626433832795); }

// D18 order: integer keys that order like the values, every NaN last; *_ABSENT is above every key of a value and marks an entry that is not in the list
constexpr uint32_t KEY32_NAN = 0xfffffffeu, KEY32_ABSENT = 0xffffffffu;
constexpr uint64_t KEY64_NAN = 0xfffffffffffffffeull, KEY64_ABSENT = 0xffffffffffffffffull;
RC_FN uint32_t key_of(float f) {
    if (f != f) return KEY32_NAN;
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RC_FN float value_of(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    if (k == KEY32_NAN) u = 0x7fc00000u;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
RC_FN uint64_t key_of(double f) {
    if (f != f) return KEY64_NAN;
    uint64_t u;
    __builtin_memcpy(&u, &f, 8);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
RC_FN double value_of(uint64_t k) {
    uint64_t u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    if (k == KEY64_NAN) u = 0x7ff8000000000000ull;
    double f;
    __builtin_memcpy(&f, &u, 8);
    return f;
}
// the k-th smallest key (k from 0) of a list with more than k entries: countBelow(t) = how many keys of the list are < t.  Built bit by bit from the top: the largest v with
// countBelow(v) <= k.  The device counts with ballots over LDS, the host with a loop.
template <class Key, class CountBelow>
RC_FN Key kth_key(int k, CountBelow countBelow) {
    Key v = 0;
    for (int bit = (int)(8 * sizeof(Key)) - 1; bit >= 0; --bit) {
        const Key t = v | ((Key)1 << bit);
        if (countBelow(t) <= k) v = t;
    }
    return v;
}

// D18 svd3: A = U diag(S) Vt, S descending.  w: WS3_DOUBLES doubles behind w.at(pnp::WS_S + k)
template <class W3>
RC_FN void svd3(W3& w, const float A[9], float U[9], float S[3], float Vt[9]) {
    RC_UNROLL
    for (int k = 0; k < 9; ++k) pnp::os_a<3, 3>(w, k / 3, k % 3) = (double)A[k];
    double Ud[9], Vd[9], s[3];
    pnp::svd3_uv(w, Ud, Vd);
    RC_UNROLL
    for (int k = 0; k < 3; ++k) s[k] = __builtin_sqrt(pnp::os_s2<3, 3>(w, k));
    int rank[3];
    RC_UNROLL
    for (int k = 0; k < 3; ++k) {
        rank[k] = 0;
        RC_UNROLL
        for (int j = 0; j < 3; ++j) if (s[j] > s[k] || (s[j] == s[k] && j < k)) ++rank[k];
    }
    // place j takes the column whose rank is j.  Written as selects over the three columns, never as a store at a computed place, so that the arrays stay in registers.
    // A singular value that is NaN ranks nowhere: ranks then repeat, the highest column of equal ranks holds the place and a place nobody takes is zero
    RC_UNROLL
    for (int j = 0; j < 3; ++j) {
        const bool t0 = rank[0] == j, t1 = rank[1] == j, t2 = rank[2] == j;
        S[j] = (float)(t2 ? s[2] : t1 ? s[1] : t0 ? s[0] : 0.0);
        RC_UNROLL
        for (int r = 0; r < 3; ++r) {
            U[r * 3 + j] = (float)(t2 ? Ud[r * 3 + 2] : t1 ? Ud[r * 3 + 1] : t0 ? Ud[r * 3] : 0.0);
            Vt[j * 3 + r] = (float)(t2 ? Vd[r * 3 + 2] : t1 ? Vd[r * 3 + 1] : t0 ? Vd[r * 3] : 0.0);
        }
    }
}

// D18 svd4: vt.row(3) of the 4 x 4 A (row-major).  w: WS4_DOUBLES doubles behind w.at(k)
template <class W>
RC_FN void svd4_last(W& w, const float A[16], float v[4]) {
    RC_UNROLL
    for (int i = 0; i < 4; ++i) {
        RC_UNROLL
        for (int j = i; j < 4; ++j) {
            double acc = 0.0;
            RC_UNROLL
            for (int r = 0; r < 4; ++r) acc += (double)A[r * 4 + i] * (double)A[r * 4 + j];
            tv::ws_a<4>(w, i, j) = acc;
        }
    }
    const int col = tv::jacobi_smallest<4, 4>(w);
    RC_UNROLL
    for (int k = 0; k < 4; ++k) v[k] = (float)tv::ws_v<4>(w, k, col);
}

// :850-867 for one hypothesis: P2 and O2 from R, t
RC_FN void hyp_setup(const Cam& c, Hyp& h) {
    float K[9], Rt[12], nRt[9];
    cam_matrix(c, K);
    RC_UNROLL
    for (int i = 0; i < 3; ++i) {
        RC_UNROLL
        for (int j = 0; j < 3; ++j) { Rt[i * 4 + j] = h.R[i * 3 + j]; nRt[i * 3 + j] = -h.R[j * 3 + i]; }
        Rt[i * 4 + 3] = h.t[i];
    }
    gemm<3, 3, 4>(K, Rt, h.P2);
    gemm<3, 3, 1>(nRt, h.t, h.O2);
}

// :872-943 for one match that is an inlier: Triangulate (:987-1000) and the checks.  p3d is defined from STAGE_NOT_FINITE on, cosv from STAGE_Z1 on (zeros before); err1 / err2
// are squareError1 / squareError2 once computed (zeros before): the host model's trace, which the kernel does not keep
struct RowOut { float p3d[3], cosv, err1, err2; int stage; };
template <class W>
RC_FN void check_row(const Cam& c, const Hyp& h, float u1, float v1, float u2, float v2, float th2, W& w, RowOut& o) {
    const float P1[12] = {c.fx, 0.f, c.cx, 0.f, 0.f, c.fy, c.cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    float A[16], v[4];
    RC_UNROLL
    for (int j = 0; j < 4; ++j) {
        A[j] = u1 * P1[8 + j] - P1[j];
        A[4 + j] = v1 * P1[8 + j] - P1[4 + j];
        A[8 + j] = u2 * h.P2[8 + j] - h.P2[j];
        A[12 + j] = v2 * h.P2[8 + j] - h.P2[4 + j];
    }
    svd4_last(w, A, v);
    const double alpha = 1.0 / (double)v[3];
    float p[3];
    RC_UNROLL
    for (int i = 0; i < 3; ++i) { p[i] = scale_f(v[i], alpha); o.p3d[i] = p[i]; }
    o.cosv = o.err1 = o.err2 = 0.f;
    if (!finite_f(p[0]) || !finite_f(p[1]) || !finite_f(p[2])) { o.stage = STAGE_NOT_FINITE; return; }
    const float n1[3] = {p[0] - 0.f, p[1] - 0.f, p[2] - 0.f};
    const float n2[3] = {p[0] - h.O2[0], p[1] - h.O2[1], p[2] - h.O2[2]};
    const float dist1 = (float)norm3(n1), dist2 = (float)norm3(n2);
    double dot = 0.0;
    RC_UNROLL
    for (int i = 0; i < 3; ++i) dot += (double)n1[i] * (double)n2[i];
    const float cosParallax = (float)(dot / (double)(dist1 * dist2));
    o.cosv = cosParallax;
    if (p[2] <= 0) { o.stage = STAGE_Z1; return; }
    float q[3];
    gemm<3, 3, 1>(h.R, p, q);
    RC_UNROLL
    for (int i = 0; i < 3; ++i) q[i] = q[i] + h.t[i];
    if (q[2] <= 0) { o.stage = STAGE_Z2; return; }
    const float invZ1 = (float)(1.0 / (double)p[2]);
    const float im1x = c.fx * p[0] * invZ1 + c.cx, im1y = c.fy * p[1] * invZ1 + c.cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    o.err1 = squareError1;
    if (squareError1 > th2) { o.stage = STAGE_ERR1; return; }
    const float invZ2 = (float)(1.0 / (double)q[2]);
    const float im2x = c.fx * q[0] * invZ2 + c.cx, im2y = c.fy * q[1] * invZ2 + c.cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    o.err2 = squareError2;
    if (squareError2 > th2) { o.stage = STAGE_ERR2; return; }
    o.stage = STAGE_GOOD;
}
RC_FN float th2_of(float sigma) { const float sigma2 = sigma * sigma; return (float)(4.0 * (double)sigma2); }      // :49, :527

// :512-520 and DecomposeE (:964-984): the four hypotheses (R1, t1), (R2, t1), (R1, t2), (R2, t2) in the order of :527-530; R and t only (hyp_setup fills the rest)
template <class W3>
RC_FN void hypotheses_f(W3& w, const float F21[9], const Cam& c, Hyp h[4]) {
    float K[9], Kt[9], tmp[9], E[9], U[9], S[3], Vt[9];
    cam_matrix(c, K);
    tv::transpose3(K, Kt);
    tv::mul3(Kt, F21, tmp);
    tv::mul3(tmp, K, E);
    svd3(w, E, U, S, Vt);
    float t[3] = {U[2], U[5], U[8]};
    const double alpha = 1.0 / norm3(t);
    RC_UNROLL
    for (int i = 0; i < 3; ++i) t[i] = scale_f(t[i], alpha);
    const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float Wt[9], R1[9], R2[9];
    tv::transpose3(Wm, Wt);
    tv::mul3(U, Wm, tmp);
    tv::mul3(tmp, Vt, R1);
    if (det3(R1) < 0) { RC_UNROLL for (int k = 0; k < 9; ++k) R1[k] = -R1[k]; }
    tv::mul3(U, Wt, tmp);
    tv::mul3(tmp, Vt, R2);
    if (det3(R2) < 0) { RC_UNROLL for (int k = 0; k < 9; ++k) R2[k] = -R2[k]; }
    RC_UNROLL
    for (int k = 0; k < 9; ++k) { h[0].R[k] = R1[k]; h[1].R[k] = R2[k]; h[2].R[k] = R1[k]; h[3].R[k] = R2[k]; }
    RC_UNROLL
    for (int i = 0; i < 3; ++i) { h[0].t[i] = t[i]; h[1].t[i] = t[i]; h[2].t[i] = -t[i]; h[3].t[i] = -t[i]; }
}

// :625-728: the eight hypotheses and their plane normals; false at the return of :639 (R, t, n are zeros then)
template <class W3>
RC_FN bool hypotheses_h(W3& w, const float H21[9], const Cam& c, Hyp h[8], float n[8][3]) {
    RC_UNROLL
    for (int i = 0; i < 8; ++i) {
        RC_UNROLL
        for (int k = 0; k < 9; ++k) h[i].R[k] = 0.f;
        RC_UNROLL
        for (int k = 0; k < 3; ++k) { h[i].t[k] = 0.f; n[i][k] = 0.f; }
    }
    float K[9], invK[9], tmp[9], A[9], U[9], S[3], Vt[9], V[9];
    cam_matrix(c, K);
    tv::inv3(K, invK);
    tv::mul3(invK, H21, tmp);
    tv::mul3(tmp, K, A);
    svd3(w, A, U, S, Vt);
    tv::transpose3(Vt, V);
    const float s = (float)(det3(U) * det3(Vt));
    const float d1 = S[0], d2 = S[1], d3 = S[2];
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    const float aux1 = sqrt_f((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrt_f((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrt_f((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrt_f((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    float sU[9];
    RC_UNROLL
    for (int k = 0; k < 9; ++k) sU[k] = scale_f(U[k], (double)s);
    RC_UNROLL
    for (int g = 0; g < 2; ++g) {
        RC_UNROLL
        for (int i = 0; i < 4; ++i) {
            float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            float tp[3] = {x1[i], 0.f, 0.f};
            float scale;
            if (g == 0) { Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta; tp[2] = -x3[i]; scale = d1 - d3; }
            else { Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi; tp[2] = x3[i]; scale = d1 + d3; }
            Hyp& o = h[g * 4 + i];
            tv::mul3(sU, Rp, tmp);
            tv::mul3(tmp, Vt, o.R);
            RC_UNROLL
            for (int k = 0; k < 3; ++k) tp[k] = scale_f(tp[k], (double)scale);
            float t[3];
            gemm<3, 3, 1>(U, tp, t);
            const double alpha = 1.0 / norm3(t);
            RC_UNROLL
            for (int k = 0; k < 3; ++k) o.t[k] = scale_f(t[k], alpha);
            const float np[3] = {x1[i], 0.f, x3[i]};
            float nn[3];
            gemm<3, 3, 1>(V, np, nn);
            if (nn[2] < 0) { RC_UNROLL for (int k = 0; k < 3; ++k) nn[k] = -nn[k]; }
            RC_UNROLL
            for (int k = 0; k < 3; ++k) n[g * 4 + i][k] = nn[k];
        }
    }
    return true;
}

// The choice among the hypotheses.  hypothesis: the candidate the reference settled on (F: the first whose nGood equals maxGood, once :550 let it through; H:
// bestSolutionIdx), -1 when there is none; ok only when that candidate also passed its gates
struct Choice { int ok, reason, hypothesis; };
// :532-607
RC_FN Choice choose_f(const int nGood[4], const float parallax[4], int N, float minParallax, int minTriangulated) {
    int maxGood = nGood[0];
    RC_UNROLL
    for (int i = 1; i < 4; ++i) maxGood = nGood[i] > maxGood ? nGood[i] : maxGood;
    const int n09 = static_cast<int>(0.9 * N);
    const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
    int nsimilar = 0;
    RC_UNROLL
    for (int i = 0; i < 4; ++i) if (nGood[i] > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) return Choice{0, REASON_NO_WINNER, -1};
    int first = 3;
    RC_UNROLL
    for (int i = 3; i >= 0; --i) if (maxGood == nGood[i]) first = i;
    float par = 0.f;
    RC_UNROLL
    for (int i = 0; i < 4; ++i) if (i == first) par = parallax[i];
    if (par > minParallax) return Choice{1, REASON_OK, first};
    return Choice{0, REASON_PARALLAX, first};
}
// :731-780
RC_FN Choice choose_h(const int nGood[8], const float parallax[8], int N, float minParallax, int minTriangulated) {
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    float bestParallax = -1;
    RC_UNROLL
    for (int i = 0; i < 8; ++i) {
        if (nGood[i] > bestGood) { secondBestGood = bestGood; bestGood = nGood[i]; bestSolutionIdx = i; bestParallax = parallax[i]; }
        else if (nGood[i] > secondBestGood) secondBestGood = nGood[i];
    }
    if (!(secondBestGood < 0.75 * bestGood) || !(bestGood > minTriangulated) || !(bestGood > 0.9 * N)) return Choice{0, REASON_NO_WINNER, bestSolutionIdx};
    if (!(bestParallax >= minParallax)) return Choice{0, REASON_PARALLAX, bestSolutionIdx};
    return Choice{1, REASON_OK, bestSolutionIdx};
}

// :1088-1158 for one line match with LineTriangulate (:1003-1055).  kl1: startPointX, startPointY, endPointX, endPointY of the line of frame 1 (the line of frame 2 gives its
// function alone, as in the reference); f1 / f2: mvKeyLineFunctions of the two lines.  A row that is not finite leaves zeros everywhere (:1102-1106)
struct LineOut { float s3d[3], e3d[3]; double err1, err2; };
template <class W>
RC_FN void line_row(const Cam& c, const Hyp& h, const float kl1[4], const double f1[3], const double f2[3], W& w, LineOut& o) {
    const float fx1 = c.fx, fy1 = c.fy, cx1 = c.cx, cy1 = c.cy;
    const float invfx1 = (float)(1.0 / (double)c.fx), invfy1 = (float)(1.0 / (double)c.fy);
    float K[9];
    cam_matrix(Cam{fx1, fy1, cx1, cy1}, K);
    const float lineF1[3] = {(float)f1[0], (float)f1[1], (float)f1[2]}, lineF2[3] = {(float)f2[0], (float)f2[1], (float)f2[2]};
    const float Tw[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    float p1[12];
    gemm<3, 3, 4>(K, Tw, p1);
    const float StartC1[3] = {(kl1[0] - cx1) * invfx1, (kl1[1] - cy1) * invfy1, 1.f};
    const float EndC1[3] = {(kl1[2] - cx1) * invfx1, (kl1[3] - cy1) * invfy1, 1.f};
    float A[16], v[4], S[3], E[3];
    gemm<1, 3, 4>(lineF1, p1, A);
    gemm<1, 3, 4>(lineF2, h.P2, A + 4);
    RC_UNROLL
    for (int j = 0; j < 4; ++j) { A[8 + j] = StartC1[0] * Tw[8 + j] - Tw[j]; A[12 + j] = StartC1[1] * Tw[8 + j] - Tw[4 + j]; }
    svd4_last(w, A, v);
    double alpha = 1.0 / (double)v[3];
    RC_UNROLL
    for (int i = 0; i < 3; ++i) S[i] = scale_f(v[i], alpha);
    RC_UNROLL
    for (int j = 0; j < 4; ++j) { A[8 + j] = EndC1[0] * Tw[8 + j] - Tw[j]; A[12 + j] = EndC1[1] * Tw[8 + j] - Tw[4 + j]; }
    svd4_last(w, A, v);
    alpha = 1.0 / (double)v[3];
    RC_UNROLL
    for (int i = 0; i < 3; ++i) E[i] = scale_f(v[i], alpha);
    RC_UNROLL
    for (int i = 0; i < 3; ++i) o.s3d[i] = o.e3d[i] = 0.f;
    o.err1 = o.err2 = 0.0;
    if (!finite_f(S[0]) || !finite_f(S[1]) || !finite_f(S[2]) || !finite_f(E[0]) || !finite_f(E[1]) || !finite_f(E[2])) return;
    RC_UNROLL
    for (int i = 0; i < 3; ++i) { o.s3d[i] = S[i]; o.e3d[i] = E[i]; }
    float S2[3], E2[3];
    gemm<3, 3, 1>(h.R, S, S2);
    gemm<3, 3, 1>(h.R, E, E2);
    RC_UNROLL
    for (int i = 0; i < 3; ++i) { S2[i] = S2[i] + h.t[i]; E2[i] = E2[i] + h.t[i]; }
    const float fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
    const float invZ1start = (float)(1.0 / (double)S[2]);
    const float im1Startx = fx * S[0] * invZ1start + cx, im1Starty = fy * S[1] * invZ1start + cy;
    const float invZ1end = (float)(1.0 / (double)E[2]);
    const float im1Endx = fx * E[0] * invZ1end + cx, im1Endy = fx * E[1] * invZ1end + cy;      // fx: :1129
    const double a0 = f1[0] * im1Startx + f1[1] * im1Starty + f1[2], a1 = f1[0] * im1Endx + f1[1] * im1Endy + f1[2];
    o.err1 = __builtin_sqrt(a0 * a0 + a1 * a1);
    const float invZ2start = (float)(1.0 / (double)S2[2]);
    const float im2Startx = fx * S2[0] * invZ2start + cx, im2Starty = fy * S2[1] * invZ2start + cy;
    const float invZ2end = (float)(1.0 / (double)E2[2]);
    const float im2Endx = fx * E2[0] * invZ2end + cx, im2Endy = fy * E2[1] * invZ2end + cy;
    const double b0 = f2[0] * im2Startx + f2[1] * im2Starty + f2[2], b1 = f2[0] * im2Endx + f2[1] * im2Endy + f2[2];
    o.err2 = __builtin_sqrt(b0 * b0 + b1 * b1);
}
// vector_mad (include/auxiliar.h:91-106) and :1162-1163 from the median of |residue - median|
RC_FN double abs_dev(double residue, double median) { return __builtin_fabs(residue - median); }
RC_FN double inlier_threshold(double mad) { return 2.0 * (1.4826 * mad); }

}  // namespace rc
}  // namespace sslam
