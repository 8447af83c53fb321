// The arithmetic of Sim3Solver (reference src/Sim3Solver.cc; LoopClosing::ComputeSim3 runs it at src/LoopClosing.cc:279-306): the constructor's per-correspondence values
// (:81-98, :108-109 FromCameraToImage :405-423), SetRansacParameters (:114-138), the draw and the control flow of iterate (:140-207), ComputeSim3 (:226-337),
// CheckInliers (:340-364) and Project (:382-403).  No HIP in here: csrc/sim3.hip compiles this text for the device and tests/sim/sim3_sim.cpp for the host with a plain
// compiler, both without contraction (-ffp-contract=off), so that the two produce the same bits.  Only + - * / and sqrt are used in double and + - * / in float on the device.
//
// Reference-owned arithmetic is restated operation for operation: FromCameraToImage, Project, CheckInliers, the N11 .. N44 entries (:251-260; the operands are floats, so each
// sum is a FLOAT sum, left to right, that is then widened to the double it is assigned to and comes back unchanged through Mat_<float> <<), the den loop (:298-306),
// ms12i = nom / den, and the gates: mvnMaxError is a vector<size_t> (include/Sim3Solver.h:78-79), so the gate is the integer part of 9.210 * sigma2, compared as a float.
// What the reference leaves to OpenCV or libm is decision D16:
//   adopted  the rules oracle/ref_pin/stub_cv/stub_cv.hpp already states: A * B, A + B, A - B, -A, A.t() in float, row by row, ((a0 b0 + a1 b1) + a2 b2) (+ c);
//            s * A = (float)((double)a * s); Mat::dot with products and the running sum in double, in element order.  They cover Rcw * X + tcw, M = Pr2 * Pr1.t(),
//            P3 = mR12i * Pr2, Pr1.dot(P3), ms12i * mR12i, (1.0 / ms12i) * mR12i.t(), -sRinv * mt12i and O1 - ms12i * mR12i * O2 = O1 - ((s * R) * O2).
//   reduce   cv::reduce(.., SUM) of a 3 x 3: (p0 + p1) + p2 in float; C / P.cols by the stub's A / s: (float)((double)c * (1.0 / 3)).
//   pow      cv::pow(P3, 2): x * x in float.
//   eigen    cv::eigen of the symmetric 4 x 4: cyclic Jacobi in double on the float entries, JACOBI_SWEEPS sweeps over (p, q), p < q, in row-major order, with D15's
//            rotation; the eigenvector of the largest diagonal entry, the lowest index among exactly equal maxima; its four components stay in double.
//   rodrigues  atan2 + cv::Rodrigues (:274-284) turn the quaternion (w, v) into 2 atan2(|v|, w) v / |v| and that into a matrix: exactly
//            R = I + (2 / (w^2 + v.v)) (w [v]x + [v]x^2), evaluated in double in the order written in rotation_from_quaternion and rounded once per element to float.
//            v == 0 exactly is 0 / 0 at :280: R12 is all NaN and the hypothesis has no inlier.
//   table    SetRansacParameters' log / pow / ceil are libm's, evaluated on the host (ransac_max_its below is host code) for every N the kernel can meet.
//
// The draw: DUtils::Random::RandomInt is rand(); here randi = hash32(seed, pair, it, j) % remaining (draw_set<3> of ransac_draw.h, which states hash32 and the replay of the
// swap-with-back of :170-176).  Fewer than three correspondences cannot be drawn from (the reference would ask RandomInt(0, -1)): such an
// iteration counts like an injected set with an index out of range -- it is walked, never becomes the best and never returns.
//
// A consequence of iterate's control flow: `mnInliersi >= mnBestInliers` (:183) sits in front of `mnInliersi > mRansacMinInliers` (:192).  So a call returns at the FIRST
// iteration whose count is >= every earlier count -- mnBestInliers carried in from earlier calls included -- and is > min_inliers; among equal counts the LATER iteration
// becomes the best.  The iterations are therefore independent up to a prefix maximum of their counts, which is what lets the kernel run 64 of them side by side.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "ransac_draw.h"

#if defined(__HIPCC__)
#define S3_FN __host__ __device__ __forceinline__
#else
#define S3_FN inline
#endif

namespace sslam {
namespace s3 {

using sslam::draw_set;      // :168-176 for one iteration over n >= 3 correspondences: set is an int[3]

struct Cam { float fx, fy, cx, cy; };
// one correspondence: mvX3Dc1 / mvX3Dc2, mvP1im1 / mvP2im2, mvnMaxError1 / 2 as the floats the comparison of :356 converts them to.  48 bytes
struct Row { float X1[3], X2[3], p1[2], p2[2], maxErr1, maxErr2; };
struct Sim3 { float s, R[9], t[3]; };                                // ms12i, mR12i (row-major), mt12i
struct Transforms { float sR[9], t12[3], sRinv[9], t21[3]; };        // the rotation-scale blocks and translations of mT12i and mT21i

// :87-88.  A sigma2 whose product is no value of size_t (negative, NaN, >= 2^64) gives the gate 0: nothing passes
S3_FN float max_error(float sigma2) {
    const double e = 9.210 * (double)sigma2;
    return (e >= 0.0 && e < 18446744073709551616.0) ? (float)(size_t)e : 0.f;
}

// :417-421 for one point
S3_FN void camera_to_image(const float X[3], const Cam& K, float p[2]) {
    const float invz = 1 / X[2];
    const float x = X[0] * invz;
    const float y = X[1] * invz;
    p[0] = K.fx * x + K.cx;
    p[1] = K.fy * y + K.cy;
}

// :396-401 for one point: A = Tcw's 3 x 3 block, t its last column
S3_FN void project(const float A[9], const float t[3], const float X[3], const Cam& K, float p[2]) {
    float c[3];
    for (int i = 0; i < 3; ++i) c[i] = ((A[i * 3] * X[0] + A[i * 3 + 1] * X[1]) + A[i * 3 + 2] * X[2]) + t[i];
    camera_to_image(c, K, p);
}

// one (p, q) rotation of the cyclic Jacobi on the upper triangle a (a[i][j], i <= j) and the eigenvector columns v; every index is a compile-time constant
template <int K, int P, int Q>
S3_FN void rotate_k(double (&a)[4][4], double (&v)[4][4], double c, double s) {
    if (K != P && K != Q) {
        constexpr int pl = K < P ? K : P, ph = K < P ? P : K, ql = K < Q ? K : Q, qh = K < Q ? Q : K;
        const double akp = a[pl][ph], akq = a[ql][qh];
        a[pl][ph] = c * akp - s * akq;
        a[ql][qh] = s * akp + c * akq;
    }
    const double vkp = v[K][P], vkq = v[K][Q];
    v[K][P] = c * vkp - s * vkq;
    v[K][Q] = s * vkp + c * vkq;
}
template <int P, int Q>
S3_FN void rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double app = a[P][P], aqq = a[Q][Q];
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    rotate_k<0, P, Q>(a, v, c, s); rotate_k<1, P, Q>(a, v, c, s); rotate_k<2, P, Q>(a, v, c, s); rotate_k<3, P, Q>(a, v, c, s);
    a[P][P] = app - t * apq;
    a[Q][Q] = aqq + t * apq;
    a[P][Q] = 0.0;
}

// D16 eigen: n = the ten entries N11 N12 N13 N14 N22 N23 N24 N33 N34 N44; q = the eigenvector (w, v0, v1, v2) of the largest eigenvalue.  Fixed trip counts: NaNs and
// infinities pass through and end
S3_FN void jacobi_largest(const float n[10], double q[4]) {
    double a[4][4], v[4][4];
    a[0][0] = n[0]; a[0][1] = n[1]; a[0][2] = n[2]; a[0][3] = n[3]; a[1][1] = n[4]; a[1][2] = n[5]; a[1][3] = n[6]; a[2][2] = n[7]; a[2][3] = n[8]; a[3][3] = n[9];
    a[1][0] = a[2][0] = a[2][1] = a[3][0] = a[3][1] = a[3][2] = 0.0;      // never read
    v[0][0] = 1.0; v[0][1] = 0.0; v[0][2] = 0.0; v[0][3] = 0.0;
    v[1][0] = 0.0; v[1][1] = 1.0; v[1][2] = 0.0; v[1][3] = 0.0;
    v[2][0] = 0.0; v[2][1] = 0.0; v[2][2] = 1.0; v[2][3] = 0.0;
    v[3][0] = 0.0; v[3][1] = 0.0; v[3][2] = 0.0; v[3][3] = 1.0;
    RANSAC_NOUNROLL
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        rotate<0, 1>(a, v); rotate<0, 2>(a, v); rotate<0, 3>(a, v); rotate<1, 2>(a, v); rotate<1, 3>(a, v); rotate<2, 3>(a, v);
    }
    int best = 0;
    double highest = a[0][0];
    if (a[1][1] > highest) { highest = a[1][1]; best = 1; }
    if (a[2][2] > highest) { highest = a[2][2]; best = 2; }
    if (a[3][3] > highest) { highest = a[3][3]; best = 3; }
    q[0] = best == 0 ? v[0][0] : best == 1 ? v[0][1] : best == 2 ? v[0][2] : v[0][3];
    q[1] = best == 0 ? v[1][0] : best == 1 ? v[1][1] : best == 2 ? v[1][2] : v[1][3];
    q[2] = best == 0 ? v[2][0] : best == 1 ? v[2][1] : best == 2 ? v[2][2] : v[2][3];
    q[3] = best == 0 ? v[3][0] : best == 1 ? v[3][1] : best == 2 ? v[3][2] : v[3][3];
}

// D16 rodrigues
S3_FN void rotation_from_quaternion(const double q[4], float R[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    if (x == 0.0 && y == 0.0 && z == 0.0) {
        const float nan = __builtin_nanf("");
        for (int k = 0; k < 9; ++k) R[k] = nan;
        return;
    }
    const double k = 2.0 / (((w * w + x * x) + y * y) + z * z);
    R[0] = (float)(1.0 - k * (y * y + z * z)); R[1] = (float)(k * (x * y - w * z));       R[2] = (float)(k * (x * z + w * y));
    R[3] = (float)(k * (x * y + w * z));       R[4] = (float)(1.0 - k * (x * x + z * z)); R[5] = (float)(k * (y * z - w * x));
    R[6] = (float)(k * (x * z - w * y));       R[7] = (float)(k * (y * z + w * x));       R[8] = (float)(1.0 - k * (x * x + y * y));
}

// :217-223.  P[i * 3 + j] = coordinate i of point j
S3_FN void centroid(const float P[9], float Pr[9], float O[3]) {
    for (int i = 0; i < 3; ++i) {
        const float sum = (P[i * 3] + P[i * 3 + 1]) + P[i * 3 + 2];
        const float c = (float)((double)sum * (1.0 / 3.0));
        O[i] = c;
        for (int j = 0; j < 3; ++j) Pr[i * 3 + j] = P[i * 3 + j] - c;
    }
}

// :243-260: the ten distinct entries of N
S3_FN void n_entries(const float Pr1[9], const float Pr2[9], float n[10]) {
    float M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i * 3 + j] = (Pr2[i * 3] * Pr1[j * 3] + Pr2[i * 3 + 1] * Pr1[j * 3 + 1]) + Pr2[i * 3 + 2] * Pr1[j * 3 + 2];
    n[0] = M[0] + M[4] + M[8];
    n[1] = M[5] - M[7];
    n[2] = M[6] - M[2];
    n[3] = M[1] - M[3];
    n[4] = M[0] - M[4] - M[8];
    n[5] = M[1] + M[3];
    n[6] = M[6] + M[2];
    n[7] = -M[0] + M[4] - M[8];
    n[8] = M[5] + M[7];
    n[9] = -M[0] - M[4] + M[8];
}

// :226-316: P1 / P2 hold the three drawn points of each keyframe as columns
S3_FN void compute_sim3(const float P1[9], const float P2[9], bool fixScale, Sim3& o) {
    float Pr1[9], Pr2[9], O1[3], O2[3], n[10];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    n_entries(Pr1, Pr2, n);
    double q[4];
    jacobi_largest(n, q);
    rotation_from_quaternion(q, o.R);
    if (!fixScale) {
        double nom = 0, den = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const float p3 = (o.R[i * 3] * Pr2[j] + o.R[i * 3 + 1] * Pr2[3 + j]) + o.R[i * 3 + 2] * Pr2[6 + j];
                nom += (double)Pr1[i * 3 + j] * (double)p3;
                den += (double)(p3 * p3);
            }
        o.s = (float)(nom / den);
    } else {
        o.s = 1.0f;
    }
    for (int i = 0; i < 3; ++i) {
        const float a0 = (float)((double)o.R[i * 3] * (double)o.s), a1 = (float)((double)o.R[i * 3 + 1] * (double)o.s), a2 = (float)((double)o.R[i * 3 + 2] * (double)o.s);
        o.t[i] = O1[i] - ((a0 * O2[0] + a1 * O2[1]) + a2 * O2[2]);
    }
}

// :323-336
S3_FN void transforms(const Sim3& h, Transforms& T) {
    const double alpha = 1.0 / (double)h.s;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            T.sR[i * 3 + j] = (float)((double)h.R[i * 3 + j] * (double)h.s);
            T.sRinv[i * 3 + j] = (float)((double)h.R[j * 3 + i] * alpha);
        }
        T.t12[i] = h.t[i];
    }
    for (int i = 0; i < 3; ++i) T.t21[i] = ((-T.sRinv[i * 3]) * h.t[0] + (-T.sRinv[i * 3 + 1]) * h.t[1]) + (-T.sRinv[i * 3 + 2]) * h.t[2];
}

// :343-363 for one correspondence
S3_FN bool check_row(const Transforms& T, const Cam& K1, const Cam& K2, const Row& r) {
    float p2im1[2], p1im2[2];
    project(T.sR, T.t12, r.X2, K1, p2im1);
    project(T.sRinv, T.t21, r.X1, K2, p1im2);
    const float d1x = r.p1[0] - p2im1[0], d1y = r.p1[1] - p2im1[1];
    const float d2x = p1im2[0] - r.p2[0], d2y = p1im2[1] - r.p2[1];
    const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
    const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
    return err1 < r.maxErr1 && err2 < r.maxErr2;
}

// One iteration of :158-181 up to and including CheckInliers.  rows(i) = correspondence i of mvnIndices1's order, n of them; set: three indices into it, valid = all in
// [0, n).  Returns mnInliersi; -1 with a zero hypothesis for an invalid set.  mark(i, bIn) receives mvbInliersi
template <class Rows, class Mark>
S3_FN int hypothesis(const Rows& rows, int n, const Cam& K1, const Cam& K2, const int set[3], bool valid, bool fixScale, Sim3& h, Mark mark) {
    if (!valid) {
        h.s = 0.f;
        for (int k = 0; k < 9; ++k) h.R[k] = 0.f;
        for (int k = 0; k < 3; ++k) h.t[k] = 0.f;
        return -1;
    }
    float P1[9], P2[9];
    for (int j = 0; j < 3; ++j) {
        const Row r = rows(set[j]);
        for (int i = 0; i < 3; ++i) { P1[i * 3 + j] = r.X1[i]; P2[i * 3 + j] = r.X2[i]; }
    }
    compute_sim3(P1, P2, fixScale, h);
    Transforms T;
    transforms(h, T);
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const bool in = check_row(T, K1, K2, rows(i));
        mark(i, in);
        if (in) ++count;
    }
    return count;
}

// :125-135 for N >= minInliers correspondences, host only (libm).  Where ceil's value is no int smaller than maxIterations -- the quotient overflows, or 1 - epsilon^3
// rounds to 1 and the quotient is -inf -- the reference's conversion is undefined; mRansacMaxIts is maxIterations then, which is what every defined value that large gives.
inline int ransac_max_its(double probability, int minInliers, int maxIterations, int N) {
    const float epsilon = (float)minInliers / N;
    if (minInliers == N) return 1;      // max(1, min(1, maxIterations))
    const double d = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
    if (!(d >= 0.0 && d < (double)maxIterations)) return maxIterations > 1 ? maxIterations : 1;
    const int nIterations = (int)d;
    const int m = nIterations < maxIterations ? nIterations : maxIterations;
    return m > 1 ? m : 1;
}

}  // namespace s3
}  // namespace sslam
