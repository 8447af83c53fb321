// The arithmetic of Initializer::Initialize's model selection (reference src/Initializer.cc:55-153): Normalize (:784-830), the RANSAC draw (:93-108), ComputeH21 / ComputeF21
// (:255-332), the compositions of FindHomography / FindFundamental (:191-192, :242), CheckHomography / CheckFundamental (:334-497) and the selection (:118, :143, :196, :246).
// No HIP in here: csrc/two_view.hip compiles this text for the device and tests/sim/two_view_sim.cpp for the host with a plain compiler, both without contraction
// (-ffp-contract=off), so that the two produce the same bits.  Only + - * / and sqrt are used in double and + - * / in float: all correctly rounded on both sides.
//
// Reference-owned arithmetic is restated operation for operation.  What the reference leaves to OpenCV is decision D15, in three parts:
//   solver   cv::SVDecomp's last right singular vector = the eigenvector of the smallest eigenvalue of A^T A.  A^T A is accumulated in double from the float entries of A
//            (row after row; a product of two floats is exact in double), diagonalised by cyclic Jacobi in double, JACOBI_SWEEPS sweeps over (p, q), p < q, in row-major
//            order; the eigenvector is rounded once to float.  Rank 2: v3 = that eigenvector of Fpre^T Fpre (n = 3), Fn = Fpre - (Fpre v3) v3^T in double, rounded once.
//   gemm     a float 3 x 3 product accumulates each element in double (acc = 0; acc += a_ik * b_kj for k = 0, 1, 2) and rounds once; A*B*C is (A*B)*C.
//   inverse  cofactors; determinant and its reciprocal in double, each element (cofactor * reciprocal) rounded once; a zero determinant gives the zero matrix.
//
// The draw (:93-108): draw_set<8> of ransac_draw.h, which states the hash that stands in for rand() and the replay of the swap-with-back.
#pragma once
#include <cstdint>
#include "ransac_draw.h"

#define TV_FN RANSAC_FN
#define TV_UNROLL RANSAC_UNROLL
#define TV_NOUNROLL RANSAC_NOUNROLL

namespace sslam {
namespace tv {

using sslam::draw_set;      // :93-108 for one iteration over nm >= 8 matches: set is an int[8]

constexpr int WS_DOUBLES = 45 + 81;      // per solve: the upper triangle of a symmetric 9 x 9 and the 9 x 9 of eigenvectors

// :784-830 for one coordinate of one frame: mean and scale over ALL n keypoints.  get(i) = vKeys[i].pt.x (or .y)
template <class Get>
TV_FN void normalize_axis(int n, Get get, float& mean, float& s) {
    float m = 0;
    for (int i = 0; i < n; ++i) m += get(i);
    m = m / n;
    float dev = 0;
    for (int i = 0; i < n; ++i) dev += __builtin_fabsf(get(i) - m);
    dev = dev / n;
    mean = m;
    s = (float)(1.0 / dev);
}
struct Norm { float meanX, sX, meanY, sY; };      // of one frame
// T of :825-829, row-major
TV_FN void norm_matrix(const Norm& n, float T[9]) {
    T[0] = n.sX; T[1] = 0.f; T[2] = -n.meanX * n.sX;
    T[3] = 0.f; T[4] = n.sY; T[5] = -n.meanY * n.sY;
    T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// D15 gemm
TV_FN void mul3(const float A[9], const float B[9], float C[9]) {
    TV_UNROLL
    for (int i = 0; i < 3; ++i) {
        TV_UNROLL
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            TV_UNROLL
            for (int k = 0; k < 3; ++k) acc += (double)A[i * 3 + k] * (double)B[k * 3 + j];
            C[i * 3 + j] = (float)acc;
        }
    }
}
// D15 inverse
TV_FN void inv3(const float m[9], float o[9]) {
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    double d = m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6) + m2 * (m3 * m7 - m4 * m6);
    if (d == 0.0) {
        TV_UNROLL
        for (int i = 0; i < 9; ++i) o[i] = 0.f;
        return;
    }
    d = 1.0 / d;
    o[0] = (float)((m4 * m8 - m5 * m7) * d); o[1] = (float)((m2 * m7 - m1 * m8) * d); o[2] = (float)((m1 * m5 - m2 * m4) * d);
    o[3] = (float)((m5 * m6 - m3 * m8) * d); o[4] = (float)((m0 * m8 - m2 * m6) * d); o[5] = (float)((m2 * m3 - m0 * m5) * d);
    o[6] = (float)((m3 * m7 - m4 * m6) * d); o[7] = (float)((m1 * m6 - m0 * m7) * d); o[8] = (float)((m0 * m4 - m1 * m3) * d);
}
TV_FN void transpose3(const float m[9], float o[9]) {
    TV_UNROLL
    for (int i = 0; i < 3; ++i) {
        TV_UNROLL
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = m[j * 3 + i];
    }
}

// Working storage of one solve: W::at(k) is a reference to double k of WS_DOUBLES.  The device keeps it in LDS, lane-interleaved (two_view.hip), so that the
// run-time indices below never make a private array; the host uses a plain array.
// LD is the width the storage is laid out for: 9 here; a caller with a smaller matrix may lay it out as narrow as that matrix (LD * (LD + 1) / 2 + LD * LD doubles).
template <int LD = 9> TV_FN int sym_index(int i, int j) {      // upper triangle of an LD-wide symmetric matrix, any order of (i, j)
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo * LD - lo * (lo - 1) / 2 + (hi - lo);
}
template <int LD = 9, class W> TV_FN double& ws_a(W& w, int i, int j) { return w.at(sym_index<LD>(i, j)); }
template <int LD = 9, class W> TV_FN double& ws_v(W& w, int i, int j) { return w.at(LD * (LD + 1) / 2 + i * LD + j); }

// D15 solver, second half: cyclic Jacobi on the symmetric N x N matrix in ws_a (N <= LD); returns the column of ws_v that belongs to the smallest diagonal entry
// (the first of equals).  Fixed trip counts: NaNs and infinities pass through and end.  The loop over k is unrolled and loads rows p and q of every k before it stores
// any (the two it must not change are loaded too and not stored), so that the loads of a rotation are in flight together.
template <int N, int LD = 9, class W>
TV_FN int jacobi_smallest(W& w) {
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) ws_v<LD>(w, i, j) = i == j ? 1.0 : 0.0;
    TV_NOUNROLL
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        TV_NOUNROLL
        for (int p = 0; p < N - 1; ++p) {
            TV_NOUNROLL
            for (int q = p + 1; q < N; ++q) {
                const double apq = ws_a<LD>(w, p, q);
                if (apq == 0.0) continue;
                const double app = ws_a<LD>(w, p, p), aqq = ws_a<LD>(w, q, q);
                double akp[N], akq[N], vkp[N], vkq[N];
                TV_UNROLL
                for (int k = 0; k < N; ++k) { akp[k] = ws_a<LD>(w, k, p); akq[k] = ws_a<LD>(w, k, q); vkp[k] = ws_v<LD>(w, k, p); vkq[k] = ws_v<LD>(w, k, q); }
                const double theta = (aqq - app) / (2.0 * apq);
                const double at = theta < 0.0 ? -theta : theta;
                double t = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
                TV_UNROLL
                for (int k = 0; k < N; ++k) {
                    if (k != p && k != q) {
                        ws_a<LD>(w, k, p) = c * akp[k] - s * akq[k];
                        ws_a<LD>(w, k, q) = s * akp[k] + c * akq[k];
                    }
                    ws_v<LD>(w, k, p) = c * vkp[k] - s * vkq[k];
                    ws_v<LD>(w, k, q) = s * vkp[k] + c * vkq[k];
                }
                ws_a<LD>(w, p, p) = app - t * apq;
                ws_a<LD>(w, q, q) = aqq + t * apq;
                ws_a<LD>(w, p, q) = 0.0;
            }
        }
    }
    int best = 0;
    double lowest = ws_a<LD>(w, 0, 0);
    for (int i = 1; i < N; ++i) { const double d = ws_a<LD>(w, i, i); if (d < lowest) { lowest = d; best = i; } }
    return best;
}

// one row of A into A^T A (upper triangle, which sym_index numbers row-major), in double.  The row is parked in the eigenvector area, which is unused until the Jacobi
// starts, so that the loops run on run-time indices without a private array; (double)r[i] * (double)r[j] is exact.
template <class W>
TV_FN void accumulate_row(W& w, const float r[9]) {
    TV_UNROLL
    for (int k = 0; k < 9; ++k) w.at(45 + k) = (double)r[k];
    int idx = 0;
    TV_NOUNROLL
    for (int i = 0; i < 9; ++i) {
        const double ri = w.at(45 + i);
        TV_NOUNROLL
        for (int j = i; j < 9; ++j, ++idx) w.at(idx) += ri * w.at(45 + j);
    }
}
template <class W> TV_FN void clear_sym(W& w) { for (int k = 0; k < 45; ++k) w.at(k) = 0.0; }

// :255-295.  p1 / p2: the eight normalised points (x, y interleaved).  h = vt.row(8) as D15's solver gives it
template <class W>
TV_FN void compute_h21(W& w, const float p1[16], const float p2[16], float h[9]) {
    clear_sym(w);
    TV_UNROLL
    for (int i = 0; i < 8; ++i) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
        accumulate_row(w, r0);
        accumulate_row(w, r1);
    }
    const int col = jacobi_smallest<9>(w);
    TV_UNROLL
    for (int k = 0; k < 9; ++k) h[k] = (float)ws_v(w, k, col);
}

// :297-332.  pre = Fpre (vt.row(8)), f = u * diag(w0, w1, 0) * vt as D15's solver gives them
template <class W>
TV_FN void compute_f21(W& w, const float p1[16], const float p2[16], float pre[9], float f[9]) {
    clear_sym(w);
    TV_UNROLL
    for (int i = 0; i < 8; ++i) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        accumulate_row(w, r);
    }
    int col = jacobi_smallest<9>(w);
    TV_UNROLL
    for (int k = 0; k < 9; ++k) pre[k] = (float)ws_v(w, k, col);
    // Fpre^T Fpre
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) ws_a(w, i, j) = 0.0;
    TV_UNROLL
    for (int r = 0; r < 3; ++r) {
        TV_UNROLL
        for (int i = 0; i < 3; ++i) {
            TV_UNROLL
            for (int j = i; j < 3; ++j) w.at(sym_index(i, j)) += (double)pre[r * 3 + i] * (double)pre[r * 3 + j];
        }
    }
    col = jacobi_smallest<3>(w);
    const double v0 = ws_v(w, 0, col), v1 = ws_v(w, 1, col), v2 = ws_v(w, 2, col);
    TV_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double wi = ((double)pre[i * 3] * v0 + (double)pre[i * 3 + 1] * v1) + (double)pre[i * 3 + 2] * v2;
        f[i * 3] = (float)((double)pre[i * 3] - wi * v0);
        f[i * 3 + 1] = (float)((double)pre[i * 3 + 1] - wi * v1);
        f[i * 3 + 2] = (float)((double)pre[i * 3 + 2] - wi * v2);
    }
}

TV_FN float inv_sigma_square(float sigma) { return (float)(1.0 / (sigma * sigma)); }

// :366-414 for one match: adds the match's terms to score (first image, then second) and returns bIn
TV_FN bool check_homography_match(const float H21[9], const float H12[9], float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += th - chiSquare2;
    return bIn;
}

// :442-494 for one match
TV_FN bool check_fundamental_match(const float F21[9], float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
    const float th = 3.841f;
    const float thScore = 5.991f;
    bool bIn = true;
    const float a2 = F21[0] * u1 + F21[1] * v1 + F21[2];
    const float b2 = F21[3] * u1 + F21[4] * v1 + F21[5];
    const float c2 = F21[6] * u1 + F21[7] * v1 + F21[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += thScore - chiSquare1;
    const float a1 = F21[0] * u2 + F21[3] * v2 + F21[6];
    const float b1 = F21[1] * u2 + F21[4] * v2 + F21[7];
    const float c1 = F21[2] * u2 + F21[5] * v2 + F21[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += thScore - chiSquare2;
    return bIn;
}

struct Row { float u1, v1, u2, v2; };      // one match: kp1.pt, kp2.pt (undistorted, not normalised)

// One RANSAC iteration of FindHomography and FindFundamental (:179-202, :229-252) up to and including the Check calls.  rows(i) = match i of the compacted list (ascending
// keypoint-1 index), nm of them; set: eight indices into it (valid = all in [0, nm); otherwise matrices and scores are zero and the hypothesis cannot win).
struct Hypothesis { float Hn[9], H21[9], H12[9], Fn[9], F21[9], Fpre[9], scoreH, scoreF; };
template <class Rows, class W>
TV_FN void hypothesis(const Rows& rows, int nm, const Norm& n1, const Norm& n2, const int set[8], bool valid, float sigma, W& w, Hypothesis& o) {
    float scoreH = 0.f, scoreF = 0.f;
    if (!valid) {
        TV_UNROLL
        for (int k = 0; k < 9; ++k) o.Hn[k] = o.H21[k] = o.H12[k] = o.Fn[k] = o.F21[k] = o.Fpre[k] = 0.f;
    } else {
        float p1[16], p2[16];
        TV_UNROLL
        for (int j = 0; j < 8; ++j) {
            const Row r = rows(set[j]);
            p1[2 * j] = (r.u1 - n1.meanX) * n1.sX; p1[2 * j + 1] = (r.v1 - n1.meanY) * n1.sY;
            p2[2 * j] = (r.u2 - n2.meanX) * n2.sX; p2[2 * j + 1] = (r.v2 - n2.meanY) * n2.sY;
        }
        float T1[9], T2[9], T2x[9], tmp[9];
        norm_matrix(n1, T1);
        norm_matrix(n2, T2);
        const float invSigmaSquare = inv_sigma_square(sigma);

        compute_h21(w, p1, p2, o.Hn);
        inv3(T2, T2x);
        mul3(T2x, o.Hn, tmp);
        mul3(tmp, T1, o.H21);
        inv3(o.H21, o.H12);
        for (int i = 0; i < nm; ++i) { const Row r = rows(i); check_homography_match(o.H21, o.H12, r.u1, r.v1, r.u2, r.v2, invSigmaSquare, scoreH); }

        compute_f21(w, p1, p2, o.Fpre, o.Fn);
        transpose3(T2, T2x);
        mul3(T2x, o.Fn, tmp);
        mul3(tmp, T1, o.F21);
        for (int i = 0; i < nm; ++i) { const Row r = rows(i); check_fundamental_match(o.F21, r.u1, r.v1, r.u2, r.v2, invSigmaSquare, scoreF); }
    }
    o.scoreH = scoreH;
    o.scoreF = scoreF;
}

// :118, :143: 1 = H, 2 = F
TV_FN void select_model(float SH, float SF, float& RH, int& model) {
    RH = SH / (SH + SF);
    model = RH > 0.40 ? 1 : 2;
}

}  // namespace tv
}  // namespace sslam
