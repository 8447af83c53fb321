// The arithmetic of the loop bodies of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:456-635) and LocalMapping::CreateNewMapLines2 (:1005-1170) with the
// first MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:335-376) and MapLine::UpdateAverageDir (src/MapLine.cpp:325-372) of the new object.  No HIP in here:
// csrc/newmap.hip compiles this text for the device and tests/sim/newmap_sim.cpp for the host with a plain compiler, both without contraction (-ffp-contract=off), so that
// the two produce the same bits.  Only + - * / and sqrt in double and + - * / in float are used; no libm call.
//
// Reference-owned arithmetic is restated operation for operation with its types: the float against double literal comparisons cosParallaxRays < 0.9998 (:497), < 0.98
// (:1053), > 5.991 * sigmaSquare (:557, :584), 1.0 / z1 (:547), ratio < 0.3 and > 0.61 (:1102-1131); z = Rcw.row(2).dot(x3Dt) + tcw(2) is a double sum rounded once (Mat::dot
// returns a double); cosParallaxRays is one double expression rounded once.  The quirks stay: CreateNewMapLines2 normalises the endpoints of key line 2 with key frame 1's
// cx1, invfx1, cy1, invfy1 (:1032-1035), builds s3D / e3D from line 1's endpoints and both line functions, and divides all five distances by the neighbour's median depth.
// A NaN behaves as the comparisons as written make it behave: a NaN cosine is "no parallax", a NaN depth or error passes its gate.
// What the reference leaves to OpenCV or Eigen is decision D19 = D18's leaves (reconstruct_math.h) and nothing new:
//   svd4     the 4 x 4 cv::SVD::compute of :507, :1063 and :1080, of which only vt.row(3) is used: rc::svd4_last
//   gemm     Rwc * x, K * Tcw, klF.t() * M: rc::gemm
//   scale    s * row (a float product: the double product of two floats is exact), x / s, (a + b) / 2, 0.5 * (a + b), normal / n: rc::scale_f with alpha = s or 1.0 / s
//   norm     cv::norm and Mat::dot: products and the running sum in double, element order; norm is the double sqrt of that sum
//   Eigen    the Vector3d arithmetic of UpdateAverageDir is plain double, element by element; Vector3d::norm() sums as Eigen's unrolled reduction of three terms does,
//            e0 * e0 + (e1 * e1 + e2 * e2), and v / s divides every element
// This fork is monocular (only GrabImageMonocularWithPL exists), so every mvuRight is negative: bStereo1 and bStereo2 are false, cosParallaxStereo is cosParallaxRays + 1,
// and the branches of :488-491, :518-525, :560-570 and :587-597 (cos(2 * atan2()), UnprojectStereo, the 7.8 gate) are not built.  Nothing here takes a d_uright.
#pragma once
#include <cstdint>
#include "../../include/sslam_frontend.h"
#include "reconstruct_math.h"

#define NM_FN RC_FN
#define NM_UNROLL RC_UNROLL

namespace sslam {
namespace nm {

// the exits of one point match (:459-617); include/sslam_frontend.h documents them
constexpr int PT_CREATED = 0, PT_NO_MATCH = 1, PT_PARALLAX = 2, PT_W_ZERO = 3, PT_Z1 = 4, PT_Z2 = 5, PT_ERR1 = 6, PT_ERR2 = 7, PT_DIST_ZERO = 8, PT_SCALE = 9;
// the exits of one line match (src/LSDmatcher.cpp:403, :1007-1148)
constexpr int LN_CREATED = 0, LN_NO_MATCH = 1, LN_NOT_FREE = 2, LN_PARALLAX = 3, LN_S_W_ZERO = 4, LN_E_W_ZERO = 5, LN_RATIO1 = 6, LN_RATIO2 = 7, LN_RATIO3 = 8, LN_RATIO4 = 9,
              LN_RATIO5 = 10, LN_SZC1 = 11, LN_SZC2 = 12, LN_EZC1 = 13, LN_EZC2 = 14;

// what a row returns.  Everything is zero until the row computes it: cosv from the parallax stage on, hom behind the SVD; x3d, normal, max_dist, min_dist of a row that
// is not created stay zero.  err1 / err2 (the two squared reprojection errors), ratio_dist / ratio_octave (:610-611) and ratio[5] (ratio1 .. ratio5) are the host model's trace,
// which the kernels do not keep
struct PointOut { float x3d[3]; int stage; float normal[3], max_dist, min_dist, cosv, hom[4], err1, err2, ratio_dist, ratio_octave; };
struct LineOut { float s3d[3], e3d[3]; int stage; double normal[3]; float max_dist, min_dist, cosv, shom[4], ehom[4], ratio[5]; };

NM_FN int clamp_level(int octave, int nlevels) { return octave < 0 ? 0 : octave >= nlevels ? nlevels - 1 : octave; }
NM_FN void transpose3(const float m[9], float o[9]) {
    NM_UNROLL
    for (int i = 0; i < 3; ++i) {
        NM_UNROLL
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = m[j * 3 + i];
    }
}
NM_FN void tcw_of(const sslam_kf_pose& P, float T[12]) {      // Tcw = [Rcw | tcw] (:386-388)
    NM_UNROLL
    for (int i = 0; i < 3; ++i) {
        NM_UNROLL
        for (int j = 0; j < 3; ++j) T[i * 4 + j] = P.Rcw[i * 3 + j];
        T[i * 4 + 3] = P.tcw[i];
    }
}
NM_FN double dot3(const float a[3], const float b[3]) { double s = 0.0; NM_UNROLL for (int i = 0; i < 3; ++i) s += (double)a[i] * (double)b[i]; return s; }
// ray1.dot(ray2) / (cv::norm(ray1) * cv::norm(ray2)) of the rays Rwc * xn (:479-482, :1038-1041)
NM_FN float cos_rays(const sslam_kf_pose& P1, const float xn1[3], const sslam_kf_pose& P2, const float xn2[3]) {
    float Rwc1[9], Rwc2[9], ray1[3], ray2[3];
    transpose3(P1.Rcw, Rwc1);
    transpose3(P2.Rcw, Rwc2);
    rc::gemm<3, 3, 1>(Rwc1, xn1, ray1);
    rc::gemm<3, 3, 1>(Rwc2, xn2, ray2);
    return (float)(dot3(ray1, ray2) / (rc::norm3(ray1) * rc::norm3(ray2)));
}
// vt.row(3) of A, then "(3) == 0: continue" and rowRange(0, 3) / (3) (:507-515); false at the continue
template <class W>
NM_FN bool solve_point(W& w, const float A[16], float hom[4], float x[3]) {
    rc::svd4_last(w, A, hom);
    if (hom[3] == 0) return false;
    const double alpha = 1.0 / (double)hom[3];
    NM_UNROLL
    for (int i = 0; i < 3; ++i) x[i] = rc::scale_f(hom[i], alpha);
    return true;
}
// Rcw.row(r).dot(x3Dt) + tcw.at<float>(r), assigned to a float (:533, :545)
NM_FN float cam_coord(const sslam_kf_pose& P, int r, const float x[3]) { return (float)(dot3(P.Rcw + 3 * r, x) + (double)P.tcw[r]); }
// cv::norm(x - O) assigned to a float (:601-605, :1099-1128)
NM_FN float dist_to(const float x[3], const float O[3]) { const float d[3] = {x[0] - O[0], x[1] - O[1], x[2] - O[2]}; return (float)rc::norm3(d); }

// :462-617 for one match of key point 1 (x1, y1, octave1) of the key frame with pose P1 and key point 2 of the neighbour P2, then UpdateNormalAndDepth of the new point with
// the observations {kf1, kf2} and mpRefKF = key frame 1.  sf / sigma2: mvScaleFactors / mvLevelSigma2 (one extractor), nlevels entries; an octave outside is clamped
template <class W>
NM_FN void point_row(const sslam_kf_pose& P1, const sslam_kf_pose& P2, float x1, float y1, int octave1, float x2, float y2, int octave2, const float* sf, const float* sigma2,
                     int nlevels, float ratioFactor, W& w, PointOut& o) {
    NM_UNROLL
    for (int i = 0; i < 3; ++i) o.x3d[i] = o.normal[i] = 0.f;
    NM_UNROLL
    for (int i = 0; i < 4; ++i) o.hom[i] = 0.f;
    o.max_dist = o.min_dist = o.err1 = o.err2 = o.ratio_dist = o.ratio_octave = 0.f;
    const int l1 = clamp_level(octave1, nlevels), l2 = clamp_level(octave2, nlevels);
    const float xn1[3] = {(x1 - P1.cx) * P1.invfx, (y1 - P1.cy) * P1.invfy, 1.f};
    const float xn2[3] = {(x2 - P2.cx) * P2.invfx, (y2 - P2.cy) * P2.invfy, 1.f};
    const float cosParallaxRays = cos_rays(P1, xn1, P2, xn2);
    o.cosv = cosParallaxRays;
    const float cosParallaxStereo = cosParallaxRays + 1;
    if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && cosParallaxRays < 0.9998)) { o.stage = PT_PARALLAX; return; }
    float T1[12], T2[12], A[16], x[3];
    tcw_of(P1, T1);
    tcw_of(P2, T2);
    NM_UNROLL
    for (int j = 0; j < 4; ++j) {
        A[j] = xn1[0] * T1[8 + j] - T1[j];
        A[4 + j] = xn1[1] * T1[8 + j] - T1[4 + j];
        A[8 + j] = xn2[0] * T2[8 + j] - T2[j];
        A[12 + j] = xn2[1] * T2[8 + j] - T2[4 + j];
    }
    if (!solve_point(w, A, o.hom, x)) { o.stage = PT_W_ZERO; return; }
    const float z1 = cam_coord(P1, 2, x);
    if (z1 <= 0) { o.stage = PT_Z1; return; }
    const float z2 = cam_coord(P2, 2, x);
    if (z2 <= 0) { o.stage = PT_Z2; return; }
    {
        const float sigmaSquare1 = sigma2[l1];
        const float cx = cam_coord(P1, 0, x), cy = cam_coord(P1, 1, x);
        const float invz1 = (float)(1.0 / (double)z1);
        const float u1 = P1.fx * cx * invz1 + P1.cx, v1 = P1.fy * cy * invz1 + P1.cy;
        const float errX1 = u1 - x1, errY1 = v1 - y1;
        o.err1 = errX1 * errX1 + errY1 * errY1;
        if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaSquare1) { o.stage = PT_ERR1; return; }
    }
    {
        const float sigmaSquare2 = sigma2[l2];
        const float cx = cam_coord(P2, 0, x), cy = cam_coord(P2, 1, x);
        const float invz2 = (float)(1.0 / (double)z2);
        const float u2 = P2.fx * cx * invz2 + P2.cx, v2 = P2.fy * cy * invz2 + P2.cy;
        const float errX2 = u2 - x2, errY2 = v2 - y2;
        o.err2 = errX2 * errX2 + errY2 * errY2;
        if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaSquare2) { o.stage = PT_ERR2; return; }
    }
    const float dist1 = dist_to(x, P1.Ow), dist2 = dist_to(x, P2.Ow);
    if (dist1 == 0 || dist2 == 0) { o.stage = PT_DIST_ZERO; return; }
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = sf[l1] / sf[l2];
    o.ratio_dist = ratioDist; o.ratio_octave = ratioOctave;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) { o.stage = PT_SCALE; return; }
    o.stage = PT_CREATED;
    // UpdateNormalAndDepth (src/MapPoint.cc:353-375): normal = (0 + n1 / |n1|) + n2 / |n2|, then / 2
    float normal[3] = {0.f, 0.f, 0.f};
    NM_UNROLL
    for (int k = 0; k < 2; ++k) {
        const float* O = k == 0 ? P1.Ow : P2.Ow;
        const float normali[3] = {x[0] - O[0], x[1] - O[1], x[2] - O[2]};
        const double alpha = 1.0 / rc::norm3(normali);
        NM_UNROLL
        for (int i = 0; i < 3; ++i) normal[i] = normal[i] + rc::scale_f(normali[i], alpha);
    }
    const float dist = dist_to(x, P1.Ow);
    const float levelScaleFactor = sf[l1];
    o.max_dist = dist * levelScaleFactor;
    o.min_dist = o.max_dist / sf[nlevels - 1];
    NM_UNROLL
    for (int i = 0; i < 3; ++i) { o.x3d[i] = x[i]; o.normal[i] = rc::scale_f(normal[i], 1.0 / 2.0); }
}

// Eigen's Vector3d::norm()
NM_FN double norm3d(const double v[3]) { return __builtin_sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])); }

// :1009-1148 for one match of key line 1 (endpoints e1 = start x, y, end x, y; function f1; octave1) with key line 2 (e2, f2) of the neighbour, then UpdateAverageDir of the new
// line.  medianDepthKF2: pKF2->ComputeSceneMedianDepth(2).  The GetMapLine filter of src/LSDmatcher.cpp:403 is the caller's (LN_NOT_FREE is decided before this is called)
template <class W>
NM_FN void line_row(const sslam_kf_pose& P1, const sslam_kf_pose& P2, const float e1[4], const double f1[3], int octave1, const float e2[4], const double f2[3],
                    float medianDepthKF2, const float* sf, int nlevels, W& w, LineOut& o) {
    NM_UNROLL
    for (int i = 0; i < 3; ++i) { o.s3d[i] = o.e3d[i] = 0.f; o.normal[i] = 0.0; }
    NM_UNROLL
    for (int i = 0; i < 4; ++i) o.shom[i] = o.ehom[i] = 0.f;
    o.max_dist = o.min_dist = 0.f;
    NM_UNROLL
    for (int i = 0; i < 5; ++i) o.ratio[i] = 0.f;
    const float cx1 = P1.cx, cy1 = P1.cy, invfx1 = P1.invfx, invfy1 = P1.invfy;
    const float klF1[3] = {(float)f1[0], (float)f1[1], (float)f1[2]}, klF2[3] = {(float)f2[0], (float)f2[1], (float)f2[2]};
    const float StartC1[3] = {(e1[0] - cx1) * invfx1, (e1[1] - cy1) * invfy1, 1.f};
    const float EndC1[3] = {(e1[2] - cx1) * invfx1, (e1[3] - cy1) * invfy1, 1.f};
    const float StartC2[3] = {(e2[0] - cx1) * invfx1, (e2[1] - cy1) * invfy1, 1.f};      // cx1 ...: :1032-1035
    const float EndC2[3] = {(e2[2] - cx1) * invfx1, (e2[3] - cy1) * invfy1, 1.f};
    float MidC1[3], MidC2[3];
    NM_UNROLL
    for (int i = 0; i < 3; ++i) { MidC1[i] = rc::scale_f(StartC1[i] + EndC1[i], 1.0 / 2.0); MidC2[i] = rc::scale_f(StartC2[i] + EndC2[i], 1.0 / 2.0); }
    const float cosParallaxRays = cos_rays(P1, MidC1, P2, MidC2);
    o.cosv = cosParallaxRays;
    const float cosParallaxStereo = cosParallaxRays + 1;
    float K1[9], K2[9], T1[12], T2[12], M1[12], M2[12];
    rc::cam_matrix(rc::Cam{P1.fx, P1.fy, P1.cx, P1.cy}, K1);
    rc::cam_matrix(rc::Cam{P2.fx, P2.fy, P2.cx, P2.cy}, K2);
    tcw_of(P1, T1);
    tcw_of(P2, T2);
    rc::gemm<3, 3, 4>(K1, T1, M1);
    rc::gemm<3, 3, 4>(K2, T2, M2);
    if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && cosParallaxRays < 0.98)) { o.stage = LN_PARALLAX; return; }
    float A[16], s[3], e[3];
    rc::gemm<1, 3, 4>(klF1, M1, A);
    rc::gemm<1, 3, 4>(klF2, M2, A + 4);
    NM_UNROLL
    for (int j = 0; j < 4; ++j) { A[8 + j] = StartC1[0] * T1[8 + j] - T1[j]; A[12 + j] = StartC1[1] * T1[8 + j] - T1[4 + j]; }
    if (!solve_point(w, A, o.shom, s)) { o.stage = LN_S_W_ZERO; return; }
    NM_UNROLL
    for (int j = 0; j < 4; ++j) { A[8 + j] = EndC1[0] * T1[8 + j] - T1[j]; A[12 + j] = EndC1[1] * T1[8 + j] - T1[4 + j]; }
    if (!solve_point(w, A, o.ehom, e)) { o.stage = LN_E_W_ZERO; return; }
    const float ratio1 = dist_to(s, P1.Ow) / medianDepthKF2;
    o.ratio[0] = ratio1;
    if (ratio1 < 0.3) { o.stage = LN_RATIO1; return; }
    const float ratio2 = dist_to(s, P2.Ow) / medianDepthKF2;
    o.ratio[1] = ratio2;
    if (ratio2 < 0.3) { o.stage = LN_RATIO2; return; }
    const float ratio3 = dist_to(e, s) / medianDepthKF2;
    o.ratio[2] = ratio3;
    if (ratio3 > 0.61) { o.stage = LN_RATIO3; return; }
    const float ratio4 = dist_to(e, P1.Ow) / medianDepthKF2;
    o.ratio[3] = ratio4;
    if (ratio4 < 0.3) { o.stage = LN_RATIO4; return; }
    const float ratio5 = dist_to(e, P2.Ow) / medianDepthKF2;
    o.ratio[4] = ratio5;
    if (ratio5 < 0.3) { o.stage = LN_RATIO5; return; }
    if (cam_coord(P1, 2, s) <= 0) { o.stage = LN_SZC1; return; }
    if (cam_coord(P2, 2, s) <= 0) { o.stage = LN_SZC2; return; }
    if (cam_coord(P1, 2, e) <= 0) { o.stage = LN_EZC1; return; }
    if (cam_coord(P2, 2, e) <= 0) { o.stage = LN_EZC2; return; }
    o.stage = LN_CREATED;
    // UpdateAverageDir (src/MapLine.cpp:343-371) on mWorldPos = the six floats widened (:1151-1152)
    double middlePos[3], normal[3] = {0.0, 0.0, 0.0};
    NM_UNROLL
    for (int i = 0; i < 3; ++i) middlePos[i] = 0.5 * ((double)s[i] + (double)e[i]);
    NM_UNROLL
    for (int k = 0; k < 2; ++k) {
        const float* O = k == 0 ? P1.Ow : P2.Ow;
        const double normali[3] = {middlePos[0] - (double)O[0], middlePos[1] - (double)O[1], middlePos[2] - (double)O[2]};
        const double n = norm3d(normali);
        NM_UNROLL
        for (int i = 0; i < 3; ++i) normal[i] = normal[i] + normali[i] / n;
    }
    float MP[3];
    NM_UNROLL
    for (int i = 0; i < 3; ++i) MP[i] = rc::scale_f(s[i] + e[i], 0.5);
    const float dist = dist_to(MP, P1.Ow);
    const float levelScaleFactor = sf[clamp_level(octave1, nlevels)];
    o.max_dist = dist * levelScaleFactor;
    o.min_dist = o.max_dist / sf[nlevels - 1];
    NM_UNROLL
    for (int i = 0; i < 3; ++i) { o.s3d[i] = s[i]; o.e3d[i] = e[i]; o.normal[i] = normal[i] / 2.0; }
}

}  // namespace nm
}  // namespace sslam
