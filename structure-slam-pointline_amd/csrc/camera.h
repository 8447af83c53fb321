// The camera model of Frame::UndistortKeyPoints / Frame::ComputeImageBounds (src/Frame.cc:483-543), shared by the device kernel
// (camera.hip) and the host bounds function: one point through cv::undistortPoints(src, dst, K, D, noArray(), K) -- OpenCV 3.4's
// cvUndistortPoints, restated in fp64 (DESIGN.md decision D13).  Both sides are compiled with -ffp-contract=off -fno-fast-math
// (build.py): every product and sum below rounds on its own, left to right, and `/` is the correctly rounded division.
#pragma once
#include "../../include/sslam_frontend.h"

#ifdef __HIPCC__
#define SSLAM_HD __host__ __device__
#else
#define SSLAM_HD
#endif

namespace sslam {

// (u, v) -> (u', v').  K and D are the reference's CV_32F matrices (src/Tracking.cc:48-72), widened to double as OpenCV reads them;
// D = k1, k2, p1, p2, k3 and k[5..13] = 0 (rational, thin-prism and tilt terms absent).  The loop is OpenCV's fixed count of five
// iterations (no epsilon test); the tilt step (invMatTilt = I) and the projection through RR = P * R = K (ww = 1) are exact and
// are written out only where they are not the identity.
SSLAM_HD inline void undistort_point(const sslam_camera& cam, float u, float v, float& uo, float& vo) {
    const double fx = (double)cam.fx, fy = (double)cam.fy, cx = (double)cam.cx, cy = (double)cam.cy;
    const double ifx = 1. / fx, ify = 1. / fy;
    const double k[14] = {(double)cam.k1, (double)cam.k2, (double)cam.p1, (double)cam.p2, (double)cam.k3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double x = ((double)u - cx) * ifx, y = ((double)v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    uo = (float)(fx * x + 0 * y + cx);
    vo = (float)(0 * x + fy * y + cy);
}

// camera.hip: enqueue the undistortion of frames [0, nframes) of d_kp (rows [f*cap, f*cap + count)) into d_kp_un on `stream`; count =
// d_counts[f], or n for every frame when d_counts is NULL.  k1 == 0 launches the copy form.  The callers have checked the arguments.
int undistort_launch(sslam_ctx* ctx, const sslam_camera& cam, const sslam_keypoint* d_kp, const int32_t* d_counts, int n, int nframes, int cap,
                     sslam_keypoint* d_kp_un, void* stream);

}  // namespace sslam
