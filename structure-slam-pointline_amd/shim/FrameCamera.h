// Drop-in bodies for Frame::UndistortKeyPoints and Frame::ComputeImageBounds (src/Frame.cc:483-543), the camera-model step of Frame::Frame
// (:95, :113).  Header-only, like shim/ORBmatcher.h: member templates over the frame type read exactly the members the reference bodies read
// -- mvKeys, N, mK (CV_32F 3x3), mDistCoef (CV_32F, 4 or 5 coefficients: src/Tracking.cc:48-72) -- and write mvKeysUn / mnMinX .. mnMaxY, so
// the two member bodies become one-line forwards:
//     void Frame::UndistortKeyPoints() { sslam_shim::UndistortKeyPoints(*this); }
//     void Frame::ComputeImageBounds(const cv::Mat &imLeft) { sslam_shim::ComputeImageBounds(*this, imLeft); }
// The undistortion (cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK), DESIGN.md decision D13) runs on the GPU through
// sslam_undistort_keypoints; the bounds are the library's host-only sslam_camera_image_bounds.  As in the reference, only k1 decides whether
// anything is undistorted.
#pragma once
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>
#include "cv_min.h"
#include "../../include/sslam_frontend.h"

namespace sslam_shim
{
// K = fx, fy, cx, cy and DistCoef = k1, k2, p1, p2 [, k3] as sslam_camera (k3 = 0 when DistCoef holds four coefficients)
inline sslam_camera CameraFromMats(const cv::Mat &K, const cv::Mat &DistCoef)
{
    sslam_camera c{};
    c.fx = K.at<float>(0, 0); c.fy = K.at<float>(1, 1); c.cx = K.at<float>(0, 2); c.cy = K.at<float>(1, 2);
    float *d[5] = {&c.k1, &c.k2, &c.p1, &c.p2, &c.k3};
    const float *src = DistCoef.ptr<float>(0);            // a column (4x1 / 5x1) or row vector, continuous
    const int nd = DistCoef.rows * DistCoef.cols;
    for (int i = 0; i < nd && i < 5; ++i) *d[i] = src[i];
    return c;
}

// The device context of these two calls: one per process, created on first use on device SSLAM_DEVICE (default 0).  No CPU fallback.
inline sslam_ctx *CameraContext()
{
    static sslam_ctx *ctx = [] {
        sslam_ctx *c = nullptr;
        const char *d = std::getenv("SSLAM_DEVICE");
        const int rc = sslam_ctx_create(d ? std::atoi(d) : 0, &c);
        if (rc != SSLAM_OK) throw std::runtime_error(std::string("sslam front-end: ") + sslam_status_str(rc) + ": " + sslam_last_error());
        return c;
    }();
    return ctx;
}

// Frame::UndistortKeyPoints (src/Frame.cc:483-513): mvKeysUn = mvKeys with pt undistorted; size, angle, response, octave, class_id unchanged
template <class FrameT>
void UndistortKeyPoints(FrameT &F)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(sslam_keypoint), "cv::KeyPoint layout");
    const sslam_camera cam = CameraFromMats(F.mK, F.mDistCoef);
    if (cam.k1 == 0.0f) { F.mvKeysUn = F.mvKeys; return; }
    F.mvKeysUn.resize(F.N);
    const int rc = sslam_undistort_keypoints(CameraContext(), &cam, reinterpret_cast<const sslam_keypoint *>(F.mvKeys.data()), F.N,
                                             reinterpret_cast<sslam_keypoint *>(F.mvKeysUn.data()));
    if (rc != SSLAM_OK) throw std::runtime_error(std::string(sslam_status_str(rc)) + ": " + sslam_last_error());
}

// Frame::ComputeImageBounds (src/Frame.cc:515-543): mnMinX, mnMaxX, mnMinY, mnMaxY from the undistorted image corners
template <class FrameT>
void ComputeImageBounds(FrameT &F, const cv::Mat &imLeft)
{
    const sslam_camera cam = CameraFromMats(F.mK, F.mDistCoef);
    float b[4];
    const int rc = sslam_camera_image_bounds(&cam, imLeft.cols, imLeft.rows, b);
    if (rc != SSLAM_OK) throw std::runtime_error(std::string(sslam_status_str(rc)) + ": " + sslam_last_error());
    F.mnMinX = b[0]; F.mnMaxX = b[1]; F.mnMinY = b[2]; F.mnMaxY = b[3];
}
}  // namespace sslam_shim
