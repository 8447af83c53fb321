// Drop-in for the colour conversion at the top of Tracking::GrabImageMonocularWithPL (src/Tracking.cc:146-161):
//     mImGray = im;
//     if (mImGray.channels() == 3) cvtColor(mImGray, mImGray, mbRGB ? CV_RGB2GRAY : CV_BGR2GRAY);
//     else if (mImGray.channels() == 4) cvtColor(mImGray, mImGray, mbRGB ? CV_RGBA2GRAY : CV_BGRA2GRAY);
// becomes one line:
//     sslam_shim::GrabGray(im, mbRGB, mImGray);
// Header-only, like shim/FrameCamera.h, whose per-process device context it shares.  The conversion (DESIGN.md decision D14) runs on the GPU
// through sslam_gray_from_color.  mbRGB is applied to the bytes of the cv::Mat as they are, exactly as the reference does: imread gives BGR
// bytes, and with Camera.RGB: 1 (the shipped configurations) the reference converts them as RGB.  A drop-in caller gets the reference's gray
// bytes only by keeping that quirk.
#pragma once
#include <stdexcept>
#include <string>
#include "FrameCamera.h"

namespace sslam_shim
{
// mImGray of Tracking::GrabImageMonocularWithPL: 1-channel input is shared, not copied (mImGray = im); 3 / 4 channels are converted into a
// new 8-bit matrix.  gray may be im itself.
inline void GrabGray(const cv::Mat &im, bool bRGB, cv::Mat &gray)
{
    const int cn = im.channels();
    if (cn != 3 && cn != 4) { gray = im; return; }
    const int format = cn == 3 ? (bRGB ? SSLAM_PIX_RGB : SSLAM_PIX_BGR) : (bRGB ? SSLAM_PIX_RGBA : SSLAM_PIX_BGRA);
    cv::Mat out(im.rows, im.cols, CV_8U);
    const int rc = sslam_gray_from_color(CameraContext(), format, im.ptr<uint8_t>(0), im.cols, im.rows, (size_t)im.step, out.ptr<uint8_t>(0), (size_t)out.step);
    if (rc != SSLAM_OK) throw std::runtime_error(std::string(sslam_status_str(rc)) + ": " + sslam_last_error());
    gray = out;
}
}  // namespace sslam_shim
