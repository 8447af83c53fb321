// The colour conversion at the top of Tracking::GrabImageMonocularWithPL (src/Tracking.cc:146-161), shared by the device kernel (color.hip)
// and the host batch (batch.hip): OpenCV 3.4's 8-bit RGB2Gray<uchar> in its fixed-point table form (DESIGN.md decision D14).  The three
// coefficients sum to 1 << 14, so R = G = B = g gives g back for every g.
#pragma once
#include "../../include/sslam_frontend.h"

#ifdef __HIPCC__
#define SSLAM_HD __host__ __device__
#else
#define SSLAM_HD
#endif

namespace sslam {

// gray = (4899 R + 9617 G + 1868 B + 8192) >> 14, exact in 32-bit unsigned arithmetic (the largest sum is 255 * 16384 + 8192)
SSLAM_HD inline unsigned gray_from_rgb(unsigned r, unsigned g, unsigned b) {
    return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;
}

// bytes per pixel of an SSLAM_PIX_* format; 0 for an unknown one
SSLAM_HD inline int pix_channels(int format) {
    return format == SSLAM_PIX_GRAY ? 1 : (format == SSLAM_PIX_RGB || format == SSLAM_PIX_BGR) ? 3 : (format == SSLAM_PIX_RGBA || format == SSLAM_PIX_BGRA) ? 4 : 0;
}

// color.hip: enqueue the conversion of frames [0, nframes) on `stream` (k_gray_from_color; SSLAM_PIX_GRAY is a pitched copy).  The callers
// have checked the arguments (gray_layout_ok below).
int gray_from_color_launch(sslam_ctx* ctx, int format, const uint8_t* d_src, int w, int h, size_t pitch, size_t image_stride, int nframes,
                           uint8_t* d_gray, size_t gray_pitch, size_t gray_image_stride, void* stream);

// the layout rules of sslam_gray_from_color*: a known format, rows of at least w * cn bytes, frames that do not overlap, and a frame whose
// 16-pixel chunks fit the launch's 32-bit lane index.  image_stride is not read for a single frame.
inline bool gray_layout_ok(int format, int w, int h, size_t pitch, size_t image_stride, int nframes) {
    const int cn = pix_channels(format);
    if (cn == 0 || w <= 0 || h <= 0 || nframes < 0 || pitch < (size_t)w * cn) return false;
    if ((size_t)h * (((size_t)w + 15) / 16) > (size_t)1 << 31) return false;
    return nframes <= 1 || image_stride >= pitch * (size_t)(h - 1) + (size_t)w * cn;
}

}  // namespace sslam
