// Frame::UndistortKeyPoints and Frame::ComputeImageBounds (src/Frame.cc:483-543) -- the last per-frame step of Frame::Frame that ran on the
// host.  One lane per keypoint row; the arithmetic of one point is camera.h's, which the host bounds function shares.
#include "common.h"
#include "camera.h"
#include <climits>

using namespace sslam;

namespace {
// rows [f*cap, f*cap + count_f) of kp -> the same rows of out, x / y undistorted (UNDISTORT) or copied (k1 == 0: mvKeysUn = mvKeys).  A lane
// reads its whole 28-byte record before it writes it, so out == kp is safe; rows at or past a frame's count are not touched.
template <bool UNDISTORT>
__global__ __launch_bounds__(256) void k_undistort_kp(const sslam_keypoint* kp, const int32_t* __restrict__ counts, int n, int cap, unsigned rows,
                                                      sslam_keypoint* out, sslam_camera cam) {
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= rows) return;
    const unsigned f = r / (unsigned)cap;
    const int j = (int)(r - f * (unsigned)cap);
    if (j >= (counts ? counts[f] : n)) return;
    sslam_keypoint k = kp[r];
    if (UNDISTORT) undistort_point(cam, k.x, k.y, k.x, k.y);
    out[r] = k;
}

bool camera_ok(const sslam_camera* cam) {
    return cam && cam->fx != 0.0f && cam->fy != 0.0f;
}
}  // namespace

int sslam::undistort_launch(sslam_ctx* ctx, const sslam_camera& cam, const sslam_keypoint* d_kp, const int32_t* d_counts, int n, int nframes, int cap,
                            sslam_keypoint* d_kp_un, void* stream) {
    const unsigned rows = (unsigned)nframes * (unsigned)cap;
    if (rows == 0) return SSLAM_OK;
    hipStream_t st = pick(ctx, stream);
    const dim3 grid((rows + 255) / 256);
    sslam::ProfScope _ps(ctx, "k_undistort_kp", st);
    if (cam.k1 == 0.0f) hipLaunchKernelGGL(k_undistort_kp<false>, grid, dim3(256), 0, st, d_kp, d_counts, n, cap, rows, d_kp_un, cam);
    else hipLaunchKernelGGL(k_undistort_kp<true>, grid, dim3(256), 0, st, d_kp, d_counts, n, cap, rows, d_kp_un, cam);
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

extern "C" int sslam_camera_image_bounds(const sslam_camera* cam, int w, int h, float bounds_out[4]) {
    if (!camera_ok(cam) || !bounds_out || w < 0 || h < 0) { set_error("sslam_camera_image_bounds: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (cam->k1 == 0.0f) {           // the reference tests only k1 (src/Frame.cc:517)
        bounds_out[0] = 0.0f; bounds_out[1] = (float)w; bounds_out[2] = 0.0f; bounds_out[3] = (float)h;
        return SSLAM_OK;
    }
    const float cu[4] = {0.0f, (float)w, 0.0f, (float)w}, cv[4] = {0.0f, 0.0f, (float)h, (float)h};
    float x[4], y[4];
    for (int i = 0; i < 4; ++i) undistort_point(*cam, cu[i], cv[i], x[i], y[i]);
    auto mn = [](float a, float b) { return b < a ? b : a; };      // std::min / std::max (:529-532)
    auto mx = [](float a, float b) { return a < b ? b : a; };
    bounds_out[0] = mn(x[0], x[2]); bounds_out[1] = mx(x[1], x[3]);
    bounds_out[2] = mn(y[0], y[1]); bounds_out[3] = mx(y[2], y[3]);
    return SSLAM_OK;
}

extern "C" int sslam_undistort_keypoints(sslam_ctx* ctx, const sslam_camera* cam, const sslam_keypoint* kp, int n, sslam_keypoint* kp_un) {
    if (!ctx || !camera_ok(cam) || n < 0 || (n > 0 && (!kp || !kp_un))) { set_error("sslam_undistort_keypoints: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (n == 0) return SSLAM_OK;
    if (cam->k1 == 0.0f) {           // mvKeysUn = mvKeys (src/Frame.cc:485-489)
        if (kp_un != kp) std::memmove(kp_un, kp, sizeof(sslam_keypoint) * (size_t)n);
        return SSLAM_OK;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->camKp.ensure(sizeof(sslam_keypoint) * (size_t)n))) return rc;
    sslam_keypoint* d = ctx->camKp.as<sslam_keypoint>();
    SSLAM_HIP(hipMemcpyAsync(d, kp, sizeof(sslam_keypoint) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = undistort_launch(ctx, *cam, d, nullptr, n, 1, n, d, ctx->stream))) return rc;
    SSLAM_HIP(hipMemcpyAsync(kp_un, d, sizeof(sslam_keypoint) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SSLAM_HIP(hipStreamSynchronize(ctx->stream));
    return SSLAM_OK;
}

extern "C" int sslam_undistort_keypoints_batch_dev(sslam_ctx* ctx, const sslam_camera* cam, const sslam_keypoint* d_kp, const int32_t* d_counts,
                                                   int nframes, int cap, sslam_keypoint* d_kp_un, void* stream) {
    if (!ctx || !camera_ok(cam) || nframes < 0 || cap <= 0 || (long long)nframes * cap > INT_MAX || (nframes > 0 && (!d_kp || !d_counts || !d_kp_un))) {
        set_error("sslam_undistort_keypoints_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (nframes == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    return undistort_launch(ctx, *cam, d_kp, d_counts, 0, nframes, cap, d_kp_un, stream);
}
