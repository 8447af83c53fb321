// RGB / BGR / RGBA / BGRA -> 8-bit gray (Tracking::GrabImageMonocularWithPL, src/Tracking.cc:146-161: cvtColor with CV_RGB2GRAY, CV_BGR2GRAY,
// CV_RGBA2GRAY or CV_BGRA2GRAY as mbRGB and the channel count say) -- the one per-pixel step of the front-end that ran outside the library.
// Purely memory-bound: one launch per batch, one lane per 16 output pixels of a row (frames x rows x chunks flattened).  A chunk whose source
// and destination rows start on 16 bytes reads its 16 * cn bytes with cn dwordx4 loads and writes one dwordx4; unaligned rows, odd pitches and
// the row tail take the byte path.  The arithmetic is color.h's, which the host side shares.
#include "common.h"
#include "color.h"
#include <climits>

using namespace sslam;

namespace {
// pixel i (0..15) of a 16-pixel chunk held as 16 * CN bytes in u[]: its gray value
template <int CN, bool BGR>
__device__ __forceinline__ unsigned chunk_gray(const unsigned* u, int i) {
    if (CN == 1) return (u[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    const int k = i * CN;      // byte offset of the pixel's first channel (compile-time after unrolling)
    const unsigned c0 = (u[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    const unsigned c1 = (u[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu;
    const unsigned c2 = (u[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 0xFFu;
    return BGR ? gray_from_rgb(c2, c1, c0) : gray_from_rgb(c0, c1, c2);
}

// lane t of the launch: frame t / (h * nchunk), row, 16-pixel chunk.  Reads stay inside [x0 * CN, min(x0 + 16, w) * CN) of the source row,
// writes inside [x0, min(x0 + 16, w)) of the destination row: nothing past a frame's last pixel is read, no output padding is written.
template <int CN, bool BGR>
__global__ __launch_bounds__(256) void k_gray_from_color(const uint8_t* __restrict__ src, size_t pitch, size_t image_stride, uint8_t* __restrict__ dst,
                                                         size_t gray_pitch, size_t gray_image_stride, int w, unsigned h, unsigned nchunk, unsigned total) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    const unsigned row = t / nchunk, j = t - row * nchunk;
    const unsigned f = row / h, y = row - f * h;
    const int x0 = (int)(j * 16u);
    const uint8_t* sp = src + f * image_stride + y * pitch + (size_t)x0 * CN;
    uint8_t* dp = dst + f * gray_image_stride + y * gray_pitch + x0;
    if (x0 + 16 <= w && (((uintptr_t)sp | (uintptr_t)dp) & 15) == 0) {
        unsigned u[4 * CN];
#pragma unroll
        for (int q = 0; q < CN; ++q) {
            const uint4 v = ((const uint4*)sp)[q];
            u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w;
        }
        unsigned o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = chunk_gray<CN, BGR>(u, 4 * q) | (chunk_gray<CN, BGR>(u, 4 * q + 1) << 8) | (chunk_gray<CN, BGR>(u, 4 * q + 2) << 16) |
                   (chunk_gray<CN, BGR>(u, 4 * q + 3) << 24);
        *(uint4*)dp = make_uint4(o[0], o[1], o[2], o[3]);
        return;
    }
    const int n = min(16, w - x0);
    for (int i = 0; i < n; ++i) {
        const uint8_t* p = sp + i * CN;
        dp[i] = (uint8_t)(CN == 1 ? p[0] : BGR ? gray_from_rgb(p[2], p[1], p[0]) : gray_from_rgb(p[0], p[1], p[2]));
    }
}

template <int CN, bool BGR>
void launch(const uint8_t* src, size_t pitch, size_t image_stride, uint8_t* dst, size_t gray_pitch, size_t gray_image_stride, int w, int h,
            unsigned nchunk, int frames, hipStream_t st) {
    const unsigned total = (unsigned)frames * (unsigned)h * nchunk;
    hipLaunchKernelGGL((k_gray_from_color<CN, BGR>), dim3((total + 255) / 256), dim3(256), 0, st, src, pitch, image_stride, dst, gray_pitch,
                       gray_image_stride, w, (unsigned)h, nchunk, total);
}
}  // namespace

int sslam::gray_from_color_launch(sslam_ctx* ctx, int format, const uint8_t* d_src, int w, int h, size_t pitch, size_t image_stride, int nframes,
                                  uint8_t* d_gray, size_t gray_pitch, size_t gray_image_stride, void* stream) {
    if (nframes == 0) return SSLAM_OK;
    hipStream_t st = pick(ctx, stream);
    const unsigned nchunk = (unsigned)((w + 15) / 16);
    const size_t perFrame = (size_t)h * nchunk;                        // <= 2^31 (gray_layout_ok)
    const int group = (int)std::min<size_t>((size_t)nframes, ((size_t)1 << 31) / perFrame);      // frames per launch: the lane index stays below 2^31
    sslam::ProfScope _ps(ctx, "k_gray_from_color", st);
    for (int f0 = 0; f0 < nframes; f0 += group) {
        const int fc = std::min(group, nframes - f0);
        const uint8_t* s = d_src + (size_t)f0 * image_stride;
        uint8_t* d = d_gray + (size_t)f0 * gray_image_stride;
        switch (format) {
            case SSLAM_PIX_GRAY: launch<1, false>(s, pitch, image_stride, d, gray_pitch, gray_image_stride, w, h, nchunk, fc, st); break;
            case SSLAM_PIX_RGB: launch<3, false>(s, pitch, image_stride, d, gray_pitch, gray_image_stride, w, h, nchunk, fc, st); break;
            case SSLAM_PIX_BGR: launch<3, true>(s, pitch, image_stride, d, gray_pitch, gray_image_stride, w, h, nchunk, fc, st); break;
            case SSLAM_PIX_RGBA: launch<4, false>(s, pitch, image_stride, d, gray_pitch, gray_image_stride, w, h, nchunk, fc, st); break;
            default: launch<4, true>(s, pitch, image_stride, d, gray_pitch, gray_image_stride, w, h, nchunk, fc, st); break;
        }
        SSLAM_HIP(hipGetLastError());
    }
    return SSLAM_OK;
}

extern "C" int sslam_gray_from_color(sslam_ctx* ctx, int format, const uint8_t* img, int w, int h, size_t stride, uint8_t* gray, size_t gray_stride) {
    if (!ctx || !img || !gray) { set_error("sslam_gray_from_color: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (!gray_layout_ok(format, w, h, stride, 0, 1)) {
        set_error("sslam_gray_from_color: invalid layout (format %d, %d x %d, stride %zu: an SSLAM_PIX_* format and stride >= w * channels)", format, w, h, stride);
        return SSLAM_ERR_INVALID;
    }
    if (gray_stride < (size_t)w) { set_error("sslam_gray_from_color: gray_stride %zu < w %d", gray_stride, w); return SSLAM_ERR_INVALID; }
    const size_t row = (size_t)w * pix_channels(format), fpx = (size_t)w * h;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->colorIn.ensure(row * h)) || (rc = ctx->colorGray.ensure(fpx))) return rc;
    // tight rows on the device: the 2-D copies read only the w * cn bytes of each source row and write only the w bytes of each gray row
    SSLAM_HIP(hipMemcpy2DAsync(ctx->colorIn.p, row, img, stride, row, h, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = gray_from_color_launch(ctx, format, ctx->colorIn.as<uint8_t>(), w, h, row, row * h, 1, ctx->colorGray.as<uint8_t>(), w, fpx, ctx->stream))) return rc;
    SSLAM_HIP(hipMemcpy2DAsync(gray, gray_stride, ctx->colorGray.p, w, w, h, hipMemcpyDeviceToHost, ctx->stream));
    SSLAM_HIP(hipStreamSynchronize(ctx->stream));
    return SSLAM_OK;
}

extern "C" int sslam_gray_from_color_batch_dev(sslam_ctx* ctx, int format, const uint8_t* d_src, int w, int h, size_t pitch, size_t image_stride,
                                               int nframes, uint8_t* d_gray, size_t gray_pitch, size_t gray_image_stride, void* stream) {
    if (!ctx || (nframes > 0 && (!d_src || !d_gray))) { set_error("sslam_gray_from_color_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (!gray_layout_ok(format, w, h, pitch, image_stride, nframes) || !gray_layout_ok(SSLAM_PIX_GRAY, w, h, gray_pitch, gray_image_stride, nframes)) {
        set_error("sslam_gray_from_color_batch_dev: invalid layout (format %d, %d x %d, pitch %zu, image_stride %zu, gray_pitch %zu, gray_image_stride %zu)",
                  format, w, h, pitch, image_stride, gray_pitch, gray_image_stride);
        return SSLAM_ERR_INVALID;
    }
    if (nframes == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    return gray_from_color_launch(ctx, format, d_src, w, h, pitch, image_stride, nframes, d_gray, gray_pitch, gray_image_stride, stream);
}
