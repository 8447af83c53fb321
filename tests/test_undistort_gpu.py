"""GPU: Frame::UndistortKeyPoints / Frame::ComputeImageBounds (src/Frame.cc:483-543) on the device -- the single-frame and batch entry points
against the fp64 restatement (tests/undistort_ref.py) bit for bit, the frame handle of an extractor with a camera, the host-buffer batch with
undistortion (sslam_frontend_batch_match_camera) against sslam_frontend_batch_match and the oracle, and the C++ drop-in shim/FrameCamera.h."""
import os, subprocess
import numpy as np
import pytest
import torch
import pkg
import undistort_ref as ur
from synth import synth_frame, warp_prev

pytestmark = pytest.mark.gpu

DISTORTED = ("tum_fr1", "tum_fr2", "euroc", "strong")
OTHER = ("size", "angle", "response", "octave", "class_id")


def _camera(fe, model):
    return fe.Camera(*[float(v) for v in ur.camera_params(model)])


def _random_keypoints(fe, rng, n, w, h):
    kp = np.zeros(n, fe.KP_DTYPE)
    kp["x"] = rng.uniform(-50, w + 50, n).astype(np.float32); kp["y"] = rng.uniform(-50, h + 50, n).astype(np.float32)
    kp["size"] = 31.0; kp["angle"] = rng.uniform(0, 360, n).astype(np.float32); kp["response"] = rng.uniform(0, 100, n).astype(np.float32)
    kp["octave"] = rng.integers(0, 8, n); kp["class_id"] = -1
    kp["x"][:4] = [0, w, 0, w]; kp["y"][:4] = [0, 0, h, h]
    return kp


def _assert_undistorted(fe, model, kp, got):
    """x / y equal the restatement's float32 bit patterns, the other five fields are byte-equal; k1 == 0 is a byte-equal copy"""
    want = ur.undistort_keypoints(ur.camera_params(model), kp)
    assert got.shape == kp.shape
    np.testing.assert_array_equal(got.view(np.uint8).reshape(-1, 28), want.view(np.uint8).reshape(-1, 28))
    for f in OTHER:
        np.testing.assert_array_equal(got[f].view(np.uint32), kp[f].view(np.uint32))
    if ur.camera_params(model)[4] == 0:
        np.testing.assert_array_equal(got.view(np.uint8), kp.view(np.uint8))


@pytest.mark.parametrize("model", sorted(ur.MODELS))
def test_single_frame_undistortion(fe, ctx, model):
    w, h = ur.MODELS[model][:2]
    cam = _camera(fe, model)
    ex = fe.OrbExtractor(ctx, 1000)
    kp, _ = ex(synth_frame(4100, w, h))
    assert len(kp) > 500
    _assert_undistorted(fe, model, kp, ctx.undistort_keypoints(cam, kp))
    rnd = _random_keypoints(fe, np.random.default_rng(5), 3001, w, h)
    got = ctx.undistort_keypoints(cam, rnd)
    _assert_undistorted(fe, model, rnd, got)
    if model in DISTORTED:
        assert np.abs(got["x"] - rnd["x"]).max() > 5.0
    assert len(ctx.undistort_keypoints(cam, rnd[:0])) == 0          # n = 0
    ex.close()


@pytest.mark.parametrize("model", ["tum_fr1", "euroc", "k1_zero"])
def test_batch_undistortion(fe, ctx, model):
    """uneven counts over 7 frames of cap 333 (2 331 rows: not a multiple of the 256-lane workgroup); rows past a count keep their sentinel"""
    w, h = ur.MODELS[model][:2]
    cam = _camera(fe, model)
    nf, cap = 7, 333
    counts = np.array([333, 0, 17, 332, 1, 150, 64], np.int32)
    rng = np.random.default_rng(11)
    kp = _random_keypoints(fe, rng, nf * cap, w, h)
    d_kp = torch.from_numpy(kp.view(np.uint8).copy()).cuda()
    d_cnt = torch.from_numpy(counts).cuda()
    sentinel = np.frombuffer(bytes([0xA5, 0x5A, 0xC3, 0x3C]) * 7, np.uint8)
    d_out = torch.from_numpy(np.tile(sentinel, nf * cap)).cuda()
    ctx.undistort_keypoints_batch_dev(cam, d_kp, d_cnt, nf, cap, d_out)
    d_inplace = d_kp.clone()
    torch.cuda.synchronize()          # the clone runs on torch's stream, the call below on the context's
    ctx.undistort_keypoints_batch_dev(cam, d_inplace, d_cnt, nf, cap, d_inplace)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(fe.KP_DTYPE).reshape(nf, cap)
    inplace = d_inplace.cpu().numpy().view(fe.KP_DTYPE).reshape(nf, cap)
    kp2 = kp.reshape(nf, cap)
    for f in range(nf):
        c = counts[f]
        _assert_undistorted(fe, model, kp2[f, :c], out[f, :c])
        np.testing.assert_array_equal(inplace[f, :c].view(np.uint8), out[f, :c].view(np.uint8))
        np.testing.assert_array_equal(out[f, c:].view(np.uint8).reshape(-1), np.tile(sentinel, cap - c))
        np.testing.assert_array_equal(inplace[f, c:].view(np.uint8), kp2[f, c:].view(np.uint8))
    ctx.undistort_keypoints_batch_dev(cam, d_kp, d_cnt, 0, cap, d_out)          # no frames: nothing to do
    # the single-frame entry point gives the same rows
    np.testing.assert_array_equal(ctx.undistort_keypoints(cam, kp2[3, :counts[3]]).view(np.uint8), out[3, :counts[3]].view(np.uint8))


@pytest.mark.parametrize("model", sorted(ur.MODELS))
def test_device_corners_reproduce_the_bounds(fe, ctx, model):
    w, h = ur.MODELS[model][:2]
    cam = _camera(fe, model)
    b = fe.camera_image_bounds(cam, w, h)
    c = ctx.undistort_keypoints(cam, _random_keypoints(fe, np.random.default_rng(1), 4, w, h))
    mn = lambda a, b_: b_ if b_ < a else a
    mx = lambda a, b_: b_ if a < b_ else a
    got = (mn(c["x"][0], c["x"][2]), mx(c["x"][1], c["x"][3]), mn(c["y"][0], c["y"][1]), mx(c["y"][2], c["y"][3]))
    if ur.camera_params(model)[4] == 0:
        got = (np.float32(0), np.float32(w), np.float32(0), np.float32(h))
    assert np.array(got, np.float32).view(np.uint32).tolist() == np.array(b, np.float32).view(np.uint32).tolist()


def _proj_queries(fe, rng, kp, mode, scales):
    """one projection query per keypoint of the previous frame, a few pixels off (SearchLocalPoints / TrackWithMotionModel windows)"""
    n = len(kp)
    q = np.zeros(n, fe.PQ_DTYPE)
    q["u"] = kp["x"] + 3 + rng.normal(0, 1.5, n); q["v"] = kp["y"] - 2 + rng.normal(0, 1.5, n)
    o = kp["octave"]
    q["radius"] = (15 if mode == 1 else 4 * 3) * scales[o]
    q["min_level"] = o - 1; q["max_level"] = o + 1 if mode == 1 else o
    q["angle"] = kp["angle"]
    q["valid"] = rng.random(n) < 0.95
    q["obs_positive"] = rng.random(n) < 0.9
    return q


@pytest.mark.parametrize("mode", [0, 1])
def test_frame_handle_holds_undistorted_keypoints(fe, ctx, mode):
    """with a camera, Frame(ctx, orb=...) is what a frame_upload of the restated mvKeysUn gives; without one (or after clearing it), mvKeys"""
    model = "tum_fr1"
    w, h = ur.MODELS[model][:2]
    cam = _camera(fe, model); P = ur.camera_params(model)
    bounds = fe.camera_image_bounds(cam, w, h)
    rng = np.random.default_rng(31 + mode)
    cur = synth_frame(2003); prev = warp_prev(cur)
    ex = fe.OrbExtractor(ctx, 1000)
    scales = ex.scales()[0]
    kp1, d1 = ex(prev)
    kpun1 = ur.undistort_keypoints(P, kp1)
    ex.set_camera(cam)
    kp2, d2 = ex(cur)
    kpun2 = ur.undistort_keypoints(P, kp2)
    fr = fe.Frame(ctx, orb=ex, bounds=bounds)
    up = ctx.frame_upload(0, kpun2, d2, bounds=bounds)
    q = _proj_queries(fe, rng, kpun1, mode, scales)
    occ = (rng.random(len(kp2)) < 0.05).astype(np.uint8)
    ea, en = up.search_by_projection(mode, q, d1, occ, 0.8, 100, True)
    a, n = fr.search_by_projection(mode, q, d1, occ, 0.8, 100, True)
    assert en > 50 and n == en
    np.testing.assert_array_equal(a, ea)
    raw = ctx.frame_upload(0, kp2, d2, bounds=bounds)
    ra, rn = raw.search_by_projection(mode, q, d1, occ, 0.8, 100, True)
    assert not np.array_equal(ra, ea)                   # the snapshot is not mvKeys
    ex.set_camera(None)
    kp3, _ = ex(cur)
    np.testing.assert_array_equal(kp3.view(np.uint8), kp2.view(np.uint8))       # sslam_orb_extract returns mvKeys either way
    plain = fe.Frame(ctx, orb=ex, bounds=bounds)
    pa, pn = plain.search_by_projection(mode, q, d1, occ, 0.8, 100, True)
    assert pn == rn
    np.testing.assert_array_equal(pa, ra)
    for f in (fr, up, raw, plain):
        f.close()
    ex.close()


def _sequence(n, w, h):
    base = synth_frame(8100, w, h)
    frames = [base]
    for i in range(1, n):
        frames.append(warp_prev(frames[-1], dx=2.0 + (i % 3), dy=-1.5, deg=0.7))
    return np.stack(frames)


@pytest.mark.parametrize("model", ["tum_fr1", "strong", "zero"])
def test_frontend_batch_match_camera(fe, ctx, oracle, model):
    """n = 8 frames of a warp_prev chain in chunks of 3 (the predecessor is carried over two chunk boundaries): the extraction half and the
    2-NN / line outputs equal sslam_frontend_batch_match byte for byte, kpun equals the restatement, and SearchForInitialization runs on
    mvKeysUn of both frames with the camera's bounds (the oracle's restatement of the reference body on the same inputs).  TUM fr1's bounds
    lie inside the 16-pixel border FAST never detects in, so the "strong" lens is the one whose undistorted keypoints leave the 64x48 grid"""
    w, h = 640, 480
    n, chunk = 8, 3
    cam = _camera(fe, model); P = ur.camera_params(model)
    bounds = fe.camera_image_bounds(cam, w, h)
    frames = _sequence(n, w, h)
    orb = fe.OrbExtractor(ctx, 1000); lines = fe.LineExtractor(ctx, 200)
    ref = fe.frontend_batch_alloc(n, orb.cap, 200); mref = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_match_raw(orb, lines, frames, ref, mref, chunk=chunk, bounds=bounds)
    out = fe.frontend_batch_camera_alloc(n, orb.cap, 200); mout = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_match_camera_raw(orb, lines, cam, frames, out, mout, chunk=chunk)
    kp, desc, nk, kl, ld, fn, nl, kpun = out
    rkp, rdesc, rnk, rkl, rld, rfn, rnl = ref
    m12, nm, ki, kd, lp, nlp = mout
    rm12, rnm, rki, rkd, rlp, rnlp = mref
    np.testing.assert_array_equal(nk, rnk); np.testing.assert_array_equal(nl, rnl)
    outside = via_un = 0
    for i in range(n):
        c, cl = nk[i], nl[i]
        np.testing.assert_array_equal(kp[i, :c].view(np.uint8), rkp[i, :c].view(np.uint8))
        np.testing.assert_array_equal(desc[i, :c], rdesc[i, :c])
        np.testing.assert_array_equal(kl[i, :cl].view(np.uint8), rkl[i, :cl].view(np.uint8))
        np.testing.assert_array_equal(ld[i, :cl], rld[i, :cl]); np.testing.assert_array_equal(fn[i, :cl], rfn[i, :cl])
        np.testing.assert_array_equal(kpun[i, :c].view(np.uint8), ur.undistort_keypoints(P, kp[i, :c]).view(np.uint8))
        x, y = kpun[i, :c]["x"], kpun[i, :c]["y"]
        outside += int(((x < bounds[0]) | (x >= bounds[1]) | (y < bounds[2]) | (y >= bounds[3])).sum())
        if i == 0:
            assert nm[0] == 0 and nlp[0] == 0
            continue
        c1 = nk[i - 1]
        np.testing.assert_array_equal(ki[i, :c1], rki[i, :c1]); np.testing.assert_array_equal(kd[i, :c1], rkd[i, :c1])
        assert nlp[i] == rnlp[i]
        np.testing.assert_array_equal(lp[i, :nlp[i]], rlp[i, :nlp[i]])
        kpun1, kpun2 = kpun[i - 1, :c1], kpun[i, :c]
        pm = np.stack([kpun1["x"], kpun1["y"]], axis=1).astype(np.float32)
        om12, _, onm = oracle.search_for_initialization(kpun1, desc[i - 1, :c1], kpun2, desc[i, :c], pm, 100, 0.9, True, bounds)
        assert nm[i] == onm, i
        np.testing.assert_array_equal(m12[i, :c1], om12)
        t = m12[i, :c1][m12[i, :c1] >= 0]                 # matched keypoints of frame i whose mvKeys lie outside the bounds: in the grid only through mvKeysUn
        rx, ry = kp[i, t]["x"], kp[i, t]["y"]
        via_un += int(((rx < bounds[0]) | (rx >= bounds[1]) | (ry < bounds[2]) | (ry >= bounds[3])).sum())
        if model == "zero":                               # no distortion: every output is sslam_frontend_batch_match's
            assert nm[i] == rnm[i]
            np.testing.assert_array_equal(m12[i, :c1], rm12[i, :c1])
    if model == "zero":
        assert outside == 0
    else:
        if model == "strong":
            assert outside > 20                           # keypoints outside the bounds, i.e. at the edge of or off the grid (Frame::PosInGrid, src/Frame.cc:462-472) ...
            assert via_un > 20                            # ... and matches the raw coordinates could not have given
        assert (nm[1:] > 10).all()
    # no match stage: extraction + undistortion only
    out2 = fe.frontend_batch_camera_alloc(n, orb.cap, 200)
    fe.frontend_batch_match_camera_raw(orb, lines, cam, frames, out2, None, chunk=5)
    np.testing.assert_array_equal(out2[2], nk)
    for i in range(n):
        np.testing.assert_array_equal(out2[7][i, :nk[i]].view(np.uint8), kpun[i, :nk[i]].view(np.uint8))
    orb.close(); lines.close()


CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "FrameCamera.h"
struct Frame {            // the members Frame::UndistortKeyPoints / ComputeImageBounds read and write (include/Frame.h)
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    cv::Mat mK, mDistCoef;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    void UndistortKeyPoints() { sslam_shim::UndistortKeyPoints(*this); }
    void ComputeImageBounds(const cv::Mat &imLeft) { sslam_shim::ComputeImageBounds(*this, imLeft); }
};
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
int main(int argc, char **argv) {
    // argv: keypoints.bin out.bin w h fx fy cx cy k1 k2 p1 p2 k3
    FILE *f = std::fopen(argv[1], "rb");
    std::fseek(f, 0, SEEK_END); const long bytes = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    Frame F; F.N = (int)(bytes / sizeof(cv::KeyPoint)); F.mvKeys.resize(F.N);
    if (F.N && std::fread(F.mvKeys.data(), sizeof(cv::KeyPoint), F.N, f) != (size_t)F.N) return 2;
    std::fclose(f);
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
    float p[9]; for (int i = 0; i < 9; ++i) p[i] = std::strtof(argv[5 + i], nullptr);
    F.mK = cv::Mat(3, 3, CV_32F); for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) F.mK.at<float>(r, c) = r == c ? 1.f : 0.f;
    F.mK.at<float>(0, 0) = p[0]; F.mK.at<float>(1, 1) = p[1]; F.mK.at<float>(0, 2) = p[2]; F.mK.at<float>(1, 2) = p[3];
    const int nd = p[8] != 0 ? 5 : 4;          // src/Tracking.cc:63-72
    F.mDistCoef = cv::Mat(nd, 1, CV_32F); for (int i = 0; i < nd; ++i) F.mDistCoef.at<float>(i) = p[4 + i];
    F.UndistortKeyPoints();
    cv::Mat img(h, w, CV_8U);
    F.ComputeImageBounds(img);
    FILE *o = std::fopen(argv[2], "wb");
    const float b[4] = {Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY};
    std::fwrite(b, sizeof(float), 4, o);
    if (F.N) std::fwrite(F.mvKeysUn.data(), sizeof(cv::KeyPoint), F.mvKeysUn.size(), o);
    std::fclose(o);
    return F.mvKeysUn.size() == (size_t)F.N ? 0 : 3;
}
"""


def test_cpp_frame_camera_dropin(fe, ctx, tmp_path):
    """shim/FrameCamera.h: the reference's two member bodies as one-line forwards, on a stand-in Frame; mvKeysUn and the bounds equal the C
    ABI's (tests above) for every model"""
    builder = pkg.builder()
    builder.build(force=False, verbose=False)
    src = tmp_path / "frame_camera.cpp"; src.write_text(CPP)
    exe = tmp_path / "frame_camera"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + builder.SHIM, str(src), "-L" + builder.LIBDIR, "-lsslam_frontend",
                           "-Wl,-rpath," + builder.LIBDIR, "-o", str(exe)])
    ex = fe.OrbExtractor(ctx, 1000)
    for model in sorted(ur.MODELS):
        w, h = ur.MODELS[model][:2]
        cam = _camera(fe, model)
        kp, _ = ex(synth_frame(4100, w, h))
        kp = np.concatenate([kp, _random_keypoints(fe, np.random.default_rng(2), 100, w, h)])
        kin = tmp_path / "kp.bin"; kout = tmp_path / "out.bin"
        kp.tofile(kin)
        r = subprocess.run([str(exe), str(kin), str(kout), str(w), str(h)] + [repr(float(v)) for v in ur.camera_params(model)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(kout, np.uint8)
        b = raw[:16].view(np.float32); kpun = raw[16:].view(fe.KP_DTYPE)
        assert b.view(np.uint32).tolist() == np.array(fe.camera_image_bounds(cam, w, h), np.float32).view(np.uint32).tolist(), model
        np.testing.assert_array_equal(kpun.view(np.uint8), ctx.undistort_keypoints(cam, kp).view(np.uint8))
    ex.close()
