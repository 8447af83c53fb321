"""GPU: colour camera frames to gray on the device (Tracking::GrabImageMonocularWithPL, src/Tracking.cc:146-161; DESIGN.md decision D14) --
k_gray_from_color against the numpy restatement tests/color_ref.py bit for bit (every 24-bit triple, odd layouts, guard bytes), the host
batch with colour input against the gray entry points on the restated gray frames, FrontendBatch on colour tensors, and the C++ drop-in
shim/TrackingImage.h."""
import ctypes as C
import functools, os, subprocess
import numpy as np
import pytest
import torch
import pkg
import color_ref as cr
import undistort_ref as ur
from synth import synth_frame, warp_prev

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()


# ---- 1. arithmetic ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _all_triples():
    rgb = cr.all_triples_rgb()
    return rgb, cr.to_gray(rgb, cr.PIX_RGB)


@pytest.mark.parametrize("fmt", cr.COLOUR, ids=lambda f: cr.NAMES[f])
def test_every_rgb_triple(fe, ctx, fmt):
    """all 2^24 RGB triples as one 4096 x 4096 frame (RGBA / BGRA: a varying alpha) equal the restatement bit for bit"""
    rgb, want = _all_triples()
    alpha = (np.arange(4096 * 4096, dtype=np.uint32) * 2654435761 >> 24).astype(np.uint8).reshape(4096, 4096)
    img = cr.from_rgb(rgb, fmt, alpha)
    cn = cr.CHANNELS[fmt]
    d_src = _dev(img)
    d_gray = torch.empty(4096 * 4096, dtype=torch.uint8, device="cuda")
    ctx.gray_from_color_batch_dev(fmt, d_src, 4096, 4096, 4096 * cn, 4096 * 4096 * cn, 1, d_gray, 4096, 4096 * 4096)
    ctx.synchronize()
    got = d_gray.cpu().numpy().reshape(4096, 4096)
    np.testing.assert_array_equal(got, want)
    assert len(np.unique(got)) == 256


# ---- 2. layouts ------------------------------------------------------------------------------------------------------------------------

def _frames(rng, n, h, w, fmt):
    cn = cr.CHANNELS[fmt]
    return rng.integers(0, 256, (n, h, w) + ((cn,) if cn > 1 else ()), dtype=np.uint8)


@pytest.mark.parametrize("fmt", (cr.PIX_GRAY,) + cr.COLOUR, ids=lambda f: cr.NAMES[f])
@pytest.mark.parametrize("h", [1, 480])
@pytest.mark.parametrize("w", [1, 3, 15, 16, 17, 641, 1280])
def test_layouts(fe, ctx, fmt, h, w):
    """padded pitches that are no multiple of 4 or 16, unaligned bases, gaps between frames, padded output rows whose guard bytes stay as they
    were; tight and 16-byte aligned layouts (the vector path and its row tails); the single call equals the batch call"""
    rng = np.random.default_rng(w * 1000 + h * 10 + fmt)
    cn = cr.CHANNELS[fmt]
    n = 3
    frames = _frames(rng, n, h, w, fmt)
    want = cr.to_gray(frames, fmt)
    row = w * cn
    layouts = [  # (source base offset, pitch, image stride gap, gray base offset, gray pitch, gray image stride gap)
        (0, row, 0, 0, w, 0),                                          # tight
        (0, (row + 15) // 16 * 16, 16, 0, (w + 15) // 16 * 16, 32),      # 16-byte aligned rows: the vector path, tails on the byte path
        (7, row + 7, 13, 3, w + 5, 11),                                # odd everything
    ] + [(o, row + 16, 0, (16 - o) % 16, w + 16, 0) for o in (1, 8, 15)]      # unaligned bases 1..15
    for so, pitch, sgap, go, gpitch, ggap in layouts:
        istride, gistride = pitch * (h - 1) + row + sgap, gpitch * (h - 1) + w + ggap
        planes = lambda buf, off, stride, p, width: np.lib.stride_tricks.as_strided(buf[off:], (n, h, width), (stride, p, 1))
        src = np.zeros(so + istride * n + 64, np.uint8)
        planes(src, so, istride, pitch, row)[...] = frames.reshape(n, h, row)
        dst = np.full(go + gistride * n + 64, GUARD, np.uint8)
        d_src = _dev(src)
        d_dst = _dev(dst)
        ctx.gray_from_color_batch_dev(fmt, d_src.data_ptr() + so, w, h, pitch, istride, n, d_dst.data_ptr() + go, gpitch, gistride)
        ctx.synchronize()
        out = d_dst.cpu().numpy()
        np.testing.assert_array_equal(planes(out, go, gistride, gpitch, w), want, err_msg=str((so, pitch, sgap, go, gpitch, ggap)))
        mask = np.zeros(out.shape, bool)
        planes(mask, go, gistride, gpitch, w)[...] = True
        assert (out[~mask] == GUARD).all(), (so, pitch, go, gpitch)          # padding, gaps and the bytes around the planes untouched
        # the single host call on frame 1 of the same layout (a numpy view with the padded rows) into padded guard rows
        view = np.lib.stride_tricks.as_strided(src[so + istride:], (h, w, cn) if cn > 1 else (h, w), (pitch, cn, 1) if cn > 1 else (pitch, 1))
        g = np.full((h, w + 9), GUARD, np.uint8)
        order = "bgr" if fmt in (cr.PIX_BGR, cr.PIX_BGRA) else "rgb"
        res = ctx.gray_from_color(view, order, out=g)
        np.testing.assert_array_equal(res, want[1])
        assert (g[:, w:] == GUARD).all()


def test_gray_is_a_pitched_copy(fe, ctx):
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (480, 641), dtype=np.uint8)
    np.testing.assert_array_equal(ctx.gray_from_color(img), img)
    padded = np.zeros((480, 700), np.uint8); padded[:, :641] = img
    np.testing.assert_array_equal(ctx.gray_from_color(padded[:, :641]), img)


def test_invalid_arguments(fe, ctx):
    L = fe.lib()
    img = np.zeros((10, 8, 4), np.uint8); g = np.zeros((10, 8), np.uint8)
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    INV = fe.SSLAM_ERR_INVALID
    host = lambda fmt, w, h, stride, gstride, src=img, dst=g: L.sslam_gray_from_color(ctx.h, fmt, fe._p(src), w, h, C.c_size_t(stride), fe._p(dst), C.c_size_t(gstride))
    assert host(cr.PIX_RGBA, 8, 10, 32, 8) == 0
    for fmt in (-1, 5, 99):
        assert host(fmt, 8, 10, 32, 8) == INV
    assert host(cr.PIX_RGBA, 8, 10, 31, 8) == INV          # stride < w * cn
    assert host(cr.PIX_RGB, 8, 10, 23, 8) == INV
    assert host(cr.PIX_GRAY, 8, 10, 7, 8) == INV
    assert host(cr.PIX_RGBA, 8, 10, 32, 7) == INV          # gray_stride < w
    assert host(cr.PIX_RGBA, 0, 10, 32, 8) == INV and host(cr.PIX_RGBA, 8, 0, 32, 8) == INV
    assert host(cr.PIX_RGBA, 8, 10, 32, 8, src=None) == INV and host(cr.PIX_RGBA, 8, 10, 32, 8, dst=None) == INV
    assert b"sslam_gray_from_color" in L.sslam_last_error()
    dev = lambda fmt, w, h, p, s, n, gp, gs: L.sslam_gray_from_color_batch_dev(ctx.h, fmt, fe._p(d), w, h, C.c_size_t(p), C.c_size_t(s), n, fe._p(d.data_ptr() + 2048),
                                                                               C.c_size_t(gp), C.c_size_t(gs), None)
    assert dev(cr.PIX_RGB, 8, 4, 24, 96, 2, 8, 32) == 0
    assert dev(cr.PIX_RGB, 8, 4, 24, 96, 0, 8, 32) == 0                    # no frames
    assert dev(7, 8, 4, 24, 96, 2, 8, 32) == INV
    assert dev(cr.PIX_RGB, 8, 4, 23, 96, 2, 8, 32) == INV                  # pitch < w * cn
    assert dev(cr.PIX_RGB, 8, 4, 24, 95, 2, 8, 32) == INV                  # overlapping frames
    assert dev(cr.PIX_RGB, 8, 4, 24, 96, 2, 7, 32) == INV                  # gray pitch < w
    assert dev(cr.PIX_RGB, 8, 4, 24, 96, 2, 8, 31) == INV                  # overlapping gray frames
    assert dev(cr.PIX_RGB, 8, 4, 24, 96, -1, 8, 32) == INV
    assert dev(cr.PIX_RGB, 8, 4, 24, 1, 1, 8, 1) == 0                      # one frame: the image strides are not read
    assert L.sslam_gray_from_color_batch_dev(ctx.h, cr.PIX_RGB, None, 8, 4, C.c_size_t(24), C.c_size_t(96), 1, fe._p(d), C.c_size_t(8), C.c_size_t(32), None) == INV
    ctx.synchronize()
    # the host batch
    orb = fe.OrbExtractor(ctx, 500)
    out = fe.frontend_batch_alloc(2, orb.cap, 8)
    frames = np.zeros((2, 240, 320, 3), np.uint8)
    batch = lambda fmt, stride, istride: L.sslam_frontend_batch_color(orb.h, None, None, fmt, fe._p(frames), 2, 320, 240, C.c_size_t(stride), C.c_size_t(istride), 0,
                                                                      fe._p(out[0]), None, fe._p(out[1]), fe._p(out[2]), orb.cap, None, None, None, None, 8, None)
    assert batch(cr.PIX_RGB, 960, 960 * 240) == 0
    assert batch(5, 960, 960 * 240) == INV and batch(-1, 960, 960 * 240) == INV
    assert batch(cr.PIX_RGB, 959, 960 * 240) == INV                       # stride < w * cn
    assert batch(cr.PIX_RGBA, 960, 960 * 240) == INV
    assert batch(cr.PIX_RGB, 960, 960 * 239 + 959) == INV                 # overlapping frames
    assert b"sslam_frontend_batch_color" in L.sslam_last_error()
    orb.close()


# ---- 3. the host batch ---------------------------------------------------------------------------------------------------------------

def _colour_sequence(n, w=640, h=480):
    """a camera drifting over one scene (frame i = the base warped by i steps, so the content does not blur away along the sequence), as colour
    frames whose three channels differ (so the channel order matters), in RGB"""
    base = synth_frame(8300, w, h)
    g = np.stack([base] + [warp_prev(base, dx=2.5 * i, dy=-1.5 * i, deg=0.7 * i) for i in range(1, n)]).astype(np.int32)
    r = g
    gg = np.clip(255 - g + 40, 0, 255)
    b = np.roll(g, 5, axis=2) // 2 + 60
    return np.stack([r, gg, b], axis=-1).astype(np.uint8)


def _pinned(a):
    t = torch.empty(a.nbytes, dtype=torch.uint8, pin_memory=True)
    v = t.numpy().view(a.dtype).reshape(a.shape)
    v[...] = a
    return v, t


def _assert_outputs_equal(out, ref, nk, nl, cam):
    kp, desc, _, kl, ld, fn, _ = out[:7]
    rkp, rdesc, rnk, rkl, rld, rfn, rnl = ref[:7]
    np.testing.assert_array_equal(out[2], rnk); np.testing.assert_array_equal(out[6], rnl)
    for i in range(len(nk)):
        c, cl = nk[i], nl[i]
        np.testing.assert_array_equal(kp[i, :c].view(np.uint8), rkp[i, :c].view(np.uint8))
        np.testing.assert_array_equal(desc[i, :c], rdesc[i, :c])
        np.testing.assert_array_equal(kl[i, :cl].view(np.uint8), rkl[i, :cl].view(np.uint8))
        np.testing.assert_array_equal(ld[i, :cl], rld[i, :cl]); np.testing.assert_array_equal(fn[i, :cl].view(np.uint8), rfn[i, :cl].view(np.uint8))
        if cam:
            np.testing.assert_array_equal(out[7][i, :c].view(np.uint8), ref[7][i, :c].view(np.uint8))


def _assert_matches_equal(mout, mref, nk, nl):
    m12, nm, ki, kd, lp, nlp = mout
    rm12, rnm, rki, rkd, rlp, rnlp = mref
    np.testing.assert_array_equal(nm, rnm); np.testing.assert_array_equal(nlp, rnlp)
    for i in range(1, len(nk)):
        c1 = nk[i - 1]
        np.testing.assert_array_equal(m12[i, :c1], rm12[i, :c1])
        np.testing.assert_array_equal(ki[i, :c1], rki[i, :c1]); np.testing.assert_array_equal(kd[i, :c1], rkd[i, :c1])
        np.testing.assert_array_equal(lp[i, :nlp[i]], rlp[i, :nlp[i]])


def test_frontend_batch_color(fe, ctx):
    """37 colour frames in chunks of 8 (the carried predecessor crosses four chunk boundaries), with the match stage and a distorted camera, in
    every colour format, from pageable and from pinned memory, and once from padded rows: every output equals
    sslam_frontend_batch_match_camera on color_ref's gray frames byte for byte"""
    n, chunk, w, h = 37, 8, 640, 480
    rgb = _colour_sequence(n, w, h)
    gray = cr.to_gray(rgb, cr.PIX_RGB)
    cam = fe.Camera(*[float(v) for v in ur.camera_params("tum_fr1")])
    orb = fe.OrbExtractor(ctx, 1000); lines = fe.LineExtractor(ctx, 200)
    ref = fe.frontend_batch_camera_alloc(n, orb.cap, 200); mref = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_match_camera_raw(orb, lines, cam, gray, ref, mref, chunk=chunk)
    nk, nl = ref[2], ref[6]
    assert (nk > 300).all() and (nl > 10).all() and (mref[1][1:] > 20).all()
    for fmt in cr.COLOUR:
        img = cr.from_rgb(rgb, fmt, alpha=(np.arange(w, dtype=np.uint32) * 7 % 256).astype(np.uint8))
        wrong = {cr.PIX_RGB: cr.PIX_BGR, cr.PIX_BGR: cr.PIX_RGB, cr.PIX_RGBA: cr.PIX_BGRA, cr.PIX_BGRA: cr.PIX_RGBA}[fmt]
        assert not np.array_equal(cr.to_gray(img, wrong), gray) and np.array_equal(cr.to_gray(img, fmt), gray)      # the order matters
        for pinned in (False, True):
            src, keep = _pinned(img) if pinned else (img, None)
            out = fe.frontend_batch_camera_alloc(n, orb.cap, 200, pinned=pinned); mout = fe.frontend_batch_match_alloc(n, orb.cap, 200, pinned=pinned)
            fe.frontend_batch_color_raw(orb, lines, fmt, src, out, mout, cam=cam, chunk=chunk)
            _assert_outputs_equal(out, ref, nk, nl, True)
            _assert_matches_equal(mout, mref, nk, nl)
    # padded rows and gaps between frames (pageable staging row by row)
    cn = 3
    big = np.zeros((n, h + 1, w + 7, cn), np.uint8); big[:, :h, :w] = rgb
    out = fe.frontend_batch_camera_alloc(n, orb.cap, 200); mout = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_color_raw(orb, lines, cr.PIX_RGB, big[:, :h, :w], out, mout, cam=cam, chunk=chunk)
    _assert_outputs_equal(out, ref, nk, nl, True)
    _assert_matches_equal(mout, mref, nk, nl)
    # no camera / no match stage: sslam_frontend_batch_match and sslam_frontend_batch on the gray frames
    mref2 = fe.frontend_batch_match_alloc(n, orb.cap, 200); ref2 = fe.frontend_batch_alloc(n, orb.cap, 200)
    fe.frontend_batch_match_raw(orb, lines, gray, ref2, mref2, chunk=chunk)
    out = fe.frontend_batch_alloc(n, orb.cap, 200); mout = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_color_raw(orb, lines, cr.PIX_BGR, cr.from_rgb(rgb, cr.PIX_BGR), out, mout, chunk=chunk)
    _assert_outputs_equal(out, ref2, nk, nl, False)
    _assert_matches_equal(mout, mref2, nk, nl)
    out = fe.frontend_batch_alloc(n, orb.cap, 200)
    fe.frontend_batch_color_raw(orb, lines, cr.PIX_RGBA, cr.from_rgb(rgb, cr.PIX_RGBA), out, chunk=5)
    _assert_outputs_equal(out, ref2, nk, nl, False)
    orb.close(); lines.close()


def test_frontend_batch_color_gray_is_the_gray_entry_points(fe, ctx):
    """SSLAM_PIX_GRAY through sslam_frontend_batch_color is byte-identical to sslam_frontend_batch / _match / _match_camera"""
    n, chunk = 11, 4
    frames = cr.to_gray(_colour_sequence(n), cr.PIX_RGB)
    cam = fe.Camera(*[float(v) for v in ur.camera_params("strong")])
    orb = fe.OrbExtractor(ctx, 1000); lines = fe.LineExtractor(ctx, 200)
    ref = fe.frontend_batch_alloc(n, orb.cap, 200)
    fe.frontend_batch_raw(orb, lines, frames, ref, chunk=chunk)
    out = fe.frontend_batch_alloc(n, orb.cap, 200)
    fe.frontend_batch_color_raw(orb, lines, cr.PIX_GRAY, frames, out, chunk=chunk)
    _assert_outputs_equal(out, ref, ref[2], ref[6], False)
    ref = fe.frontend_batch_alloc(n, orb.cap, 200); mref = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_match_raw(orb, lines, frames, ref, mref, chunk=chunk)
    out = fe.frontend_batch_alloc(n, orb.cap, 200); mout = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_color_raw(orb, lines, cr.PIX_GRAY, frames, out, mout, chunk=chunk)
    _assert_outputs_equal(out, ref, ref[2], ref[6], False)
    _assert_matches_equal(mout, mref, ref[2], ref[6])
    ref = fe.frontend_batch_camera_alloc(n, orb.cap, 200); mref = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_match_camera_raw(orb, lines, cam, frames, ref, mref, chunk=chunk)
    out = fe.frontend_batch_camera_alloc(n, orb.cap, 200); mout = fe.frontend_batch_match_alloc(n, orb.cap, 200)
    fe.frontend_batch_color_raw(orb, lines, cr.PIX_GRAY, frames, out, mout, cam=cam, chunk=chunk)
    _assert_outputs_equal(out, ref, ref[2], ref[6], True)
    _assert_matches_equal(mout, mref, ref[2], ref[6])
    orb.close(); lines.close()


def test_grey_replicated_icl_frame(fe, ctx):
    """R = G = B = the ICL gray frame, one frame (the single-frame colour call) in every colour format: exactly what the gray path gives on
    icl_input_gray.npz (and through the existing parity, the committed ICL goldens)"""
    gray = np.load(os.path.join(pkg.ROOT, "tests", "golden", "icl_input_gray.npz"))["gray"][None]
    orb = fe.OrbExtractor(ctx, 1000); lines = fe.LineExtractor(ctx, 200)
    ref = fe.frontend_batch_alloc(1, orb.cap, 200)
    fe.frontend_batch_raw(orb, lines, gray, ref)
    assert ref[2][0] > 300 and ref[6][0] > 5
    for fmt in cr.COLOUR:
        out = fe.frontend_batch_alloc(1, orb.cap, 200)
        fe.frontend_batch_color_raw(orb, lines, fmt, cr.grey_replicated(gray, fmt), out)
        _assert_outputs_equal(out, ref, ref[2], ref[6], False)
    orb.close(); lines.close()


# ---- 4. the pipeline -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [False, True])
def test_pipeline_colour_tensors(fe, ctx, overlap):
    """FrontendBatch.step on [B, h, w, 3] and [B, h, w, 4] tensors gives the features and matches it gives on the converted [B, h, w] tensor"""
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    B, w, h = 6, 640, 480
    seq = _colour_sequence(2 * B, w, h)
    results = {}
    for tag, rgb_order, fmt in (("gray", True, None), ("rgb", True, cr.PIX_RGB), ("bgra", False, cr.PIX_BGRA)):
        pb = pipeline.FrontendBatch(fe, ctx, w, h, B, rgb=rgb_order)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for k in range(2):
                frames = seq[k * B:(k + 1) * B]
                x = cr.to_gray(frames, cr.PIX_RGB) if fmt is None else cr.from_rgb(frames, fmt)
                if k == 1:
                    for key in pb.feat["cur"]:
                        pb.feat["prev"][key].copy_(pb.feat["cur"][key])
                pb.step(torch.from_numpy(x).cuda(), overlap=overlap)
        s.synchronize()
        c = pb.feat["cur"]
        results[tag] = dict(pn=pb.feat["prev"]["n"].cpu(), n=c["n"].cpu(), nl=c["nl"].cpu(), kp=c["kp"].cpu().view(torch.int32), desc=c["desc"].cpu(), ldesc=c["ldesc"].cpu(), m12=pb.m12.cpu(),
                            nmatch=pb.nmatch.cpu(), knn=pb.knn_idx.cpu(), lp=pb.lpairs.cpu(), nlp=pb.nlpairs.cpu())
        pb.close()
    g = results["gray"]
    assert (g["n"] > 300).all() and (g["nmatch"] > 20).all() and (g["nlp"] > 2).all()
    for tag in ("rgb", "bgra"):
        r = results[tag]
        for key in ("n", "nl", "nmatch", "nlp"):
            assert torch.equal(r[key], g[key]), (tag, key)
        assert torch.equal(r["pn"], g["pn"])
        for i in range(B):
            c, cl, c1, p = int(g["n"][i]), int(g["nl"][i]), int(g["pn"][i]), int(g["nlp"][i])
            assert torch.equal(r["kp"][i, :c], g["kp"][i, :c]) and torch.equal(r["desc"][i, :c], g["desc"][i, :c]), (tag, i)
            assert torch.equal(r["ldesc"][i, :cl], g["ldesc"][i, :cl]), (tag, i)
            assert torch.equal(r["m12"][i, :c1], g["m12"][i, :c1]) and torch.equal(r["knn"][i, :c1], g["knn"][i, :c1]), (tag, i)
            assert torch.equal(r["lp"][i, :p], g["lp"][i, :p]), (tag, i)


# ---- 5. the C++ drop-in --------------------------------------------------------------------------------------------------------------

CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "TrackingImage.h"
int main(int argc, char **argv) {
    // argv: image.raw out.raw w h channels bRGB pad -- the image rows are read into a cv::Mat (rows padded by `pad` bytes when pad > 0)
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), cn = std::atoi(argv[5]), bRGB = std::atoi(argv[6]), pad = std::atoi(argv[7]);
    const int type = cn == 1 ? CV_8U : cn == 3 ? CV_8UC3 : CV_8UC4;
    std::vector<unsigned char> buf((size_t)(w * cn + pad) * h);
    cv::Mat im(h, w, type, buf.data(), (size_t)(w * cn + pad));
    if (im.channels() != cn) return 4;
    FILE *f = std::fopen(argv[1], "rb");
    for (int y = 0; y < h; ++y) if (std::fread(im.ptr(y), 1, (size_t)w * cn, f) != (size_t)w * cn) return 2;
    std::fclose(f);
    cv::Mat mImGray;
    sslam_shim::GrabGray(im, bRGB != 0, mImGray);
    if (mImGray.rows != h || mImGray.cols != w || mImGray.channels() != 1) return 3;
    if (cn == 1 && mImGray.data != im.data) return 5;          // mImGray = im: shared, not copied
    cv::Mat self = im;                                         // the reference's in-place form: cvtColor(mImGray, mImGray, ...)
    sslam_shim::GrabGray(self, bRGB != 0, self);
    FILE *o = std::fopen(argv[2], "wb");
    for (int y = 0; y < h; ++y) { std::fwrite(mImGray.ptr(y), 1, w, o); std::fwrite(self.ptr(y), 1, w, o); }
    std::fclose(o);
    return 0;
}
"""


def test_cpp_tracking_image_dropin(fe, ctx, tmp_path):
    """shim/TrackingImage.h: the four cvtColor lines of Tracking.cc:148-161 as sslam_shim::GrabGray on a 3- and a 4-channel cv::Mat with both
    bRGB values (and a 1-channel one, passed through) equal the restatement"""
    builder = pkg.builder()
    builder.build(force=False, verbose=False)
    src = tmp_path / "tracking_image.cpp"; src.write_text(CPP)
    exe = tmp_path / "tracking_image"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + builder.SHIM, str(src), "-L" + builder.LIBDIR, "-lsslam_frontend",
                           "-Wl,-rpath," + builder.LIBDIR, "-o", str(exe)])
    w, h = 641, 480
    rng = np.random.default_rng(17)
    for cn in (1, 3, 4):
        img = rng.integers(0, 256, (h, w, cn) if cn > 1 else (h, w), dtype=np.uint8)
        for bRGB in (1, 0):
            for pad in (0, 5):
                kin = tmp_path / "im.raw"; kout = tmp_path / "out.raw"
                img.tofile(kin)
                r = subprocess.run([str(exe), str(kin), str(kout), str(w), str(h), str(cn), str(bRGB), str(pad)], capture_output=True, text=True, timeout=120)
                assert r.returncode == 0, (cn, bRGB, pad, r.returncode, r.stdout + r.stderr)
                got = np.fromfile(kout, np.uint8).reshape(h, 2, w)
                fmt = cr.PIX_GRAY if cn == 1 else fe.pix_format(cn, bool(bRGB))
                want = cr.to_gray(img, fmt)
                np.testing.assert_array_equal(got[:, 0], want, err_msg=str((cn, bRGB, pad)))
                np.testing.assert_array_equal(got[:, 1], want, err_msg=str((cn, bRGB, pad, "in place")))
