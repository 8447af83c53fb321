"""GPU: the line tail (k_keylines, k_blur_sobel, k_lbd: csrc/lbd.h) on injected segments -- sslam_testing_lines_tail runs the product path's preparation and launches on the
lists of tests/line_tail_cases.py (whose reach tests/test_line_tail_cases_cpu.py proves from the oracle alone) -- against the oracle's tail.  The bar: counts, every
KeyLine field but `angle` and the line equations bit for bit; `angle` within 1 ulp (libm against ocml atan2); EVERY descriptor row equal to the oracle's LBD of the
keylines the device produced; the direction pairs equal to (float)cos / sin((double)angle) of the device's angle; nothing written past a frame's count."""
import ctypes as C
import math
import numpy as np
import pytest
import line_tail_cases as lc
from synth import synth_frame
from test_lines_gpu import _ulp_diff

pytestmark = pytest.mark.gpu

ANGLES = {"compared": 0, "one_ulp": 0}       # KeyLine.angle against the oracle's over this module's cases (printed by every test that adds to it)


class Tail:
    """a sslam_lines handle of the TESTING library (its kernels' constant tables are uploaded per library) and its injection entry point"""
    def __init__(self, fe, ctx, max_lines):
        self.T = fe.testing_lib()
        self.T.sslam_testing_lines_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fe = fe
        self.h = C.c_void_p()
        assert self.T.sslam_lines_create(ctx.h, int(max_lines), C.byref(self.h)) == 0

    def __enter__(self): return self

    def __exit__(self, *a):
        self.T.sslam_lines_destroy(self.h)

    def raw(self, images, segs, nsegs, cap, accept=None):
        """-> status, (keylines [nf, cap], ldesc [nf, cap, 32], linefn [nf, cap, 3], counts [nf], directions [nf, cap, 2])"""
        images = np.ascontiguousarray(images, np.uint8); segs = np.ascontiguousarray(segs, np.float32); nsegs = np.ascontiguousarray(nsegs, np.int32)
        nf, h, w = images.shape
        assert segs.shape[0] == nf and segs.shape[2] == 4 and len(nsegs) == nf
        if accept is not None:
            accept = np.ascontiguousarray(accept, np.uint8); assert accept.shape == segs.shape[:2]
        kl = np.zeros((nf, cap), self.fe.KL_DTYPE); ld = np.zeros((nf, cap, 32), np.uint8); fn = np.zeros((nf, cap, 3), np.float64)
        cnt = np.zeros(nf, np.int32); dr = np.zeros((nf, cap, 2), np.float32)
        p = lambda a: None if a is None else a.ctypes.data
        rc = self.T.sslam_testing_lines_tail(self.h, p(images), w, h, w, w * h, nf, p(segs), p(accept), p(nsegs), segs.shape[1], cap, p(kl), p(ld), p(fn), p(cnt), p(dr))
        return rc, (kl, ld, fn, cnt, dr)

    def __call__(self, images, segs, nsegs, cap, accept=None):
        rc, out = self.raw(images, segs, nsegs, cap, accept)
        assert rc == 0, self.T.sslam_last_error()
        return out


def _untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == 0xA5).all()


def _check_frame(oracle, img, seg, max_lines, cap, kl, ld, fn, n, dr, tag):
    """one frame of a hook call against the oracle's tail on the same (accepted) segments"""
    okl, old, ofn = oracle.lines_tail(img, seg, max_lines, cap=cap)
    assert n == len(okl), (tag, n, len(okl))
    g = kl[:n]
    for f in g.dtype.names:
        if f != "angle": np.testing.assert_array_equal(g[f], okl[f], err_msg="%s %s" % (tag, f))
    ulp = _ulp_diff(g["angle"], okl["angle"])
    ANGLES["compared"] += n; ANGLES["one_ulp"] += int((ulp == 1).sum())
    print("%s: %d lines, %d angles one ulp from the oracle's (module so far: %d of %d)" % (tag, n, int((ulp == 1).sum()), ANGLES["one_ulp"], ANGLES["compared"]))
    assert ulp.max(initial=0) <= 1, (tag, "KeyLine.angle")
    np.testing.assert_array_equal(fn[:n].view(np.uint64), ofn.view(np.uint64), err_msg=tag + " line equations")
    want = oracle.lbd_from_keylines(img, g)
    bad = np.nonzero((ld[:n] != want).any(axis=1))[0]
    assert len(bad) == 0, (tag, "LBD rows", bad[:10], g[bad[:10]])
    ang = g["angle"].astype(np.float64)
    wdir = np.array([[math.cos(a), math.sin(a)] for a in ang], np.float64).astype(np.float32).reshape(-1, 2)
    bad = np.nonzero((dr[:n].view(np.uint32) != wdir.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (tag, "direction pairs", [(hex(int(g["angle"][i:i + 1].view(np.uint32)[0])), dr[i], wdir[i]) for i in bad[:10]])
    assert _untouched(kl[n:]) and _untouched(ld[n:]) and _untouched(fn[n:]) and _untouched(dr[n:]), (tag, "rows past the count were written")


def _run_single(fe, ctx, oracle, case, tag):
    with Tail(fe, ctx, case["max_lines"]) as t:
        seg = case["segs"]
        kl, ld, fn, cnt, dr = t(case["img"][None], seg[None], [len(seg)], case["cap"])
    _check_frame(oracle, case["img"], seg, case["max_lines"], case["cap"], kl[0], ld[0], fn[0], int(cnt[0]), dr[0], tag)
    return kl[0][:cnt[0]]


@pytest.mark.parametrize("name", list(lc.IMAGES))
def test_directions_and_lengths(fe, ctx, oracle, name):
    """every whole degree and the exact axis / diagonal directions x numOfPixels 2 .. 17, and the line that spans the image (16 384 / 16 388 steps on the strips): the four
    gather mappings of k_lbd, walks shorter than a block, k_lbd<true> at its largest image and k_lbd<false> through either side of the launch's condition"""
    kl = _run_single(fe, ctx, oracle, lc.direction_case(name), "directions " + name)
    assert kl["numOfPixels"][lc.LONG_AT] == max(lc.IMAGES[name][:2])


@pytest.mark.parametrize("name", lc.SMALL)
def test_borders_and_clamps(fe, ctx, oracle, name):
    """lines on every border row / column and into every corner (the support region clamped on that side), every checkLineExtremes condition"""
    _run_single(fe, ctx, oracle, lc.border_case(name), "borders " + name)


def test_counts_and_the_sort(fe, ctx, oracle):
    """ONE batch call, 0 .. 8 192 accepted segments per frame under max_lines 40: the compaction across 256-candidate chunks, no sort / the LDS sort / the sort in the
    frame's workspace at 1 024 | 1 025 and the powers of two, response ties across the cut (decision D3: emission order)"""
    c = lc.count_case()
    with Tail(fe, ctx, c["max_lines"]) as t:
        kl, ld, fn, cnt, dr = t(c["images"], c["segs"], c["ncand"], c["cap"], accept=c["accept"])
        for f, n in enumerate(lc.COUNTS):          # the compaction left the accepted segments in order
            out = np.zeros((lc.MAX_SEG, 4), np.float32); m = C.c_int(0)
            assert t.T.sslam_lines_debug_segments(t.h, f, C.c_void_p(out.ctypes.data), lc.MAX_SEG, C.byref(m)) == 0
            assert m.value == n
            np.testing.assert_array_equal(out[:n], lc.accepted(c, f), err_msg="frame %d" % f)
    np.testing.assert_array_equal(cnt, np.minimum(c["counts"], c["max_lines"]))
    for f, n in enumerate(lc.COUNTS):
        _check_frame(oracle, c["img"], lc.accepted(c, f), c["max_lines"], c["cap"], kl[f], ld[f], fn[f], int(cnt[f]), dr[f], "counts n=%d" % n)


def test_full_frame_without_sort(fe, ctx, oracle):
    """8 192 segments under max_lines 8 192: no sort, 8 192 descriptors"""
    c = lc.full_case()
    kl = _run_single(fe, ctx, oracle, c, "full")
    assert len(kl) == lc.MAX_SEG and (kl["class_id"] == np.arange(lc.MAX_SEG)).all()


def test_count_clamps_to_capacity(fe, ctx, oracle):
    c = lc.small_cap_case()
    kl = _run_single(fe, ctx, oracle, c, "small cap")
    assert len(kl) == 17


def test_too_many_segments_are_refused(fe, ctx):
    img = lc.image("noise160")
    with Tail(fe, ctx, 40) as t:
        rc, _ = t.raw(img[None], np.zeros((1, lc.MAX_SEG + 1, 4), np.float32), [lc.MAX_SEG + 1], 40)
        assert rc == -1 and b"8193" in t.T.sslam_last_error()


@pytest.mark.parametrize("frame,cap", [("synth2000", 200), ("synth1280", 400)])
def test_hook_equals_product(fe, ctx, frame, cap):
    """the segments of a normal extraction by the PRODUCT library, fed to the hook: keylines, descriptors and equations byte for byte"""
    img = synth_frame(2000) if frame == "synth2000" else synth_frame(1235, w=1280, h=960)
    ex = fe.LineExtractor(ctx, cap)
    try:
        kl, ld, fn = ex(img); raw = ex.debug_segments(0)
    finally:
        ex.close()
    assert len(raw) > cap == len(kl)
    with Tail(fe, ctx, cap) as t:
        hkl, hld, hfn, cnt, dr = t(img[None], raw[None], [len(raw)], cap)
    assert cnt[0] == len(kl)
    assert hkl[0].tobytes() == kl.tobytes() and hld[0].tobytes() == ld.tobytes() and hfn[0].tobytes() == fn.tobytes()


def test_whole_frame_of_equal_responses(fe, ctx, oracle):
    """the public path on a frame whose 70 segments all have the same response: max_lines 40 keeps the first 40 in emission order"""
    img = lc.squares_frame()
    okl, old, ofn, oraw = oracle.lines_extract(img, 40)
    ex = fe.LineExtractor(ctx, 40)
    try:
        kl, ld, fn = ex(img)
        np.testing.assert_array_equal(ex.debug_segments(0), oraw)
    finally:
        ex.close()
    assert len(kl) == len(okl) == 40 and len(oraw) == 70
    for f in kl.dtype.names:
        if f != "angle": np.testing.assert_array_equal(kl[f], okl[f], err_msg=f)
    assert _ulp_diff(kl["angle"], okl["angle"]).max() <= 1
    for f, col in (("startPointX", 0), ("startPointY", 1), ("endPointX", 2), ("endPointY", 3)):
        np.testing.assert_array_equal(kl[f], oraw[:40, col])
    np.testing.assert_array_equal(ld, oracle.lbd_from_keylines(img, kl)); np.testing.assert_array_equal(fn, ofn)
