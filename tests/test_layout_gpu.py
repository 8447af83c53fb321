"""GPU: sslam_orb_extract_batch_dev and sslam_lines_extract_batch_dev on the image layouts a caller may hand them -- padded rows, gaps between
frames, unaligned bases, odd pitches and odd frame strides (include/sslam_frontend.h: level 0 is read IN PLACE for a dword-aligned base, pitch and
image stride with whole-block frames, anything else is copied; the line kernels choose their row loads per frame from the same three numbers).

Three distinct frames per call, placed inside ONE device allocation whose every non-pixel byte (in front of the base, row padding, gaps, a tail
of 64 bytes) holds a fill pattern.  Per layout, for both extractors:
  * every frame against the CPU oracle, by the bars of tests/test_orb_gpu.py and tests/test_lines_gpu.py (no tolerance of this module's own);
  * every output byte against the compact layout's (the arithmetic is the same, only the loads differ);
  * fill 0x00 against a random fill: byte-identical outputs (a load that uses padding or a neighbour's bytes shows here, without any fault);
  * the source buffer unchanged, the guard rows behind the outputs and behind d_counts[nframes] untouched;
  * which kernels ran (sslam_profile_drain): k_copy_level0 exactly for the layouts the header says are copied, k_blur7 exactly where the fused
    gradient kernel does not apply.  The fused kernel and k_lsd_grad share the profile label "k_lsd_grad" (bench.py's byte model is keyed by it):
    the fused form is "k_lsd_grad without k_blur7".
The host batch (sslam_frontend_batch) at widths that are no multiple of four hands the device entry points pitch == w with odd frame bases; the
argument errors of the two entry points close the module."""
import ctypes as C
import functools, os
import numpy as np
import pytest
import torch
import pkg
from synth import synth_frame

pytestmark = pytest.mark.gpu

NFEAT, SCALE, NLEVELS, LCAP, NF = 300, 1.2, 4, 60, 3
GUARD, GUARD_I32, GUARD_ROWS = 0xA5, np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0], 8
# seeds chosen on the CPU with the oracle: synth_frame(seed, w, h, nshapes=14, nstrokes=10) has >= 50 keypoints and >= 5 line segments (asserted in _ref)
SEEDS = {(160, 120): (7160, 7161, 7162), (220, 140): (7220, 7221, 7222), (202, 150): (7202, 7203, 7204), (199, 151): (7199, 7200, 7201)}
SIZES = list(SEEDS)
FUSED_SIZES = {(160, 120), (220, 140)}                 # 20k x 20j: the geometry lines_build_plan admits for k_lsd_grad_fused
TAP_SIZES, TAP_CASES = {(160, 120), (199, 151)}, {"a", "c", "d", "f1", "f2", "f3", "h"}
CASES = ("a", "b", "c", "d", "e", "f1", "f2", "f3", "g1", "g3", "h", "i")


def _layout(case, w, h):
    """(base offset, pitch, image stride) of a case of the matrix; a pitch that has to be aligned is taken from (w + 3) & ~3"""
    wa = (w + 3) & ~3
    return {"a": (0, w, w * h),                                   # compact
            "b": (0, w, w * h + 20),                              # gaps of 4k bytes between the frames
            "c": (0, wa + 4, (wa + 4) * h),                       # padding smaller than a 12-byte window
            "d": (0, wa + 36, (wa + 36) * h + 8),                 # padded rows and a gap
            "e": (0, wa + 4, (wa + 4) * (h - 1) + w),             # aligned, but the frames are no whole blocks
            "f1": (1, w, w * h), "f2": (2, w, w * h), "f3": (3, w, w * h),      # unaligned bases
            "g1": (0, w + 1, (w + 1) * h), "g3": (0, w + 3, (w + 3) * h),     # the row alignment changes from row to row
            "h": (0, w, w * h + 1),                               # the frames of one launch differ in alignment
            "i": (4, wa + 4, (wa + 4) * h)}[case]                 # an aligned base inside a larger buffer


def _aligned(lay):
    return all(v % 4 == 0 for v in lay)


def _in_place(lay, w, h):
    """include/sslam_frontend.h: base, pitch and image stride multiples of 4 and whole blocks (pitch == w, or image_stride >= pitch * h)"""
    base, pitch, stride = lay
    return _aligned(lay) and (pitch == w or stride >= pitch * h)


def _fused(lay, size):
    return size in FUSED_SIZES and _aligned(lay)


def _row_loaders(lay, w):
    """which of k_blur7's / k_blur_sobel's three row loaders the frames of a layout take (lsd_front.h: row12_uniform, load_row12 fast / bytes)"""
    base, pitch, stride = lay
    out = set()
    for b in range(NF):
        al = ((base + b * stride) | pitch) % 4 == 0
        out |= {"uniform"} if al and w % 4 == 0 and w >= 12 else {"fast", "bytes"} if al else {"bytes"}      # fast: interior lanes; the border lanes reflect byte-wise
    return out


def _copy_paths(lay, w, h):
    """k_copy_level0: 16 bytes per lane where a row's 16-byte group is 16-byte aligned and inside the row, bytes elsewhere"""
    base, pitch, stride = lay
    out = set()
    for b in range(NF):
        for y in range(h):
            a = base + b * stride + y * pitch
            out |= {"vec16" if (a + x) % 16 == 0 and x + 16 <= w else "bytes" for x in range(0, w, 16)}
    return out


@functools.lru_cache(maxsize=None)
def _frames(size):
    w, h = size
    f = np.stack([synth_frame(s, w, h, nshapes=14, nstrokes=10) for s in SEEDS[size]])
    f.setflags(write=False)
    return f


_REF = {}


def _ref(oracle, size):
    """the oracle's results for the three frames of a size, computed once"""
    if size not in _REF:
        frames = _frames(size)
        r = []
        for f in frames:
            kp, desc = oracle.orb_extract(f, NFEAT, SCALE, NLEVELS)
            kl, ld, fn, raw = oracle.lines_extract(f, LCAP)
            assert len(kp) >= 50 and len(raw) >= 5 and len(kl) >= 5, (size, len(kp), len(raw), len(kl))      # nothing below passes vacuously
            r.append(dict(kp=kp, desc=desc, kl=kl, ld=ld, fn=fn, raw=raw))
        assert len({len(x["kp"]) for x in r}) == NF                                                            # first, middle and last frame are told apart
        _REF[size] = r
    return _REF[size]


def _tap_ref(oracle, size):
    """the oracle's pyramid levels and FAST candidates of the three frames, computed once"""
    if ("taps", size) not in _REF:
        _REF["taps", size] = [[(oracle.pyramid_level(f, l, SCALE, NLEVELS), oracle.candidates(f, l, NFEAT, SCALE, NLEVELS)) for l in range(NLEVELS)] for f in _frames(size)]
    return _REF["taps", size]


def _place(frames, lay, fill):
    """the frames at (base, pitch, image stride) inside one flat buffer: the last frame keeps its full pitch * h bytes (the header asks for it with
    padded rows) and 64 more follow; every byte that is no pixel is 0 (fill None) or random (fill = a seed)"""
    base, pitch, stride = lay
    n, h, w = frames.shape
    total = base + stride * (n - 1) + pitch * h + 64
    buf = np.zeros(total, np.uint8) if fill is None else np.random.default_rng(fill).integers(0, 256, total, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(buf[base:], (n, h, w), (stride, pitch, 1))[...] = frames
    return buf


def _ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64); bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai); bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


class _Rig:
    """one extractor pair per size (created on first use, closed with the module) and the compact layout's outputs the other layouts are held against"""
    def __init__(self, fe, ctx):
        self.fe, self.ctx, self.ex, self.baseline = fe, ctx, {}, {}
        self.pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))

    def extractor(self, kind, size):
        if (kind, size) not in self.ex:
            self.ex[kind, size] = self.fe.OrbExtractor(self.ctx, NFEAT, SCALE, NLEVELS, 20, 7) if kind == "orb" else self.fe.LineExtractor(self.ctx, LCAP)
        return self.ex[kind, size]

    def close(self):
        for e in self.ex.values():
            e.close()

    def run(self, kind, size, lay, fill):
        """one call of the entry point on a layout: the per-frame output rows as bytes, the kernel names, and the device source (alive for the taps).
        Checks the source and the guards."""
        fe, ctx = self.fe, self.ctx
        w, h = size
        base, pitch, stride = lay
        ex = self.extractor(kind, size)
        host = _place(_frames(size), lay, fill)
        d_src = torch.from_numpy(host).cuda()
        assert d_src.data_ptr() % 256 == 0                     # the base offset alone decides the alignment
        cap = ex.cap if kind == "orb" else LCAP
        rows = NF * cap
        widths = (28, 32) if kind == "orb" else (68, 32, 24)    # sslam_keypoint, descriptor / sslam_keyline, LBD, three doubles
        d_out = [torch.full(((rows + GUARD_ROWS) * wd,), GUARD, dtype=torch.uint8, device="cuda") for wd in widths]
        d_cnt = torch.full((NF + GUARD_ROWS,), int(GUARD_I32), dtype=torch.int32, device="cuda")
        self.pipeline.profile_drain(fe, ctx)                                       # (synchronises the device: the fills above are done; no stale record)
        fe.lib().sslam_profile_enable(ctx.h, 1)
        try:
            ex.extract_batch_dev(d_src.data_ptr() + base, w, h, pitch, stride, NF, *d_out, d_cnt, cap)
        finally:
            fe.lib().sslam_profile_enable(ctx.h, 0)
            names = set(self.pipeline.profile_drain(fe, ctx))                  # (synchronises the device)
        ctx.synchronize()
        np.testing.assert_array_equal(d_src.cpu().numpy(), host, err_msg="the source buffer changed")
        cnt = d_cnt.cpu().numpy()
        assert (cnt[NF:] == GUARD_I32).all(), "d_counts holds more than nframes values"
        assert ((cnt[:NF] >= 0) & (cnt[:NF] <= cap)).all(), cnt[:NF]
        out = []
        for d, wd in zip(d_out, widths):
            a = d.cpu().numpy().reshape(rows + GUARD_ROWS, wd)
            assert (a[rows:] == GUARD).all(), "rows behind nframes * cap were written"
            out.append([a[f * cap:f * cap + cnt[f]].copy() for f in range(NF)])
        return dict(n=cnt[:NF].copy(), out=out, names=names), d_src

    def compact(self, kind, size):
        if (kind, size) not in self.baseline:
            self.baseline[kind, size] = self.run(kind, size, _layout("a", *size), None)[0]
        return self.baseline[kind, size]


@pytest.fixture(scope="module")
def rig(fe, ctx):
    r = _Rig(fe, ctx)
    yield r
    r.close()


def _assert_same(got, want, what):
    np.testing.assert_array_equal(got["n"], want["n"], err_msg="%s: counts" % what)
    for k, (g, w_) in enumerate(zip(got["out"], want["out"])):
        for f in range(NF):
            np.testing.assert_array_equal(g[f], w_[f], err_msg="%s: output array %d of frame %d" % (what, k, f))


def test_matrix_reaches_every_form():
    """the expectations the tests below hold the profile names against, spelled out: which cases are read in place and which take the fused kernel,
    and that the matrix reaches k_copy_level0's two paths and the three row loaders (frames of case h with different ones)"""
    for size in SIZES:
        w, h = size
        in_place = {c for c in CASES if _in_place(_layout(c, w, h), w, h)}
        fused = {c for c in CASES if _fused(_layout(c, w, h), size)}
        if w % 4 == 0:
            assert in_place == {"a", "b", "c", "d", "i"} and fused == {"a", "b", "c", "d", "e", "i"}
        else:      # pitch == w is unaligned: only the padded layouts with an aligned pitch are read in place (199 + 1 happens to be one more)
            assert in_place == {"c", "d", "i"} | ({"g1"} if w % 4 == 3 else set()) and not fused
    w, h = 160, 120
    assert _copy_paths(_layout("e", w, h), w, h) == {"vec16", "bytes"} and _copy_paths(_layout("f1", w, h), w, h) == {"bytes"}
    assert _copy_paths(_layout("a", 199, 151), 199, 151) == {"vec16", "bytes"}
    assert _row_loaders(_layout("a", w, h), w) == {"uniform"} and _row_loaders(_layout("f2", w, h), w) == {"bytes"}
    assert _row_loaders(_layout("h", w, h), w) == {"uniform", "bytes"}                     # frame 0 aligned, frames 1 and 2 not
    assert _row_loaders(_layout("c", 202, 150), 202) == {"fast", "bytes"} and _row_loaders(_layout("i", 199, 151), 199) == {"fast", "bytes"}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_orb_layout(fe, ctx, oracle, rig, size, case):
    w, h = size
    lay = _layout(case, w, h)
    ref = _ref(oracle, size)
    got, d_src = rig.run("orb", size, lay, None)
    # which kernels ran
    assert ("k_copy_level0" not in got["names"]) == _in_place(lay, w, h), (lay, sorted(got["names"]))
    assert {"k_resize", "k_fast_cells", "k_octree", "k_describe"} <= got["names"]
    # the stage taps: level 0 through the caller's buffer where it was read in place, level 1 resized from the caller's pitch
    if size in TAP_SIZES and case in TAP_CASES:
        ex, taps = rig.extractor("orb", size), _tap_ref(oracle, size)
        for f in range(NF):
            np.testing.assert_array_equal(ex.debug_level(f, 0), _frames(size)[f], err_msg="level 0 of frame %d" % f)
            for l in range(NLEVELS):
                np.testing.assert_array_equal(ex.debug_level(f, l), taps[f][l][0], err_msg="frame %d level %d" % (f, l))
                np.testing.assert_array_equal(ex.debug_candidates(f, l), taps[f][l][1], err_msg="candidates: frame %d level %d" % (f, l))
    # the oracle, per frame
    for f in range(NF):
        assert got["n"][f] == len(ref[f]["kp"]), (f, got["n"], [len(r["kp"]) for r in ref])
        np.testing.assert_array_equal(got["out"][0][f], ref[f]["kp"].view(np.uint8).reshape(-1, 28), err_msg="keypoints of frame %d" % f)
        np.testing.assert_array_equal(got["out"][1][f], ref[f]["desc"], err_msg="descriptors of frame %d" % f)
    # the compact layout, and a random fill of everything that is no pixel
    _assert_same(got, rig.compact("orb", size), "against the compact layout")
    rnd, _ = rig.run("orb", size, lay, 1000 + CASES.index(case))
    assert rnd["names"] == got["names"]
    _assert_same(rnd, got, "random against zero fill")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_lines_layout(fe, ctx, oracle, rig, size, case):
    w, h = size
    lay = _layout(case, w, h)
    ref = _ref(oracle, size)
    ex = rig.extractor("lines", size)
    got, d_src = rig.run("lines", size, lay, None)
    # which kernels ran: the fused kernel carries k_lsd_grad's label, so "fused" is "no k_blur7"
    assert ("k_blur7" not in got["names"]) == _fused(lay, size), (lay, sorted(got["names"]))
    assert {"k_lsd_grad", "k_blur_sobel", "k_keylines", "k_lbd"} <= got["names"]
    raws = [ex.debug_segments(f) for f in range(NF)]
    for f in range(NF):
        r = ref[f]
        np.testing.assert_array_equal(raws[f], r["raw"], err_msg="LSD segments of frame %d" % f)
        assert got["n"][f] == len(r["kl"]), (f, got["n"])
        kl = got["out"][0][f].reshape(-1).view(fe.KL_DTYPE)
        for name in kl.dtype.names:
            if name == "angle":
                assert _ulp_diff(kl[name], r["kl"][name]).max(initial=0) <= 1, "KeyLine.angle of frame %d" % f
            else:
                np.testing.assert_array_equal(kl[name], r["kl"][name], err_msg="%s of frame %d" % (name, f))
        ham = np.unpackbits(got["out"][1][f] ^ r["ld"], axis=1).sum(axis=1)
        same_angle = kl["angle"].view(np.uint32) == r["kl"]["angle"].view(np.uint32)
        assert (ham[same_angle] == 0).all() and ham.max(initial=0) <= 8, (f, ham)
        np.testing.assert_array_equal(got["out"][2][f].reshape(-1).view(np.float64).reshape(-1, 3), r["fn"], err_msg="line functions of frame %d" % f)
    _assert_same(got, rig.compact("lines", size), "against the compact layout")
    rnd, _ = rig.run("lines", size, lay, 2000 + CASES.index(case))
    assert rnd["names"] == got["names"]
    for f in range(NF):
        np.testing.assert_array_equal(ex.debug_segments(f), raws[f], err_msg="LSD segments of frame %d, random fill" % f)
    _assert_same(rnd, got, "random against zero fill")


# ---- the host batch at widths that are no multiple of four -----------------------------------------------------------------------------

def _host_batch(fe, orb, lines, images, out, chunk):
    """sslam_frontend_batch on a [n, h, w] array or view (rows and frames may be padded)"""
    n, h, w, stride, istride = fe._image_layout(images, fe.PIX_GRAY, True)
    kp, desc, nk, kl, ld, fn, nl = out
    fe._chk(fe.lib().sslam_frontend_batch(orb.h, lines.h, fe._p(images), n, w, h, C.c_size_t(stride), C.c_size_t(istride), int(chunk),
                                          fe._p(kp), fe._p(desc), fe._p(nk), orb.cap, fe._p(kl), fe._p(ld), fe._p(fn), fe._p(nl), int(kl.shape[1])))
    return out


@pytest.mark.parametrize("size", [(199, 151), (202, 150)], ids=lambda s: "%dx%d" % s)
def test_host_batch_unaligned_width(fe, ctx, oracle, size):
    """7 frames in chunks of 3 (two full chunks and a tail): the device entry points get pitch == w, so ORB copies level 0 and the line kernels see frame
    bases of every alignment.  A compact array, a padded view (row stride w + 5, a gap between the frames, random bytes in both: the row-wise staging) and a
    compact array in pinned memory (copied directly) give, frame by frame, what the single-frame host calls give; two frames also against the oracle."""
    w, h = size
    n, chunk = 7, 3
    frames = np.stack([synth_frame(7500 + w + i, w, h, nshapes=14, nstrokes=10) for i in range(n)])
    orb = fe.OrbExtractor(ctx, NFEAT, SCALE, NLEVELS, 20, 7); lines = fe.LineExtractor(ctx, LCAP)
    try:
        single = [orb(f) + lines(f) for f in frames]
        assert all(len(s[0]) >= 50 and len(s[2]) >= 5 for s in single)
        big = np.random.default_rng(w).integers(0, 256, (n, h + 2, w + 5), dtype=np.uint8)
        big[:, :h, :w] = frames
        view = big[:, :h, :w]
        assert view.strides == ((h + 2) * (w + 5), w + 5, 1)
        pinned = torch.empty(frames.nbytes, dtype=torch.uint8, pin_memory=True)
        pv = pinned.numpy().reshape(frames.shape); pv[...] = frames
        for tag, images in (("compact", frames), ("padded view", view), ("pinned", pv)):
            out = fe.frontend_batch_alloc(n, orb.cap, LCAP)
            for a in out:
                a.view(np.uint8).reshape(-1)[...] = GUARD
            kp, desc, nk, kl, ld, fn, nl = _host_batch(fe, orb, lines, images, out, chunk)
            for i, (skp, sdesc, skl, sld, sfn) in enumerate(single):
                assert nk[i] == len(skp) and nl[i] == len(skl), (tag, i, nk, nl)
                np.testing.assert_array_equal(kp[i, :nk[i]].view(np.uint8), skp.view(np.uint8), err_msg="%s: keypoints of frame %d" % (tag, i))
                np.testing.assert_array_equal(desc[i, :nk[i]], sdesc, err_msg="%s: descriptors of frame %d" % (tag, i))
                np.testing.assert_array_equal(kl[i, :nl[i]].view(np.uint8), skl.view(np.uint8), err_msg="%s: keylines of frame %d" % (tag, i))
                np.testing.assert_array_equal(ld[i, :nl[i]], sld, err_msg="%s: LBD of frame %d" % (tag, i))
                np.testing.assert_array_equal(fn[i, :nl[i]], sfn, err_msg="%s: line functions of frame %d" % (tag, i))
        np.testing.assert_array_equal(big[:, :h, :w], frames)
        for i in (1, n - 1):                                   # an odd frame base inside a chunk, and the tail chunk
            skp, sdesc, skl, sld, sfn = single[i]
            okp, odesc = oracle.orb_extract(frames[i], NFEAT, SCALE, NLEVELS)
            okl, old, ofn, oraw = oracle.lines_extract(frames[i], LCAP)
            np.testing.assert_array_equal(skp.view(np.uint8), okp.view(np.uint8)); np.testing.assert_array_equal(sdesc, odesc)
            assert len(skl) == len(okl)
            for name in skl.dtype.names:
                if name == "angle":
                    assert _ulp_diff(skl[name], okl[name]).max(initial=0) <= 1
                else:
                    np.testing.assert_array_equal(skl[name], okl[name], err_msg=name)
            ham = np.unpackbits(sld ^ old, axis=1).sum(axis=1)
            assert (ham[skl["angle"].view(np.uint32) == okl["angle"].view(np.uint32)] == 0).all() and ham.max(initial=0) <= 8, ham
            np.testing.assert_array_equal(sfn, ofn)
    finally:
        orb.close(); lines.close()


# ---- argument errors of the two entry points --------------------------------------------------------------------------------------------

def test_invalid_layouts_are_rejected(fe, ctx):
    """a pitch below the width and frames that overlap (image_stride < pitch * (h - 1) + w with more than one frame) give SSLAM_ERR_INVALID before anything is
    enqueued: the outputs keep their guard bytes.  One frame never reads its image stride."""
    L = fe.lib()
    w, h, n = 160, 120, 2
    orb = fe.OrbExtractor(ctx, NFEAT, SCALE, NLEVELS, 20, 7); lines = fe.LineExtractor(ctx, LCAP)
    try:
        d_img = torch.zeros(2 * (w + 4) * h + 64, dtype=torch.uint8, device="cuda")
        d_a = torch.full((n * orb.cap * 68,), GUARD, dtype=torch.uint8, device="cuda"); d_b = torch.full((n * orb.cap * 32,), GUARD, dtype=torch.uint8, device="cuda")
        d_c = torch.full((n * orb.cap * 24,), GUARD, dtype=torch.uint8, device="cuda"); d_n = torch.full((n,), int(GUARD_I32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        o = lambda pitch, stride, nf: L.sslam_orb_extract_batch_dev(orb.h, fe._p(d_img), w, h, C.c_size_t(pitch), C.c_size_t(stride), nf, fe._p(d_a), fe._p(d_b), fe._p(d_n), orb.cap, None)
        l = lambda pitch, stride, nf: L.sslam_lines_extract_batch_dev(lines.h, fe._p(d_img), w, h, C.c_size_t(pitch), C.c_size_t(stride), nf, fe._p(d_a), fe._p(d_b), fe._p(d_c), fe._p(d_n), LCAP, None)
        INV = fe.SSLAM_ERR_INVALID
        for call, name in ((o, b"sslam_orb_extract_batch_dev"), (l, b"sslam_lines_extract_batch_dev")):
            assert call(w - 1, w * h, n) == INV and name in L.sslam_last_error()                    # pitch < w
            assert call(w - 1, w * h, 1) == INV
            assert call(w, w * h - 1, n) == INV and name in L.sslam_last_error()                    # overlapping frames, compact rows
            assert call(w + 4, (w + 4) * (h - 1) + w - 1, n) == INV                                 # overlapping frames, padded rows
            assert call(w, 0, n) == INV
            ctx.synchronize()
            for d in (d_a, d_b, d_c):
                assert bool((d == GUARD).all())
            assert bool((d_n == int(GUARD_I32)).all())
        for call in (o, l):
            assert call(w + 4, (w + 4) * (h - 1) + w, n) == 0                                       # the closest frames that do not overlap
            assert call(w, 0, 1) == 0                                                               # one frame: the image stride is not read
            ctx.synchronize()
    finally:
        orb.close(); lines.close()
