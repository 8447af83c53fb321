"""GPU: the ORB tail (k_octree, k_describe: csrc/orb.hip) on injected candidates -- sslam_testing_orb_tail runs the product path's preparation, front and tail on the lists
of tests/orb_tail_cases.py (whose reach tests/test_orb_tail_cases_cpu.py proves from the oracle's trace alone) -- against the oracle's tail.  Every comparison is byte for
byte: all seven words of every keypoint, every descriptor, the frame counts, the per-level counts; rows at and past a frame's count still hold the fill byte.  Then the
limits of the point branch: the quadtree's LDS beyond 64 KB, the sizes build_plan refuses, the widest level it takes."""
import ctypes as C
import re
import numpy as np
import pytest
import orb_tail_cases as oc
from synth import synth_frame, noise_frame

pytestmark = pytest.mark.gpu


class OrbTail:
    """a sslam_orb handle of the TESTING library (its kernels' constant tables are uploaded per library) and its injection entry point"""
    def __init__(self, fe, ctx, nfeatures, nlevels):
        self.T = fe.testing_lib()
        self.T.sslam_testing_orb_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fe, self.nlevels = fe, nlevels
        self.h = C.c_void_p()
        assert self.T.sslam_orb_create(ctx.h, int(nfeatures), C.c_float(1.2), int(nlevels), 20, 7, C.byref(self.h)) == 0

    def __enter__(self): return self

    def __exit__(self, *a):
        self.T.sslam_orb_destroy(self.h)

    def raw(self, images, cands, cap):
        """cands[frame][level] = n x 3 -> status, (keypoints [nf, cap], descriptors [nf, cap, 32], counts [nf], level counts [nf, nlevels], k_octree's dynamic LDS)"""
        images = np.ascontiguousarray(images, np.uint8)
        nf, h, w = images.shape
        cand, nc = oc.pack(cands, self.nlevels)
        assert len(cand) == nf
        kp = np.zeros((nf, cap), self.fe.KP_DTYPE); desc = np.zeros((nf, cap, 32), np.uint8); cnt = np.zeros(nf, np.int32); lc = np.zeros((nf, self.nlevels), np.int32)
        lds = C.c_size_t(0)
        p = lambda a: a.ctypes.data
        rc = self.T.sslam_testing_orb_tail(self.h, p(images), w, h, w, w * h, nf, p(cand), p(nc), cand.shape[2], cap, p(kp), p(desc), p(cnt), p(lc), C.addressof(lds))
        return rc, (kp, desc, cnt, lc, lds.value)

    def __call__(self, images, cands, cap):
        rc, out = self.raw(images, cands, cap)
        assert rc == 0, self.T.sslam_last_error()
        return out


def _untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == 0xA5).all()


def _check_frame(oracle, img, per, nfeatures, nlevels, cap, kp, desc, n, lc, tag):
    """one frame of a hook call against the oracle's tail on the same lists"""
    okp, odesc, olc, total, tr = oracle.orb_tail(img, per, nfeatures, nlevels=nlevels, cap=cap)
    assert lc.tolist() == olc.tolist(), (tag, "level counts", lc, olc)
    assert n == min(total, cap) == len(okp), (tag, n, total, cap)
    g, w = kp[:n].view(np.uint32).reshape(n, 7), okp.view(np.uint32).reshape(n, 7)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, (tag, "keypoints", len(bad), bad[:5], kp[bad[:5]], okp[bad[:5]])
    bad = np.nonzero((desc[:n] != odesc).any(axis=1))[0]
    assert len(bad) == 0, (tag, "descriptors", len(bad), bad[:5], kp[bad[:5]])
    assert _untouched(kp[n:]) and _untouched(desc[n:]), (tag, "rows past the count were written")
    return tr


def _run_octree(fe, ctx, oracle, case):
    cap = case["N"] + 24          # (a first pass may leave four nodes per root strip, whatever N)
    with OrbTail(fe, ctx, case["N"], 1) as t:
        kp, desc, cnt, lc, lds = t(oc.image(case["img"])[None], [[case["cand"]]], cap)
    tr = _check_frame(oracle, oc.image(case["img"]), [case["cand"]], case["N"], 1, cap, kp[0], desc[0], int(cnt[0]), lc[0], case["name"])
    assert lc[0, 0] == tr[0]["final_nodes"] == cnt[0] <= cap
    return kp[0][:cnt[0]], lds


def _family(fe, ctx, oracle, prefix, at_least):
    cases = [c for k, c in oc.octree_cases(oracle).items() if k.startswith(prefix)]
    assert len(cases) >= at_least
    return {c["name"]: _run_octree(fe, ctx, oracle, c)[0] for c in cases}


def test_loop_ends(fe, ctx, oracle):
    """a second-phase break at N, N + 1 and N + 2, a second-phase round that runs out, the first phase ending at >= N and without growth, N = 0 and 1"""
    out = _family(fe, ctx, oracle, "end_", 9)
    assert len(out["end_N0"]) == 4 and len(out["end_N1_one_candidate"]) == 1


def test_sorted_lengths(fe, ctx, oracle):
    """the bitonic sort of the expandable nodes at 1, 2, 63, 64, 65, 128, 129 and 300 entries"""
    _family(fe, ctx, oracle, "sort_", 8)


def test_ties(fe, ctx, oracle):
    """every sorted entry of one size (creation order alone decides), all responses equal and the maximal response twice in a node (the first in arrival order wins),
    each in a cell-raster-like and in a shuffled arrival order"""
    out = _family(fe, ctx, oracle, "tie_", 6)
    assert out["tie_all_responses_raster"].tobytes() != out["tie_all_responses_shuffled"].tobytes()


def test_node_sizes(fe, ctx, oracle):
    """a node of exactly 64, 65, 128 and 129 candidates, a chunked division with empty classes, the dense lattice"""
    _family(fe, ctx, oracle, "node_", 7)


def test_root_strips(fe, ctx, oracle):
    """five root strips with hX = 73.6: candidates on and beside every strip edge, empty strips, a strip of one and strips of more than 64"""
    _family(fe, ctx, oracle, "roots_", 5)


def _run_batch(fe, ctx, oracle, c, tag, cap=None):
    cap = cap or c["cap"]
    with OrbTail(fe, ctx, c["nfeatures"], c["nlevels"]) as t:
        kp, desc, cnt, lc, lds = t(c["images"], c["cands"], cap)
    for f in range(len(c["images"])):
        _check_frame(oracle, c["images"][f], c["cands"][f], c["nfeatures"], c["nlevels"], cap, kp[f], desc[f], int(cnt[f]), lc[f], "%s frame %d" % (tag, f))
    return kp, desc, cnt, lc


def test_batch_of_73_frames_by_3_levels(fe, ctx, oracle):
    """every (frame, level) list different, some empty: the level a workgroup of k_octree takes beyond 8 and 64 frames"""
    kp, desc, cnt, lc = _run_batch(fe, ctx, oracle, oc.batch_case(), "batch")
    assert cnt[0] == 0 and (lc == 0).sum() >= 10 and (cnt > 100).sum() >= 30


@pytest.mark.parametrize("img", ["noise192", "noise199"])
def test_describe_at_the_borders(fe, ctx, oracle, img):
    """every position within 12 pixels of a border of the detection range on 3 levels: both staging paths of k_describe, all four shifts of the aligned one, and on the
    192-wide level 0 the keypoints that fail only `ax + 48 <= pitch`"""
    c = oc.border_case(img)
    kp, desc, cnt, lc = _run_batch(fe, ctx, oracle, c, "border " + img)
    assert lc.tolist() == [[len(x) for x in per] for per in c["cands"]]          # everything survives


def test_describe_moments_and_scores(fe, ctx, oracle):
    """a constant image and the eight exact ramps: zero, axis and diagonal moments; scores 1 and 255"""
    c = oc.moments_case()
    kp, desc, cnt, lc = _run_batch(fe, ctx, oracle, c, "moments")
    assert (cnt == 60).all() and (kp[0][:60]["angle"] == 0).all() and {1.0, 255.0} <= set(kp[3][:60]["response"].tolist())
    for f, a in ((1, 0.0), (2, 180.0), (3, 90.0), (4, 270.0)):
        assert (kp[f][:60]["angle"] == np.float32(a)).all(), oc.RAMPS[f]


def test_describe_cuts_at_the_cap(fe, ctx, oracle):
    """cap at the total, one below, inside the middle level and 1"""
    c = oc.cap_case()
    for cap in (150, 149, 65, 1):
        kp, desc, cnt, lc = _run_batch(fe, ctx, oracle, c, "cap %d" % cap, cap=cap)
        assert cnt[0] == cap and lc[0].tolist() == [40, 50, 60]


def test_hook_equals_product(fe, ctx):
    """the candidates of a normal extraction by the PRODUCT library, fed to the hook: keypoints and descriptors byte for byte"""
    img = synth_frame(2001, w=320, h=240)
    ex = fe.OrbExtractor(ctx, 500, 1.2, 8, 20, 7)
    try:
        kp, desc = ex(img)
        cands = [ex.debug_candidates(0, l) for l in range(8)]
        cap = ex.cap
    finally:
        ex.close()
    assert len(kp) > 300 and sum(len(c) for c in cands) > len(kp)
    with OrbTail(fe, ctx, 500, 8) as t:
        hkp, hdesc, cnt, lc, lds = t(img[None], [cands], cap)
        back = np.zeros((4000, 3), np.int32); m = C.c_int(0)          # what the hook left in the cells reads back as the injected list
        assert t.T.sslam_orb_debug_candidates(t.h, 0, 0, C.c_void_p(back.ctypes.data), 4000, C.byref(m)) == 0
        assert np.array_equal(back[:m.value], cands[0])
    assert cnt[0] == len(kp) == lc[0].sum()
    assert hkp[0][:len(kp)].tobytes() == kp.tobytes() and hdesc[0][:len(kp)].tobytes() == desc.tobytes()


def test_invalid_lists_are_refused(fe, ctx):
    img = oc.image("noise160")[None]
    L = oc.levels(160, 120, 1)[0]
    ok = np.array([[5, 5, 10], [9, 9, 20], [100, 70, 30]], np.int32)          # (the first two share every box down to no growth: one node; the third is another)
    with OrbTail(fe, ctx, 100, 1) as t:
        for bad, what in (([L["W"], 5, 10], b"outside"), ([5, L["H"], 10], b"outside"), ([-1, 5, 10], b"outside"), ([5, 5, 0], b"outside"), ([5, 5, 256], b"outside"), ([9, 9, 30], b"one pixel")):
            rc, _ = t.raw(img, [[np.vstack([ok, [bad]]).astype(np.int32)]], 50)
            assert rc == -1 and what in t.T.sslam_last_error(), (bad, t.T.sslam_last_error())
        many = np.zeros((L["cand_cap"] + 1, 3), np.int32)
        rc, _ = t.raw(img, [[many]], 50)
        assert rc == -1 and str(L["cand_cap"]).encode() in t.T.sslam_last_error()
        kp, desc, cnt, lc, lds = t(img, [[ok]], 50)          # and the handle still works
        assert cnt[0] == 2 and lc[0, 0] == 2


# ---------------------------------------------------------------------------------------------------------------- size limits of the point branch
def test_octree_lds_beyond_64k(fe, ctx, oracle):
    """N = 2000 on one level, 4200 candidates: the k_octree launch asks for more than 64 KB of dynamic LDS and runs"""
    c = oc.big_lds_case()
    kp, lds = _run_octree(fe, ctx, oracle, c)
    want, nc = oc.octree_lds_bytes([c["N"]], [oc.levels(199, 151, 1)[0]])
    print("k_octree dynamic LDS: %d bytes, %d keypoints" % (lds, len(kp)))
    assert lds == want > 65536 and 2000 <= len(kp) <= 2002


def _refused(fe, ctx, nfeatures, img):
    ex = fe.OrbExtractor(ctx, nfeatures, 1.2, 1, 20, 7)
    try:
        with pytest.raises(fe.SslamError) as e:
            ex(img)
        assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED, e.value
        return str(e.value)
    finally:
        ex.close()


def _exact(fe, ctx, oracle, nfeatures, img, nlevels=1):
    ex = fe.OrbExtractor(ctx, nfeatures, 1.2, nlevels, 20, 7)
    try:
        kp, desc = ex(img)
    finally:
        ex.close()
    okp, odesc = oracle.orb_extract(img, nfeatures, nlevels=nlevels)
    assert len(kp) == len(okp) and kp.tobytes() == okp.tobytes() and desc.tobytes() == odesc.tobytes()
    return kp


def test_nfeatures_beyond_the_lds_limit_is_refused(fe, ctx, oracle):
    """build_plan holds k_octree's LDS need against the device's limit and the node capacity against the 16-bit slot: SSLAM_ERR_UNSUPPORTED naming nfeatures and the level,
    nothing launched; just below the limit the extractor runs and is exact, and so is a normal extractor afterwards"""
    img = oc.image("noise160")
    L = oc.levels(160, 120, 1)[0]
    msg = _refused(fe, ctx, 70000, img)
    assert "nfeatures 70000" in msg and "level 0" in msg and "16-bit" in msg
    msg = _refused(fe, ctx, 60000, img)
    assert "nfeatures 60000" in msg and "level 0" in msg and "LDS" in msg
    limit = int(re.search(r"the device allows (\d+)", msg).group(1))
    need = lambda n: oc.octree_lds_bytes([n], [L])[0]
    assert 65536 <= limit < need(60000)
    n = next(n for n in range(1, 60000) if need(n) > limit)          # the formula's first nfeatures above the limit
    print("device LDS limit %d bytes: nfeatures %d needs %d, %d needs %d" % (limit, n, need(n), n - 1, need(n - 1)))
    msg = _refused(fe, ctx, n, img)
    assert "nfeatures %d" % n in msg and str(need(n)) in msg
    assert need(n - 1) <= limit
    assert len(_exact(fe, ctx, oracle, n - 1, img)) > 50          # the largest quadtree the device takes
    assert len(_exact(fe, ctx, oracle, 500, img, nlevels=3)) > 50


def test_widest_and_narrowest_levels(fe, ctx, oracle):
    """4111 x 100: the widest level build_plan takes (12-bit coordinates), 60 root strips; 64 x 4111: no root (nIni == 0), no keypoints; a side of 4112 is refused; 4111 x 64
    would start with 127 roots and is refused; the same extractor is exact again after a refused size"""
    wide = noise_frame(801, w=4111, h=100)
    assert oc.levels(4111, 100, 1)[0]["nIni"] == 60
    kp = _exact(fe, ctx, oracle, 3000, wide)
    assert len(kp) > 1000 and kp["x"].max() > 4000
    assert len(_exact(fe, ctx, oracle, 3000, noise_frame(802, w=64, h=4111))) == 0
    small = oc.image("noise160")
    ex = fe.OrbExtractor(ctx, 300, 1.2, 1, 20, 7)
    try:
        kp0, d0 = ex(small)
        for bad, what in ((noise_frame(803, w=4112, h=100), "unsupported"), (noise_frame(804, w=100, h=4112), "unsupported"), (noise_frame(805, w=4111, h=64), "root nodes")):
            with pytest.raises(fe.SslamError) as e:
                ex(bad)
            assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED and what in str(e.value)
            kp1, d1 = ex(small)
            assert kp1.tobytes() == kp0.tobytes() and d1.tobytes() == d0.tobytes()
    finally:
        ex.close()
    okp, od = oracle.orb_extract(small, 300, nlevels=1)
    assert kp0.tobytes() == okp.tobytes() and d0.tobytes() == od.tobytes()
