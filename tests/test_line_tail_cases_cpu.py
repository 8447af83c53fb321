"""The preconditions of tests/test_line_tail_gpu.py, from the generators (tests/line_tail_cases.py) and the oracle alone: a case that does not reach the branch,
the clamp or the tie it is named after would pass on the device without testing anything."""
import numpy as np
import pytest
import line_tail_cases as lc


def _tail(oracle, case, segs=None):
    segs = case["segs"] if segs is None else segs
    return oracle.lines_tail(case["img"], segs, case["max_lines"], cap=case["cap"])


def test_images():
    for name, (w, h, _) in lc.IMAGES.items():
        assert lc.image(name).shape == (h, w)
    assert lc.IMAGES["noise160"][0] % 4 == 0 and lc.IMAGES["noise199"][0] % 4 != 0
    assert lc.IMAGES["strip16384"][0] == 16384 and lc.IMAGES["strip16388"][0] > 16384 >= lc.IMAGES["strip16388"][1] and lc.IMAGES["tower16388"][1] > 16384 >= lc.IMAGES["tower16388"][0]
    assert len(lc.directions()) == 368


@pytest.mark.parametrize("name", list(lc.IMAGES))
def test_direction_case_reaches_every_mapping_and_length(oracle, name):
    """no sort, no clamp: row i is segment i; the lengths are the intended ones (every residue mod 8, walks shorter than one block), every gather mapping of k_lbd gets
    at least 40 lines, the exact directions give the exact angles, and the long line spans the image"""
    c = lc.direction_case(name)
    kl, ld, fn = _tail(oracle, c)
    w, h = lc.IMAGES[name][:2]
    assert len(kl) == len(c["segs"]) == 368 * len(lc.NPX) + 1 <= lc.MAX_SEG
    for f, col in (("startPointX", 0), ("startPointY", 1), ("endPointX", 2), ("endPointY", 3)):
        np.testing.assert_array_equal(kl[f], c["segs"][:, col])
    short = np.arange(len(kl)) != lc.LONG_AT
    np.testing.assert_array_equal(kl["numOfPixels"][short], c["npx"][short])
    assert sorted(set(kl["numOfPixels"][short])) == list(range(2, 18)) and set(kl["numOfPixels"][short] % 8) == set(range(8)) and (kl["numOfPixels"][short] < lc.LBD_TB).any()
    assert kl["numOfPixels"][lc.LONG_AT] == max(w, h) == c["npx"][lc.LONG_AT]
    if max(w, h) > 1000: assert kl["numOfPixels"][lc.LONG_AT] > 16000
    cls = lc.lgs_class(kl["angle"])
    assert (np.bincount(cls, minlength=4) >= 40).all(), np.bincount(cls, minlength=4)
    for n in lc.NPX:          # every length in every mapping
        assert set(cls[short & (kl["numOfPixels"] == n)]) == {0, 1, 2, 3}
    exact = kl["angle"][short][-8 * len(lc.NPX)::len(lc.NPX)]
    want = np.array([0, np.pi / 2, np.pi, -np.pi / 2, np.pi / 4, 3 * np.pi / 4, -np.pi / 4, -3 * np.pi / 4]).astype(np.float32)
    np.testing.assert_array_equal(exact, want)
    assert len(np.unique(kl["angle"][short])) >= 360


@pytest.mark.parametrize("name", lc.SMALL)
def test_border_case_fires_every_clamp_and_border(oracle, name):
    c = lc.border_case(name)
    kl, ld, fn = _tail(oracle, c)
    h, w = c["img"].shape
    assert len(kl) == len(c["segs"])
    fired = lc.clamps_fired(c, kl)
    assert (fired.sum(axis=0) >= 1).all(), dict(zip(lc.CLAMPS, fired.sum(axis=0)))
    s = c["segs"]
    # a coordinate exactly w / h is clamped, the float just below it is not
    wb, hb = np.nextafter(np.float32(w), np.float32(0)), np.nextafter(np.float32(h), np.float32(0))
    for col, f, lim, below, k in ((0, "startPointX", w, wb, 1), (2, "endPointX", w, wb, 3), (1, "startPointY", h, hb, 5), (3, "endPointY", h, hb, 7)):
        at = s[:, col] == np.float32(lim)
        assert at.any() and fired[at, k].all() and (kl[f][at] == lim - 1).all()
        jb = s[:, col] == below
        assert jb.any() and not fired[jb].any() and (kl[f][jb] == below).all()
    assert (kl["lineLength"] > 0).all() and np.isfinite(fn).all()          # nothing clamps to zero length
    for f, v in (("startPointY", 0), ("startPointY", h - 1), ("startPointX", 0), ("startPointX", w - 1)):          # lines lying ON each border row / column
        other = f.replace("start", "end")
        assert ((kl[f] == v) & (kl[other] == v)).sum() >= 4
    for cx in (0, w - 1):          # lines into and out of each corner
        for cy in (0, h - 1):
            assert ((kl["endPointX"] == cx) & (kl["endPointY"] == cy)).sum() >= 10 and ((kl["startPointX"] == cx) & (kl["startPointY"] == cy)).sum() >= 10
    xmn, xmx, ymn, ymx = lc.walk_extent(kl)
    assert (xmn < -1).sum() >= 20 and (xmx > w).sum() >= 20 and (ymn < -1).sum() >= 20 and (ymx > h).sum() >= 20          # walks clamped at each border


def test_count_case_ties_and_chunks(oracle):
    c = lc.count_case()
    assert tuple(c["counts"]) == lc.COUNTS == (0, 1, 39, 40, 41, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8192) and c["max_lines"] == 40 < c["cap"]
    assert c["segs"].shape == (15, lc.MAX_SEG, 4) and c["images"].shape == (15, 120, 160)
    assert lc.KL_LDS in lc.COUNTS and lc.KL_LDS + 1 in lc.COUNTS and max(lc.COUNTS) == lc.MAX_SEG
    for f, n in enumerate(lc.COUNTS):
        nc = int(c["ncand"][f]); fl = c["accept"][f, :nc]
        seg = lc.accepted(c, f)
        assert len(seg) == n == fl.sum() and nc <= lc.MAX_SEG
        assert len(np.unique(c["segs"][f, :nc], axis=0)) == nc          # a row identifies its candidate
        if n == lc.MAX_SEG: assert nc == n                               # (the candidate limit leaves no room for a rejected one)
        else: assert nc > n and (n == 0 or 0.2 <= (nc - n) / nc <= 0.5)
        if n >= 255 and n < lc.MAX_SEG:                                  # rejected candidates on both sides of the first 256-candidate chunk boundary, accepted ones behind it
            assert fl[255] == 0 and fl[256] == 0 and fl[:255].any() and fl[257:].any()
        kall = oracle.lines_tail(c["img"], seg, max(n, 1), cap=max(n, 1))[0]
        k40 = oracle.lines_tail(c["img"], seg, 40, cap=c["cap"])[0]
        assert len(kall) == n and len(k40) == min(n, 40)
        for fld, col in (("startPointX", 0), ("startPointY", 1), ("endPointX", 2), ("endPointY", 3)):          # inside the image: no clamp
            np.testing.assert_array_equal(kall[fld], seg[:, col])
        if n <= 40:
            assert k40.tobytes() == kall.tobytes()
            continue
        order = np.argsort(-kall["response"].astype(np.float64), kind="stable")          # descending response, emission order among equals
        r = kall["response"][order]
        assert r[39] == r[40], "no response tie across the cut"
        assert len(np.unique(r)) == 5
        want = kall[order[:40]].copy(); want["class_id"] = np.arange(40)
        assert k40.tobytes() == want.tobytes()                           # the oracle's tied rows follow emission order
        tied = order[:40][r[:40] == r[39]]
        assert (np.diff(tied) > 0).all() and tied.max() < order[40]


def test_full_and_small_cap_cases(oracle):
    c = lc.full_case()
    kl = _tail(oracle, c)[0]
    assert len(kl) == lc.MAX_SEG == c["max_lines"] and (kl["class_id"] == np.arange(lc.MAX_SEG)).all()
    c = lc.small_cap_case()
    kl = _tail(oracle, c)[0]
    assert len(c["segs"]) > c["max_lines"] > c["cap"] == len(kl) == 17


def test_squares_frame_has_70_segments_of_one_response(oracle):
    img = lc.squares_frame()
    assert img.shape == (240, 320) and set(np.unique(img)) == {110, 200} and (img == 200).sum() == 35 * 400 and img[20, 20] == 200 and img[19, 19] == 110
    kl, ld, fn, raw = oracle.lines_extract(img, 1000)
    assert len(raw) == len(kl) == 70 and len(np.unique(kl["response"])) == 1
    k40 = oracle.lines_extract(img, 40)[0]
    want = kl[:40].copy()
    assert k40.tobytes() == want.tobytes()                               # the first 40 in emission order
