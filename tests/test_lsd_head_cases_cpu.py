"""The preconditions of tests/test_lsd_head_gpu.py, from the generators (tests/lsd_head_cases.py) and the oracle's own prologue alone (orc_lsd_prologue / orc_lsd_grad_table:
oracle/lsd_oracle.cpp, the per-pixel expressions the detector itself calls): a frame that does not fill a segment's list, cross a lane group with one bin or leave a tile
empty would pass on the device without testing the code it is named after.  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import lsd_head_cases as hc

_PRO = {}
NOTDEF = np.float32(-1024.0)


def _pro(oracle, name):
    """(oracle prologue, reach figures) of a case, computed once"""
    if name not in _PRO:
        p = oracle.lsd_prologue(hc.frame(name))
        h, w = hc.frame(name).shape
        _PRO[name] = (p, hc.reach(p, w, h))
    return _PRO[name]


def _show(name, r):
    print(name, {k: v for k, v in r.items() if k not in ("seg_cnt", "tile_cnt")}, "tiles", r["tile_cnt"].tolist())


@pytest.mark.parametrize("name", list(hc.CASES))
def test_export_is_consistent(oracle, name):
    """the planes describe one frame: defined <=> an angle in [0, 360) <=> |g|^2 at or above the table's smallest defined value; the border row and column are undefined;
    (cos, sin) are those of the gradient table's entry for the pixel's (gx, gy), recomputed here from the oracle's scaled image; the list holds every defined pixel once"""
    p, r = _pro(oracle, name)
    tab, smin = oracle.lsd_grad_table()
    deg, S, cs = p["deg"], p["S"], p["cs"]
    d = deg != NOTDEF
    assert (deg[d] >= 0).all() and (deg[d] < 360).all() and not np.signbit(deg[d]).any()
    assert not d[-1].any() and not d[:, -1].any() and (S[-1] == 0).all() and (S[:, -1] == 0).all()
    assert ((S >= smin) == d)[:-1, :-1].all() and p["n_defined"] == int(d.sum()) == len(p["order"]) == r["defined"]
    assert p["max_s"] == (int(S[d].max()) if d.any() else 0)
    assert len(np.unique(p["order"])) == len(p["order"]) and d.reshape(-1)[p["order"]].all()
    sc = oracle.lsd_scaled(hc.frame(name)).astype(np.int32)
    assert sc.shape == deg.shape
    DA, BC = sc[1:, 1:] - sc[:-1, :-1], sc[:-1, 1:] - sc[1:, :-1]
    gx, gy = DA + BC, DA - BC
    np.testing.assert_array_equal(S[:-1, :-1], gx * gx + gy * gy)
    e = tab[gy + 510, gx + 510]
    np.testing.assert_array_equal(e[..., 0].view(np.uint32), deg[:-1, :-1].view(np.uint32))
    np.testing.assert_array_equal(e[..., 1:3].view(np.uint32), cs[:-1, :-1].view(np.uint32))
    np.testing.assert_array_equal(e[..., 3].view(np.int32), S[:-1, :-1])


def test_gradient_table_structure(oracle):
    """orc_lsd_grad_table: |g|^2 in the fourth word, defined <=> sqrt(S / 4) > rho (float64 here, rho = 2 / sin(22.5 deg)) <=> S >= smin (the smallest integer the
    test accepts), undefined entries are
    (-1024, 0, 0), defined angles lie in [0, 360) with unit (cos, sin) to fp32, and the angle of the axis gradients is exact"""
    tab, smin = oracle.lsd_grad_table()
    g = np.arange(-510, 511, dtype=np.int64)
    S = g[None, :] ** 2 + g[:, None] ** 2
    np.testing.assert_array_equal(tab[..., 3].view(np.int32), S)
    rho = 2.0 / np.sin(np.pi * 22.5 / 180)
    d = np.sqrt(S / 4.0) > rho
    every = np.arange(0, 2 * 510 * 510 + 1)
    assert smin == int(every[np.sqrt(every / 4.0) > rho].min()) and ((S >= smin) == d).all()          # the smallest INTEGER the test accepts, a threshold
    print("smallest |g|^2 a gradient takes at or above it:", int(S[d].min()))          # [110; 113 = 64 + 49]
    assert smin <= int(S[d].min())
    np.testing.assert_array_equal(tab[..., 0] != NOTDEF, d)
    assert (tab[~d][:, 1:3] == 0).all() and (tab[d][:, 0] >= 0).all() and (tab[d][:, 0] < 360).all()
    n = np.hypot(tab[d][:, 1].astype(np.float64), tab[d][:, 2].astype(np.float64))
    assert np.abs(n - 1).max() < 2e-7
    # level-line angle = fastAtan2(gx, -gy): gy = 0, gx > 0 -> 90; gx = 0, gy < 0 -> 0; gy = 0, gx < 0 -> 270; gx = 0, gy > 0 -> 180
    assert tab[510, 510 + 100, 0] == 90 and tab[510 - 100, 510, 0] == 0 and tab[510, 510 - 100, 0] == 270 and tab[510 + 100, 510, 0] == 180
    print("smin", smin, "defined entries", int(d.sum()), "of", d.size)


def test_sort_edges(oracle):
    """the frames of the counting sort's edges reach them (figures of the run that chose the bounds in brackets)"""
    p, r = _pro(oracle, "tritri_640x60"); _show("tritri_640x60", r)
    assert (r["sw"], r["sh"], r["nxb"], r["tile_rows"]) == (512, 48, 2, 16)
    assert r["rows_with_full_segment"] >= 1 and r["tile_cnt"].max() > 8000          # [256 defined in a segment of 47 of the 48 rows; busiest tile 8 176 of 8 192]
    assert hc.forms("tritri_640x60") == (True, True)
    p, r = _pro(oracle, "tritri_330x40"); _show("tritri_330x40", r)
    assert (r["sw"], r["sh"], r["tile_rows"], r["ntiles"]) == (264, 32, 31, 2) and r["tile_cnt"][1] == 0 and r["tile_cnt"][0] > 0          # the second tile is the last row alone
    p, r = _pro(oracle, "tritri_645x60"); _show("tritri_645x60", r)
    assert (r["sw"], r["nxb"]) == (516, 3) and r["sw"] - 2 * hc.SEG_PX == 4 and r["seg_cnt"][:, 2].max() == 3          # a 4-pixel last segment, its last column undefined
    assert r["sw"] % 4 == 0 and 645 % 4 != 0 and hc.forms("tritri_645x60") == (False, True)          # k_blur7 + k_lsd_grad with the vector stores
    p, r = _pro(oracle, "ramp_320x240"); _show("ramp_320x240", r)
    assert r["distinct_bins"] < 32 and r["per_tile_bin_max"] > 64 * 12 and r["clamp_bin"] > 64          # [17 bins; 6 720 entries of one bin in a tile; 191 at bin 1023]
    p, r = _pro(oracle, "noise_320x240"); _show("noise_320x240", r)
    assert (r["sw"], r["nxb"]) == (256, 1) and r["distinct_bins"] > 500 and r["per_tile_bin_max"] <= 64 and r["near_int"] >= 1          # [760 bins; at most 54 a bin and tile; 47 near an integer]
    p, r = _pro(oracle, "noise_322x240"); _show("noise_322x240", r)
    assert (r["sw"], r["nxb"]) == (258, 2) and r["seg_cnt"][:, 1].max() == 1 and (r["seg_cnt"][:, 1] == 0).any()          # a 2-pixel second segment: one pixel can be defined
    p, r = _pro(oracle, "noise_333x251"); _show("noise_333x251", r)
    assert r["sw"] == 266 and r["sw"] % 4 != 0 and hc.forms("noise_333x251") == (False, True)          # the scalar-store branch
    p, r = _pro(oracle, "noise_2570x13"); _show("noise_2570x13", r)
    assert r["sw"] == 2056 > hc.SORT_XY and hc.forms("noise_2570x13") == (False, False) and (r["tile_cnt"] == 0).any() and r["tile_cnt"].max() > 0


def test_sparse_frames(oracle):
    p, r = _pro(oracle, "const_320x240"); _show("const_320x240", r)
    assert r["defined"] == 0 and p["max_s"] == 0 and len(p["order"]) == 0
    p, r = _pro(oracle, "one_square_320x240"); _show("one_square_320x240", r)
    assert 200 <= r["defined"] <= 999 and (r["tile_cnt"] == 0).any()          # [380]
    p, r = _pro(oracle, "dot_320x240"); _show("dot_320x240", r)
    assert 0 < r["defined"] < 64          # [26]
    p, r = _pro(oracle, "flat_top_320x240"); _show("flat_top_320x240", r)
    assert (r["tile_cnt"][:4] == 0).all() and r["tile_cnt"][5] > 1000          # [0, 0, 0, 0, 407, 7 640]


def test_smallest_frames(oracle):
    """the sizes at and around 10 x 10 and 20 x 10: the scaled sizes, which of them fuse, and something defined in each"""
    want = {(20, 10): (16, 8, True), (25, 10): (20, 8, False), (10, 10): (8, 8, False), (10, 40): (8, 32, False), (40, 10): (32, 8, True), (11, 13): (9, 10, False),
            (12, 12): (10, 10, False)}
    assert set(want) == set(hc.SMALL)
    for (w, h), (sw, sh, fused) in want.items():
        name = "strokes_%dx%d" % (w, h)
        p, r = _pro(oracle, name); _show(name, r)
        assert (r["sw"], r["sh"]) == (sw, sh) and hc.forms(name) == (fused, True) and r["defined"] > 0 and r["ntiles"] == 1


def test_batch_of_nine(oracle):
    """nine different 320 x 240 frames: eight go to the eight XCDs of sort_tile's first round, the ninth alone to the second; their largest |g|^2 differ, so a frame binned
    by a neighbour's maximum would show"""
    assert len(hc.BATCH9) == 9 and len(set(hc.BATCH9)) == 9
    ms = [oracle.lsd_prologue(hc.frame(n))["max_s"] for n in hc.BATCH9]
    print("max_s", ms)
    assert all(hc.frame(n).shape == (240, 320) for n in hc.BATCH9) and len(set(ms)) == 9


@pytest.mark.parametrize("name", list(hc.CASES) + [n for n in hc.BATCH9 if isinstance(n, tuple)])
def test_order_is_a_stable_sort_by_descending_bin(oracle, name):
    """independent of the C++: the oracle's defined-only seed list is a STABLE numpy argsort of the defined pixels in raster order by descending bin, the bin computed here
    in float64 as ll_angle's expression associates it, int(sqrt(S / 4) * (1023 / sqrt(maxS / 4))), clamped to 1023"""
    p = oracle.lsd_prologue(hc.frame(name)) if isinstance(name, tuple) else _pro(oracle, name)[0]
    d = (p["deg"] != NOTDEF).reshape(-1)
    idx = np.nonzero(d)[0]
    b = hc.bins(p["S"].reshape(-1)[idx], p["max_s"])
    want = idx[np.argsort(-b, kind="stable")]
    np.testing.assert_array_equal(p["order"], want)


def test_variants_change_the_prologue(oracle):
    """orc_lsd_prologue honours orc_set_lsd_resize and orc_set_lsd_seed_sort: the planes differ under the other resize, the planes are equal and the order differs (same
    multiset, same bins in descending order) under the other seed sort; the defaults come back"""
    img = hc.frame("noise_320x240"); base = _pro(oracle, "noise_320x240")[0]
    old = oracle.set_lsd_resize(1)
    try:
        q = oracle.lsd_prologue(img)
    finally:
        oracle.set_lsd_resize(old)
    assert (q["sw"], q["sh"]) == (base["sw"], base["sh"]) and (q["S"] != base["S"]).any()
    for name in ("noise_320x240", "ramp_320x240"):
        base = _pro(oracle, name)[0]
        old = oracle.set_lsd_seed_sort(1)
        try:
            q = oracle.lsd_prologue(hc.frame(name))
        finally:
            oracle.set_lsd_seed_sort(old)
        np.testing.assert_array_equal(q["deg"], base["deg"]); np.testing.assert_array_equal(q["S"], base["S"])
        assert q["max_s"] == base["max_s"] and (q["order"] != base["order"]).any()
        np.testing.assert_array_equal(np.sort(q["order"]), np.sort(base["order"]))
        coef = 1023.0 / np.sqrt(q["max_s"] / 4.0)          # (upstream's sort key is not clamped)
        key = (np.sqrt(q["S"].reshape(-1)[q["order"]] / 4.0) * coef).astype(np.int64)
        assert (np.diff(key) <= 0).all()
    again = oracle.lsd_prologue(img)
    np.testing.assert_array_equal(again["order"], _pro(oracle, "noise_320x240")[0]["order"])
