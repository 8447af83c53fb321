"""The inputs of tests/test_tri_batch_gpu.py reach what they are meant to reach, shown on the CPU with helper + oracle (tests/tri_batch_cases.py): every
named gate case has exactly the stated outcome and sits on the number its name says, the ragged batch matches, the rotation cases prune.  Where the
reference's own SearchForTriangulation was built (oracle/_ref/libref_slices.so), it agrees with helper + oracle on every case: it takes the node
arrays directly, and forms its epipole from a pose (identity) and a camera centre chosen so that the epipole is the case's."""
import ctypes as C
import os
import numpy as np
import pytest
import tri_batch_cases as tc
import match_cases as mc
import rot_cases

SLICES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_slices.so")


def gate_cases():
    """name -> (pair, winning candidate position or None / matched flag): the generators at the seeds the GPU test uses"""
    out = {}
    out.update(tc.lane_cases(np.random.default_rng(7600)))
    out.update(tc.tie_cases(np.random.default_rng(7610)))
    out.update(tc.epipole_cases(np.random.default_rng(7620)))
    out.update(tc.epipolar_cases(np.random.default_rng(7630)))
    return out


def all_pairs():
    out = {k: v[0] for k, v in gate_cases().items()}
    sides, pairs = tc.ragged_pool(np.random.default_rng(7700))
    for os_ in (0, 1):
        for a, b in pairs:
            out["ragged_%d_%d_stereo%d" % (a, b, os_)] = tc.pair(sides[a], sides[b], only_stereo=bool(os_))
    out.update({"rot_" + k: v for k, v in tc.rot_pairs().items()})
    m = tc.two_motions(np.random.default_rng(7640))
    out["motion_0"], out["motion_1"] = m
    out["zero_F12"] = tc.zero_F12(m[0])
    out["bow_case"] = tc.from_bow_case(np.random.default_rng(7650), 60)
    return out


def test_motion_is_the_existing_one():
    mot = tc.motion()
    np.testing.assert_array_equal(mot["F12"], mc.tri_F12())
    assert (mot["ex"], mot["ey"]) == mc.TRI_EPIPOLE
    assert (tc.W, tc.ROW_BYTES, tc.LDS_CAP, tc.PLAIN_CAP) == (8, 48, 1365, 1024)


def winner(c, m):
    """position among the candidates of the row the query was matched to, None without a match"""
    r = int(m[c["q"]])
    return None if r < 0 else int(np.flatnonzero(c["cand"] == r)[0])


def test_gate_cases_have_the_stated_outcome(oracle):
    for name, (c, want) in gate_cases().items():
        m, n = tc.expect(oracle, c)
        got = winner(c, m)
        if isinstance(want, bool):
            assert (got is not None) == want, (name, got)
        else:
            assert got == want, (name, got, want)
        assert n == (0 if got is None else 1), name             # the fillers never match


def test_gate_cases_sit_on_their_numbers(oracle):
    G = gate_cases()
    d = lambda c, k: tc.hamming(c["s1"]["desc"][c["q"]], c["s2"]["desc"][c["cand"][k]])
    c = G["tie_3"][0]; assert [d(c, k) for k in range(4)] == [12, 12, 12, 40]
    c = G["tie_2"][0]; assert [d(c, k) for k in range(2)] == [12, 12] and not np.array_equal(c["s2"]["desc"][c["cand"][0]], c["s2"]["desc"][c["cand"][1]])
    assert d(G["dist_50"][0], 0) == 50 == tc.TH_LOW and d(G["dist_51"][0], 0) == 51
    for name, closer, farther in (("closer_fails_before", 0, 1), ("closer_fails_after", 1, 0)):
        c = G[name][0]
        assert d(c, closer) == 5 and d(c, farther) == 20 and (c["cand"][closer] < c["cand"][farther]) == (name == "closer_fails_before")
        k1 = c["s1"]["kp"][c["q"]]; k2 = c["s2"]["kp"][c["cand"]]
        ok = [tc.epi_ok(c["F12"], k1["x"], k1["y"], k2["x"][k], k2["y"][k], tc.SIGMA2[0]) for k in (closer, farther)]
        assert ok == [False, True], name
    for m in (1, 63, 64, 65, 129):
        names = [k for k in G if k.startswith("lane_%d_" % m)]
        assert len(names) == (1 if m == 1 else 3)
        for k in names:
            c = G[k][0]
            assert (c["s2"]["node"] == tc.QNODE).sum() == m and (c["s1"]["node"] == tc.QNODE).sum() == 1
    # the epipole gate: the two x coordinates are neighbouring floats on either side of the strict <, for a scale of 1 and a scale above 1
    for octave in (0, 3):
        ci, co = G["epipole_oct%d_inside" % octave][0], G["epipole_oct%d_outside" % octave][0]
        xi = ci["s2"]["kp"]["x"][ci["cand"][0]]; xo = co["s2"]["kp"]["x"][co["cand"][0]]
        assert np.nextafter(xi, np.float32(1e9)) == xo and ci["s2"]["kp"]["octave"][ci["cand"][0]] == octave
        assert tc.epipole_rejects(ci["ex"], ci["ey"], xi, ci["ey"], tc.SCALE[octave]) and not tc.epipole_rejects(ci["ex"], ci["ey"], xo, ci["ey"], tc.SCALE[octave])
        for which in ("inside_stereo1", "inside_stereo2"):
            cs = G["epipole_oct%d_%s" % (octave, which)][0]
            assert cs["s2"]["kp"]["x"][cs["cand"][0]] == xi
            assert (cs["s1"]["uright"][cs["q"]] >= 0) != (cs["s2"]["uright"][cs["cand"][0]] >= 0)
    assert tc.SCALE[0] == 1 and tc.SCALE[3] > 1.7
    # the epipolar gate: neighbouring offsets on either side of 3.84 * sigma2, for two octaves
    for octave in (0, 2):
        cb, ca = G["epipolar_oct%d_below" % octave][0], G["epipolar_oct%d_above" % octave][0]
        k1 = cb["s1"]["kp"][cb["q"]]
        yb = cb["s2"]["kp"]["y"][cb["cand"][0]]; ya = ca["s2"]["kp"]["y"][ca["cand"][0]]; x = cb["s2"]["kp"]["x"][cb["cand"][0]]
        db, da = tc.epi_dsqr(cb["F12"], k1["x"], k1["y"], x, yb), tc.epi_dsqr(ca["F12"], k1["x"], k1["y"], x, ya)
        lim = 3.84 * float(tc.SIGMA2[octave])
        assert float(db) < lim <= float(da) and float(da) - float(db) < 1e-3 * lim and 0 < ya - yb < 1e-3, (octave, db, da, lim)


def test_ragged_batch_matches(oracle):
    sides, pairs = tc.ragged_pool(np.random.default_rng(7700))
    counts = sorted(set(len(s["kp"]) for s in sides))
    assert counts == [0, 1, 63, 64, 65, 70, 80, tc.RAGGED_CAP] and len(sides) == 12
    assert (sides[7]["node"] < 0).all() and not np.intersect1d(sides[8]["node"], np.concatenate([s["node"] for i, s in enumerate(sides) if i != 8])).size
    combos = set((len(sides[a]["kp"]) == 0, len(sides[b]["kp"]) == 0) for a, b in pairs)
    assert combos == {(False, False), (True, False), (False, True), (True, True)}
    for s in sides[:2]:
        assert 0 < (s["uright"] >= 0).sum() < len(s["kp"]) and 0 < s["free"].sum() < len(s["kp"])      # both kinds of row on both kinds of side
    for only_stereo, need in ((0, 10), (1, 3)):
        for ori in (0, 1):
            n = {(a, b): tc.expect(oracle, tc.pair(sides[a], sides[b], only_stereo=bool(only_stereo), ori=bool(ori)))[1] for a, b in pairs}
            full = [k for k in pairs if len(sides[k[0]]["kp"]) and len(sides[k[1]]["kp"])]
            assert 2 * sum(n[k] >= need for k in full) >= len(full), (only_stereo, ori, n)
            assert all(n[k] == 0 for k in pairs if k not in full) and n[(7, 0)] == 0 and n[(1, 8)] == 0
    assert any(n[k] >= 10 for k in pairs)          # (even under bOnlyStereo)


def test_rotation_cases_prune(oracle):
    R = tc.rot_pairs()
    for name, c in R.items():
        rc = c["rc"]
        m, n = tc.expect(oracle, c)
        plain, nplain = tc.expect(oracle, dict(c, ori=False))
        wm, wn = rot_cases.want_12(rc, True)
        assert nplain == len(rc["i1"]) and n == wn < nplain, (name, n, wn, nplain)
        if not name.startswith("neighbour_90"): np.testing.assert_array_equal(m, wm, err_msg=name)
    # the neighbours: equal matches before the check, each loses its own group of 2; added histograms would keep it in the first pair
    c0, c1 = R["neighbour_0"], R["neighbour_90"]
    m0, m1 = tc.expect(oracle, c0)[0], tc.expect(oracle, c1)[0]
    np.testing.assert_array_equal(m0, m1)
    b0 = rot_cases.rot_bin(c0["s1"]["kp"]["angle"][m0 >= 0], c0["s2"]["kp"]["angle"][m0[m0 >= 0]]); b1 = rot_cases.rot_bin(c1["s1"]["kp"]["angle"][m1 >= 0], c1["s2"]["kp"]["angle"][m1[m1 >= 0]])
    assert sorted(set(b0.tolist())) == [3, 6] and sorted(set(b1.tolist())) == [6, 9]
    h = np.bincount(np.concatenate([rot_cases.rot_bin(c["s1"]["kp"]["angle"][c["rc"]["i1"]], c["s2"]["kp"]["angle"][c["rc"]["i2"]]) for c in (c0, c1)]), minlength=13)
    assert h[[3, 6, 9]].tolist() == [30, 33, 5] and h[12] + h[0] == 2          # (the turned group of 2 straddles 360 degrees: bins 12 and 0)


def test_other_cases(oracle):
    m = tc.two_motions(np.random.default_rng(7640))
    own = [tc.expect(oracle, c)[1] for c in m]
    crossed = [tc.expect(oracle, dict(m[i], F12=m[1 - i]["F12"], ex=m[1 - i]["ex"], ey=m[1 - i]["ey"]))[1] for i in (0, 1)]
    assert min(own) > 20 and max(crossed) < min(own) // 2, (own, crossed)          # a kernel that reads another pair's F12 shows
    assert tc.expect(oracle, tc.zero_F12(m[0]))[1] == 0
    sides = tc.neighbours_pool(np.random.default_rng(7660))
    n = [tc.expect(oracle, tc.pair(sides[0], s))[1] for s in sides[1:]]
    assert len(n) == 20 and min(n) > 5 and len(set(n)) > 3, n
    assert tc.expect(oracle, tc.from_bow_case(np.random.default_rng(7650), 60))[1] > 30
    for cap in (tc.PLAIN_CAP, tc.LDS_CAP + 1):
        sides = tc.full_pool(np.random.default_rng(8200 + cap), cap)
        assert [len(s["kp"]) for s in sides] == [cap, cap, 200, 200]
        n = [tc.expect(oracle, tc.pair(sides[a], sides[b]))[1] for a, b in tc.FULL_PAIRS]
        assert n[0] > 300 and n[3] > 40, n


def test_pack_helpers():
    rng = np.random.default_rng(3)
    sides, _ = tc.ragged_pool(np.random.default_rng(7700))
    P = tc.pack_pool(rng, sides, tc.RAGGED_CAP)
    assert P["n"].tolist() == [len(s["kp"]) for s in sides] and P["kp"].shape == (12, tc.RAGGED_CAP)
    np.testing.assert_array_equal(P["node"][3, :65], sides[3]["node"]); np.testing.assert_array_equal(P["uright"][5, :63], sides[5]["uright"])
    rows = tc.pack_pairs([(tc.pair(sides[1], sides[0]), 1, 0)])
    assert rows.dtype.itemsize == 52 and rows["kf1"][0] == 1 and rows["F12"][0].tolist() == mc.tri_F12().reshape(9).tolist() and rows["ex"][0] == -2000.0


@pytest.mark.skipif(not os.path.exists(SLICES), reason="oracle/_ref/libref_slices.so was not built (the reference tree is absent)")
def test_reference_agrees_on_every_case(oracle):
    R = C.CDLL(SLICES)
    p = lambda a: C.c_void_p(a.ctypes.data)
    T2 = np.eye(4, dtype=np.float32); cam2 = np.array([1, 1, 0, 0], np.float32)
    for name, c in all_pairs().items():
        s1, s2 = c["s1"], c["s2"]
        n1, n2 = len(s1["kp"]), len(s2["kp"])
        node1, node2 = tc.ref_nodes(c)
        ur1 = np.ascontiguousarray(s1.get("uright", np.full(n1, -1, np.float32)), np.float32); ur2 = np.ascontiguousarray(s2.get("uright", np.full(n2, -1, np.float32)), np.float32)
        C1 = np.array([c["ex"], c["ey"], 1.0], np.float32)          # pose = identity, fx = fy = 1, cx = cy = 0: the reference's epipole is (C1.x / C1.z, C1.y / C1.z)
        F = np.ascontiguousarray(c["F12"], np.float32)
        for ori in (True, False):
            want, nwant = tc.expect(oracle, dict(c, ori=ori))
            out = np.full(max(n1, 1), -7, np.int32)
            nr = R.ref_search_for_triangulation(p(np.ascontiguousarray(s1["kp"])), p(s1["desc"]), n1, p(node1), p(np.ascontiguousarray(s1["free"])), p(ur1),
                                                p(np.ascontiguousarray(s2["kp"])), p(s2["desc"]), n2, p(node2), p(np.ascontiguousarray(s2["free"])), p(ur2),
                                                p(F), p(T2), p(C1), p(cam2), p(tc.SCALE), p(tc.SIGMA2), int(c["only_stereo"]), int(ori), p(out))
            np.testing.assert_array_equal(out[:n1], want, err_msg=name)
            assert nr == nwant, (name, ori, nr, nwant)
