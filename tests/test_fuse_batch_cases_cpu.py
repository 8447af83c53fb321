"""The inputs of tests/test_fuse_batch_gpu.py reach what they are meant to reach, shown on the CPU with helper + oracle (tests/fuse_batch_cases.py):
every tie case has the stated winner, every gate pair sits on neighbouring floats either side of its threshold and has the stated outcome, the keypoint
outside the grid is the nearest descriptor and never wins, the ragged pool finds candidates.  Where the reference's own Fuse was built
(oracle/_ref/libref_slices.so), one family of each kind is held against it: map points (lines) and a pose become windows through the reference's own
projection block, and the oracle's best indices, replayed through Fuse's bookkeeping, must be what the reference's Fuse did."""
import ctypes as C
import os
import numpy as np
import pytest
import fuse_batch_cases as fc

SLICES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_slices.so")
up = lambda a: np.nextafter(np.float32(a), np.float32(1e9))


def one(oracle, c):
    """(best_idx, best_dist) of a case's first job's first query"""
    bi, bd = fc.expect_job(oracle, c, c["jobs"][0])
    return int(bi[0]), int(bd[0])


def gate_case(g, kind):
    return fc.case(kind, g[4] if kind == 0 else 0, [g[0]], [g[1]], [fc.job(0, g[2], 0)])


def test_tie_cases_have_the_stated_winner(oracle):
    T = fc.tie_cases(np.random.default_rng(8410))
    assert sorted(T) == ["tie_lines", "tie_one_cell", "tie_two_cells"]
    for name, (c, row) in T.items():
        k = c["pool"][0]; qd = c["blocks"][0][0]
        d = np.array([fc.hamming(qd, x) for x in k["desc"]])
        tied = np.flatnonzero(d == 10)
        assert len(tied) == 2 and row in tied and (d[np.setdiff1d(np.arange(len(d)), tied)] > 60).all(), (name, d)
        assert one(oracle, c) == (row, 10), name
    k = T["tie_two_cells"][0]["pool"][0]["feats"]
    col = lambda r: int(np.round(k["x"][r] / 10)); cell_row = lambda r: int(np.round(k["y"][r] / 10))
    assert col(7) < col(3) and T["tie_two_cells"][1] == 7                     # the higher row index sits in the earlier column: it wins
    k = T["tie_one_cell"][0]["pool"][0]["feats"]
    assert (col(7), cell_row(7)) == (col(3), cell_row(3)) and T["tie_one_cell"][1] == 3


def test_lane_cases(oracle):
    L = fc.lane_cases(np.random.default_rng(8400))
    assert len(L) == 1 + 4 * 3
    for name, (c, row) in L.items():
        m = int(name.split("_")[1])
        k = c["pool"][0]; q = c["jobs"][0]["q"][0]
        inside = [i for i in range(len(k["feats"])) if fc.point_window_ok(q["u"], q["v"], q["radius"], k["feats"]["x"][i], k["feats"]["y"][i])]
        assert len(inside) == m and row in inside and inside.index(row) == int(name.split("_")[2]), name
        assert one(oracle, c) == (row, 5), name


def test_point_gates_sit_on_their_thresholds(oracle):
    G = fc.point_gate_cases(np.random.default_rng(8420))
    for name, g in G.items():
        bi, bd = one(oracle, gate_case(g, 0))
        assert (bi, bd) == ((2, 0) if g[3] else (-1, fc.INT_MAX)), (name, bi, bd)
    x = lambda n: G[n][0]["feats"]["x"][2]; y = lambda n: G[n][0]["feats"]["y"][2]
    q = G["window_dx_in"][2][0]
    assert up(x("window_dx_in")) == x("window_dx_out") and up(y("window_dy_in")) == y("window_dy_out")
    assert abs(np.float32(x("window_dx_out") - q["u"])) == q["radius"] == abs(np.float32(y("window_dy_out") - q["v"]))          # |d| < r is strict: d == r is out
    for octave in (0, 2):
        for kind, lim in (("mono", 5.99), ("stereo", 7.8)):
            a, b = "chi2_%s_oct%d_in" % (kind, octave), "chi2_%s_oct%d_out" % (kind, octave)
            assert up(x(a)) == x(b) and G[a][4] == 1
            e2 = lambda n: (float(x(n)) - 300.0) ** 2 + (1.0 if kind == "stereo" else 0.0)
            assert e2(a) * float(fc.INV_SIGMA2[octave]) < lim < e2(b) * float(fc.INV_SIGMA2[octave]) + 1e-3 and abs(e2(b) - e2(a)) < 1e-3
            assert (G[a][0]["uright"][2] >= 0) == (kind == "stereo")
    for g in G.values():
        ur = g[0]["uright"]
        assert (ur >= 0).any() and (ur < 0).any()          # stereo and monocular rows in one keyframe
    assert [G["level_" + n][0]["feats"]["octave"][2] for n in ("min-1", "min", "max", "max+1")] == [1, 2, 3, 4] and G["level_min"][2]["min_level"][0] == 2 and G["level_max"][2]["max_level"][0] == 3
    assert G["octave_past_table"][0]["feats"]["octave"][2] >= fc.NLEVELS and x("octave_past_table") == x("octave_in_table") and fc.ORACLE_TABLE[fc.NLEVELS:].max() == 0
    assert G["not_valid"][2]["valid"][0] == 0 and G["valid"][2]["valid"][0] == 1 and x("not_valid") == x("valid")


def test_line_gates_sit_on_their_thresholds(oracle):
    G = fc.line_gate_cases(np.random.default_rng(8430))
    seen = {}
    for name, g in G.items():
        bi, bd = one(oracle, gate_case(g, 1))
        seen[name] = bi
        if g[3] is not None:
            assert (bi, bd) == ((2, 0) if g[3] else (-1, fc.INT_MAX)), (name, bi, bd)
    px = lambda n: G[n][0]["feats"]["pt_x"][2]; ang = lambda n: G[n][0]["feats"]["angle"][2]
    assert up(px("distance_in")) == px("distance_out") and 309.9 < px("distance_in") < 310.1          # distance > r * r: 10 px from the midpoint
    assert np.nextafter(ang("slope_in"), np.float32(-1e9)) == ang("slope_out")                        # slope - angle > 0.01 r: 0.4 - 0.1
    assert abs(float(ang("slope_in")) - 0.3) < 1e-6
    assert [G["level_" + n][0]["feats"]["octave"][2] for n in ("min-1", "min", "max", "max+1")] == [0, 1, 2, 3]
    for n in ("vertical_down", "vertical_up", "degenerate"):
        q = G[n][2][0]
        assert q["u"] == q["u2"] and (q["v"] == q["v2"]) == (n == "degenerate")
    assert seen["vertical_down"] != seen["vertical_up"]          # -inf passes the slope gate, +inf does not


def test_keypoint_outside_the_grid_never_wins(oracle):
    c, winner, outside = fc.outside_grid_case(np.random.default_rng(8440))
    k = c["pool"][0]; q = c["jobs"][0]["q"][0]; qd = c["blocks"][0][0]
    d = [fc.hamming(qd, x) for x in k["desc"]]
    assert d[outside] == 0 == min(d) and d[winner] == 12 and sorted(d)[1] == 12
    assert fc.point_window_ok(q["u"], q["v"], q["radius"], k["feats"]["x"][outside], k["feats"]["y"][outside])          # inside the window
    assert int(np.floor(k["feats"]["x"][outside] * np.float32(0.1) + 0.5)) == 64 and int(np.floor(k["feats"]["x"][winner] * np.float32(0.1) + 0.5)) == 63
    assert one(oracle, c) == (winner, 12)
    # with the only other row of the window gone, the query finds nothing
    k2 = dict(k, feats=k["feats"].copy()); k2["feats"]["x"][winner] = 100.0
    assert one(oracle, dict(c, pool=[k2])) == (-1, fc.INT_MAX)


@pytest.mark.parametrize("kind,chi2", fc.RAGGED_MODES)
def test_ragged_pool_finds_candidates(oracle, kind, chi2):
    c = fc.ragged_pool(np.random.default_rng(8500 + 10 * kind + chi2), kind, chi2)
    assert [len(k["feats"]) for k in c["pool"]] == [96, 0, 1, 63, 64, 65] and len(c["jobs"]) == 36 and len(c["blocks"]) == 1
    assert sorted(set(len(j["q"]) for j in c["jobs"])) == [0, 1, 255, 256, 257, fc.RAGGED_QCAP]
    combos = set((len(c["pool"][j["kf"]]["feats"]) == 0, len(j["q"]) == 0) for j in c["jobs"])
    assert combos == {(False, False), (True, False), (False, True), (True, True)}
    want = fc.expect(oracle, c)
    full, good = 0, 0
    for j, (bi, bd) in zip(c["jobs"], want):
        n = len(c["pool"][j["kf"]]["feats"])
        if n == 0 or len(j["q"]) == 0:
            assert (bi == -1).all() and (bd == fc.INT_MAX).all()
            continue
        valid = j["q"]["valid"] != 0
        assert (bi[~valid] == -1).all() and (bi < n).all()
        full += 1; good += 2 * (bi >= 0).sum() >= valid.sum() > 0
    assert full == 25 and 2 * good >= full, (good, full)
    if kind == 0:
        k = c["pool"][0]["uright"]
        assert 0 < (k >= 0).sum() < len(k)


def test_other_cases(oracle):
    c = fc.neighbours_case(np.random.default_rng(8450))
    want = fc.expect(oracle, c)
    assert len(c["jobs"]) == 22 and all(j["kf"] == 0 and j["block"] == 0 for j in c["jobs"][:20]) and [j["block"] for j in c["jobs"][20:]] == [1, 2]
    assert len(set(w[0].tobytes() for w in want[:20])) == 20 and min((w[0] >= 0).sum() for w in want) > 20          # other windows per job: other results
    for cap in (fc.PLAIN_CAP, fc.LDS_CAP + 1):
        c = fc.full_case(np.random.default_rng(8600 + cap), 0, 1, cap)
        want = fc.expect(oracle, c)
        assert [len(k["feats"]) for k in c["pool"]] == [cap, 200] and (want[0][0] >= 0).sum() > 150 and (want[1][0] >= 0).sum() > 150 and want[0][0].max() > cap - 200


def test_pack_helpers():
    rng = np.random.default_rng(3)
    c = fc.full_case(np.random.default_rng(8601), 0, 1, 120)
    Q = fc.pack_jobs(rng, c, 300)
    c["pool"][1] = fc.cut(c["pool"][1], 50)
    P = fc.pack_pool(rng, c, 128)
    assert P["n"].tolist() == [120, 50] and P["feats"].shape == (2, 128) and P["desc"].shape == (2, 128, 32)
    np.testing.assert_array_equal(P["feats"][1, :50], c["pool"][1]["feats"]); np.testing.assert_array_equal(P["uright"][0, :120], c["pool"][0]["uright"])
    assert Q["jobs"].dtype.itemsize == 12 and Q["jobs"]["kf"].tolist() == [0, 1, 0, 1] and Q["jobs"]["nq"].tolist() == [300, 300, 300, 77]
    assert Q["jobs"]["qdesc0"].tolist() == [0, 300, 300, 100] and Q["nqdesc"] == 600 and Q["q"].shape == (4, 300)
    np.testing.assert_array_equal(Q["q"][3, :77], c["jobs"][3]["q"]); np.testing.assert_array_equal(Q["qdesc"][100:177], fc.job_desc(c, c["jobs"][3]))


def _replay_is_the_reference(name, fused, act, nr, bi, bd, valid, bad, in_kf, nobs, state, sobs):
    idx, action, nfused = fc.replay_fuse(bi, bd, valid, bad, in_kf, nobs, state, sobs)
    np.testing.assert_array_equal(fused, idx, err_msg=name); np.testing.assert_array_equal(act, action, err_msg=name)
    assert nr == nfused and nfused > 30 and len(set(action.tolist())) >= 4, (name, nr, nfused, sorted(set(action.tolist())))


@pytest.mark.skipif(not os.path.exists(SLICES), reason="oracle/_ref/libref_slices.so was not built (the reference tree is absent)")
def test_reference_fuse_agrees_with_oracle_plus_bookkeeping(oracle):
    R = C.CDLL(SLICES)
    p = lambda a: C.c_void_p(a.ctypes.data)
    bb = np.array(fc.BOUNDS, np.float32)
    for th in (3.0, 5.0):
        f = fc.ref_point_family(np.random.default_rng(8700))
        n = len(f["kp"]); nmp = len(f["mp"])
        kp = np.ascontiguousarray(f["kp"])
        fused = np.zeros(nmp, np.int32); act = np.zeros(nmp, np.int32); fq = np.zeros(nmp, fc.FQ)
        nr = R.ref_fuse(p(kp), p(f["desc"]), n, p(bb), p(fc.SCALE), p(fc.INV_SIGMA2), C.c_float(fc.LOG_SF), p(f["uright"]), p(f["state"]), p(f["sobs"]), p(f["cam"]), p(f["Tcw"]),
                        p(f["Ow"]), p(f["mp"]), p(f["mpd"]), nmp, C.c_float(th), p(fused), p(act))
        R.ref_fuse_queries(p(bb), p(fc.SCALE), C.c_float(fc.LOG_SF), p(f["cam"]), p(f["Tcw"]), p(f["Ow"]), p(f["mp"]), nmp, C.c_float(th), p(fq))
        q = np.zeros(nmp, fc.PQ_DTYPE)
        q["u"] = fq["u"]; q["v"] = fq["v"]; q["ur"] = fq["ur"]; q["radius"] = fq["radius"]; q["min_level"] = fq["level"] - 1; q["max_level"] = fq["level"]; q["valid"] = fq["valid"]
        c = fc.case(0, 1, [fc.keyframe(kp, f["desc"], f["uright"])], [f["mpd"]], [fc.job(0, q, 0)])
        bi, bd = fc.expect_job(oracle, c, c["jobs"][0])
        _replay_is_the_reference("points th=%g" % th, fused, act, nr, bi, bd, fq["valid"], f["mp"]["bad"], f["mp"]["inKF"], f["mp"]["nObs"], f["state"], f["sobs"])
    f = fc.ref_line_family(np.random.default_rng(8710))
    n = len(f["kl"]); nml = len(f["ml"])
    kl = np.ascontiguousarray(f["kl"])
    fql = np.zeros(nml, fc.FQL); fused = np.zeros(nml, np.int32); act = np.zeros(nml, np.int32)
    R.ref_line_fuse_queries(p(bb), p(fc.SCALE), C.c_float(fc.LOG_SF), p(f["cam"]), p(f["Tcw"]), p(f["Ow"]), p(f["ml"]), nml, C.c_float(3.0), p(fql))
    assert (fql["valid"] != 2).all()
    nr = R.ref_line_fuse(p(kl), p(f["desc"]), n, p(bb), p(fc.SCALE), C.c_float(fc.LOG_SF), p(f["state"]), p(f["sobs"]), p(f["cam"]), p(f["Tcw"]), p(f["Ow"]), p(f["ml"]), p(f["mld"]), nml,
                         C.c_float(3.0), p(fused), p(act))
    q = np.zeros(nml, fc.PQ_DTYPE)
    q["u"] = fql["u1"]; q["v"] = fql["v1"]; q["u2"] = fql["u2"]; q["v2"] = fql["v2"]; q["radius"] = fql["radius"]; q["min_level"] = fql["level"] - 1; q["max_level"] = fql["level"]; q["valid"] = fql["valid"]
    c = fc.case(1, 0, [fc.keyframe(kl, f["desc"])], [f["mld"]], [fc.job(0, q, 0)])
    bi, bd = fc.expect_job(oracle, c, c["jobs"][0])
    _replay_is_the_reference("lines", fused, act, nr, bi, bd, fql["valid"], f["ml"]["bad"], np.zeros(nml, np.int32), f["ml"]["nObs"], f["state"], f["sobs"])
