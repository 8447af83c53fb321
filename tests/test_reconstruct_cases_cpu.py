"""CPU suite of the reconstruct unit: csrc/reconstruct_math.h as the host model (tests/reconstruct_sim.py: plain and under -fsanitize=address,undefined, as stand-alone
programs) on the cases of tests/reconstruct_cases.py.

  test_cases_reach_what_they_name   on the model's trace: every case goes where its name says (the F and H paths, each F winner, the tie, nsimilar, the gates of :537-550,
                                    :639 and :763, the min(50, size - 1) edge, each exit of CheckRT with both reprojection errors on the float at th2 and the one above, the
                                    match counts around a wave and a workgroup, unmatched rows, model 0, the line counts and their even / odd medians, the row that is not
                                    finite, lines of a pair that fails, a line error on 2 * 1.4826 * MAD and on the double above)
  test_winner_is_the_truth          where the pose is ok, R21 and the direction of t21 are the scene's, and the triangulated points are the scene's points up to the scale
                                    of t
  test_no_nan_reaches_a_sort        no accepted cosine and no line error of any case is a NaN (decision D18 orders NaNs last; the reference's sort is undefined there)
  test_acos_against_libm            the header's acos_f itself (an entry of the sim evaluates it) against this machine's acosf: a dense sweep of [-1, 1] and every float within 1e-4 of cos(1 degree); the selected
                                    cosines of the parallax gate cases are values where both agree"""
import ctypes
import ctypes.util
import numpy as np
import pytest
import reconstruct_cases as rcases
import reconstruct_sim as sim


@pytest.fixture(scope="module")
def cases():
    return rcases.all_cases()


@pytest.fixture(scope="module")
def results(cases):
    return sim.run(list(cases))


def by_name(cases, results):
    return {c["name"]: (c, r) for c, r in zip(cases, results)}


def test_cases_reach_what_they_name(cases, results):
    R = by_name(cases, results)
    pose = lambda n: R[n][1]["pose"]
    for h in range(4):
        p = pose("f_winner_%d" % h)
        assert p["ok"] == 1 and p["model"] == 2 and p["hypothesis"] == h
    p = pose("h_winner"); assert p["ok"] == 1 and p["model"] == 1 and 0 <= p["hypothesis"] < 8
    p = pose("h_planar_twins"); assert p["ok"] == 0 and p["reason"] == 3 and np.sort(p["n_good"])[-2] >= 0.75 * p["n_good"].max()
    # every exit of CheckRT somewhere, and rows that are no inliers
    allst = np.concatenate([r["stage"].ravel() for r in results])
    assert set(range(7)) <= set(allst.tolist())
    assert (R["f_not_finite"][1]["stage"] == 1).sum() == 4 and not np.isfinite(R["f_not_finite"][1]["rows_p3d"][R["f_not_finite"][1]["stage"] == 1]).all()
    # :537-550
    a, b = pose("f_maxgood_below_min"), pose("f_maxgood_at_min")
    assert a["n_good"].max() + 1 == R["f_maxgood_below_min"][0]["min_triangulated"] and (a["ok"], a["reason"]) == (0, 3)
    assert b["n_good"].max() == R["f_maxgood_at_min"][0]["min_triangulated"] and b["ok"] == 1
    assert int(0.9 * a["n_inliers"]) < a["n_good"].max()
    a, b = pose("f_parallax_at_min"), pose("f_parallax_above_min")
    assert (a["ok"], a["reason"]) == (0, 4) and a["parallax"][a["hypothesis"]] == np.float32(R["f_parallax_at_min"][0]["min_parallax"])
    assert b["ok"] == 1 and np.nextafter(b["parallax"][b["hypothesis"]], np.float32(0)) == np.float32(R["f_parallax_above_min"][0]["min_parallax"])
    a, b = pose("f_tie_first_taken"), pose("f_tie_first_taken_wins")
    assert a["n_inliers"] == 1 and not a["n_good"].any() and (a["ok"], a["reason"], a["hypothesis"]) == (0, 4, 0)
    assert (b["ok"], b["hypothesis"], b["n_triangulated"]) == (1, 0, 0)
    a = pose("f_nsimilar")
    assert (a["ok"], a["reason"], a["hypothesis"]) == (0, 3, -1) and (a["n_good"][:4] > 0.7 * a["n_good"].max()).sum() == 2
    # :639 and :763
    for n in ("h_d1d2_below", "h_d2d3_below"):
        assert (pose(n)["ok"], pose(n)["reason"]) == (0, 2) and not R[n][1]["hyp"].any()
    for n in ("h_d1d2_above", "h_d2d3_above"):
        assert pose(n)["reason"] != 2 and R[n][1]["hyp"].any()
    a, b = pose("h_09n_54_of_60"), pose("h_09n_55_of_60")
    assert a["n_inliers"] == 60 and a["n_good"].max() == 54 and (a["ok"], a["reason"]) == (0, 3) and np.sort(a["n_good"])[-2] < 0.75 * 54
    assert b["n_inliers"] == 60 and b["n_good"].max() == 55 and b["ok"] == 1
    a, b = pose("h_second_at_075"), pose("h_second_below_075")
    s = np.sort(a["n_good"]); assert 4 * s[-2] == 3 * s[-1] and (a["ok"], a["reason"]) == (0, 3) and s[-1] > 0.9 * a["n_inliers"]
    s = np.sort(b["n_good"]); assert 0 < 3 * s[-1] - 4 * s[-2] <= 3 and b["ok"] == 1
    a, b = pose("h_parallax_at_min"), pose("h_parallax_below_min")
    assert a["ok"] == 1 and a["parallax"][a["hypothesis"]] == np.float32(R["h_parallax_at_min"][0]["min_parallax"])
    assert (b["ok"], b["reason"]) == (0, 4) and np.nextafter(b["parallax"][b["hypothesis"]], np.float32(np.inf)) == np.float32(R["h_parallax_below_min"][0]["min_parallax"])
    # :923 / :934 with th2 = 1
    for which, col, bad in ((1, 0, 4), (2, 1, 5)):
        for n, e, st in (("err%d_at_th2" % which, np.float32(1.0), 6), ("err%d_above_th2" % which, np.nextafter(np.float32(1.0), np.float32(2.0)), bad)):
            c, r = R[n]
            h, slot = c["gate_row"]
            assert r["rows_err"][h, slot, col] == e and r["stage"][h, slot] == st, (n, r["rows_err"][h, slot], r["stage"][h, slot])
    # min(50, size - 1)
    for n in (1, 50, 51, 52):
        c, r = R["f_accepted_%d" % n]
        p = r["pose"]; h = int(p["hypothesis"])
        assert p["ok"] == 1 and p["n_good"][h] == n
        assert r["sel"][h] == np.sort(r["rows_cos"][h][r["stage"][h] == 6])[min(50, n - 1)]
    for n in (8, 63, 64, 65, 257):
        c, r = R["f_matches_%d" % n]
        assert r["stage"].shape[1] == n and len(c["kp1"]) > n and r["pose"]["ok"] == 1 and r["pose"]["n_triangulated"] == n
        assert (r["tri"] == (c["m12"] >= 0)).all()
    c, r = R["f_partial_inliers"]; assert 0 < r["pose"]["n_inliers"] < r["stage"].shape[1] and (r["stage"] == 0).any()
    assert (pose("model_0")["ok"], pose("model_0")["reason"], pose("model_0")["hypothesis"]) == (0, 1, -1) and not R["model_0"][1]["p3d"].any()
    assert R["no_matches"][1]["stage"].shape[1] == 0
    # lines
    for n in (0, 1, 2, 65):
        p = pose("lines_%d" % n); assert p["ok"] == 1 and p["n_lines"] == n
    assert pose("lines_65")["n_lines_triangulated"] not in (0, 65)
    c, r = R["lines_even_bad_index"]; assert r["pose"]["n_lines"] == 8 and not r["line_tri"][[1, 9]].any() and not r["line_s3d"][[1, 9]].any()
    c, r = R["lines_odd_nonfinite"]
    assert r["pose"]["n_lines"] == 9 and r["line_tri"][3] == 1 and not r["line_s3d"][3].any() and not r["line_err"][3].any()
    assert pose("h_lines")["model"] == 1 and pose("h_lines")["n_lines_triangulated"] > 0
    c, r = R["lines_not_ok"]; assert r["pose"]["ok"] == 0 and r["pose"]["n_lines"] == 6 and not r["line_tri"].any() and not r["line_s3d"].any() and not r["line_e3d"].any()
    # the fx of :1129: with fx != fy the errors of frame 1 dwarf those of frame 2
    r = R["lines_65"][1]; assert np.median(r["line_err"][:, 0]) > 100 * np.median(r["line_err"][:, 1])
    # the threshold is 2 * 1.4826 * MAD of the valid rows, by the reference's own recipe
    for n in ("lines_2", "lines_65", "lines_even_bad_index", "lines_odd_nonfinite"):
        c, r = R[n]
        valid = (c["lp"][:, 0] >= 0) & (c["lp"][:, 0] < len(c["fn1"])) & (c["lp"][:, 1] >= 0) & (c["lp"][:, 1] < len(c["fn2"]))
        for k in range(2):
            e = np.sort(r["line_err"][valid, k]); med = e[len(e) // 2]
            mad = np.sort(np.abs(e - med))[len(e) // 2]
            assert r["mad"][k] == 2.0 * (1.4826 * mad), n
        np.testing.assert_array_equal(r["line_tri"][valid], ~((r["line_err"][valid, 0] > r["mad"][0]) | (r["line_err"][valid, 1] > r["mad"][1])))

    # :1166: an error on the threshold stays, the double above it goes (the row's errorC2 passes in both)
    for n, up, flag in (("line_err_at_mad", False, 1), ("line_err_above_mad", True, 0)):
        c, r = R[n]
        row = c["line_row"]
        want = np.nextafter(r["mad"][0], np.inf) if up else r["mad"][0]
        assert r["pose"]["ok"] == 1 and r["line_err"][row, 0] == want and r["line_err"][row, 1] <= r["mad"][1] and r["line_tri"][row] == flag, (n, r["line_err"][row], r["mad"])


def test_winner_is_the_truth(cases, results):
    seen = 0
    for c, r in zip(cases, results):
        p = r["pose"]
        if not p["ok"] or c["name"].startswith(("h_d", "f_tie", "err", "f_accepted_1", "line_err")) or c["K"][0] == 1.0:
            continue
        Rt, tt = c["truth"]
        R21 = p["R21"].reshape(3, 3).astype(np.float64)
        assert np.abs(R21 - Rt).max() < 2e-4, (c["name"], R21, Rt)
        t = p["t21"].astype(np.float64)
        assert abs(np.linalg.norm(t) - 1) < 1e-5 and np.abs(t - tt / np.linalg.norm(tt)).max() < 2e-3, (c["name"], t, tt)
        rows = c["rows1"][r["tri"][c["rows1"]] == 1]
        if len(rows) and len(c["X"]) == len(c["rows1"]):
            X = c["X"][np.searchsorted(c["rows1"], rows)] / np.linalg.norm(tt)
            assert np.abs(r["p3d"][rows] - X).max() < 2e-2 * np.abs(X).max(), c["name"]
        seen += 1
    assert seen >= 20


def test_no_nan_reaches_a_sort(cases, results):
    for c, r in zip(cases, results):
        assert not np.isnan(r["rows_cos"][r["stage"] == 6]).any(), c["name"]
        assert not np.isnan(r["line_err"]).any(), c["name"]


def test_acos_against_libm(cases, results):
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.acosf.restype = ctypes.c_float; libm.acosf.argtypes = [ctypes.c_float]
    acosf = lambda a: np.array([libm.acosf(float(v)) for v in a], np.float32)
    # the parallax of every hypothesis is :955 on the header's acos_f of its selected cosine
    sels = np.array([r["sel"][h] for r in results for h in range(8)], np.float32)
    asel = sim.acos(sels).reshape(-1, 8)
    for k, (c, r) in enumerate(zip(cases, results)):
        p = r["pose"]
        for h in range(8):
            if p["n_good"][h] > 0:
                want = np.float32(np.float64(asel[k, h] * np.float32(180.0)) / 3.1415926535897932384626433832795)
                assert p["parallax"][h] == want or (np.isnan(want) and np.isnan(p["parallax"][h])), (c["name"], h)
    sweep = np.linspace(-1.0, 1.0, 200001).astype(np.float32)
    c1 = np.float32(np.cos(np.deg2rad(1.0)))
    lo, hi = np.float32(c1 - 1e-4), np.float32(c1 + 1e-4)
    near = np.arange(lo.view(np.uint32), hi.view(np.uint32) + 1, dtype=np.uint32).view(np.float32)
    m_sweep, m_near, l_sweep, l_near = sim.acos(sweep), sim.acos(near), acosf(sweep), acosf(near)
    d_sweep = int((m_sweep.view(np.uint32) != l_sweep.view(np.uint32)).sum())
    d_near = int((m_near.view(np.uint32) != l_near.view(np.uint32)).sum())
    print("acos_f against acosf: %d of %d differ over the sweep, %d of %d within 1e-4 of cos(1 degree)" % (d_sweep, len(sweep), d_near, len(near)))
    assert np.abs(m_sweep.astype(np.float64) - np.arccos(sweep.astype(np.float64))).max() < 2.4e-7      # half an ulp of pi in float, and a little
    # acos_f is the correctly rounded value but for double rounding, libm's acosf is within one ulp of the true value: the two differ by one ulp at the most.  The counts
    # are recorded in DESIGN.md (D18): 15545 of 200001 and 0 of 3357 with the libm this was written on
    for m, l in ((m_sweep, l_sweep), (m_near, l_near)):
        assert np.abs(m.view(np.int32).astype(np.int64) - l.view(np.int32).astype(np.int64)).max() <= 1
    names = ("f_parallax_at_min", "f_parallax_above_min", "h_parallax_at_min", "h_parallax_below_min")
    gate = np.array([r["sel"][int(r["pose"]["hypothesis"])] for c, r in zip(cases, results) if c["name"] in names], np.float32)
    assert len(gate) == 4 and (sim.acos(gate).view(np.uint32) == acosf(gate).view(np.uint32)).all()
