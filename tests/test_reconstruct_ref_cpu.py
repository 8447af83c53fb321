"""The host model of the reconstruct unit (csrc/reconstruct_math.h through tests/reconstruct_sim.py) against the two references the header does not own.

  test_host_model_equals_the_reference_fixture   tests/golden/reconstruct_ref.npz holds what the REFERENCE's own lines (src/Initializer.cc:499-782, :833-1171 and
                                                 include/auxiliar.h:91-106, compiled unmodified by tests/golden/make_reconstruct_ref.py with D18's leaves handed back)
                                                 compute on every case: per hypothesis R, t, nGood, parallax, every vP3D and vbGood; the return value, R21, t21, vP3D,
                                                 vbTriangulated; every line endpoint, both errors and the flag.  The host model must give the same bits (a NaN equals a NaN)
  test_numpy_restatement                         tests/reconstruct_ref.py: LAPACK SVD, float64 products and numpy arccos, on the cases whose outcome does not hang on a gate:
                                                 same ok, model, winning pose and triangulated set; R21, t21 and the points within four times the deviation measured over the
                                                 cases"""
import os
import numpy as np
import pytest
import reconstruct_sim as sim
import reconstruct_ref as ref

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reconstruct_ref.npz")


def same(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    assert a.dtype == b.dtype
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def fixture_cases():
    fx = np.load(FX)
    cases = []
    for n in fx["names"]:
        n = str(n)
        sigma, mp, mt, model = fx[n + "/params"]
        c = {"name": n, "sigma": float(sigma), "min_parallax": float(mp), "min_triangulated": int(mt), "model": int(model), "lp": None}
        for k in ("kp1", "kp2", "m12", "inliers", "H21", "F21", "K"):
            c[k] = fx[n + "/" + k]
        if n + "/lp" in fx:
            for k in ("kl1", "fn1", "fn2", "lp"):
                c[k] = fx[n + "/" + k]
        cases.append(c)
    return fx, cases


@pytest.fixture(scope="module")
def model(fixture_cases):
    return sim.run(fixture_cases[1])


def test_host_model_equals_the_reference_fixture(fixture_cases, model):
    fx, cases = fixture_cases
    assert len(cases) >= 48
    seen_calls = 0
    for c, r in zip(cases, model):
        n = c["name"]; g = lambda k: fx[n + "/" + k]
        p = r["pose"]
        ncalls = int(g("ncalls"))
        assert ncalls == (0 if p["reason"] in (1, 2) else 4 if c["model"] == 2 else 8), n
        seen_calls += ncalls
        # every hypothesis: R, t, nGood, parallax, vP3D and vbGood by keypoint 1
        assert same(r["hyp"][:, :12], g("hyp")), (n, r["hyp"][:, :12], g("hyp"))
        np.testing.assert_array_equal(p["n_good"], g("n_good"), err_msg=n)
        assert same(p["parallax"], g("parallax")), (n, p["parallax"], g("parallax"))
        rows = np.nonzero(c["m12"] >= 0)[0]                                   # the match list, ascending keypoint 1
        n1 = len(c["kp1"])
        for h in range(8):
            good = r["stage"][h] == 6
            hp = np.zeros((n1, 3), np.float32); hg = np.zeros(n1, np.uint8)
            hp[rows[good]] = r["rows_p3d"][h][good]; hg[rows[good]] = 1
            assert same(hp, g("hyp_p3d")[h]) and same(hg, g("hyp_good")[h]), (n, h)
        # Initialize's return value and out-parameters
        assert int(p["ok"]) == int(g("ok")), n
        assert same(p["R21"], g("R21")) and same(p["t21"], g("t21")), n
        assert same(r["p3d"], g("p3d")) and same(r["tri"], g("tri")), n
        # ReconstructLine: endpoints, errorC1 / errorC2 and the flag by row of line_pairs
        if c["lp"] is not None:
            assert int(g("nmad")) == (2 if p["ok"] else 0), n      # ReconstructLine runs, also over no lines, exactly when the pose is ok
            assert int(g("line_valid").sum()) == int(p["n_lines"]), n
            assert same(r["line_s3d"], g("line_s3d")) and same(r["line_e3d"], g("line_e3d")), n
            assert same(r["line_tri"], g("line_tri")), n
            assert same(r["line_err"], g("line_err")), (n, r["line_err"], g("line_err"))
    assert seen_calls >= 200


def test_numpy_restatement(fixture_cases, model):
    fx, cases = fixture_cases
    worst = {"R21": 0.0, "t21": 0.0, "p3d": 0.0}
    used = 0
    for c, r in zip(cases, model):
        if not ref.robust(c["name"]):
            continue
        want = ref.reconstruct(c)
        p = r["pose"]
        assert int(p["ok"]) == want["ok"] and int(p["model"]) == c["model"], c["name"]
        if not want["ok"]:
            continue
        used += 1
        np.testing.assert_array_equal(r["tri"], want["tri"], err_msg=c["name"])
        worst["R21"] = max(worst["R21"], float(np.abs(p["R21"].astype(np.float64) - want["R21"].ravel()).max()))
        worst["t21"] = max(worst["t21"], float(np.abs(p["t21"].astype(np.float64) - want["t21"]).max()))
        scale = np.abs(want["p3d"]).max()
        worst["p3d"] = max(worst["p3d"], float(np.abs(r["p3d"].astype(np.float64) - want["p3d"]).max() / scale))
    print("numpy restatement over %d cases: largest deviation R21 %.3g, t21 %.3g, p3d %.3g of the extent" % (used, worst["R21"], worst["t21"], worst["p3d"]))
    assert used >= 20
    for k, bound in ref.MEASURED.items():
        assert worst[k] <= 4 * bound, (k, worst[k], bound)
