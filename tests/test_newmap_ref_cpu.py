"""The host model of the map-creation unit (csrc/newmap_math.h through tests/newmap_sim.py: plain and under -fsanitize=address,undefined, as stand-alone programs) against
its two references.

  test_model_equals_the_reference_fixture   tests/golden/newmap_ref.npz holds what the reference's own lines (src/LocalMapping.cc:459-617 and :1007-1148,
                                            src/MapPoint.cc:353-375, src/MapLine.cpp:343-371, cut and compiled unmodified by tests/golden/make_newmap_ref.py) return for
                                            every case of tests/newmap_cases.py: stage, coordinates, normal and distances are equal bit for bit, and so are the inputs
                                            (the fixture was made from these cases)
  test_model_against_numpy                  tests/newmap_ref.py (float64, the null vector from LAPACK): equal stages and counts on the well-conditioned rows, coordinates
                                            within a tolerance
  test_numpy_against_the_fixture            the same restatement against the fixture: the measurement the tolerance comes from, kept as a test

The tolerance.  Measured on this fixture (2113 rows, 930 of them created, whose every gate is further than MARGIN = 1e-4, relatively, from its threshold): the restatement's coordinates differ
from the reference's by at most 1.5e-6 of the row's largest coordinate for x3D, 2.0e-7 for s3D / e3D, 7.6e-8 for the normals and 1.5e-6 for the distances, and no stage
differs.  That is the float32 arithmetic of the reference itself (2^-24 = 6e-8 per rounding, amplified by depth / baseline, up to 17 here, in the triangulated depth): TOL =
1e-5 for points and distances and 1e-6 for the unit normals leave a factor of about seven over the measurement and stay three orders of magnitude below any error of
substance (a wrong row, a swapped camera or the wrong intrinsics move a point by 1e-2 and more)."""
import os
import numpy as np
import pytest
import newmap_cases as ncases
import newmap_ref as ref
import newmap_sim as sim

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-4
TOL, TOL_NORMAL = 1e-5, 1e-6
POINT_KEYS, LINE_KEYS = ("stage", "x3d", "normal", "dist"), ("stage", "s3d", "e3d", "normal", "dist")


@pytest.fixture(scope="module")
def cases():
    return ncases.all_cases()


@pytest.fixture(scope="module")
def results(cases):
    return sim.run(list(cases))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "newmap_ref.npz"))


@pytest.fixture(scope="module")
def restated(cases):
    out = []
    for c in cases:
        if sim.is_lines(c):
            st, s, e, n, d, m = ref.line_rows(c); out.append(dict(stage=st, s3d=s, e3d=e, normal=n, dist=d, margin=m))
        else:
            st, x, n, d, m = ref.point_rows(c); out.append(dict(stage=st, x3d=x, normal=n, dist=d, margin=m))
    return out


def test_model_equals_the_reference_fixture(cases, results, fixture):
    assert [c["name"] for c in cases] == fixture["names"].tolist()
    created = 0
    for c, r in zip(cases, results):
        n = c["name"]
        L = sim.is_lines(c)
        for k in (mr_inputs_lines if L else mr_inputs_points):
            np.testing.assert_array_equal(np.asarray(c[k]).view(np.uint8), fixture[n + "/" + k].view(np.uint8), err_msg="%s input %s" % (n, k))
        for k in (LINE_KEYS if L else POINT_KEYS):
            want = fixture[n + "/" + k]
            assert r[k].dtype == want.dtype and r[k].shape == want.shape, (n, k)
            np.testing.assert_array_equal(r[k].view(np.uint8), want.view(np.uint8), err_msg="%s %s" % (n, k))
        assert r["nnew"] == int((fixture[n + "/stage"] == 0).sum())
        created += r["nnew"]
    assert created > 800


mr_inputs_points = ("pose1", "pose2", "kp1", "oct1", "kp2", "oct2", "m12", "sf", "sigma2")
mr_inputs_lines = ("pose1", "pose2", "kl1", "loct1", "fn1", "kl2", "loct2", "fn2", "lp", "sf")


def _compare(cases, got, want_of, label):
    rows = created = 0
    worst = {}
    for c, g, w in zip(cases, got, want_of):
        ok = w["margin"] > MARGIN
        np.testing.assert_array_equal(np.asarray(g["stage"])[ok], w["stage"][ok], err_msg="%s stage of %s" % (label, c["name"]))
        rows += int(ok.sum())
        cr = ok & (w["stage"] == 0)
        created += int(cr.sum())
        if not cr.any():
            continue
        for k in (("s3d", "e3d", "normal", "dist") if sim.is_lines(c) else ("x3d", "normal", "dist")):
            a, b = np.asarray(g[k], np.float64)[cr], w[k][cr]
            err = float((np.abs(a - b) / np.abs(b).max(1, keepdims=True)).max())
            worst[k] = max(worst.get(k, 0.0), err)
            assert err <= (TOL_NORMAL if k == "normal" else TOL), (label, c["name"], k, err)
    print(label, "rows", rows, "created", created, "largest relative differences", worst)
    assert rows > 2000 and created > 900
    return rows


def test_model_against_numpy(cases, results, restated):
    _compare(cases, results, restated, "model vs numpy")
    # counts: where every row of a case is well conditioned, nnew is the restatement's
    whole = 0
    for c, r, w in zip(cases, results, restated):
        if (w["margin"] > MARGIN).all():
            assert r["nnew"] == int((w["stage"] == 0).sum()), c["name"]
            whole += 1
    assert whole >= 10


def test_numpy_against_the_fixture(cases, fixture, restated):
    fx = [{k: fixture[c["name"] + "/" + k] for k in (LINE_KEYS if sim.is_lines(c) else POINT_KEYS)} for c in cases]
    _compare(cases, fx, restated, "fixture vs numpy")
