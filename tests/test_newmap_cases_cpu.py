"""CPU suite of the map-creation unit: csrc/newmap_math.h as the host model (tests/newmap_sim.py: plain and under -fsanitize=address,undefined, as stand-alone programs) on
the cases of tests/newmap_cases.py.  Everything is asserted on the model's output and its own trace.

  test_every_exit_occurs          every stage code of both tables of include/sslam_frontend.h, and the rows built for one exit take it
  test_gates_on_neighbours        0.9998 and 0.98 (the cosines on the two sides are neighbouring floats), 5.991 sigma^2 (neighbouring sigma^2, both errors), both sides of
                                  :615 (neighbouring scale factors), 0.3 and 0.61 (neighbouring median depths)
  test_special_values             a cosine <= 0, an exactly zero homogeneous coordinate (point, start and end of a line), NaN / inf key points, octaves outside
                                  [0, nlevels) on created rows, a line with its endpoints in the other order, other intrinsics per keyframe
  test_match_counts               0 / 1 / 63 / 64 / 65 / 255 / 256 / 257 / 513 matches, 0 / 1 / 63 / 64 / 65 / 125 line rows, rows without a match of every kind
  test_exports_are_declared       the new entry points are in the two headers (tests/test_abi_cpu.py derives its list from them)"""
import os
import re
import numpy as np
import pytest
import newmap_cases as ncases
import newmap_sim as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
nxt = ncases.nxt


@pytest.fixture(scope="module")
def R():
    cases = ncases.all_cases()
    return {c["name"]: (c, r) for c, r in zip(cases, sim.run(list(cases)))}


def test_every_exit_occurs(R):
    pts = np.concatenate([r["stage"] for c, r in R.values() if not sim.is_lines(c)])
    lns = np.concatenate([r["stage"] for c, r in R.values() if sim.is_lines(c)])
    assert set(pts.tolist()) == set(range(10)) and set(lns.tolist()) == set(range(15))
    named = 0
    for c, r in R.values():
        for row, stage in (c.get("want") or {}).items():
            assert r["stage"][row] == stage, (c["name"], row, r["stage"][row], stage)
            named += 1
    assert named == 20      # the two created rows of the swapped line, two points and two line ends on w == 0, three behind keyframe 2, two centres on the point, four ratios and a created line, four depths
    for c, r in R.values():      # what a row that is not created returns, and the count
        dead = r["stage"] != 0
        for k in (("s3d", "e3d", "normal", "dist") if sim.is_lines(c) else ("x3d", "normal", "dist")):
            assert not r[k][dead].any(), (c["name"], k)
        assert r["nnew"] == int((~dead).sum())
        assert np.isfinite(r["dist"][~dead]).all() and (r["dist"][~dead] > 0).all()


def test_gates_on_neighbours(R):
    # :497 and :1053: one float of an input between the rows, and the cosines themselves are neighbours around the constant
    for name, key, col, const, stage in (("p_cos_edge", "kp2", 0, 0.9998, 2), ("l_cos_edge", "kl2", 2, 0.98, 3)):
        c, r = R[name]
        a, b = c["edge"]
        assert nxt(c[key][a, col]) == c[key][b, col]
        assert r["stage"][a] == 0 and r["stage"][b] == stage
        assert float(r["cos"][a]) < const <= float(r["cos"][b]) and nxt(r["cos"][a]) == r["cos"][b]
    # :557 and :584
    c, r = R["p_err_edge"]
    for (a, b), which, stage, lvl in zip(c["edge"], (0, 1), (6, 7), ("oct1", "oct2")):
        sa, sb = c["sigma2"][c[lvl][a]], c["sigma2"][c[lvl][b]]
        assert nxt(sa) == sb and r["err"][a, which] == r["err"][b, which] > 0
        assert float(r["err"][a, which]) > 5.991 * float(sa) and not float(r["err"][b, which]) > 5.991 * float(sb)
        assert r["stage"][a] == stage and r["stage"][b] == 0
    # :615, first and second side
    c, r = R["p_scale_edge"]
    rf = f32(1.5) * f32(c["scale_factor"])
    (a, b), (d, e) = c["edge"]
    assert nxt(c["sf"][c["oct1"][a]]) == c["sf"][c["oct1"][b]] and nxt(c["sf"][c["oct2"][d]]) == c["sf"][c["oct2"][e]]
    assert list(r["stage"][[a, b, d, e]]) == [0, 9, 0, 9]
    rd, ro = r["ratio"][:, 0], r["ratio"][:, 1]
    assert not f32(rd[a] * rf) < ro[a] and f32(rd[b] * rf) < ro[b] and not rd[b] > f32(ro[b] * rf)
    assert not rd[d] > f32(ro[d] * rf) and rd[e] > f32(ro[e] * rf) and not f32(rd[e] * rf) < ro[e]
    # :1102-1131
    (ca, ra), (cb, rb) = R["l_ratio_lo_pass"], R["l_ratio_lo_trip"]
    assert nxt(f32(ca["median"])) == f32(cb["median"]) and ra["stage"][0] == 0 and rb["stage"][0] in (6, 7, 9, 10)
    k = {6: 0, 7: 1, 9: 3, 10: 4}[int(rb["stage"][0])]
    assert float(rb["ratio"][0, k]) < 0.3 <= float(ra["ratio"][0, k])
    (ca, ra), (cb, rb) = R["l_ratio3_pass"], R["l_ratio3_trip"]
    assert nxt(f32(ca["median"]), False) == f32(cb["median"]) and ra["stage"][0] == 0 and rb["stage"][0] == 8
    assert float(ra["ratio"][0, 2]) <= 0.61 < float(rb["ratio"][0, 2])


def test_special_values(R):
    c, r = R["p_count_513"]
    matched = (c["m12"] >= 0) & (c["m12"] < len(c["oct2"]))
    assert ((r["stage"] == 2) & (r["cos"] <= 0)).any()
    k1, k2 = c["kp1"][matched], c["kp2"][c["m12"][matched]]
    odd = ~(np.isfinite(k1).all(1) & np.isfinite(k2).all(1))
    assert np.isnan(k1).any() and np.isinf(k1).any() and np.isinf(k2).any() and (r["stage"][matched][odd] == 2).all()
    nl = len(c["sf"])
    out1 = (c["oct1"] < 0) | (c["oct1"] >= nl); out2 = np.zeros(len(out1), bool); out2[matched] = (c["oct2"][c["m12"][matched]] < 0) | (c["oct2"][c["m12"][matched]] >= nl)
    assert (out1 & matched & (r["stage"] == 0)).any() and (out2 & matched & (r["stage"] == 0)).any() and (c["oct1"] < 0).any() and (c["oct1"] >= nl).any()
    # exact zeros
    c, r = R["p_w_zero"]
    assert (r["hom"][:2, 3] == 0).all() and (r["hom"][:2, :3] != 0).any(1).all() and r["hom"][2, 3] != 0 and (r["cos"][:2] < 0.9998).all()
    c, r = R["l_w_zero"]
    assert r["hom"][0, 3] == 0 and r["hom"][0, :3].any() and r["hom"][1, 3] != 0 and r["hom"][1, 7] == 0 and r["hom"][1, 4:7].any()
    np.testing.assert_array_equal(c["kl1"][1], c["kl1"][0][[2, 3, 0, 1]])
    # the line whose endpoints are in the other order gives the same two points the other way round, and the same normal and distances
    c, r = R["l_swapped"]
    np.testing.assert_array_equal(c["kl1"][1], c["kl1"][0][[2, 3, 0, 1]])
    assert (r["stage"] == 0).all() and r["s3d"][0].any() and (r["s3d"][0] != r["e3d"][0]).any()
    for a, b in ((r["s3d"][1], r["e3d"][0]), (r["e3d"][1], r["s3d"][0]), (r["normal"][1], r["normal"][0]), (r["dist"][1], r["dist"][0])):
        assert a.tobytes() == b.tobytes()
    # other intrinsics per keyframe on a pair that creates lines: the cx1-for-line-2 quirk of :1032-1035 takes part
    c, r = R["l_count_125"]
    assert (c["pose1"][15:19] != c["pose2"][15:19]).all() and r["nnew"] > 10


def test_match_counts(R):
    for n in ncases.COUNTS:
        c, r = R["p_count_%d" % n]
        m = c["m12"]
        assert int(((m >= 0) & (m < len(c["oct2"]))).sum()) == n and (r["stage"] == 1).sum() == len(m) - n
        assert (m == -1).any() and (m < -1).any() and (m == len(c["oct2"])).any()
    for n in ncases.LINE_COUNTS:
        c, r = R["l_count_%d" % n]
        assert len(c["lp"]) == n == len(r["stage"])
    c, r = R["l_rows_300"]
    assert len(r["stage"]) == 300 > 256 and set(r["stage"][256:].tolist()) >= {0, 2} and r["nnew"] > (r["stage"][:256] == 0).sum()      # the lanes' second turn creates too
    c, r = R["l_count_125"]
    assert (c["lp"] < 0).any() and (c["lp"][:, 1] >= len(c["loct2"])).any() and (c["lp"][:, 0] >= len(c["loct1"])).any() and c["free1"] is not None and (r["stage"] == 2).any()


def test_exports_are_declared():
    front = open(os.path.join(ROOT, "include", "sslam_frontend.h")).read()
    testing = open(os.path.join(ROOT, "include", "sslam_testing.h")).read()
    for n in ("sslam_new_map_points_batch_dev", "sslam_new_map_lines_batch_dev", "sslam_new_map_points", "sslam_new_map_lines"):
        assert re.search(r"\bint %s\s*\(" % n, front), n
    for n in ("sslam_testing_new_map_points", "sslam_testing_new_map_lines"):
        assert re.search(r"\bint %s\s*\(" % n, testing), n
    assert "typedef struct sslam_kf_pose" in front and "typedef struct sslam_newmap_pair" in front
