"""The preconditions of tests/test_lsd_core_gpu.py, from the generators (tests/lsd_core_cases.py, tests/lsd_cases.py) and the oracle's core record alone (orc_lsd_core:
oracle/lsd_oracle.cpp LsdCore, filled by the detector's own loop and functions): that the record describes the SAME run as tests/nfa_topn_sim.py oracle_rects (the records
are bit-equal) and as orc_lsd_trace, that the used map is consistent with the regions, and that every frame reaches the threshold of the device code it is named after --
a helper torus reach of 253 / 254 / 255, list lengths 1 / 2 / 32 / 33 around CL_STG, the contention bound, the LDS / global bitmap boundary.  A frame that does not would
pass on the device without testing anything."""
import re
import os
import numpy as np
import pytest
import lsd_cases as lc
import lsd_core_cases as cc
import nfa_topn_sim as ts

_CORE = {}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "structure-slam-pointline_amd", "csrc")


def core(oracle, group, name):
    """Oracle.lsd_core of a case, computed once (tests/test_lsd_core_gpu.py shares it)"""
    if (group, name) not in _CORE:
        _CORE[group, name] = oracle.lsd_core(cc.frame(group, name))
    return _CORE[group, name]


def _consistent(c):
    """the record against itself: seeds, candidates, point counts and the used map"""
    cd, sd, used = c["cand"], c["seeds"], c["used"]
    assert used.shape == (c["sh"], c["sw"]) and len(cd) == len(c["rects"]) <= len(sd)
    assert not used[-1].any() and not used[:, -1].any()          # (no gradient in the last row and column)
    nused = int(used.sum())
    assert (sd["first"] >= 1).all() and (sd["list_len"] >= sd["first"]).all() and (sd["first"] <= nused).all() if len(sd) else nused == 0
    assert (cd["points"] >= 2).all() and (cd["points"] <= nused).all()
    assert used[sd["y"], sd["x"]].all()          # a seed that grew stays USED whatever became of its region (too small, refine() false, reduced)
    assert len(set(zip(sd["x"].tolist(), sd["y"].tolist()))) == len(sd)
    # every candidate is a grown seed, in the same order, of at least min_reg_size first points; its record's points lie inside its box, its box inside its reach
    pos = {(int(s["x"]), int(s["y"])): i for i, s in enumerate(sd)}
    idx = np.array([pos[int(q["x"]), int(q["y"])] for q in cd], np.int64)
    assert (np.diff(idx) > 0).all()
    assert (sd["first"][idx] >= c["min_reg_size"]).all()
    assert ((sd["list_len"][idx] > sd["first"][idx]) == (cd["regrew"] != 0)).all() and (cd["regrew"] >= cd["reduced"]).all()
    assert (cd["x0"] <= cd["x"]).all() and (cd["x"] <= cd["x1"]).all() and (cd["y0"] <= cd["y"]).all() and (cd["y"] <= cd["y1"]).all()
    assert (np.maximum(np.maximum(cd["x"] - cd["x0"], cd["x1"] - cd["x"]), np.maximum(cd["y"] - cd["y0"], cd["y1"] - cd["y"])) <= cd["reach"]).all()
    assert (cd["points"] <= (cd["x1"] - cd["x0"] + 1) * (cd["y1"] - cd["y0"] + 1)).all()
    # the used pixels are at least the points of the candidates and of the seeds that stayed below min_reg_size (those regions are never released)
    small = sd["first"] < c["min_reg_size"]
    assert nused >= int(cd["points"].sum()) + int(sd["first"][small].sum())
    # a record's centre is a weighted mean of its points (up to the rounding of the sums: a region one pixel wide can give 126.00000000000001)
    r, eps = c["rects"], 1e-9
    assert (r[:, 5] >= cd["x0"] - eps).all() and (r[:, 5] <= cd["x1"] + eps).all() and (r[:, 6] >= cd["y0"] - eps).all() and (r[:, 6] <= cd["y1"] + eps).all()


def _same_run(oracle, c, img):
    fr, rects = ts.oracle_rects(img)
    n = min(len(c["rects"]), 8192)          # (oracle_rects keeps the first 8 192)
    assert len(rects) == n
    np.testing.assert_array_equal(c["rects"][:n].view(np.uint64), rects.view(np.uint64))


@pytest.mark.parametrize("group,name", cc.existing(), ids=lambda v: str(v).replace(" ", ""))
def test_existing_frames(oracle, group, name):
    """the 17 core frames and the 12 head sizes of tests/lsd_cases.py: the record equals oracle_rects bit for bit and agrees with the trace's counters"""
    img = cc.frame(group, name)
    c = core(oracle, group, name)
    _consistent(c)
    _same_run(oracle, c, img)
    t = oracle.lsd_trace(img)[0]
    assert (c["sw"], c["sh"], c["min_reg_size"]) == (t["sw"], t["sh"], t["min_reg_size"])
    assert len(c["rects"]) == t["candidates"] and len(c["seeds"]) == t["seeds"]
    assert int(c["cand"]["points"].max(initial=0)) <= max(t["reg_max"], t["regrown_max"]) and int(c["seeds"]["first"].max(initial=0)) == t["reg_max"]
    assert int((c["seeds"]["first"] == c["min_reg_size"] - 1).sum()) == t["reg_min_m1"] and int((c["seeds"]["first"] == 767).sum()) == t["reg767"]
    assert int((c["seeds"]["list_len"] > c["seeds"]["first"]).sum()) == t["refines"]
    print(group, name, "candidates", len(c["rects"]), "seeds", len(c["seeds"]), "used", int(c["used"].sum()), "blocked_joins", c["blocked_joins"],
          "max reach", int(c["cand"]["reach"].max(initial=0)))


def test_constant_frame_leaves_an_empty_map(oracle):
    c = core(oracle, "core", "constant")
    assert not c["used"].any() and len(c["rects"]) == 0 and len(c["seeds"]) == 0 and c["blocked_joins"] == 0


def test_limit_frames_export_every_candidate(oracle):
    """the over-limit frames: the record holds ALL candidates (oracle_rects stops at 8 192 and serves the frame of exactly 8 192 only) and counts what the trace counts; the
    device keeps the first 8 192"""
    for name in lc.LIMIT:
        c = core(oracle, "limit", name)
        assert len(c["rects"]) == oracle.lsd_trace(cc.frame("limit", name))[0]["candidates"] >= lc.MAX_SEG
        if len(c["rects"]) == lc.MAX_SEG: _same_run(oracle, c, cc.frame("limit", name))
        _consistent(c)


def _some(values, want):
    return (values >= want[1]).any() if isinstance(want, tuple) else (values == want).any()


@pytest.mark.parametrize("group,name", cc.new(), ids=lambda v: str(v))
def test_new_case_reaches_its_threshold(oracle, group, name):
    img = cc.frame(group, name)
    want = cc.GROUPS[group][name][1]
    c = core(oracle, group, name)
    _consistent(c)
    _same_run(oracle, c, img)
    cd, sd = c["cand"], c["seeds"]
    if group == "reach":
        assert img.shape == (cc.REACH_H, cc.REACH_W) and (c["sw"], c["sh"]) == (320, 48)
        assert _some(cd["reach"][cd["points"] <= want.get("points_max", 1 << 30)], want["reach"]), (sorted(cd["reach"].tolist()), cd["points"].tolist())
        assert not cd["regrew"].any()
        print(name, "reaches", sorted(cd["reach"].tolist()), "points", cd["points"].tolist(), "regrew", cd["regrew"].tolist())
    if group == "stg":
        assert img.shape == (lc.CORE_H, lc.CORE_W)
        for v in want["list_len"]:
            hit = sd["list_len"] == v
            assert hit.any(), (v, sorted(set(sd["list_len"].tolist())))
            print(name, "list length", v, "seeds", int(hit.sum()), "first growth", sd["first"][hit].tolist())
    if group == "contention":
        assert img.shape == (lc.CORE_H, lc.CORE_W)
        base = core(oracle, "core", "step160")["blocked_joins"]
        print(name, "blocked_joins", c["blocked_joins"], "step160", base, "candidates", len(cd), "seeds", len(sd), "regrown", int(cd["regrew"].sum()))
        assert c["blocked_joins"] >= want["blocked_joins"][1] >= cc.CONTENTION_MIN and c["blocked_joins"] >= 10 * base
    if group == "bitmap":
        assert (c["sw"], c["sh"]) == want["size"]
        big = c["sw"] > cc.LDS_SW or c["sh"] > cc.LDS_SH
        assert big == (name != "lds_1024x512")
        if "cross_col" in want: assert ((cd["x0"] <= want["cross_col"]) & (cd["x1"] >= want["cross_col"])).any()
        if "cross_row" in want: assert ((cd["y0"] <= want["cross_row"]) & (cd["y1"] >= want["cross_row"])).any()
        if "touch_col" in want: assert (cd["x1"] == want["touch_col"]).any() and want["touch_col"] == c["sw"] - 2
        if "touch_row" in want: assert (cd["y1"] == want["touch_row"]).any() and want["touch_row"] == c["sh"] - 2
        print(name, c["sw"], c["sh"], "candidates", len(cd), "boxes to", int(cd["x1"].max()), int(cd["y1"].max()), "max reach", int(cd["reach"].max()))


def test_the_three_reaches_sit_around_the_torus(oracle):
    """253, 254 and 255 exactly, in both sets: `abs(xx - seedX) > REACH` gives up, so 254 is the last reach a helper keeps and 255 the first it gives up on; and one far beyond"""
    for kind in ("step", "thin"):
        got = [int(core(oracle, "reach", "%s%d" % (kind, v))["cand"]["reach"].max()) for v in (253, 254, 255)]
        assert got == [cc.TORUS_REACH - 1, cc.TORUS_REACH, cc.TORUS_REACH + 1], (kind, got)
    for v in (253, 254, 255):          # step: beyond the helpers' point limit and around the LDS queue's end; thin: far below both
        assert int(core(oracle, "reach", "step%d" % v)["cand"]["points"].max()) > lc.QCAP - 64 and int(core(oracle, "reach", "thin%d" % v)["cand"]["points"].max()) <= cc.HELPER_POINTS
    assert int(core(oracle, "reach", "step300")["cand"]["reach"].max()) >= 300


def test_list_lengths_sit_around_the_staging_limit(oracle):
    """1 (never staged: cnt > 1), 2 (the shortest staged list), CL_STG (the longest) and CL_STG + 1 (the global path), each as some seed's result"""
    seen = set()
    for name in cc.STG: seen |= set(core(oracle, "stg", name)["seeds"]["list_len"].tolist())
    assert {1, 2, cc.CL_STG, cc.CL_STG + 1} <= seen


def test_constants_are_the_headers(oracle):
    """the copies in tests/lsd_core_cases.py against the headers' text as it stands (csrc/lines.hip also pins them with a static_assert)"""
    reg = open(os.path.join(CSRC, "lsd_regions.h")).read(); clu = open(os.path.join(CSRC, "lsd_cluster.h")).read(); form = open(os.path.join(CSRC, "lines_form.h")).read()
    assert int(re.search(r"struct TorusWide \{[^}]*REACH = (\d+)", reg).group(1)) == cc.TORUS_REACH
    assert int(re.search(r"#define SSLAM_CL_STG (\d+)", clu).group(1)) == cc.CL_STG
    assert re.search(r"#define SSLAM_CL_HELPERS_PER_WG 3\b", clu)          # (three helpers per workgroup: ClTorus is TorusWide)
    m = re.search(r"LINES_CLUSTER_LDS_SW = (\d+), LINES_CLUSTER_LDS_SH = (\d+)", form)
    assert (int(m.group(1)), int(m.group(2))) == (cc.LDS_SW, cc.LDS_SH)
