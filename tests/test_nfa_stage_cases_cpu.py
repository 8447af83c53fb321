"""What the rectangle lists of tests/nfa_stage_cases.py reach, proved from the CPU oracle's verdicts (tests/sim/nfa_topn_oracle.cpp nfa_topn_verdicts: the oracle's own
rect_nfa / rect_improve per record) and the host model of csrc/nfa_topn.h (tests/sim/nfa_topn_sim.cpp) alone -- no GPU.  Every case is there for something
tests/test_nfa_stage_gpu.py means to drive k_nfa_topn through; this module asserts that it gets there, and that the set as a whole tells every mutant of the model
(nfa_topn_sim.MUTANTS: one wrong decision each, of the kind a kernel could make) from the rule by its flags."""
import numpy as np
import pytest
import nfa_stage_cases as nc
import nfa_topn_sim as sim


def _stats(name):
    """what the assertions below read of a case"""
    c = nc.case(name); v = nc.verdicts(name); flags, ranked, slices, validated = nc.expected(name)
    h, w = c.frame.shape
    mc = nc.model_case(name)
    n = len(c.rects); u = mc[3]
    acc = v["accepted"] == 1
    order = np.lexsort((np.arange(n), -u.astype(np.float64)))          # descending u, ties by ascending emission index
    first = min(n, nc.slice_size(c.N + 1))
    return dict(c=c, v=v, flags=flags, ranked=bool(ranked), slices=slices, validated=validated, n=n, u=u, acc=acc, order=order, first=first, w=w, h=h,
                acc_first=int(acc[order[:first]].sum()), twos=int((flags == 2).sum()), tau=nc.tau_of(name),
                m_in=np.float32(0.125) / np.float32(max(w, h)), r0=v["r0"].astype(np.float32), fin=v["final"].astype(np.float32), margin=v["margin"].astype(np.float32))


def _valid_record(r, sw, sh):
    """the tap's own test of a record (include/sslam_testing.h)"""
    ok = np.isfinite(r).all(1) & (r[:, 4] > 0) & (r[:, 4] <= max(sw, sh)) & (np.abs(r[:, 8] ** 2 + r[:, 9] ** 2 - 1) <= 1e-9)
    ok &= (r[:, 10] == np.pi * 22.5 / 180) & (r[:, 11] == 22.5 / 180)
    ok &= (r[:, 5] >= 0) & (r[:, 5] <= sw - 1) & (r[:, 6] >= 0) & (r[:, 6] <= sh - 1)
    for x, y in ((0, 1), (2, 3)):
        ok &= (r[:, x] >= -r[:, 4]) & (r[:, x] <= sw - 1 + r[:, 4]) & (r[:, y] >= -r[:, 4]) & (r[:, y] <= sh - 1 + r[:, 4])
    return ok


@pytest.mark.parametrize("name", nc.NAMES)
def test_every_record_is_one_the_core_emits_and_the_model_is_consistent(name):
    s = _stats(name)
    sw, sh = round(s["w"] * 0.8), round(s["h"] * 0.8)
    assert s["c"].frame.shape in ((nc.H, nc.W), (nc.ODD_H, nc.ODD_W)) and s["n"] <= 8192
    assert _valid_record(s["c"].rects, sw, sh).all()
    flags, acc = s["flags"], s["acc"]
    v = flags != 2
    assert np.array_equal(flags[v], acc[v].astype(np.int64)) and s["validated"] == v.sum()
    assert s["ranked"] == (s["c"].N >= 1 and s["c"].N < s["n"] <= nc.RANK_CAP)
    if not s["ranked"]: assert v.all() and s["slices"] == 1
    else: assert v[s["order"][:s["validated"]]].all() and not v[s["order"][s["validated"]:]].any()          # the validated ones are a prefix of the ranking
    # the top N of the validated subset are the top N of all candidates
    assert np.array_equal(sim.top_n(s["fin"], acc, s["c"].N), sim.top_n(s["fin"], acc & v, s["c"].N))
    # the oracle's verdict on a record taken over its own frame is the one the main loop gave it
    if name in ("one_slice", "waves200", "N1", "edge_margin", "odd_edge_margin", "odd_one_slice", "spiral_grows"):
        src = {"one_slice": "dense0", "waves200": "waves", "N1": "dense3", "edge_margin": "dense0", "odd_edge_margin": "odd0", "odd_one_slice": "odd3", "spiral_grows": "spiral8"}[name]
        fr, rects = sim.oracle_rects(nc.source(src)[0])
        assert np.array_equal(rects, s["c"].rects) and all(np.array_equal(fr[k], s["v"][k]) for k in sim.FIELDS)


def test_slices():
    s = _stats("one_slice")
    assert s["ranked"] and s["slices"] == 1 and s["validated"] == s["first"] == 20 and s["twos"] == s["n"] - 20 > 100
    s = _stats("odd_one_slice")          # 333 x 251: off the fused-gradient geometry
    assert s["ranked"] and s["slices"] == 1 and s["validated"] == 20 and s["twos"] > 100 and (s["w"], s["h"]) == (nc.ODD_W, nc.ODD_H)
    s = _stats("waves200")               # the whole frame: 716 candidates, 268 accepted, 716 distinct u
    assert (s["n"], int(s["acc"].sum()), len(np.unique(s["u"]))) == (716, 268, 716)
    assert s["ranked"] and s["slices"] == 9 and s["validated"] == 426 and s["twos"] == 290
    assert s["acc_first"] <= s["c"].N          # ... and its first slice does not settle it either
    s = _stats("foreign_short_first_slice")          # the first slice ends with no more than N accepted: the next one is slice_size(N + 1 - accepted), and in the end something is left out
    assert s["ranked"] and s["acc_first"] <= s["c"].N < int(s["acc"][s["flags"] != 2].sum()) and s["slices"] >= 3 and s["twos"] > 0
    second = s["first"] + nc.slice_size(s["c"].N + 1 - s["acc_first"])
    assert second < s["n"] and s["validated"] > second
    for name in ("never_more_than_n", "n960_N700"):          # never more than N accepted: everything is validated, slice after slice
        s = _stats(name)
        assert s["ranked"] and s["acc"].sum() <= s["c"].N and s["twos"] == 0 and s["validated"] == s["n"] and s["slices"] >= 2 and s["tau"] is None
    assert _stats("never_more_than_n")["slices"] >= 3
    s = _stats("checker10_ties")          # more than N accepted, and still nothing left out: every candidate's u is above the one response there is -- eighteen slices
    assert s["ranked"] and s["acc"].sum() > s["c"].N and s["twos"] == 0 and s["slices"] >= 10


def test_accept_count_boundaries():
    s = _stats("exactly_n_accepted")
    assert s["ranked"] and s["n"] > s["c"].N == s["acc"].sum() and s["twos"] == 0 and s["slices"] >= 2
    assert (s["u"][s["order"][s["first"]:]] < np.sort(s["fin"][s["acc"]])[0]).any()          # ... although candidates BELOW the N-th response are left when the N-th is accepted
    s = _stats("n_plus_1_accepted")
    assert s["ranked"] and s["acc"].sum() == s["c"].N + 1 and s["twos"] > 0 and (s["flags"][s["acc"]] == 1).all()


def test_count_boundaries():
    s = _stats("n_eq_N"); assert s["n"] == s["c"].N and not s["ranked"]
    s = _stats("n_eq_N_plus_1"); assert s["n"] == s["c"].N + 1 and s["ranked"] and s["validated"] == s["n"]
    s = _stats("n960"); assert s["n"] == nc.RANK_CAP and s["ranked"] and s["twos"] > 800 and s["slices"] >= 2
    s = _stats("n961"); assert s["n"] == nc.RANK_CAP + 1 and not s["ranked"] and s["n"] < nc.RANK_BASE
    s = _stats("N1"); assert s["c"].N == 1 and s["ranked"] and s["first"] == 10 and s["twos"] > 200
    s = _stats("N_ge_n"); assert s["c"].N >= s["n"] > 200 and not s["ranked"]
    s = _stats("n960_N700")
    assert s["c"].N == 700 and s["n"] == nc.RANK_CAP and s["first"] == 796 > nc.CHUNK and (s["first"] - nc.CHUNK) % 64 != 0 and s["slices"] == 2


def test_ties():
    s = _stats("ties_at_tau")          # eight records whose u IS tau, bit for bit: validated (excluded() is strict), and left out by a rule with <=
    tied = s["u"].view(np.uint32) == s["tau"].view(np.uint32)
    assert tied.sum() >= 8 and (s["flags"][tied] != 2).all() and s["twos"] > 0
    b = nc.source("waves")[1][nc.TIE_B]
    assert all(np.array_equal(r, b) for r in s["c"].rects[tied])
    assert s["order"].tolist().index(int(np.flatnonzero(tied)[0])) >= s["first"]          # ... behind the first slice: it is tau that lets them in
    mut = sim.model([nc.model_case("ties_at_tau")], mutant=3)[0][0]
    assert (mut[tied] == 2).all()
    s = _stats("checker10_ties")          # 2 distinct u among 960 records
    assert len(np.unique(s["u"])) == 2 and np.unique(s["u"], return_counts=True)[1].min() >= 8
    s = _stats("repeat_one")          # twelve copies of one record across the end of the first slice: the copies of the smaller emission index are validated, the others left out
    same = (s["c"].rects == s["c"].rects[s["order"][s["first"] - 1]]).all(1)
    assert same.sum() == 12 and len(np.unique(s["u"][same])) == 1
    f = s["flags"][same]
    assert 0 < (f == 2).sum() < 12 and (np.diff((f == 2).astype(int)) >= 0).all()
    s = _stats("n960")          # every record five times (one 960 / 190 = 5.05): ties all over the ranking
    assert len(np.unique(s["u"])) == 190


@pytest.mark.parametrize("name", ["edge_margin", "odd_edge_margin", "spiral_grows"])
def test_border_margin(name):
    """a candidate with MARGIN_EDGE_PX whose u is at or above the final tau while r0 + MARGIN_IN_PX is below it: validated only because of the wider margin"""
    s = _stats(name)
    edge = s["margin"] > s["m_in"]
    only = edge & (s["u"] >= s["tau"]) & ((s["r0"] + s["m_in"]).astype(np.float32) < s["tau"])
    assert only.any() and (s["flags"][only] != 2).all() and s["twos"] > 0
    mut = sim.model([nc.model_case(name)], mutant=4)[0][0]
    assert (mut[only] == 2).any()


def test_moved_and_growing_rectangles():
    for name in ("waves200", "spiral_grows"):          # an accepted candidate among the top N whose final response is not r0: rect_improve moved it
        s = _stats(name)
        top = sim.top_n(s["fin"], s["acc"], s["c"].N)
        assert (s["fin"][top] != s["r0"][top]).any() and (s["flags"][top] == 1).all()
    s = _stats("spiral_grows")          # ... and one whose response GREW beyond the inner margin: only the edge margin covers it
    g = nc.SPIRAL_GROWS
    assert s["acc"][g] and s["fin"][g] > s["r0"][g] + s["m_in"] and s["margin"][g] > s["m_in"] and s["fin"][g] <= s["u"][g]
    assert s["flags"][g] == 1 and g in sim.top_n(s["fin"], s["acc"], s["c"].N)


def test_mixed_call():
    frames, rects, ver, exp = nc.mixed()
    N = nc.MIXED_N
    n = [len(r) for r in rects]
    ranked = [bool(e[1]) for e in exp]
    assert frames.shape == (9, nc.H, nc.W)
    assert n[0] == 0 and n[1] == 1 and not ranked[0] and not ranked[1]
    assert ranked[2] and nc.RANK_CAP < n[3] <= nc.RANK_BASE and not ranked[3] and n[4] > nc.RANK_BASE + 500 and not ranked[4]
    assert all(ranked[5:]) and n[6] == N + 1 and n[7] == nc.RANK_CAP and len({n[i] for i in (2, 5, 6, 7, 8)}) == 5
    assert all((e[0] == 2).any() for i, e in enumerate(exp) if ranked[i] and i != 6)
    sw, sh = round(nc.W * 0.8), round(nc.H * 0.8)
    assert all(_valid_record(r, sw, sh).all() for r in rects if len(r))


def test_every_mutant_is_told_apart():
    cases = [nc.model_case(name) for name in nc.NAMES]
    want = [nc.expected(name)[0] for name in nc.NAMES]
    for k, what in sim.MUTANTS.items():
        got = sim.model(cases, mutant=k)
        differ = [name for name, g, w in zip(nc.NAMES, got, want) if not np.array_equal(g[0], w)]
        print("mutant %d (%s):" % (k, what), differ)
        assert differ, "no case tells mutant %d (%s) from the rule" % (k, what)
