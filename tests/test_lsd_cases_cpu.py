"""The preconditions of tests/test_lsd_forms_gpu.py, from the generators (tests/lsd_cases.py) and the oracle's trace alone (orc_lsd_trace: oracle/lsd_oracle.cpp LsdTrace, filled
by the detector's own functions): a frame that does not reach the region size, the branch or the candidate count it is named after would pass on the device without testing
anything.  LSD is not part of the reference tree (un-vendored OpenCV: oracle/lsd_oracle.cpp's header), so oracle/_ref has no binary to hold this oracle against; what is
checked here is that the trace describes the SAME run as orc_lines_extract (the segments are equal) and that its counters are consistent with each other."""
import math
import numpy as np
import pytest
import lsd_cases as lc

_TR = {}


def _trace(oracle, group, name):
    """(trace, segments, candidate ordinals) of a case, computed once"""
    if (group, name) not in _TR:
        _TR[group, name] = oracle.lsd_trace(lc.frame(group, name))
    return _TR[group, name]


def _holds(t, want):
    return [(k, v, t[k]) for k, v in want.items() if not (t[k] >= v[1] if isinstance(v, tuple) else t[k] == v)]


def _consistent(t, seg, cand):
    assert t["segments"] == len(seg) == len(cand)
    assert sum(t["improve%d" % i] for i in range(6)) == t["segments"] and t["segments"] + t["rejected"] == t["candidates"]
    assert (np.diff(cand) > 0).all() and (len(cand) == 0 or (cand[0] >= 0 and cand[-1] < t["candidates"]))
    assert t["seeds"] <= t["defined"] and t["reg_max"] <= t["defined"] and t["refines_big"] <= t["refines"] and t["reduce_iters_big"] <= t["reduce_iters"]
    assert t["min_reg_size"] == int(-(5 * (math.log10(t["sw"]) + math.log10(t["sh"])) / 2 + math.log10(11.0)) / math.log10(0.125))


@pytest.mark.parametrize("name", list(lc.CORE))
def test_core_case_reaches_its_edge(oracle, name):
    img = lc.frame("core", name)
    assert img.shape == (lc.CORE_H, lc.CORE_W)
    t, seg, cand = _trace(oracle, "core", name)
    print(name, {k: v for k, v in t.items() if v})
    assert (t["sw"], t["sh"]) == (256, 192)
    _consistent(t, seg, cand)
    assert not _holds(t, lc.CORE[name][1]), _holds(t, lc.CORE[name][1])
    np.testing.assert_array_equal(seg, oracle.lines_extract(img, 40)[3])          # the traced run is the run the GPU tests compare with


@pytest.mark.parametrize("name", list(lc.LIMIT))
def test_limit_case_reaches_its_count(oracle, name):
    img = lc.frame("limit", name)
    assert img.shape == (lc.LIMIT_H, lc.LIMIT_W)
    t, seg, cand = _trace(oracle, "limit", name)
    print(name, {k: v for k, v in t.items() if v})
    _consistent(t, seg, cand)
    assert not _holds(t, lc.LIMIT[name][1]), _holds(t, lc.LIMIT[name][1])
    np.testing.assert_array_equal(seg, oracle.lines_extract(img, 40)[3])


def test_limit_cases_straddle_the_limit(oracle):
    """8 192 exactly, one more, an overflow with fewer than 8 192 segments, and one with more than 8 192 segments among the first 8 192 candidates or not: what the device
    keeps of an overflowing frame (the segments of candidates 0 .. 8 191) differs from what the oracle emits"""
    c = {n: _trace(oracle, "limit", n) for n in lc.LIMIT}
    assert c["squares2048"][0]["candidates"] == lc.MAX_SEG and c["squares2048_bar"][0]["candidates"] == lc.MAX_SEG + 1
    assert c["checker16"][0]["candidates"] > lc.MAX_SEG > c["checker16"][0]["segments"]
    assert c["checker12"][0]["candidates"] > 2 * lc.MAX_SEG and c["checker12"][0]["segments"] > lc.MAX_SEG
    for n in ("squares2048_bar", "checker12", "checker16"):
        t, seg, cand = c[n]
        kept = int((cand < lc.MAX_SEG).sum())
        print(n, "candidates", t["candidates"], "segments", len(seg), "kept below the limit", kept)
        assert 0 < kept <= len(seg) and (n == "squares2048_bar" or kept < len(seg))


def test_core_list_reaches_everything(oracle):
    """over the core list: every accepting stage of rect_improve and the rejection, every reachable return of nfa() (lsd_cases.py says why the tail loop cannot run to n), both
    outside-the-image skips of rect_nfa, the three region sizes about QCAP, refine() and reduce_region_radius() on more than QCAP points, refine() returning false, regions of
    min_reg_size - 1 and min_reg_size points, regions on every border of the gradient image, and the candidate counts 0, 1, 8 and 9; over the limit list 8 192, more, and
    more than twice as many"""
    tr = {n: _trace(oracle, "core", n)[0] for n in lc.CORE}
    reached = lambda k: [n for n, t in tr.items() if t[k] > 0]
    for k in ["improve%d" % i for i in range(6)] + ["rejected", "nfa_zero", "nfa_all", "nfa_term0_above", "nfa_term0_below", "nfa_break", "rows_outside", "cols_outside",
                                                    "reg767", "reg768", "reg769", "refines_big", "reduce_iters_big", "refine_false", "reg_min_m1", "reg_min",
                                                    "touch_row0", "touch_row_last", "touch_col0", "touch_col_last"]:
        print("%-18s %s" % (k, ", ".join(reached(k))))
        assert reached(k), k
    assert not reached("nfa_full")
    assert max(t["regrown_max"] for t in tr.values()) > lc.QCAP
    counts = {t["candidates"] for t in tr.values()}
    assert {0, 1, lc.NFA_STREAM_BLOCK, lc.NFA_STREAM_BLOCK + 1} <= counts, sorted(counts)
    assert [n for n, t in tr.items() if t["candidates"] == 0 and t["seeds"] > 0] and [n for n, t in tr.items() if t["defined"] == 0]
    lim = sorted(_trace(oracle, "limit", n)[0]["candidates"] for n in lc.LIMIT)
    assert lim[0] == lc.MAX_SEG and lim[1] == lc.MAX_SEG + 1 and lim[-1] > 2 * lc.MAX_SEG


def test_head_sizes(oracle):
    """the scaled sizes the head cases are chosen for, on both sides of each bound, and something to detect in every accepted one but the very smallest"""
    sc = lambda w, h: tuple(oracle.lsd_scaled(lc.frame("head", (w, h))).shape[::-1])
    assert sc(320, 240) == (256, 192) and sc(321, 240) == (257, 192) and sc(320, 241) == (256, 193) and sc(640, 480) == (512, 384) and sc(641, 480) == (513, 384)
    assert sc(20, 10) == (16, 8) and sc(25, 10) == (20, 8) and sc(10, 10) == (8, 8)
    for w, h in lc.HEADS:
        assert min(w, h) >= lc.MIN_SIDE
        t, seg, cand = _trace(oracle, "head", (w, h))
        _consistent(t, seg, cand)
        assert t["seeds"] > 0 and t["candidates"] > 0, (w, h)
        np.testing.assert_array_equal(seg, oracle.lines_extract(lc.frame("head", (w, h)), 40)[3])
    assert sum(len(_trace(oracle, "head", wh)[1]) > 0 for wh in lc.HEADS) >= len(lc.HEADS) - 1
    for w, h in lc.TOO_SMALL:          # the oracle itself handles them; the library refuses them (tests/test_lsd_forms_gpu.py)
        assert min(w, h) < lc.MIN_SIDE
        _trace(oracle, "head", (w, h))
