"""The host-side plan of sslam_orb_search_by_bow_keyframes_batch_dev (csrc/match_plan.h: batch_plan at BOW_BATCH_ROW_BYTES -- the staged keyframe-2
row is the KeyFrame -> Frame batch's row: 32 bytes of descriptor, 4 of node id, 4 of state word, so the constant is shared and tests/plan_dump.py serves
as it is: tests/sim/match_plan_dump.cpp compiled with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program;
nothing is loaded into Python).  Every expected value is worked out here from the documented rule, never read back from the header:

  workgroup   one per pair of keyframe slots, 8 waves of 64 lanes (wave w owns the nodes with id % 8 == w)
  form        keyframe 2 in LDS, 40 bytes per row of the pool's capacity, while 40 * cap <= 64 KB; beyond that the same kernel on global memory with
              the state words in the pair's d_matches21 rows, and no dynamic LDS
  opt-in      more than 48 KB of dynamic LDS needs the per-kernel opt-in"""
import os
import re
import pytest
import plan_dump
import bow_kf_batch_cases as kc

WAVES, LDS_MAX, LDS_DEFAULT, LDS_CU = 8, 64 * 1024, 48 * 1024, 160 * 1024
ROW = 32 + 4 + 4          # descriptor, node id, state word
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "structure-slam-pointline_amd", "csrc")


@pytest.fixture(scope="module")
def ask():
    return plan_dump.asker("bow_batch")


def expect_plan(cap, npairs):
    lds = ROW * cap
    if lds <= LDS_MAX:
        return ["lds", str(lds), str(int(lds > LDS_DEFAULT)), str(64 * WAVES), str(npairs)]
    return ["global", "0", "0", str(64 * WAVES), str(npairs)]


def test_the_entry_point_plans_with_the_shared_row_constant(ask):
    """the row constant the dump program reports is the one the new entry point passes to batch_plan, and the kernel stages exactly that row"""
    assert ask(["consts"]) == [[str(WAVES), str(ROW), str(LDS_MAX), str(LDS_DEFAULT)]]
    assert (kc.W, kc.ROW_BYTES, kc.LDS_MAX, kc.LDS_CAP, kc.OPT_IN_CAP) == (WAVES, ROW, LDS_MAX, 1638, 1228)      # what the case module and the GPU test assume
    src = open(os.path.join(CSRC, "match.hip")).read()
    body = src[src.index('extern "C" int sslam_orb_search_by_bow_keyframes_batch_dev('):]
    assert re.search(r"batch_plan\(BOW_BATCH_ROW_BYTES, cap\)", body) and "launch_batch(ctx, \"k_search_bow_kf_batch\", k_search_bow_kf_batch<true>, k_search_bow_kf_batch<false>" in body


LAST_LDS = LDS_MAX // ROW                 # 1638
LAST_PLAIN = LDS_DEFAULT // ROW           # 1228: the last capacity without the opt-in
CASES = [(0, 1), (1, 1), (64, 20), (1000, 20), (1000, 64), (1000, 1024), (1000, 12288), (LAST_PLAIN, 3), (LAST_PLAIN + 1, 3), (LAST_LDS, 2), (LAST_LDS + 1, 2),
         (2000, 7), ((1 << 19) - 1, 4), (1000, 0)]


def test_plan_on_both_sides_of_48_and_64_kb(ask):
    assert (LAST_LDS, LAST_PLAIN) == (1638, 1228)
    assert ROW * LAST_LDS <= LDS_MAX < ROW * (LAST_LDS + 1) and ROW * LAST_PLAIN <= LDS_DEFAULT < ROW * (LAST_PLAIN + 1)
    got = dict(zip(CASES, ask(["plan %d %d" % c for c in CASES])))
    for c in CASES:
        assert got[c] == expect_plan(*c), (c, got[c])
    assert got[(LAST_PLAIN, 3)][:3] == ["lds", str(ROW * 1228), "0"] and got[(LAST_PLAIN + 1, 3)][:3] == ["lds", str(ROW * 1229), "1"]
    assert got[(LAST_LDS, 2)][:3] == ["lds", str(ROW * 1638), "1"] and got[(LAST_LDS + 1, 2)][:3] == ["global", "0", "0"]
    assert got[(1000, 20)][1] == "40000" and got[(1000, 20)][4] == "20"                # one loop closure: 20 candidates, 40 KB each
    assert got[(1000, 20)][:4] == got[(1000, 12288)][:4]                              # the form follows the capacity alone, the grid the number of pairs alone


def test_lds_fits_a_compute_unit(ask):
    caps = [0, 1, 63, 64, 65, 1000, LAST_PLAIN, LAST_PLAIN + 1, LAST_LDS, LAST_LDS + 1, 5000, (1 << 19) - 1]
    for c, row in zip(caps, ask(["plan %d 9" % c for c in caps])):
        lds, opt_in = int(row[1]), int(row[2])
        assert lds <= LDS_MAX and 2 * (lds + 256) <= LDS_CU          # two pairs per compute unit beside the kernel's static arrays (histogram, kept bins, count)
        assert opt_in == int(lds > LDS_DEFAULT) and int(row[3]) == 512 and row[4] == "9"
