"""The host-side plan of sslam_orb_search_by_bow_batch_dev (csrc/match_plan.h: batch_plan at BOW_BATCH_ROW_BYTES).  The header holds no HIP:
tests/sim/match_plan_dump.cpp compiles it with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program;
nothing is loaded into Python.  Every expected value is worked out here from the documented rule, never read back from the header:

  workgroup   one per pair, 8 waves of 64 lanes (wave w owns the nodes with id % 8 == w)
  form        the frame side of a pair in LDS -- 32 bytes of descriptor, 4 of node id, 4 of live assignment per row of the FRAME capacity -- while
              40 * cap <= 64 KB; beyond that the same kernel on global memory, with no dynamic LDS
  opt-in      more than 48 KB of dynamic LDS needs the per-kernel opt-in"""
import pytest
import plan_dump
import bow_batch_cases as bc

WAVES, ROW, LDS_MAX, LDS_DEFAULT, LDS_CU = 8, 40, 64 * 1024, 48 * 1024, 160 * 1024


@pytest.fixture(scope="module")
def ask():
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean (plan_dump.py)"""
    return plan_dump.asker("bow_batch")


def expect_plan(cap, npairs):
    lds = ROW * cap
    if lds <= LDS_MAX:
        return ["lds", str(lds), str(int(lds > LDS_DEFAULT)), str(64 * WAVES), str(npairs)]
    return ["global", "0", "0", str(64 * WAVES), str(npairs)]


def test_constants(ask):
    assert ask(["consts"]) == [[str(WAVES), str(ROW), str(LDS_MAX), str(LDS_DEFAULT)]]
    assert (bc.W, bc.ROW_BYTES, bc.LDS_MAX) == (WAVES, ROW, LDS_MAX)          # what the case module and the GPU test assume


LAST_LDS = LDS_MAX // ROW                 # 1638
LAST_PLAIN = LDS_DEFAULT // ROW           # 1228: the last capacity without the opt-in
CASES = [(0, 1), (1, 1), (64, 5), (1000, 64), (1000, 12288), (LAST_PLAIN, 3), (LAST_PLAIN + 1, 3), (LAST_LDS, 2), (LAST_LDS + 1, 2), (2000, 7), (8192, 1),
         ((1 << 19) - 1, 4), (1000, (1 << 31) - 1), (1000, 0)]


def test_plan_on_both_sides_of_every_boundary(ask):
    assert (LAST_LDS, LAST_PLAIN) == (1638, 1228) == (bc.LDS_CAP, LAST_PLAIN)
    assert ROW * LAST_LDS <= LDS_MAX < ROW * (LAST_LDS + 1) and ROW * LAST_PLAIN <= LDS_DEFAULT < ROW * (LAST_PLAIN + 1)
    got = dict(zip(CASES, ask(["plan %d %d" % c for c in CASES])))
    for c in CASES:
        assert got[c] == expect_plan(*c), (c, got[c])
    assert got[(LAST_LDS, 2)][:2] == ["lds", str(ROW * LAST_LDS)] and got[(LAST_LDS + 1, 2)][:2] == ["global", "0"]
    assert got[(LAST_PLAIN, 3)][2] == "0" and got[(LAST_PLAIN + 1, 3)][2] == "1" and got[(LAST_LDS, 2)][2] == "1" and got[(LAST_LDS + 1, 2)][2] == "0"
    assert got[(1000, 64)][1] == "40000" and got[(1000, 12288)][4] == "12288"        # a 1000-keypoint frame: 40 KB, three pairs per compute unit
    # the form follows the capacity alone, the grid the number of pairs alone
    assert got[(1000, 64)][:4] == got[(1000, 12288)][:4] == got[(1000, (1 << 31) - 1)][:4]


def test_lds_fits_a_compute_unit(ask):
    caps = [0, 1, 63, 64, 65, 1000, LAST_PLAIN, LAST_PLAIN + 1, LAST_LDS, LAST_LDS + 1, 5000, (1 << 19) - 1]
    for c, row in zip(caps, ask(["plan %d 9" % c for c in caps])):
        lds, opt_in = int(row[1]), int(row[2])
        assert lds <= LDS_MAX and 2 * (lds + 256) <= LDS_CU          # two pairs per compute unit beside the kernel's static arrays (histogram, kept bins, count)
        assert opt_in == int(lds > LDS_DEFAULT)
        assert int(row[3]) == 512 <= 1024 and row[4] == "9"
