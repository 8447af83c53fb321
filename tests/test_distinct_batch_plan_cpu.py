"""The host-side plan of sslam_distinctive_descriptors_batch_dev (csrc/match_plan.h: distinct_class, distinct_batch_plan).  The header holds no HIP:
tests/sim/match_plan_dump.cpp compiles it with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program;
nothing is loaded into Python.  Every expected value is worked out here from the documented rule, never read back from the header:

  class       by the ENTRY count of a set: 0 .. 8 small, 9 .. 64 medium, 65 .. 1024 large, more (or a malformed range, handed in as a negative count) refused
  first       k_distinct_batch: 4 waves of 64 lanes per workgroup, eight consecutive sets per wave, so 32 sets per workgroup; the grid is
              ceil(nsets / 32), capped at 2048 workgroups whose waves stride over the runs of eight; per wave 2 KB of rows and an 8 KB matrix of 16-bit
              distances (64 x 64), 40 KB per workgroup: four workgroups, sixteen waves, per compute unit
  second      k_distinct_large: one wave per workgroup, chunks of 64 sets (lane = set), ceil(nsets / 64) workgroups capped at 1024; 1024 rows of 32
              bytes and their 16-bit entry positions, 34 KB
  launches    both kernels whenever there is a set -- the host never reads d_ptr -- and none without"""
import pytest
import plan_dump
import distinct_batch_cases as dc

SMALL, MEDIUM, LARGE = 8, 64, 1024
SETS_PER_WAVE, WAVES, GRID_MAX = 8, 4, 2048
ROW_BYTES, DIST_BYTES = 32 * 64, 2 * 64 * 64
CHUNK, LARGE_GRID_MAX, LARGE_LDS = 64, 1024, (32 + 2) * 1024
LDS_CU, LDS_STATIC_MAX = 160 * 1024, 64 * 1024


@pytest.fixture(scope="module")
def ask():
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean (plan_dump.py)"""
    return plan_dump.asker("distinct_batch")


def expect_plan(nsets):
    per = SETS_PER_WAVE * WAVES
    fixed = [str(64 * WAVES), None, str(WAVES * (ROW_BYTES + DIST_BYTES)), "64", None, str(LARGE_LDS)]
    if nsets <= 0:
        fixed[1] = fixed[4] = "0"
        return ["0"] + fixed
    fixed[1] = str(min(-(-nsets // per), GRID_MAX)); fixed[4] = str(min(-(-nsets // CHUNK), LARGE_GRID_MAX))
    return ["2"] + fixed


def test_constants(ask):
    assert ask(["consts"]) == [[str(v) for v in (SMALL, MEDIUM, LARGE, SETS_PER_WAVE, WAVES, GRID_MAX, ROW_BYTES, DIST_BYTES, CHUNK, LARGE_GRID_MAX, LARGE_LDS)]]
    assert (dc.SMALL_MAX, dc.MEDIUM_MAX, dc.LARGE_MAX, dc.SETS_PER_WAVE, dc.WAVES, dc.GRID_MAX) == (SMALL, MEDIUM, LARGE, SETS_PER_WAVE, WAVES, GRID_MAX)      # what the case module and the GPU test assume
    assert SETS_PER_WAVE * SMALL == 64 and MEDIUM == 64          # a small set fills a group of eight lanes, a medium set a wave


def test_class_on_both_sides_of_every_bound(ask):
    counts = [-1, 0, 1, 8, 9, 64, 65, 1024, 1025, (1 << 31) - 1]
    got = [r[0] for r in ask(["class %d" % c for c in counts])]
    assert got == ["refused", "small", "small", "small", "medium", "medium", "large", "large", "refused", "refused"]


NSETS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65,
         32 * (GRID_MAX - 1), 32 * (GRID_MAX - 1) + 1, 32 * GRID_MAX - 1, 32 * GRID_MAX, 32 * GRID_MAX + 1, 32 * (GRID_MAX + 1),
         64 * (LARGE_GRID_MAX - 1), 64 * (LARGE_GRID_MAX - 1) + 1, 64 * LARGE_GRID_MAX - 1, 64 * LARGE_GRID_MAX, 64 * LARGE_GRID_MAX + 1, GRID_MAX - 1, GRID_MAX, GRID_MAX + 1, 2000 * 64, 2000 * 1024, (1 << 31) - 1]


def test_grids_on_both_sides_of_every_bound(ask):
    got = dict(zip(NSETS, ask(["plan %d" % n for n in NSETS])))
    for n in NSETS:
        assert got[n] == expect_plan(n), (n, got[n])
    grid = {n: int(got[n][2]) for n in NSETS}; large = {n: int(got[n][5]) for n in NSETS}
    assert [grid[n] for n in (0, 1, 7, 8, 9, 32, 33)] == [0, 1, 1, 1, 1, 1, 2]
    assert grid[32 * (GRID_MAX - 1) + 1] == GRID_MAX and grid[32 * (GRID_MAX - 1)] == GRID_MAX - 1          # the last grid below the cap, the first at it
    assert grid[32 * GRID_MAX] == grid[32 * GRID_MAX + 1] == grid[(1 << 31) - 1] == GRID_MAX                  # behind the cap the waves stride
    assert [large[n] for n in (0, 1, 64, 65)] == [0, 1, 1, 2] and large[64 * LARGE_GRID_MAX] == large[64 * LARGE_GRID_MAX + 1] == large[(1 << 31) - 1] == LARGE_GRID_MAX
    assert large[64 * (LARGE_GRID_MAX - 1)] == LARGE_GRID_MAX - 1 and large[64 * (LARGE_GRID_MAX - 1) + 1] == large[64 * LARGE_GRID_MAX - 1] == LARGE_GRID_MAX
    assert [got[n][0] for n in (0, 1, (1 << 31) - 1)] == ["0", "2", "2"]
    assert ask(["plan -5"]) == [expect_plan(0)]


def test_lds_fits_a_compute_unit(ask):
    row = ask(["plan 128000"])[0]
    lds, large_lds = int(row[3]), int(row[6])
    assert lds == 40 * 1024 <= LDS_STATIC_MAX and large_lds == 34 * 1024 <= LDS_STATIC_MAX          # static arrays: no opt-in
    assert LDS_CU // lds == 4 and 4 * WAVES == 16          # sixteen waves of the first kernel per compute unit, half its wave slots
    assert LDS_CU // large_lds == 4
    assert int(row[1]) == 256 <= 1024 and int(row[4]) == 64
