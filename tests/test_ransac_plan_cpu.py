"""The host-side plans of the two RANSAC units (csrc/match_plan.h: two_view_plan for sslam_two_view_ransac*, sim3_plan for sslam_sim3_ransac*).  The header holds no HIP:
tests/sim/match_plan_dump.cpp compiles it with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program; nothing is loaded into
Python.  Every expected value is worked out here from the documented rule, never read back from the header:

  workgroup   one wave of 64 lanes per pair
  two-view    16 bytes of LDS per row of the capacity (u1, v1, u2, v2) and behind them the Jacobi workspace of the 64 lanes, 45 + 81 doubles each
  Sim3        48 bytes of LDS per row of the capacity (X1, X2, P1im1, P2im2, maxErr1, maxErr2), nothing behind them
  opt-in      more than 48 KB of dynamic LDS needs the per-kernel opt-in
  capacity    whole steps of 1024 rows: what fits the 160 KB of a compute unit beside 256 bytes for the kernel's static words -- and, for two-view, rows of 64 KB at most"""
import pytest
import plan_dump

LDS_CU, LDS_DEFAULT, STATIC, STEP, LANES = 160 * 1024, 48 * 1024, 256, 1024, 64
TV_ROW, TV_WS, TV_ROWS_MAX = 16, 8 * (45 + 81) * 64, 64 * 1024
S3_ROW = 48
TV_MAX = min(LDS_CU - STATIC - TV_WS, TV_ROWS_MAX) // TV_ROW // STEP * STEP
S3_MAX = (LDS_CU - STATIC) // S3_ROW // STEP * STEP


@pytest.fixture(scope="module")
def ask():
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean (plan_dump.py)"""
    return plan_dump.asker()


def expect(row, fixed, max_cap, cap):
    lds = row * cap + fixed
    return [str(row), str(lds), str(int(lds > LDS_DEFAULT)), str(LANES), str(max_cap)]


def test_capacity_bounds():
    assert (TV_MAX, S3_MAX) == (4096, 3072)                                  # what include/sslam_frontend.h promises
    assert TV_ROW * TV_MAX + TV_WS + STATIC <= LDS_CU and S3_ROW * S3_MAX + STATIC <= LDS_CU
    assert TV_ROW * TV_MAX == TV_ROWS_MAX and S3_ROW * (S3_MAX + STEP) + STATIC > LDS_CU      # each bound is the last step that fits its rule
    assert TV_WS == 64512


def test_two_view_plan_on_both_sides_of_every_boundary(ask):
    caps = [1, 63, 64, 65, 1000, 4095, 4096, 4097]
    got = dict(zip(caps, ask(["twoview %d" % c for c in caps])))
    for c in caps:
        assert got[c] == expect(TV_ROW, TV_WS, TV_MAX, c), (c, got[c])
    assert got[1][2] == "1"                                                   # the workspace alone passes 48 KB: every launch opts in
    assert got[1000][1] == "80512" and got[4096][1] == "130048"               # two waves per compute unit at 1000 rows, one at the bound
    assert got[4096][4] == got[4097][4] == "4096"                             # an entry point refuses cap > maxCap: 4096 is admitted, 4097 is not
    assert int(got[4096][1]) + STATIC <= LDS_CU


def test_sim3_plan_on_both_sides_of_every_boundary(ask):
    caps = [1, 1000, 1024, 1025, 1100, 1400, 3072, 3073]
    got = dict(zip(caps, ask(["sim3 %d" % c for c in caps])))
    for c in caps:
        assert got[c] == expect(S3_ROW, 0, S3_MAX, c), (c, got[c])
    assert got[1024][1:3] == ["49152", "0"] and got[1025][1:3] == ["49200", "1"]      # 48 KB exactly: no opt-in; one row more: opt-in
    assert got[1000][2] == "0" and got[1100][2] == got[1400][2] == got[3072][2] == "1"
    assert got[3072][1] == "147456" and got[3072][4] == got[3073][4] == "3072"      # an entry point refuses cap > maxCap: 3072 is admitted, 3073 is not
    assert int(got[3072][1]) + STATIC <= LDS_CU
