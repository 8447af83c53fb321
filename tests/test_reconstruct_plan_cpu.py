"""reconstruct_plan (csrc/match_plan.h) and the argument rules of sslam_two_view_reconstruct* (csrc/match_check.h) through tests/sim/reconstruct_plan_dump.cpp, built plain and
under -fsanitize=address,undefined as stand-alone programs (tests/host_sim.py): the LDS layout and its size on both sides of the 48 KB opt-in and of the cap / lcap bounds, and
every rule on both sides."""
import os
import numpy as np
import host_sim

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim", "reconstruct_plan_dump.cpp")
WS = 8 * 26 * 128          # the 4 x 4 Jacobi workspace of 128 lanes


def ask(lines):
    return [[int(x) for x in l.split()] for l in host_sim.run(SRC, "\n".join(lines) + "\n").splitlines()]


def test_plan_layout_and_bounds():
    shapes = [(1, 0), (1, 1), (1073, 0), (1074, 0), (1000, 100), (2048, 1024), (4096, 1024), (5120, 1024), (5121, 1025)]
    for (cap, lcap), p in zip(shapes, ask(["plan %d %d" % s for s in shapes])):
        row, lrow, ws, line, rows, key, flag, lds, optin, threads, maxcap, maxlcap = p
        assert (row, lrow, threads, maxcap, maxlcap) == (21, 16, 128, 5120, 1024)
        assert (ws, line, rows, key, flag) == (0, WS, WS + 16 * lcap, WS + 16 * lcap + 16 * cap, WS + 16 * lcap + 20 * cap)
        assert lds == (flag + cap + 15) // 16 * 16 and rows % 16 == 0 and key % 4 == 0 and line % 8 == 0
        assert optin == (1 if lds > 48 * 1024 else 0)
    # both sides of the opt-in: 26 624 + 21 * cap crosses 49 152 between cap 1072 and 1074
    a, b = ask(["plan 1072 0", "plan 1074 0"])
    assert a[8] == 0 and b[8] == 1
    # the bounds fit the compute unit's 160 KB beside 2 KB of static words; one step of 1024 rows more does not
    top = ask(["plan 5120 1024", "plan 6144 1024"])
    assert top[0][7] + 2048 <= 160 * 1024 < top[1][7] + 2048


def test_argument_rules():
    bits = lambda f: int(np.float32(f).view(np.uint32))
    q = ["params %d 50" % bits(1.0), "params %d 0" % bits(1e-30), "params %d 50" % bits(0.0), "params %d 50" % bits(-1.0), "params %d 50" % bits(np.nan),
         "params %d -1" % bits(1.0)]
    assert [r[0] for r in ask(q)] == [1, 1, 0, 0, 0, 0]
    q = ["sizes 1 1 0", "sizes 0 1 0", "sizes 1 0 0", "sizes 1 1 -1", "sizes 419430 5120 0", "sizes 419431 5120 0", "sizes 2097151 1024 1024", "sizes 2097152 1000 1024"]
    assert [r[0] for r in ask(q)] == [1, 0, 0, 0, 1, 0, 1, 0]
    none, full = [0] * 11, [1] * 11
    q = ["lines %s 0" % " ".join(map(str, none)), "lines %s 7" % " ".join(map(str, none)), "lines %s 1" % " ".join(map(str, full)), "lines %s 0" % " ".join(map(str, full))]
    want = [0, 0, 1, -1]
    for k in range(11):
        part = list(full); part[k] = 0
        q.append("lines %s 4" % " ".join(map(str, part))); want.append(-1)
        one = list(none); one[k] = 1
        q.append("lines %s 4" % " ".join(map(str, one))); want.append(-1)
    assert [r[0] for r in ask(q)] == want
