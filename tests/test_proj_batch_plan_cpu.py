"""The host-side plan of sslam_search_by_projection_batch_dev (csrc/match_plan.h: proj_batch_plan, proj_batch_slice, proj_batch_arena).  The header holds no
HIP: tests/sim/match_plan_dump.cpp compiles it with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program;
nothing is loaded into Python.  Every expected value is worked out here from the documented rule, never read back from the header:

  form        row capacity <= 8192: two kernels (candidates per (frame, query), one committing wave per frame); beyond: the one-wave kernel per frame
  commit LDS  8 bytes per row + 64 (occupancy and stamps); 64 per row only where the testing library asks for it and cap <= 2048;
              more than 48 KB needs the per-kernel opt-in
  scratch     per frame of a slice 8 (cap + qcap) + 8 K qcap + 4 qcap bytes, K = 8
  slice       as many frames as fit 256 MiB, at most 32768 (and the testing library's limit), at most nframes, at least 1"""
import pytest
import plan_dump

K = 8
SCRATCH_MAX = 256 << 20
MAX_SLICE = 32768
LDS_DEFAULT = 48 * 1024
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def ask():
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean (plan_dump.py)"""
    return plan_dump.asker("proj_batch")


def frame_bytes(cap, qcap):
    return 8 * (cap + qcap) + 8 * K * qcap + 4 * qcap


def expect_slice(cap, qcap, nframes, max_slice=0):
    s = min(SCRATCH_MAX // max(frame_bytes(cap, qcap), 1), MAX_SLICE)
    if max_slice > 0: s = min(s, max_slice)
    return max(1, min(s, nframes))


def expect_plan(cap, qcap, nframes, max_slice=0, feats=0):
    if cap > 8192:
        return ["one-wave", "0", "0", "0", "0", str(frame_bytes(cap, qcap)), str(expect_slice(cap, qcap, nframes, max_slice))]
    in_lds = 1 if feats and cap <= 2048 else 0
    lds = (64 if in_lds else 8) * cap + 64
    return ["two-kernel", str(in_lds), str(lds), str(int(lds > LDS_DEFAULT)), str(max(1, (qcap + 3) // 4)), str(frame_bytes(cap, qcap)),
            str(expect_slice(cap, qcap, nframes, max_slice))]


def test_constants(ask):
    assert ask(["consts"]) == [["2048", "8192", str(K), str(SCRATCH_MAX), str(MAX_SLICE), str(LDS_DEFAULT)]]


LAST_PLAIN_LDS = (LDS_DEFAULT - 64) // 8          # 6136: the last row capacity whose commit needs no opt-in
FIT_1000 = SCRATCH_MAX // frame_bytes(1000, 1000)  # frames of 1000 keypoints and 1000 queries per slice
CASES = [(8192, 1000, 4), (8193, 1000, 4), (8200, 437, 2), (2048, 1000, 4), (2049, 1000, 4), (2100, 300, 2), (LAST_PLAIN_LDS, 10, 4), (LAST_PLAIN_LDS + 1, 10, 4),
         (6200, 300, 2), (1000, 1000, 1024), (1000, 1000, 6144), (1000, 1000, 12288), (1000, 1000, FIT_1000), (1000, 1000, FIT_1000 + 1),
         (1000, 1000, 1), (1, 1, 1), (0, 0, 5), (0, 0, 100000), (16, 0, 100000), (400, 0, 3), (0, 7, 3), (50, 20, 40000), (1024, 0, 100000), (1025, 0, 100000), ((1 << 19) - 1, 1000, 9),
         ((1 << 19) - 1, 4000000, 9), (1000, 5, 3), (1000, 4, 3), (1000, 3, 3)]


def test_plan_on_both_sides_of_every_boundary(ask):
    assert 8 * LAST_PLAIN_LDS + 64 <= LDS_DEFAULT < 8 * (LAST_PLAIN_LDS + 1) + 64
    assert 1 < FIT_1000 < MAX_SLICE and frame_bytes(1000, 1000) == 84000
    r = ask(["plan %d %d %d" % c for c in CASES])
    got = dict(zip(CASES, r))
    for c in CASES:
        assert got[c] == expect_plan(*c), (c, got[c])
    # the form follows the row capacity alone
    assert got[(8192, 1000, 4)][0] == "two-kernel" and got[(8193, 1000, 4)][0] == "one-wave"
    # occupancy and stamps only, on both sides of the single call's features-in-LDS limit
    assert got[(2048, 1000, 4)][1:3] == ["0", str(8 * 2048 + 64)] and got[(2049, 1000, 4)][1:3] == ["0", str(8 * 2049 + 64)]
    # the dynamic-LDS opt-in
    assert got[(LAST_PLAIN_LDS, 10, 4)][3] == "0" and got[(LAST_PLAIN_LDS + 1, 10, 4)][3] == "1" and got[(8192, 1000, 4)][3] == "1"
    # the slice: by nframes, by the scratch bound, by the grid limit, and never below one frame
    assert got[(1000, 1000, 1024)][6] == "1024" and got[(1000, 1000, FIT_1000)][6] == str(FIT_1000) and got[(1000, 1000, FIT_1000 + 1)][6] == str(FIT_1000)
    assert got[(1000, 1000, 12288)][6] == str(FIT_1000)
    assert got[(0, 0, 100000)][6] == str(MAX_SLICE) and got[(16, 0, 100000)][6] == str(MAX_SLICE) and got[(50, 20, 40000)][6] == str(MAX_SLICE)
    assert frame_bytes(1024, 0) * MAX_SLICE == SCRATCH_MAX and got[(1024, 0, 100000)][6] == str(MAX_SLICE) and got[(1025, 0, 100000)][6] == str(SCRATCH_MAX // 8200)
    assert frame_bytes((1 << 19) - 1, 4000000) > SCRATCH_MAX and got[((1 << 19) - 1, 4000000, 9)][6] == "1"
    # the candidate grid: four queries per workgroup, never empty
    assert [got[(1000, q, 3)][4] for q in (5, 4, 3)] == ["2", "1", "1"] and got[(400, 0, 3)][4] == "1"


def test_commit_lds_fits(ask):
    caps = [0, 1, 600, 2048, 2049, LAST_PLAIN_LDS, LAST_PLAIN_LDS + 1, 8191, 8192]
    for feats in (0, 1):
        r = ask(["plan %d 100 8 0 %d" % (c, feats) for c in caps])
        for c, row in zip(caps, r):
            assert row == expect_plan(c, 100, 8, 0, feats), (c, feats, row)
            lds, opt_in = int(row[2]), int(row[3])
            assert lds <= LDS_CU - 1024                 # next to the kernel's static arrays (the rotation histogram)
            assert opt_in or lds <= LDS_DEFAULT < 64 * 1024
            assert int(row[1]) == (1 if feats and c <= 2048 else 0)


def test_testing_limit_lowers_the_slice_only(ask):
    r = ask(["plan 1000 1000 6144 0 0", "plan 1000 1000 6144 2 0", "plan 1000 1000 6144 100000 0", "plan 1000 1000 1 2 0", "plan 400 200 3 2 0", "plan 8200 40 3 2 0"])
    assert [x[6] for x in r] == [str(FIT_1000), "2", str(FIT_1000), "1", "2", "2"]
    assert r[0][:6] == r[1][:6] == r[2][:6]


@pytest.mark.parametrize("cap,qcap,max_slice", [(1000, 1000, 0), (400, 200, 2), (400, 200, 3), (8200, 40, 2), (2000, 500000, 0), (0, 0, 0), (50, 20, 1)])
def test_slices_cover_the_batch_once(ask, cap, qcap, max_slice):
    full = expect_slice(cap, qcap, 1 << 30, max_slice)          # the slice of a batch long enough not to limit it
    counts = sorted({1, max(full - 1, 1), full, full + 1, 3 * full + 2})
    rows = ask(["slices %d %d %d %d" % (cap, qcap, n, max_slice) for n in counts])
    plans = ask(["plan %d %d %d %d 0" % (cap, qcap, n, max_slice) for n in counts])
    bound = max(SCRATCH_MAX, frame_bytes(cap, qcap)) + 3 * 256
    for n, row, plan in zip(counts, rows, plans):
        slice_ = int(plan[6])
        assert slice_ == expect_slice(cap, qcap, n, max_slice) and 1 <= slice_ <= n
        pairs = [tuple(int(x) for x in t.split(":")) for t in row]
        nxt = 0
        for first, count in pairs:
            assert first == nxt and 1 <= count <= slice_
            nxt += count
        assert nxt == n and len(pairs) == -(-n // slice_)
        assert all(c == slice_ for _, c in pairs[:-1])
        # the arena of the slice: three blocks of `slice` rows each, 256-aligned, inside the bound the header states
        a = [int(x) for x in ask(["arena %d %d %d %d" % (cap, qcap, slice_, K)])[0]]
        al = lambda v: (v + 255) // 256 * 256
        blocks = [slice_ * 8 * (cap + qcap), slice_ * 8 * K * qcap, slice_ * 4 * qcap]
        assert a == [0, al(blocks[0]), al(blocks[0]) + al(blocks[1]), sum(al(b) for b in blocks)]
        assert sum(blocks) == slice_ * frame_bytes(cap, qcap) and a[3] <= bound


def test_single_frame_agrees_with_the_single_call(ask):
    """for one frame that fills its rows, the batch runs the kernel family the single call would (the commit's LDS layout is the batch's own)"""
    sizes = [(1, 1), (600, 300), (2048, 1000), (2049, 1000), (6200, 300), (8192, 1), (8193, 1), (8200, 40), (500000, 7)]
    single = ask(["single %d %d" % s for s in sizes])
    batch = ask(["plan %d %d 1" % s for s in sizes])
    for s, a, b in zip(sizes, single, batch):
        assert a[0] == b[0], (s, a, b)
        assert b[0] == ("two-kernel" if s[0] <= 8192 else "one-wave")
