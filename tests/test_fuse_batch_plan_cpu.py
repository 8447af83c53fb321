"""The host-side plan of sslam_fuse_search_batch_dev (csrc/match_plan.h: batch_plan at FUSE_BATCH_ROW_BYTES, fuse_batch_grid).  The header holds no HIP:
tests/sim/match_plan_dump.cpp compiles it with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program;
nothing is loaded into Python.  Every expected value is worked out here from the documented rule, never read back from the header:

  workgroup   8 waves of 64 lanes per (job, chunk of 256 queries); the grid is one-dimensional, njobs * ceil(qcap / 256) -- and njobs where qcap is 0,
              because chunk 0 of a job is the workgroup that reports a skipped job
  form        the keyframe's geometry in LDS -- four words per row of the capacity: x, y, uright, octave or pt_x, pt_y, angle, octave -- while
              16 * cap <= 64 KB; beyond that the same kernel on global memory, with no dynamic LDS
  opt-in      more than 48 KB of dynamic LDS needs the per-kernel opt-in"""
import pytest
import plan_dump
import fuse_batch_cases as fc

WAVES, ROW, CHUNK, LDS_MAX, LDS_DEFAULT, LDS_CU = 8, 16, 256, 64 * 1024, 48 * 1024, 160 * 1024


@pytest.fixture(scope="module")
def ask():
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean (plan_dump.py)"""
    return plan_dump.asker("fuse_batch")


def expect_plan(cap, qcap, njobs):
    lds = ROW * cap
    chunks = max(1, -(-qcap // CHUNK))
    form = ["lds", str(lds), str(int(lds > LDS_DEFAULT))] if lds <= LDS_MAX else ["global", "0", "0"]
    return form + [str(64 * WAVES), str(chunks), str(njobs * chunks)]


def test_constants(ask):
    assert ask(["consts"]) == [[str(WAVES), str(ROW), str(CHUNK), str(LDS_MAX), str(LDS_DEFAULT)]]
    assert (fc.W, fc.ROW_BYTES, fc.CHUNK, fc.LDS_MAX, fc.LDS_DEFAULT) == (WAVES, ROW, CHUNK, LDS_MAX, LDS_DEFAULT)          # what the case module and the GPU test assume
    assert ROW == 4 * 4


LAST_LDS = LDS_MAX // ROW                 # 4096
LAST_PLAIN = LDS_DEFAULT // ROW           # 3072: the last capacity without the opt-in
CAPS = [0, 1, LAST_PLAIN, LAST_PLAIN + 1, LAST_LDS, LAST_LDS + 1, (1 << 19) - 1]
QCAPS = [0, 1, 255, 256, 257]


def test_form_and_opt_in_on_both_sides_of_every_boundary(ask):
    assert (LAST_LDS, LAST_PLAIN) == (4096, 3072) == (fc.LDS_CAP, fc.PLAIN_CAP)
    assert ROW * LAST_LDS <= LDS_MAX < ROW * (LAST_LDS + 1) and ROW * LAST_PLAIN <= LDS_DEFAULT < ROW * (LAST_PLAIN + 1)
    cases = [(c, 300, 21) for c in CAPS] + [(1000, 1000, 21 * 1024)]
    got = dict(zip(cases, ask(["plan %d %d %d" % c for c in cases])))
    for c in cases:
        assert got[c] == expect_plan(*c), (c, got[c])
    form = {c[0]: got[c][:3] for c in cases}
    assert form[0] == ["lds", "0", "0"] and form[1] == ["lds", "16", "0"]
    assert form[LAST_PLAIN] == ["lds", str(48 * 1024), "0"] and form[LAST_PLAIN + 1] == ["lds", str(48 * 1024 + 16), "1"]
    assert form[LAST_LDS] == ["lds", str(64 * 1024), "1"] and form[LAST_LDS + 1] == ["global", "0", "0"] == form[(1 << 19) - 1]
    assert got[(1000, 1000, 21 * 1024)] == ["lds", "16000", "0", "512", "4", str(4 * 21 * 1024)]          # 1024 sessions of SearchInNeighbors


def test_grid_follows_the_jobs_and_the_query_capacity(ask):
    cases = [(1000, q, n) for q in QCAPS + [300, 1000, 1 << 20] for n in (0, 1, 21, 12288)]
    got = dict(zip(cases, ask(["plan %d %d %d" % c for c in cases])))
    for c in cases:
        assert got[c] == expect_plan(*c), (c, got[c])
    chunks = {q: int(got[(1000, q, 21)][4]) for q in QCAPS}
    assert chunks == {0: 1, 1: 1, 255: 1, 256: 1, 257: 2}          # a job always has its chunk 0
    assert got[(1000, 257, 21)][5] == "42" and got[(1000, 0, 21)][5] == "21" and got[(1000, 257, 0)][5] == "0"
    # the largest batch the entry point admits stays below 2^64 here and is refused there (2^31 workgroups and more)
    big = ask(["plan 1000 %d %d" % ((1 << 31) - 1, (1 << 31) - 1)])[0]
    assert int(big[5]) == ((1 << 31) - 1) * (1 << 23) and int(big[4]) == 1 << 23


def test_form_follows_the_capacity_alone(ask):
    for cap in CAPS + [1000]:
        rows = ask(["plan %d %d %d" % (cap, q, n) for q in (0, 1, 300, 5000) for n in (0, 1, 64, 12288)])
        assert len(set(tuple(r[:4]) for r in rows)) == 1, cap
    # and the grid follows njobs and qcap alone
    for q in QCAPS:
        rows = ask(["plan %d %d 7" % (cap, q) for cap in CAPS])
        assert len(set(tuple(r[4:]) for r in rows)) == 1, q


def test_lds_fits_a_compute_unit(ask):
    caps = [0, 1, 63, 64, 65, 1000, LAST_PLAIN, LAST_PLAIN + 1, LAST_LDS, LAST_LDS + 1, 5000, (1 << 19) - 1]
    for c, row in zip(caps, ask(["plan %d 300 9" % c for c in caps])):
        lds, opt_in = int(row[1]), int(row[2])
        assert lds <= LDS_MAX and 2 * (lds + 1024) <= LDS_CU          # two workgroups per compute unit beside the kernel's static arrays (level table, count)
        assert opt_in == int(lds > LDS_DEFAULT)
        assert int(row[3]) == 512 <= 1024 and row[5] == "18"
