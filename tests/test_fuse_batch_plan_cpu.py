"""The host-side plan of sslam_fuse_search_batch_dev (csrc/match_plan.h: fuse_batch_plan).  The header holds no HIP:
tests/sim/fuse_batch_plan_dump.cpp compiles it with plain g++, once as it is and once with -fsanitize=address,undefined, as a stand-alone program;
nothing is loaded into Python.  Every expected value is worked out here from the documented rule, never read back from the header:

  workgroup   8 waves of 64 lanes per (job, chunk of 256 queries); the grid is one-dimensional, njobs * ceil(qcap / 256) -- and njobs where qcap is 0,
              because chunk 0 of a job is the workgroup that reports a skipped job
  form        the keyframe's geometry in LDS -- four words per row of the capacity: x, y, uright, octave or pt_x, pt_y, angle, octave -- while
              16 * cap <= 64 KB; beyond that the same kernel on global memory, with no dynamic LDS
  opt-in      more than 48 KB of dynamic LDS needs the per-kernel opt-in"""
import os, subprocess
import pytest
import fuse_batch_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
WAVES, ROW, CHUNK, LDS_MAX, LDS_DEFAULT, LDS_CU = 8, 16, 256, 64 * 1024, 48 * 1024, 160 * 1024


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean"""
    d = tmp_path_factory.mktemp("fuse_batch_plan")
    src = os.path.join(HERE, "sim", "fuse_batch_plan_dump.cpp")
    plain, san = str(d / "fuse_batch_plan_dump"), str(d / "fuse_batch_plan_dump_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", san])

    def run(lines):
        text = "\n".join(lines) + "\n"
        outs = []
        for exe in (plain, san):
            r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr)
            outs.append(r.stdout)
        assert outs[0] == outs[1]
        rows = [l.split() for l in outs[0].splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


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
