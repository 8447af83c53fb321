"""GPU parity of sslam_fuse_search_batch_dev: the candidate search of Fuse / SearchBySim3 for jobs (keyframe slot, block of queries) on one cap strided
device pool, enqueued on the caller's stream.  Every expectation is the CPU oracle's -- oracle.fuse_search job by job, through the helpers of
tests/fuse_batch_cases.py (their reach is shown in tests/test_fuse_batch_cases_cpu.py) -- and every comparison is exact; one test checks that the
library's single call agrees row for row.  Rows past every count hold random bytes, queries past a job's count included; the outputs hold a sentinel
before every call.

  test_ragged_pool             six slots of capacity 96 with counts 0 / 1 / 63 / 64 / 65 / 96 x jobs of 0 / 1 / 255 / 256 / 257 / 300 queries on one
                               descriptor block; keypoints without and with the chi-square gates, keylines
  test_against_the_single_call the same jobs through sslam_fuse_search on uploaded handles
  test_lane_loop_edges         a window of 1 / 63 / 64 / 65 / 129 admissible rows, the winner first, in the middle, last
  test_ties                    equal distances in two grid cells (the higher row in the earlier column wins), in one cell, between lines
  test_gates                   every gate on neighbouring floats, stereo and monocular rows in one keyframe, an octave outside the table, valid == 0,
                               a keypoint outside the grid, vertical and degenerate line queries
  test_jobs                    20 jobs on one slot and one descriptor block, jobs with blocks of their own, skipped jobs, njobs == 0, qcap == 0
  test_counts_are_clamped      keyframe counts of -3 and capacity + 5, query counts of -3 and qcap + 5
  test_null_uright             the chi-square gates on a monocular pool
  test_size_bound              capacities 3072 / 3073 (the dynamic-LDS opt-in) and 4096 / 4097 (the geometry leaves LDS), full slots
  test_streams_*               two calls back to back on a side stream; a call beside the synchronous single call
  test_argument_errors         SSLAM_ERR_INVALID leaves the outputs at the sentinel"""
import numpy as np
import pytest
import torch
import fuse_batch_cases as fc

pytestmark = pytest.mark.gpu

SENT = -77          # what the outputs hold before a call


def dev(a):
    """the array's bytes on the device (16 bytes at least: an empty array still has an address)"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(max(0, 16 - b.size), np.uint8)])).cuda()


class Call:
    """one call: device inputs (kept alive) and sentinel-filled outputs, made by the constructor; launch() enqueues it.  n / rows replace the keyframe
    counts / the job rows the case would give"""
    def __init__(self, c, cap, qcap, seed=99, n=None, rows=None, njobs=None, nqdesc=None, with_uright=True):
        rng = np.random.default_rng(seed)
        P = fc.pack_pool(rng, c, cap); Q = fc.pack_jobs(rng, c, qcap)
        self.c, self.cap, self.qcap, self.nk = c, cap, qcap, len(c["pool"])
        rows = Q["jobs"] if rows is None else rows
        self.njobs = len(rows) if njobs is None else njobs
        self.nqdesc = Q["nqdesc"] if nqdesc is None else nqdesc
        self.d = dict(feats=dev(P["feats"]), desc=dev(P["desc"]), uright=dev(P["uright"]) if with_uright else None, n=dev(P["n"] if n is None else np.asarray(n, np.int32)),
                      q=dev(np.concatenate([Q["q"], Q["q"][:1]])), qdesc=dev(np.concatenate([Q["qdesc"], np.zeros((1, 32), np.uint8)])),
                      jobs=dev(np.concatenate([rows, rows[:1]])))                  # one row more than the call may read
        out_rows = len(rows) + 1                                                   # one row more than the call may write
        self.bi = torch.full((out_rows, max(qcap, 1)), SENT, dtype=torch.int32, device="cuda"); self.bd = torch.full((out_rows, max(qcap, 1)), SENT, dtype=torch.int32, device="cuda")
        self.nf = torch.full((out_rows,), SENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()          # the buffers were filled on torch's stream

    def launch(self, ctx, stream=None, nlevels=None):
        c = self.c
        ctx.fuse_search_batch_dev(c["kind"], c["chi2"], self.d["feats"], self.d["desc"], self.d["n"], self.cap, self.nk, self.d["q"], self.qcap, self.d["qdesc"], self.nqdesc,
                                  self.d["jobs"], self.njobs, self.bi, self.bd, self.nf, d_uright=self.d["uright"], inv_level_sigma2=fc.INV_SIGMA2 if c["chi2"] else None,
                                  nlevels=nlevels, bounds=fc.BOUNDS, stream=stream)
        return self

    def results(self):
        """after a synchronise"""
        q = max(self.qcap, 1)
        return self.bi.cpu().numpy().reshape(-1, q), self.bd.cpu().numpy().reshape(-1, q), self.nf.cpu().numpy()


def check(got, want, njobs=None):
    """rows and count of job j against want[j] = (best_idx, best_dist), or None for a skipped job (-1, no row written); rows at or past a job's count and
    everything behind the last job keep the sentinel"""
    bi, bd, nf = got
    for j, w in enumerate(want):
        if w is None:
            assert nf[j] == -1 and (bi[j] == SENT).all() and (bd[j] == SENT).all(), j
            continue
        nq = len(w[0])
        np.testing.assert_array_equal(bi[j, :nq], w[0], err_msg="job %d" % j); np.testing.assert_array_equal(bd[j, :nq], w[1], err_msg="job %d" % j)
        assert nf[j] == (w[0] >= 0).sum(), (j, nf[j])
        assert (bi[j, nq:] == SENT).all() and (bd[j, nq:] == SENT).all(), j
    n = len(want) if njobs is None else njobs
    assert (bi[n:] == SENT).all() and (bd[n:] == SENT).all() and (nf[n:] == SENT).all()


def run(ctx, oracle, c, cap, qcap, want=None, **kw):
    want = fc.expect(oracle, c) if want is None else want
    call = Call(c, cap, qcap, **kw).launch(ctx)
    ctx.synchronize()
    got = call.results()
    check(got, want)
    return got, want


# ---- 1. the ragged pool
@pytest.fixture(scope="module")
def ragged(oracle):
    out = {}
    for kind, chi2 in fc.RAGGED_MODES:
        c = fc.ragged_pool(np.random.default_rng(8500 + 10 * kind + chi2), kind, chi2)
        out[(kind, chi2)] = (c, fc.expect(oracle, c))
    return out


@pytest.mark.parametrize("kind,chi2", fc.RAGGED_MODES)
def test_ragged_pool(ctx, oracle, ragged, kind, chi2):
    c, want = ragged[(kind, chi2)]
    got, _ = run(ctx, oracle, c, fc.RAGGED_CAP, fc.RAGGED_QCAP, want)
    assert got[2][:36].sum() > 500


@pytest.mark.parametrize("kind,chi2", fc.RAGGED_MODES)
def test_against_the_single_call(ctx, oracle, ragged, kind, chi2):
    c, want = ragged[(kind, chi2)]
    got, _ = run(ctx, oracle, c, fc.RAGGED_CAP, fc.RAGGED_QCAP, want)
    frames = {i: ctx.frame_upload(kind, k["feats"], k["desc"], k.get("uright"), bounds=fc.BOUNDS) for i, k in enumerate(c["pool"]) if len(k["feats"])}
    for j, jb in enumerate(c["jobs"]):
        nq = len(jb["q"])
        if jb["kf"] not in frames: continue
        bi, bd = frames[jb["kf"]].fuse_search(jb["q"], fc.job_desc(c, jb), chi2, fc.INV_SIGMA2 if chi2 else None)
        np.testing.assert_array_equal(bi, got[0][j, :nq], err_msg="job %d" % j); np.testing.assert_array_equal(bd, got[1][j, :nq], err_msg="job %d" % j)
    for f in frames.values(): f.close()


def merged(cases):
    """independent cases of one (kind, chi2) as ONE call: every case's slots, blocks and jobs behind the previous case's"""
    pool, blocks, jobs = [], [], []
    for c in cases:
        jobs += [fc.job(len(pool) + j["kf"], j["q"], len(blocks) + j["block"], j["off"]) for j in c["jobs"]]
        pool += c["pool"]; blocks += c["blocks"]
    return fc.case(cases[0]["kind"], cases[0]["chi2"], pool, blocks, jobs)


# ---- 2. the lane loop's edges
def test_lane_loop_edges(ctx, oracle):
    L = fc.lane_cases(np.random.default_rng(8400))
    got, want = run(ctx, oracle, merged([c for c, _ in L.values()]), 160, 3)
    for j, (name, (c, row)) in enumerate(L.items()):
        assert (got[0][j, 0], got[1][j, 0], got[2][j]) == (row, 5, 1), name


# ---- 3. ties
def test_ties(ctx, oracle):
    T = fc.tie_cases(np.random.default_rng(8410))
    for names in (("tie_two_cells", "tie_one_cell"), ("tie_lines",)):
        got, want = run(ctx, oracle, merged([T[n][0] for n in names]), 16, 2)
        for j, n in enumerate(names):
            assert (got[0][j, 0], got[1][j, 0]) == (T[n][1], 10), n


# ---- 4. gates
def test_gates(ctx, oracle):
    G = fc.point_gate_cases(np.random.default_rng(8420))
    for chi2 in (0, 1):
        c, names = fc.gates_as_case(G, 0, chi2)
        assert len(names) >= 8
        got, want = run(ctx, oracle, c, 8, 1)
        for j, n in enumerate(names):
            assert (got[0][j, 0], got[1][j, 0]) == ((2, 0) if G[n][3] else (-1, fc.INT_MAX)), n
    # every point gate case again under the chi-square gates it was not written for, whatever the oracle says
    run(ctx, oracle, dict(fc.gates_as_case(G, 0, 0)[0], chi2=1), 8, 1)
    c, winner, outside = fc.outside_grid_case(np.random.default_rng(8440))
    got, want = run(ctx, oracle, c, 8, 1)
    assert got[0][0, 0] == winner != outside and got[1][0, 0] == 12
    got, want = run(ctx, oracle, dict(c, chi2=1), 8, 1)          # 3 px off at a weight of 1: the chi-square gate leaves nothing, and still not the row outside the grid
    assert got[0][0, 0] == -1
    GL = fc.line_gate_cases(np.random.default_rng(8430))
    c, names = fc.gates_as_case(GL, 1, 0)
    got, want = run(ctx, oracle, c, 8, 1)
    for j, n in enumerate(names):
        if GL[n][3] is not None:
            assert (got[0][j, 0], got[1][j, 0]) == ((2, 0) if GL[n][3] else (-1, fc.INT_MAX)), n


# ---- 5. jobs
@pytest.fixture(scope="module")
def neighbours(oracle):
    c = fc.neighbours_case(np.random.default_rng(8450))
    return c, fc.expect(oracle, c)


def test_jobs(ctx, oracle, neighbours):
    c, want = neighbours
    got, _ = run(ctx, oracle, c, 96, 64, want)
    assert len(set(got[0][j].tobytes() for j in range(20))) == 20 and got[2][:22].min() > 20
    # skipped jobs between jobs that are computed: a slot out of range, a descriptor block that starts before or ends behind d_qdesc
    sel = (0, 1, 2, 3, 20, 21, 4, 5)
    picked = dict(c, jobs=[c["jobs"][k] for k in sel])
    rows = fc.pack_jobs(np.random.default_rng(1), picked, 64)["jobs"]
    nqdesc = 180
    assert rows["qdesc0"].tolist() == [0, 0, 0, 0, 60, 120, 0, 0] and (rows["nq"] == 60).all() and rows["qdesc0"][5] == nqdesc - 60          # job 21's block is the last that fits
    rows["kf"][1] = -1; rows["kf"][2] = 2; rows["qdesc0"][3] = -1; rows["qdesc0"][6] = nqdesc - 60 + 1; rows["kf"][7] = 1 << 30
    call = Call(picked, 96, 64, rows=rows).launch(ctx); ctx.synchronize()
    assert call.nqdesc == nqdesc and call.nk == 2
    check(call.results(), [want[0], None, None, None, want[20], want[21], None, None])
    # no job at all; no query capacity at all (d_nfound alone is written)
    call = Call(picked, 96, 64, rows=rows, njobs=0).launch(ctx); ctx.synchronize()
    check(call.results(), [], 0)
    empty = dict(c, jobs=[fc.job(j["kf"], j["q"][:0], j["block"]) for j in picked["jobs"]])
    rows0 = rows.copy(); rows0["nq"] = [0, 5, 0, 0, 0, -2, 0, 0]; rows0["qdesc0"][6] = nqdesc; rows0["qdesc0"][4] = nqdesc + 1
    call = Call(empty, 96, 0, rows=rows0, nqdesc=nqdesc).launch(ctx); ctx.synchronize()
    bi, bd, nf = call.results()
    assert nf[:8].tolist() == [0, -1, -1, -1, -1, 0, 0, -1] and nf[8] == SENT and (bi == SENT).all() and (bd == SENT).all()


def test_counts_are_clamped(ctx, oracle, ragged):
    c, _ = ragged[(0, 1)]
    full = c["pool"][0]; empty = fc.cut(full, 0)
    q = c["jobs"][5]["q"]
    assert len(full["feats"]) == fc.RAGGED_CAP and len(q) == fc.RAGGED_QCAP
    cap, qcap = fc.RAGGED_CAP, fc.RAGGED_QCAP
    cc = fc.case(0, 1, [full, full, full], c["blocks"], [fc.job(0, q, 0), fc.job(1, q, 0), fc.job(2, q, 0), fc.job(2, q, 0)])
    rows = fc.pack_jobs(np.random.default_rng(1), cc, qcap)["jobs"]
    rows["nq"] = [qcap, qcap, qcap + 5, -3]
    seen = fc.case(0, 1, [empty, full, full], c["blocks"], [fc.job(0, q, 0), fc.job(1, q, 0), fc.job(2, q, 0), fc.job(2, q[:0], 0)])
    want = fc.expect(oracle, seen)
    assert (want[0][0] == -1).all() and (want[1][0] >= 0).sum() > 100
    call = Call(cc, cap, qcap, n=[-3, cap + 5, cap], rows=rows).launch(ctx); ctx.synchronize()
    check(call.results(), want)


def test_null_uright(ctx, oracle, ragged):
    c, with_ur = ragged[(0, 1)]
    mono = dict(c, pool=[{k: v for k, v in kf.items() if k != "uright"} for kf in c["pool"]])
    got, want = run(ctx, oracle, mono, fc.RAGGED_CAP, fc.RAGGED_QCAP, with_uright=False)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(want, with_ur))          # the right coordinates of the pool did decide some gates


# ---- 6. the size bounds of the plan
@pytest.mark.parametrize("kind,chi2", [(0, 1), (1, 0)])
@pytest.mark.parametrize("cap", [fc.PLAIN_CAP, fc.PLAIN_CAP + 1, fc.LDS_CAP, fc.LDS_CAP + 1])
def test_size_bound(ctx, oracle, cap, kind, chi2):
    """16 * 3072 bytes is the last launch without the dynamic-LDS opt-in, 16 * 4096 = 64 KB the last capacity with the geometry in LDS.  One slot is full,
    one holds 200 rows"""
    assert fc.ROW_BYTES * fc.LDS_CAP <= fc.LDS_MAX < fc.ROW_BYTES * (fc.LDS_CAP + 1) and fc.ROW_BYTES * fc.PLAIN_CAP <= fc.LDS_DEFAULT < fc.ROW_BYTES * (fc.PLAIN_CAP + 1)
    c = fc.full_case(np.random.default_rng(8600 + cap + kind), kind, chi2, cap)
    got, want = run(ctx, oracle, c, cap, 300)
    assert got[2][0] > 150 and got[2][1] > 150 and got[0][0].max() > cap - 200


# ---- 7. streams
@pytest.fixture(scope="module")
def two_calls(oracle):
    A = fc.neighbours_case(np.random.default_rng(8460), njobs=6, n=100, nq=40)
    B = fc.neighbours_case(np.random.default_rng(8470), kind=1, chi2=0, njobs=4, n=120, nq=50)
    return dict(A=A, B=B, wantA=fc.expect(oracle, A), wantB=fc.expect(oracle, B))


def test_streams_back_to_back(ctx, two_calls):
    t = two_calls
    s = torch.cuda.Stream()
    c1 = Call(t["A"], 128, 40); c2 = Call(t["B"], 128, 50, seed=98)
    c1.launch(ctx, stream=s.cuda_stream); c2.launch(ctx, stream=s.cuda_stream)
    s.synchronize()
    check(c1.results(), t["wantA"]); check(c2.results(), t["wantB"])
    assert min((w[0] >= 0).sum() for w in t["wantA"] + t["wantB"]) > 10


def test_streams_batch_beside_the_synchronous_call(ctx, two_calls):
    t = two_calls
    s = torch.cuda.Stream()
    B = t["B"]; jb = B["jobs"][1]; k = B["pool"][jb["kf"]]
    f = ctx.frame_upload(1, k["feats"], k["desc"], None, bounds=fc.BOUNDS)
    c1 = Call(t["A"], 128, 40).launch(ctx, stream=s.cuda_stream)
    bi, bd = f.fuse_search(jb["q"], fc.job_desc(B, jb), 0)          # on the context stream
    s.synchronize()
    check(c1.results(), t["wantA"])
    np.testing.assert_array_equal(bi, t["wantB"][1][0]); np.testing.assert_array_equal(bd, t["wantB"][1][1])
    f.close()


# ---- 8. argument errors
def test_argument_errors(fe, ctx, oracle, neighbours):
    cs, want = neighbours
    c = Call(cs, 96, 64)
    base = dict(kind=0, chi2=1, feats=c.d["feats"], desc=c.d["desc"], n=c.d["n"], cap=96, nk=2, q=c.d["q"], qcap=64, qdesc=c.d["qdesc"], nqdesc=c.nqdesc, jobs=c.d["jobs"], njobs=22,
                bi=c.bi, bd=c.bd, nf=c.nf, uright=c.d["uright"], sg=fc.INV_SIGMA2, nlevels=None, bounds=fc.BOUNDS)

    def call(ok=False, **kw):
        a = dict(base, **kw)
        args = (a["kind"], a["chi2"], a["feats"], a["desc"], a["n"], a["cap"], a["nk"], a["q"], a["qcap"], a["qdesc"], a["nqdesc"], a["jobs"], a["njobs"], a["bi"], a["bd"], a["nf"])
        opt = dict(d_uright=a["uright"], inv_level_sigma2=a["sg"], nlevels=a["nlevels"], bounds=a["bounds"])
        if ok:
            return ctx.fuse_search_batch_dev(*args, **opt)
        with pytest.raises(fe.SslamError) as e:
            ctx.fuse_search_batch_dev(*args, **opt)
        assert e.value.code == fe.SSLAM_ERR_INVALID and "sslam_fuse_search_batch_dev" in str(e.value)
    for kind, chi2 in ((2, 0), (-1, 0), (0, 2), (0, -1), (1, 1)):
        call(kind=kind, chi2=chi2)
    call(sg=None, nlevels=8); call(nlevels=0); call(nlevels=65); call(nlevels=-1)
    for name in ("feats", "desc", "n", "q", "qdesc", "jobs", "bi", "bd", "nf", "bounds"):
        call(**{name: None})
    p_ = fe._p
    b = (fe.C.c_float * 4)(*fc.BOUNDS)
    assert fe.lib().sslam_fuse_search_batch_dev(None, 0, 1, p_(c.d["feats"]), p_(c.d["desc"]), p_(c.d["uright"]), p_(c.d["n"]), 96, 2, b, p_(fc.INV_SIGMA2), 8, p_(c.d["q"]), 64,
                                                p_(c.d["qdesc"]), c.nqdesc, p_(c.d["jobs"]), 22, p_(c.bi), p_(c.bd), p_(c.nf), None) == fe.SSLAM_ERR_INVALID      # no context
    for name in ("cap", "qcap", "nk", "njobs", "nqdesc"):
        call(**{name: -1})
    call(cap=1 << 19)
    call(qcap=1 << 16, njobs=1 << 15)                  # njobs * qcap = 2^31
    call(desc=c.d["desc"].data_ptr() + 8); call(qdesc=c.d["qdesc"].data_ptr() + 4)          # descriptor rows are read as 16-byte words
    for name in ("feats", "n", "q", "jobs", "bi", "bd", "nf", "uright"):
        call(**{name: base[name].data_ptr() + 2})
    ctx.synchronize(); torch.cuda.synchronize()
    bi, bd, nf = c.results()
    assert (bi == SENT).all() and (bd == SENT).all() and (nf == SENT).all()
    assert fe.FUSE_JOB_DTYPE.itemsize == 12 and fe.FUSE_JOB_DTYPE == fc.JOB_DTYPE
    call(ok=True); ctx.synchronize()                   # the same buffers are accepted once the arguments are valid
    check(c.results(), want)
    call(ok=True, sg=np.concatenate([fc.INV_SIGMA2, np.ones(56, np.float32)])); ctx.synchronize()          # the largest table; the keypoints' octaves stay below 8
    check(c.results(), want)
    call(ok=True, chi2=0, sg=None); ctx.synchronize()                                                    # no table is needed without the chi-square gates
    check(c.results(), fc.expect(oracle, dict(cs, chi2=0)))
