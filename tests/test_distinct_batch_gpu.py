"""GPU parity of sslam_distinctive_descriptors_batch_dev: MapPoint / MapLine::ComputeDistinctiveDescriptors for observation sets that name rows of one cap
strided device pool, enqueued on the caller's stream.  Every expectation is tests/distinct_batch_cases.py's expect() -- the admissible entries in entry
order through oracle.distinctive; the reach of the inputs is shown in tests/test_distinct_batch_cases_cpu.py -- and every comparison is exact.  The pool
(capacity 37, 40 slots) lies between two guard slots and holds the poison in every row that must not be read; the outputs hold a sentinel before a call.

  test_named_sets                 one call: admissible N of 0 .. 1024 on both sides of every class bound, the tie, skip, k and count cases, a set of 1025
                                  entries; d_best, d_median and the table against expect(), the stated winners, and row for row against the single call
  test_malformed_ranges           decreasing, negative start, end beyond nobs: -2 with the neighbours as they were
  test_packing                    runs of eight sets of sizes (0, 8, 1, 9, 7, 64, 2, 65) and the rotations; nsets of 1, 7 and 9
  test_grid_cap                   32 * the grid cap + 19 small sets: the waves' stride loop (the cap counts workgroups of 32 sets)
  test_table                      d_out_row NULL with a short table, a permutation, rows outside [0, nout); no table; no d_median
  test_chain                      the table as d_qdesc of fuse_search_batch_dev against the host-gathered descriptors
  test_argument_errors            SSLAM_ERR_INVALID leaves the outputs at the sentinel; nsets == 0 writes nothing
  test_side_stream                two calls back to back on a torch stream
  test_profile_names_both_kernels the launches the plan states, with and without a large set"""
import ctypes as C
import numpy as np
import pytest
import torch
import distinct_batch_cases as dc
import fuse_batch_cases as fc

pytestmark = pytest.mark.gpu

SENT = -77          # what d_best / d_median hold before a call
FILL = 0xEE         # what the table holds before a call


def dev(a):
    """the array's bytes on the device (16 bytes at least: an empty array still has an address)"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(max(0, 16 - b.size), np.uint8)])).cuda()


class Call:
    """one call: device inputs (kept alive) and sentinel-filled outputs, made by the constructor; launch() enqueues it.  The descriptor pointer is the first
    slot behind the front guard; one entry more than nobs, one result more than nsets and one table row more than nout exist and must stay as they were"""
    def __init__(self, pool, o, ptr, nobs=None, nsets=None, out_row=None, nout=None, table=True, median=True):
        self.pool, self.o, self.ptr = pool, o, np.asarray(ptr, np.int32)
        self.cap = pool["raw"].shape[1]; self.nk = len(pool["n"])
        self.nobs = len(o) if nobs is None else nobs
        self.nsets = len(ptr) - 1 if nsets is None else nsets
        self.nout = (len(ptr) - 1 if nout is None else nout) if table else 0
        self.out_row = None if out_row is None else np.asarray(out_row, np.int32)
        self.d = dict(raw=dev(pool["raw"]), n=dev(pool["n"]), bad=dev(pool["bad"]), obs=dev(np.concatenate([o, dc.obs([(0, 0)])])), ptr=dev(self.ptr),
                      out_row=None if out_row is None else dev(self.out_row))
        self.desc = self.d["raw"].data_ptr() + 32 * self.cap
        self.best = torch.full((len(ptr),), SENT, dtype=torch.int32, device="cuda")
        self.median = torch.full((len(ptr),), SENT, dtype=torch.int32, device="cuda") if median else None
        self.table = torch.full((self.nout + 1, 32), FILL, dtype=torch.uint8, device="cuda") if table else None
        torch.cuda.synchronize()          # the buffers were filled on torch's stream

    def launch(self, ctx, stream=None):
        ctx.distinctive_descriptors_batch_dev(self.desc, self.d["n"], self.cap, self.nk, self.d["obs"], self.nobs, self.d["ptr"], self.nsets, self.best, d_median=self.median,
                                              d_kf_bad=self.d["bad"], d_out_desc=self.table, d_out_row=self.d["out_row"], nout=self.nout, stream=stream)
        return self

    def check(self, oracle, want=None):
        """after a synchronise: d_best, d_median and the table against expect(); everything behind nsets / nout and every row no set names as it was"""
        best, med, chosen = dc.expect(oracle, self.pool, self.o, self.ptr[:self.nsets + 1], self.nobs) if want is None else want
        ns = self.nsets
        got = self.best.cpu().numpy()
        np.testing.assert_array_equal(got[:ns], best); assert (got[ns:] == SENT).all()
        if self.median is not None:
            gm = self.median.cpu().numpy()
            np.testing.assert_array_equal(gm[:ns], med); assert (gm[ns:] == SENT).all()
        if self.table is not None:
            t = self.table.cpu().numpy()
            target = np.arange(ns) if self.out_row is None else self.out_row[:ns].astype(np.int64)
            hit = (best >= 0) & (target >= 0) & (target < self.nout)
            assert len(np.unique(target[hit])) == hit.sum()          # the cases here name a row once
            exp = np.full_like(t, FILL); exp[target[hit]] = chosen[hit]
            np.testing.assert_array_equal(t, exp)
        return best, med, chosen


@pytest.fixture(scope="module")
def pool():
    return dc.make_pool(np.random.default_rng(9100))


# ---- 1. sizes, ties, skips, k, counts, one refusal: one call
@pytest.fixture(scope="module")
def named(oracle, pool):
    rng = np.random.default_rng(9300)
    sets, names = [], []
    def add(name, s): names.append(name); sets.append(s)
    for m, s in zip(dc.SIZES + ("all_skipped",), dc.size_sets(rng, pool)): add("size_%s" % m, s)
    T = dc.tie_sets(rng, pool); S = dc.skip_sets(rng, pool); K = dc.k_sets(rng, pool); Cn = dc.count_sets(rng, pool)
    for n, (s, _) in T.items(): add("tie_" + n, s)
    for n, (s, _) in S.items(): add("skip_" + n, s)
    for n, s in list(K.items()) + list(Cn.items()): add(n, s)
    add("refused_1025", dc.random_entries(rng, pool, dc.LARGE_MAX + 1))
    add("behind_the_refusal", dc.random_entries(rng, pool, 5))
    o, ptr = dc.pack(sets)
    return dict(names=names, sets=sets, o=o, ptr=ptr, T=T, S=S, want=dc.expect(oracle, pool, o, ptr))


def test_named_sets(ctx, oracle, pool, named):
    c = Call(pool, named["o"], named["ptr"]).launch(ctx); ctx.synchronize()
    best, med, chosen = c.check(oracle, named["want"])
    at = {n: i for i, n in enumerate(named["names"])}
    assert [best[at["size_%d" % m]] >= 0 for m in dc.SIZES] == [m > 0 for m in dc.SIZES] and best[at["size_all_skipped"]] == -1
    for n, (_, w) in named["T"].items(): assert best[at["tie_" + n]] == w, n
    for n, (_, p) in named["S"].items(): assert best[at["skip_" + n]] not in (-1, -2, p), n
    assert best[at["refused_1025"]] == -2 and med[at["refused_1025"]] == dc.INT_MAX and best[at["behind_the_refusal"]] >= 0
    # row for row against the single call on the rows a caller would gather on the host
    rows, ptr2, off_a, ok = dc.gather(pool, named["o"], named["ptr"])
    single = ctx.distinctive_descriptors(rows, ptr2)
    has = best >= 0
    assert ((single >= 0) == has).all()
    np.testing.assert_array_equal(off_a[(ptr2[:-1] + single)[has]], best[has])


# ---- 2. malformed ranges
def test_malformed_ranges(ctx, oracle, pool):
    rng = np.random.default_rng(9310)
    sets = [dc.random_entries(rng, pool, m) for m in (5, 12, 4, 6, 70, 3, 9, 7)]
    o, ptr = dc.pack(sets)
    good = dc.expect(oracle, pool, o, ptr)[0]
    bad = ptr.copy()
    bad[0] = -1                     # set 0 starts below 0
    bad[3] = bad[2] - 2             # set 2 decreases; set 3 starts earlier than packed and is a range like any other
    c = Call(pool, o, bad, nobs=len(o) - 1).launch(ctx); ctx.synchronize()          # and set 7 ends beyond nobs
    best, _, _ = c.check(oracle)
    assert best[[0, 2, 7]].tolist() == [-2, -2, -2] and (best[[1, 4, 5, 6]] == good[[1, 4, 5, 6]]).all() and best[3] >= 0


# ---- 3. packing
def test_packing(ctx, oracle, pool):
    sets = dc.packing_sets(np.random.default_rng(9170), pool)
    o, ptr = dc.pack(sets)
    c = Call(pool, o, ptr).launch(ctx); ctx.synchronize()
    best, _, _ = c.check(oracle)
    assert ((best >= 0) == (np.diff(ptr) > 0)).all()
    for first, ns in ((3, 1), (5, 1), (7, 1), (1, 7), (8, 9), (59, 5)):          # one medium, one large, one small set; seven; nine; the last five
        o, ptr = dc.pack(sets[first:first + ns])
        c = Call(pool, o, ptr).launch(ctx); ctx.synchronize()
        c.check(oracle)
    # fewer sets than d_ptr describes: the rest is not touched
    o, ptr = dc.pack(sets[:20])
    c = Call(pool, o, ptr, nsets=9, nout=9).launch(ctx); ctx.synchronize()
    c.check(oracle)


def test_grid_cap(ctx, oracle, pool):
    ns = 32 * dc.GRID_MAX + 19
    assert dc.SETS_PER_WAVE * dc.WAVES == 32
    o, ptr = dc.many_small_sets(np.random.default_rng(9180), pool, ns)
    c = Call(pool, o, ptr).launch(ctx); ctx.synchronize()
    best, _, _ = c.check(oracle)
    assert (best[-19:] >= 0).all() and (best[-19:] > 0).any() and (best[32 * dc.GRID_MAX - 40:32 * dc.GRID_MAX] > 0).any()


# ---- 4. the descriptor table
def test_table(ctx, oracle, pool, named):
    o, ptr, want = named["o"], named["ptr"], named["want"]
    ns = len(ptr) - 1
    assert (want[0] == -1).sum() >= 2 and (want[0] == -2).sum() == 1
    c = Call(pool, o, ptr, nout=ns - 7).launch(ctx); ctx.synchronize(); c.check(oracle, want)          # d_out_row NULL: row s, the last seven outside the table
    rng = np.random.default_rng(9320)
    perm = rng.permutation(ns).astype(np.int32)
    c = Call(pool, o, ptr, out_row=perm).launch(ctx); ctx.synchronize(); c.check(oracle, want)
    rows = rng.permutation(ns + 3)[:ns].astype(np.int32); rows[::5] = -1; rows[1::5] = ns + 40; rows[2::5] = ns + 3          # a table of ns + 3 rows; rows below 0, far behind it, the first behind it
    c = Call(pool, o, ptr, out_row=rows, nout=ns + 3).launch(ctx); ctx.synchronize(); c.check(oracle, want)
    c = Call(pool, o, ptr, table=False).launch(ctx); ctx.synchronize(); c.check(oracle, want)
    c = Call(pool, o, ptr, median=False).launch(ctx); ctx.synchronize(); c.check(oracle, want)
    c = Call(pool, o, ptr, table=False, median=False).launch(ctx); ctx.synchronize(); c.check(oracle, want)


# ---- 5. the table is the next fusion's d_qdesc
def test_chain(ctx, oracle):
    rng = np.random.default_rng(9330)
    fcase = fc.neighbours_case(np.random.default_rng(8460), njobs=6, n=100, nq=40)
    P = fc.pack_pool(rng, fcase, 128); Q = fc.pack_jobs(rng, fcase, 40)
    nqd = Q["nqdesc"]
    # map point t was observed 1 .. 12 times: noisy copies of the fuse case's query descriptor t, spread over 12 keyframe slots
    sizes = rng.integers(1, 13, nqd)
    nk, cap = 12, int(-(-sizes.sum() // 12)) + 3
    desc = rng.integers(0, 256, (nk, cap, 32), dtype=np.uint8)
    o = np.zeros(int(sizes.sum()), dc.OBS_DTYPE)
    o["kf"] = np.arange(len(o)) % nk; o["row"] = np.arange(len(o)) // nk
    desc[o["kf"], o["row"]] = np.repeat(Q["qdesc"], sizes, axis=0) ^ np.packbits(rng.random((len(o), 256)) < 0.04, axis=1)
    pool = dc.plain_pool(desc)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    c = Call(pool, o, ptr).launch(ctx)                  # on the context stream, and so is the fusion behind it
    d = dict(feats=dev(P["feats"]), desc=dev(P["desc"]), uright=dev(P["uright"]), n=dev(P["n"]), q=dev(Q["q"]), jobs=dev(Q["jobs"]))
    nj = len(Q["jobs"])
    outs = []
    for qdesc in (c.table, None):
        if qdesc is None:
            ctx.synchronize()
            best, _, chosen = c.check(oracle)
            assert (best >= 0).all() and (best > 0).any()
            qdesc = dev(chosen)                         # what the host would have gathered and uploaded
        bi = torch.full((nj, 40), SENT, dtype=torch.int32, device="cuda"); bd = torch.full((nj, 40), SENT, dtype=torch.int32, device="cuda")
        nf = torch.full((nj,), SENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.fuse_search_batch_dev(0, 1, d["feats"], d["desc"], d["n"], 128, len(fcase["pool"]), d["q"], 40, qdesc, nqd, d["jobs"], nj, bi, bd, nf, d_uright=d["uright"],
                                  inv_level_sigma2=fc.INV_SIGMA2, bounds=fc.BOUNDS)
        ctx.synchronize()
        outs.append((bi.cpu().numpy(), bd.cpu().numpy(), nf.cpu().numpy()))
    for a, b in zip(*outs): np.testing.assert_array_equal(a, b)
    assert outs[0][2].min() > 10 and (outs[0][1][outs[0][0] >= 0] < 60).mean() > 0.5          # the chosen descriptors do find their features


# ---- 6. the call
def test_argument_errors(fe, ctx, oracle, pool, named):
    o, ptr, want = named["o"], named["ptr"], named["want"]
    c = Call(pool, o, ptr, out_row=np.arange(len(ptr) - 1))
    base = dict(desc=c.desc, n=c.d["n"], cap=c.cap, nk=c.nk, bad=c.d["bad"], obs=c.d["obs"], nobs=c.nobs, ptr=c.d["ptr"], nsets=c.nsets, best=c.best, median=c.median,
                table=c.table, out_row=c.d["out_row"], nout=c.nout)

    def call(ok=False, **kw):
        a = dict(base, **kw)
        args = (a["desc"], a["n"], a["cap"], a["nk"], a["obs"], a["nobs"], a["ptr"], a["nsets"], a["best"])
        opt = dict(d_median=a["median"], d_kf_bad=a["bad"], d_out_desc=a["table"], d_out_row=a["out_row"], nout=a["nout"])
        if ok:
            return ctx.distinctive_descriptors_batch_dev(*args, **opt)
        with pytest.raises(fe.SslamError) as e:
            ctx.distinctive_descriptors_batch_dev(*args, **opt)
        assert e.value.code == fe.SSLAM_ERR_INVALID and "sslam_distinctive_descriptors_batch_dev" in str(e.value)
    for name in ("desc", "n", "ptr", "best", "obs"):
        call(**{name: None})
    call(table=None)                                   # d_out_row without d_out_desc
    p_ = fe._p
    assert fe.lib().sslam_distinctive_descriptors_batch_dev(None, p_(c.desc), p_(c.d["n"]), c.cap, c.nk, p_(c.d["bad"]), p_(c.d["obs"]), c.nobs, p_(c.d["ptr"]), c.nsets, p_(c.best),
                                                            p_(c.median), p_(c.table), p_(c.d["out_row"]), c.nout, None) == fe.SSLAM_ERR_INVALID      # no context
    for name in ("cap", "nk", "nobs", "nsets", "nout"):
        call(**{name: -1})
    call(cap=1 << 19)
    call(cap=1 << 16, nk=1 << 15)                      # nkeyframes * cap = 2^31
    call(desc=c.desc + 8); call(table=c.table.data_ptr() + 4)          # descriptor rows are read and written as 16-byte words
    for name in ("n", "obs", "ptr", "best", "median", "out_row"):
        call(**{name: base[name].data_ptr() + 2})
    call(ok=True, nsets=0)                              # no set: SSLAM_OK, nothing enqueued
    ctx.synchronize(); torch.cuda.synchronize()
    assert (c.best.cpu().numpy() == SENT).all() and (c.median.cpu().numpy() == SENT).all() and (c.table.cpu().numpy() == FILL).all()
    assert fe.OBS_DTYPE.itemsize == 8 and fe.OBS_DTYPE == dc.OBS_DTYPE
    call(ok=True); ctx.synchronize()                   # the same buffers are accepted once the arguments are valid
    c.check(oracle, want)
    call(ok=True, obs=None, nobs=0, bad=None); ctx.synchronize()          # no observation at all: the empty set at 0 is -1, every other range ends beyond nobs
    got = c.best.cpu().numpy()[:c.nsets]
    assert ptr[1] == 0 and ptr[2] > 0 and got[0] == -1 and (got[1:] == -2).all()


def test_side_stream(ctx, oracle, pool, named):
    s = torch.cuda.Stream()
    sets = dc.packing_sets(np.random.default_rng(9171), pool)
    o, ptr = dc.pack(sets)
    c1 = Call(pool, named["o"], named["ptr"]); c2 = Call(pool, o, ptr)
    c1.launch(ctx, stream=s.cuda_stream); c2.launch(ctx, stream=s.cuda_stream)
    s.synchronize()
    c1.check(oracle, named["want"]); c2.check(oracle)


def test_profile_names_both_kernels(fe, ctx, oracle, pool, named):
    """the host never reads d_ptr, so the plan launches both kernels whatever the sets are: distinct_batch_plan(nsets).launches == 2"""
    def drain():
        names = (C.c_char_p * 16)(); ms = (C.c_double * 16)(); cnt = (C.c_int * 16)()
        n = fe.lib().sslam_profile_drain(ctx.h, names, ms, cnt, 16)
        return {names[i].decode(): cnt[i] for i in range(n)}
    o, ptr = dc.many_small_sets(np.random.default_rng(9181), pool, 100)
    small = Call(pool, o, ptr); mixed = Call(pool, named["o"], named["ptr"])
    assert np.diff(ptr).max() <= dc.SMALL_MAX < dc.MEDIUM_MAX < np.diff(named["ptr"]).max()
    ctx.synchronize()
    assert fe.lib().sslam_profile_enable(ctx.h, 1) == 0
    try:
        mixed.launch(ctx); ctx.synchronize()
        assert drain() == {"k_distinct_batch": 1, "k_distinct_large": 1}
        small.launch(ctx); ctx.synchronize()
        assert drain() == {"k_distinct_batch": 1, "k_distinct_large": 1}
    finally:
        fe.lib().sslam_profile_enable(ctx.h, 0)
    mixed.check(oracle, named["want"]); small.check(oracle)
