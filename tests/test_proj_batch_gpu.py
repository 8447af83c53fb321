"""GPU parity of sslam_search_by_projection_batch_dev: the projection-window matcher for B frames in cap / qcap strided device buffers, enqueued
on the caller's stream.  Every expectation is the CPU oracle's (oracle.search_by_projection on each frame's slices); one assertion in the parity
test checks that the library's single call agrees too.  Inputs are tests/match_cases.py::cluster_case frames at small sizes: their clusters
exhaust the per-query top-8 list, so the ordered commit re-scans in every ordinary frame.  Unused rows of every input hold random bytes, the
outputs a sentinel.

  test_ragged_batch              five frames of different counts (n == cap, nq == qcap, 65 ordinary queries, n == 1), all four (kind, mode) pairs,
                                 with / without uright and occupied
  test_degenerate_frames         n = 0, nq = 0, both, all queries invalid, all features occupied, counts of -3 and capacity + 7; B = 1; nframes = 0
  test_state_does_not_leak       equal features under query angles 90 degrees apart, equal queries on other features (rotation histogram per frame)
  test_size_boundaries           row capacities 6136 / 6200 (commit LDS beyond 48 KB) and 8192 / 8200 (the one-wave kernel per frame), counts at and
                                 well below the capacity
  test_slice_boundary            a batch of five frames in slices of two (testing library), both forms
  test_streams_*                 back-to-back calls on one side stream, a batch beside the synchronous call, two side streams of one context
  test_argument_errors           SSLAM_ERR_INVALID leaves the outputs alone
  test_frontend_batch            FrontendBatch.search_by_projection on extracted frames, points and lines"""
import os
import numpy as np
import pytest
import torch
import pkg
import match_cases as mc
from oracle_lib import KP_DTYPE, KL_DTYPE
from synth import synth_frame

pytestmark = pytest.mark.gpu

SENT = -77          # what the outputs hold before a call


def params(kind, mode):
    """(nnratio, th_dist, check_orientation): the reference's values; the rotation check where the call accepts it (keypoints, mode 1)"""
    ratio, th, _ = mc.proj_params(kind, mode)
    return ratio, th, kind == 0 and mode == 1


def frame(seed, n, kind, C_, nq_extra, take_n=None, ordinary_only=False):
    """one frame of the batch: a cluster_case, optionally cut to its first take_n features or to its ordinary (non-cluster) queries"""
    c = mc.cluster_case(np.random.default_rng(seed), n, kind, C=C_, nq_extra=nq_extra)
    f = dict(feats=c["feats"], desc=c["desc"], occ=c["occ"], uright=c["uright"], q=c["q"], qdesc=c["qdesc"], case=c, whole=True)
    if take_n is not None:
        for k in ("feats", "desc", "occ", "uright"):
            if f[k] is not None: f[k] = f[k][:take_n].copy()
        f["whole"] = False
    if ordinary_only:
        ext = np.setdiff1d(np.arange(len(c["q"])), c["cquery"].ravel())
        f["q"] = c["q"][ext].copy(); f["qdesc"] = c["qdesc"][ext].copy(); f["whole"] = False
    return f


def junk(rng, shape, dtype):
    dt = np.dtype(dtype)
    return rng.integers(0, 256, size=int(np.prod(shape)) * dt.itemsize, dtype=np.uint8).view(dt).reshape(shape)


def pack(frames, kind, cap, qcap, seed=99):
    """the batch buffers (numpy) of `frames`: rows past a frame's counts are random bytes"""
    rng = np.random.default_rng(seed)
    B = len(frames)
    P = dict(feats=junk(rng, (B, cap), KP_DTYPE if kind == 0 else KL_DTYPE), desc=junk(rng, (B, cap, 32), np.uint8), uright=junk(rng, (B, cap), np.float32),
             occ=junk(rng, (B, cap), np.uint8), q=junk(rng, (B, qcap), mc.PQ_DTYPE), qdesc=junk(rng, (B, qcap, 32), np.uint8),
             n=np.zeros(B, np.int32), nq=np.zeros(B, np.int32))
    for i, f in enumerate(frames):
        n, nq = len(f["feats"]), len(f["q"])
        assert n <= cap and nq <= qcap, (i, n, cap, nq, qcap)
        P["feats"][i, :n] = f["feats"]; P["desc"][i, :n] = f["desc"]; P["occ"][i, :n] = f["occ"]
        if f["uright"] is not None: P["uright"][i, :n] = f["uright"]
        P["q"][i, :nq] = f["q"]; P["qdesc"][i, :nq] = f["qdesc"]
        P["n"][i] = n; P["nq"][i] = nq
    return P


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Call:
    """one batch call: device inputs (kept alive) and sentinel-filled outputs, made by the constructor; launch() enqueues it"""
    def __init__(self, P, kind, mode, cap, qcap, with_ur=False, with_occ=True, nframes=None, n=None, nq=None):
        self.B = len(P["n"]) if nframes is None else nframes
        self.kind, self.mode, self.cap, self.qcap, self.with_ur, self.with_occ = kind, mode, cap, qcap, with_ur, with_occ
        self.d = {k: dev(P[k]) for k in ("feats", "desc", "uright", "occ", "q", "qdesc")}
        self.d["n"] = dev(P["n"] if n is None else np.asarray(n, np.int32)); self.d["nq"] = dev(P["nq"] if nq is None else np.asarray(nq, np.int32))
        self.assigned = torch.full((len(P["n"]), cap), SENT, dtype=torch.int32, device="cuda")
        self.nm = torch.full((len(P["n"]),), SENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()          # the buffers were filled on torch's stream

    def launch(self, ctx, stream=None):
        ratio, th, ori = params(self.kind, self.mode)
        ctx.search_by_projection_batch_dev(self.kind, self.mode, self.d["feats"], self.d["desc"], self.d["n"], self.cap, self.B, self.d["q"], self.d["qdesc"], self.d["nq"],
                                           self.qcap, self.assigned, self.nm, d_occupied=self.d["occ"] if self.with_occ else None,
                                           d_uright=self.d["uright"] if self.with_ur else None, nnratio=ratio, th_dist=th, check_orientation=ori, stream=stream)
        return self

    def results(self):
        """after a synchronise"""
        return self.assigned.cpu().numpy(), self.nm.cpu().numpy()


def expect(oracle, f, kind, mode, with_ur=False, with_occ=True):
    n, nq = len(f["feats"]), len(f["q"])
    if n == 0 or nq == 0:
        return np.full(n, -1, np.int32), 0
    ratio, th, ori = params(kind, mode)
    return oracle.search_by_projection(kind, mode, f["feats"], f["desc"], f["q"], f["qdesc"], f["occ"] if with_occ else None, f["uright"] if with_ur else None, ratio, th, ori)


def check(got, frames, want, cap):
    """assigned rows and count of every frame against `want` = [(assigned, count)]; rows at or past a frame's count keep the sentinel"""
    a, nm = got
    for i, (f, (oa, on)) in enumerate(zip(frames, want)):
        n = len(f["feats"])
        np.testing.assert_array_equal(a[i, :n], oa, err_msg="frame %d" % i)
        assert nm[i] == on, (i, nm[i], on)
        assert (a[i, n:] == SENT).all(), i
    assert (a[len(frames):] == SENT).all() and (nm[len(frames):] == SENT).all()


# ---- 1. a ragged batch
CAP1, QCAP1 = 400, 152


@pytest.fixture(scope="module")
def ragged():
    """kind -> five frames: n == cap; nq == qcap; 65 ordinary queries (one past the commit's step of 64); n == 1; an ordinary one"""
    out = {}
    for kind in (0, 1):
        s = 5000 + 100 * kind
        out[kind] = [frame(s + 1, CAP1, kind, 6, 60), frame(s + 2, 300, kind, 6, 80), frame(s + 3, 260, kind, 3, 65, ordinary_only=True),
                     frame(s + 4, 200, kind, 3, 40, take_n=1), frame(s + 5, 250, kind, 4, 50)]
        assert [len(f["feats"]) for f in out[kind]] == [CAP1, 300, 260, 1, 250] and [len(f["q"]) for f in out[kind]] == [132, QCAP1, 65, 76, 98]
    return out


@pytest.mark.parametrize("with_occ", [True, False])
@pytest.mark.parametrize("kind,mode,with_ur", [(0, 0, False), (0, 0, True), (0, 1, False), (0, 1, True), (1, 0, False), (1, 1, False)])
def test_ragged_batch(ctx, oracle, ragged, kind, mode, with_ur, with_occ):
    frames = ragged[kind]
    want = [expect(oracle, f, kind, mode, with_ur, with_occ) for f in frames]
    for f, (oa, _) in zip(frames, want):
        if f["whole"]: assert mc.clusters_taken_in_order(f["case"], oa)
    c = Call(pack(frames, kind, CAP1, QCAP1), kind, mode, CAP1, QCAP1, with_ur, with_occ).launch(ctx)
    ctx.synchronize()
    got = c.results()
    check(got, frames, want, CAP1)
    for i, f in enumerate(frames):
        if f["whole"]: assert mc.clusters_taken_in_order(f["case"], got[0][i, :len(f["feats"])])
    # the single call on one frame's slices agrees as well
    f = frames[4]
    ratio, th, ori = params(kind, mode)
    a, nm = ctx.search_by_projection(kind, mode, f["feats"], f["desc"], f["q"], f["qdesc"], f["occ"] if with_occ else None, f["uright"] if with_ur else None, ratio, th, ori)
    np.testing.assert_array_equal(a, got[0][4, :len(a)]); assert nm == got[1][4]


# ---- 2. empty and degenerate frames
def test_degenerate_frames(ctx, oracle):
    kind, mode, cap, qcap = 0, 1, 200, 112
    def ordinary(seed, n=180): return frame(seed, n, kind, 4, 50)
    none_valid = ordinary(6105); none_valid["q"] = none_valid["q"].copy(); none_valid["q"]["valid"] = 0
    all_occ = ordinary(6106); all_occ["occ"] = np.ones_like(all_occ["occ"])
    full = frame(6108, cap, kind, 4, qcap - 48)          # n == cap and nq == qcap: the frame whose counts arrive as capacity + 7
    assert len(full["q"]) == qcap
    frames = [frame(6100, 150, kind, 3, 40, take_n=0),                 # n = 0
              ordinary(6101),
              frame(6102, 150, kind, 3, 40), frame(6103, 150, kind, 3, 40, take_n=0),      # nq = 0 (cut below), both zero
              ordinary(6104),
              none_valid, all_occ,
              ordinary(6107),                                          # count -3 in d_n: read as no features
              full,
              ordinary(6109)]                                          # count -3 in d_nq: read as no queries
    for i in (2, 3): frames[i]["q"] = frames[i]["q"][:0]; frames[i]["qdesc"] = frames[i]["qdesc"][:0]
    P = pack(frames, kind, cap, qcap)
    n, nq = P["n"].copy(), P["nq"].copy()
    assert list(n[:4]) == [0, 180, 150, 0] and list(nq[:4]) == [76, 98, 0, 0]
    n[7] = -3; n[8] = cap + 7; nq[8] = qcap + 7; nq[9] = -3
    seen = [dict(f) for f in frames]                                   # what the call sees: the clamped slices
    for k in ("feats", "desc", "occ", "uright"): seen[7][k] = seen[7][k][:0]
    seen[9]["q"] = seen[9]["q"][:0]; seen[9]["qdesc"] = seen[9]["qdesc"][:0]
    want = [expect(oracle, f, kind, mode) for f in seen]
    for i in (0, 2, 3, 5, 6, 7, 9):
        assert want[i][1] == 0 and (want[i][0] == -1).all(), i
    assert want[1][1] > 20 and want[8][1] > 20
    c = Call(P, kind, mode, cap, qcap, n=n, nq=nq).launch(ctx)
    ctx.synchronize()
    check(c.results(), seen, want, cap)
    # B = 1: every frame alone; and no frame at all
    for i in (1, 3, 8):
        one = Call(pack([seen[i]], kind, cap, qcap), kind, mode, cap, qcap).launch(ctx)
        ctx.synchronize()
        check(one.results(), [seen[i]], [want[i]], cap)
    z = Call(P, kind, mode, cap, qcap, nframes=0).launch(ctx)
    ctx.synchronize()
    check(z.results(), [], [], cap)


# ---- 3. per-frame state
def test_state_does_not_leak(ctx, oracle):
    kind, mode, cap, qcap = 0, 1, 300, 160
    a = frame(6200, 300, kind, 5, 100)
    b = dict(a); b["q"] = a["q"].copy(); b["q"]["angle"] = (a["q"]["angle"] + 90) % 360; b["whole"] = False
    # the first frame's queries on other features: its keypoints in reverse order, turned by 0 / 40 / 80 degrees (other matches, other rotation bins)
    c3 = dict(a); c3["whole"] = False
    for k in ("feats", "desc", "occ", "uright"): c3[k] = a[k][::-1].copy()
    c3["feats"]["angle"] = (c3["feats"]["angle"] + 40 * (np.arange(300) % 3)) % 360
    frames = [a, b, c3]
    want = [expect(oracle, f, kind, mode) for f in frames]
    assert all((w[0] == -2).any() and w[1] > 50 for w in want)           # the rotation check removes matches in every frame
    assert not np.array_equal(want[0][0], want[2][0][::-1])             # and not the same ones under the turned keypoints
    c = Call(pack(frames, kind, cap, qcap), kind, mode, cap, qcap).launch(ctx)
    ctx.synchronize()
    check(c.results(), frames, want, cap)


# ---- 4. the size boundaries of the plan
SIZE_FRAMES = {}


def size_frames(cap, nq_extra):
    if cap not in SIZE_FRAMES:
        SIZE_FRAMES[cap] = [frame(mc.proj_seed(cap, 0, 0), cap, 0, 30, nq_extra), frame(mc.proj_seed(cap, 0, 1), 600, 0, 30, nq_extra)]
    return SIZE_FRAMES[cap]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cap,nq_extra", [(6136, 300), (6200, 300), (8192, 300), (8200, 40)])
def test_size_boundaries(ctx, oracle, cap, nq_extra, mode):
    """8 * 6136 + 64 bytes is the last commit launch without the dynamic-LDS opt-in; 8192 the last row capacity of the two-kernel form.  One frame
    fills its rows, the other uses 600 of them (the form follows the capacity, not the count)."""
    frames = size_frames(cap, nq_extra)
    qcap = 360 + nq_extra
    want = [expect(oracle, f, 0, mode, with_ur=True) for f in frames]
    for f, (oa, _) in zip(frames, want): assert mc.clusters_taken_in_order(f["case"], oa)
    c = Call(pack(frames, 0, cap, qcap), 0, mode, cap, qcap, with_ur=True).launch(ctx)
    ctx.synchronize()
    check(c.results(), frames, want, cap)


@pytest.mark.parametrize("cap,n", [(400, 400), (8200, 300)])
def test_slice_boundary(fe, oracle, cap, n):
    """five frames in slices of two, two and one (sslam_testing_proj_batch_tuning lowers the slice of the testing library); every slice reuses
    the same scratch rows, in stream order"""
    kind, mode, qcap = 0, 1, 120
    frames = [frame(6300 + i, n - 20 * i, kind, 4, 50 + 4 * i) for i in range(5)]
    want = [expect(oracle, f, kind, mode) for f in frames]
    with fe.use_testing_library() as T:
        tctx = fe.Context(0)
        try:
            assert T.sslam_testing_proj_batch_tuning(2, 0) == 0
            c = Call(pack(frames, kind, cap, qcap), kind, mode, cap, qcap).launch(tctx)
            tctx.synchronize()
            got = c.results()
        finally:
            T.sslam_testing_proj_batch_tuning(0, 0)
            tctx.close()
    check(got, frames, want, cap)


# ---- 5. streams and the shared context
@pytest.fixture(scope="module")
def two_batches(oracle):
    kind, mode, cap, qcap = 0, 1, 320, 140
    A = [frame(6400 + i, 320 - 30 * i, kind, 4, 60 + 5 * i) for i in range(4)]
    B = [frame(6410 + i, 200 + 25 * i, kind, 3, 50 + 7 * i) for i in range(3)]
    return dict(kind=kind, mode=mode, cap=cap, qcap=qcap, A=A, B=B, wantA=[expect(oracle, f, kind, mode) for f in A], wantB=[expect(oracle, f, kind, mode) for f in B])


def test_streams_back_to_back(ctx, two_batches):
    t = two_batches
    s = torch.cuda.Stream()
    PA, PB = pack(t["A"], t["kind"], t["cap"], t["qcap"]), pack(t["B"], t["kind"], t["cap"], t["qcap"], seed=98)
    c1, c2 = Call(PA, t["kind"], t["mode"], t["cap"], t["qcap"]), Call(PB, t["kind"], t["mode"], t["cap"], t["qcap"])
    c1.launch(ctx, s.cuda_stream); c2.launch(ctx, s.cuda_stream)          # the second call's slices reuse the arena behind the first's, in stream order
    s.synchronize()
    check(c1.results(), t["A"], t["wantA"], t["cap"]); check(c2.results(), t["B"], t["wantB"], t["cap"])


def test_streams_batch_beside_the_synchronous_call(ctx, oracle, two_batches):
    t = two_batches
    s = torch.cuda.Stream()
    f = t["B"][2]
    ratio, th, ori = params(t["kind"], t["mode"])
    c1 = Call(pack(t["A"], t["kind"], t["cap"], t["qcap"]), t["kind"], t["mode"], t["cap"], t["qcap"]).launch(ctx, s.cuda_stream)
    a, nm = ctx.search_by_projection(t["kind"], t["mode"], f["feats"], f["desc"], f["q"], f["qdesc"], f["occ"], None, ratio, th, ori)      # on the context stream, its own arena
    s.synchronize()
    check(c1.results(), t["A"], t["wantA"], t["cap"])
    np.testing.assert_array_equal(a, t["wantB"][2][0]); assert nm == t["wantB"][2][1]


def test_streams_two_side_streams(ctx, two_batches):
    t = two_batches
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    PA, PB = pack(t["A"], t["kind"], t["cap"], t["qcap"]), pack(t["B"], t["kind"], t["cap"], t["qcap"], seed=98)
    c1, c2 = Call(PA, t["kind"], t["mode"], t["cap"], t["qcap"]), Call(PB, t["kind"], t["mode"], t["cap"], t["qcap"])
    c1.launch(ctx, s1.cuda_stream); c2.launch(ctx, s2.cuda_stream)      # one arena: c2's kernels wait for the context's event behind c1
    s1.synchronize(); s2.synchronize()
    check(c1.results(), t["A"], t["wantA"], t["cap"]); check(c2.results(), t["B"], t["wantB"], t["cap"])


# ---- 6. argument errors
def test_argument_errors(fe, ctx):
    kind, cap, qcap = 0, 120, 90
    frames = [frame(6500, 120, 0, 3, 50), frame(6501, 100, 0, 3, 40)]
    P = pack(frames, kind, cap, qcap)
    d = {k: dev(P[k]) for k in P}
    assigned = torch.full((2, cap), SENT, dtype=torch.int32, device="cuda"); nm = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    dl = {k: dev(pack([frame(6502, 120, 1, 3, 50)], 1, cap, qcap)[k]) for k in P}
    torch.cuda.synchronize()

    def call(kind=0, mode=0, cap=cap, qcap=qcap, n="n", assigned=assigned, nm=nm, ori=False, src=d):
        with pytest.raises(fe.SslamError) as e:
            ctx.search_by_projection_batch_dev(kind, mode, src["feats"], src["desc"], src[n] if n else None, cap, 2 if src is d else 1, src["q"], src["qdesc"], src["nq"], qcap,
                                               assigned, nm, d_occupied=src["occ"], check_orientation=ori)
        assert e.value.code == fe.SSLAM_ERR_INVALID
    call(kind=2)
    call(mode=2)
    call(kind=1, mode=1, ori=True, src=dl)
    call(cap=1 << 19)
    call(qcap=-1)
    call(n=None)
    call(assigned=None)
    call(nm=None)
    ctx.synchronize(); torch.cuda.synchronize()
    assert (assigned.cpu().numpy() == SENT).all() and (nm.cpu().numpy() == SENT).all()
    # the same buffers are accepted once the arguments are valid (kind 1, mode 1 without the rotation check included)
    ctx.search_by_projection_batch_dev(1, 1, dl["feats"], dl["desc"], dl["n"], cap, 1, dl["q"], dl["qdesc"], dl["nq"], qcap, assigned, nm, d_occupied=dl["occ"], check_orientation=False)
    ctx.synchronize()
    assert nm.cpu().numpy()[0] >= 0


# ---- 7. the pipeline's method
def test_frontend_batch(fe, ctx, oracle):
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    w, h, B = 320, 240, 4
    imgs = [synth_frame(6600 + i, w, h, nshapes=14 + 5 * i, nstrokes=4 + 2 * i) for i in range(B)]
    pipe = pipeline.FrontendBatch(fe, ctx, w, h, B, 500, 100, "cuda:0")
    assert not hasattr(pipe, "_proj_out")                             # nothing held for the matcher until it is used
    pipe.extract(torch.from_numpy(np.stack(imgs)).cuda())
    torch.cuda.synchronize()
    c = pipe.feat["cur"]
    scales = oracle.orb_params()[0]
    bounds = (0.0, float(w), 0.0, float(h))
    for kind, mode, ratio in ((0, 1, 0.9), (1, 0, 0.6)):
        cap = pipe.cap if kind == 0 else pipe.lcap
        cnt = (c["n"] if kind == 0 else c["nl"]).cpu().numpy()
        raw = (c["kp"] if kind == 0 else c["kl"]).cpu().numpy().view(np.uint8).reshape(B, cap, -1)
        dsc = (c["desc"] if kind == 0 else c["ldesc"]).cpu().numpy()
        rng = np.random.default_rng(6600 + kind)
        feats = [raw[i, :cnt[i]].copy().view(KP_DTYPE if kind == 0 else KL_DTYPE).reshape(-1) for i in range(B)]
        assert cnt.min() > (100 if kind == 0 else 5)
        qcap = int(cnt.max())
        q = junk(rng, (B, qcap), mc.PQ_DTYPE); qd = junk(rng, (B, qcap, 32), np.uint8)
        occ = (rng.random((B, cap)) < 0.05).astype(np.uint8)
        for i in range(B):                                             # queries from the frame's own features, jittered
            qi = _own_queries(rng, feats[i], kind, mode, scales)
            q[i, :cnt[i]] = qi; qd[i, :cnt[i]] = mc.flip_bits(rng, dsc[i, :cnt[i]], 12)
        ori = kind == 0
        a, nm = pipe.search_by_projection(kind, mode, dev(q), dev(qd).view(B, qcap, 32), torch.from_numpy(cnt.astype(np.int32)).cuda(), torch.from_numpy(occ).cuda(),
                                          nnratio=ratio, th_dist=100, check_orientation=ori)
        torch.cuda.synchronize()
        assert a.shape == (B, cap) and nm.shape == (B,)
        a, nm = a.cpu().numpy(), nm.cpu().numpy()
        for i in range(B):
            oa, on = oracle.search_by_projection(kind, mode, feats[i], dsc[i, :cnt[i]], q[i, :cnt[i]], qd[i, :cnt[i]], occ[i, :cnt[i]], None, ratio, 100, ori, bounds=bounds)
            assert on > (50 if kind == 0 else 3), (kind, i, on)
            np.testing.assert_array_equal(a[i, :cnt[i]], oa); assert nm[i] == on
    pipe.close()


def _own_queries(rng, feats, kind, mode, scales):
    """as tests/test_match_gpu.py::_proj_queries builds them"""
    n = len(feats)
    q = np.zeros(n, mc.PQ_DTYPE)
    if kind == 0:
        q["u"] = feats["x"] + 3 + rng.normal(0, 1.5, n); q["v"] = feats["y"] - 2 + rng.normal(0, 1.5, n)
        o = feats["octave"]
        q["radius"] = 15 * scales[o]; q["min_level"] = o - 1; q["max_level"] = o + 1
        q["angle"] = feats["angle"]
    else:
        q["u"] = feats["startPointX"] + 3; q["v"] = feats["startPointY"] - 2
        q["u2"] = feats["endPointX"] + 3; q["v2"] = feats["endPointY"] - 2
        q["radius"] = np.where(rng.random(n) < 0.5, 5.0, 8.0) * 3; q["min_level"] = -1; q["max_level"] = 0
    q["valid"] = rng.random(n) < 0.95
    q["obs_positive"] = rng.random(n) < 0.9
    return q
