"""GPU parity of sslam_two_view_ransac / sslam_two_view_ransac_batch_dev (Initializer::Initialize's model selection, reference src/Initializer.cc:55-118, :155-497, :784-830)
with the host model of the same header: tests/two_view_sim.py runs csrc/two_view_math.h under g++.  Every comparison is bit for bit (a NaN equals a NaN), and through the
testing tap it covers EVERY hypothesis -- sets, Hn, H21i, H12i, Fn, F21i and both scores -- not only the winner.  The cases are tests/two_view_cases.py's (what each reaches
is shown in tests/test_two_view_cases_cpu.py).

  test_single_call_and_every_hypothesis   every case through sslam_two_view_ransac and through sslam_testing_two_view_hypotheses
  test_batch_of_two                       every case as pairs 0 and 1 of a batch of another capacity: pair 0 equals the single call row for row, pair 1 draws other sets;
                                          0xA5 behind every count and behind the last pair
  test_batch_of_70                        one launch, 70 pairs of every status; on a side stream
  test_size_bound                         cap 4096 accepted, 4097 SSLAM_ERR_UNSUPPORTED with nothing written
  test_argument_errors                    SSLAM_ERR_INVALID leaves the outputs alone
  test_behind_search_for_initialization   sslam_orb_search_for_initialization_batch_dev -> this call on the ICL frame and a shifted copy, matches12 never leaving the device
  (the Python methods are what the tests call: they return the C ABI's bytes)"""
import ctypes as C
import os
import numpy as np
import pytest
import torch
import two_view_cases as tc
import two_view_sim as sim

pytestmark = pytest.mark.gpu

FILL = 0xA5


def same_floats(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_result(got, want):
    return all(int(got[k]) == int(want[k]) for k in ("nmatches", "model", "best_it_h", "best_it_f")) and \
        all(same_floats(got[k], want[k]) for k in ("score_h", "score_f", "rh", "H21", "F21"))


def keypoints(fe, xy, rng):
    """KP_DTYPE rows at xy; the fields the call must not read hold junk"""
    kp = rng.integers(0, 256, (len(xy), fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(-1)
    kp["x"] = xy[:, 0]; kp["y"] = xy[:, 1]
    return kp


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def tap(fe, ctx, c, kp1, kp2, pair=0):
    it = c["iterations"]
    res = np.zeros(1, fe.TWO_VIEW_RESULT_DTYPE); inl = np.zeros(len(kp1), np.uint8)
    sets = np.full((it, 8), -9, np.int32); mats = np.full((it, 5, 9), -9, np.float32); scores = np.full((it, 2), -9, np.float32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    m12 = np.ascontiguousarray(c["m12"], np.int32)
    rc = fe.testing_lib().sslam_testing_two_view_hypotheses(ctx.h, p(kp1), len(kp1), p(kp2), len(kp2), p(m12), p(c["sets"]), it, C.c_float(c["sigma"]), C.c_uint32(c["seed"]),
                                                            int(pair), p(res), p(inl), p(sets), p(mats), p(scores))
    assert rc == 0, fe.testing_lib().sslam_last_error()
    return res[0], inl, sets, mats, scores


def check_hypotheses(name, got, want):
    res, inl, sets, mats, scores = got
    assert same_result(res, want["result"]), (name, res, want["result"])
    np.testing.assert_array_equal(inl, want["inliers"], err_msg=name)
    np.testing.assert_array_equal(sets, want["sets"], err_msg=name)
    for it in range(len(sets)):
        for k, m in enumerate(("Hn", "H21i", "H12i", "Fn", "F21i")):
            assert same_floats(mats[it, k], want["mats"][it, k]), (name, it, m, mats[it, k], want["mats"][it, k])
        assert same_floats(scores[it], want["scores"][it]), (name, it, scores[it], want["scores"][it])


def test_single_call_and_every_hypothesis(fe, ctx):
    rng = np.random.default_rng(1)
    for c, want in zip(tc.all_cases(), tc.expected()):
        kp1, kp2 = keypoints(fe, c["kp1"], rng), keypoints(fe, c["kp2"], rng)
        res, inl = ctx.two_view_ransac(kp1, kp2, c["m12"], c["sets"], c["iterations"], c["sigma"], c["seed"])
        assert same_result(res, want["result"]), (c["name"], res, want["result"])
        np.testing.assert_array_equal(inl, want["inliers"], err_msg=c["name"])
        check_hypotheses(c["name"], tap(fe, ctx, c, kp1, kp2), want)


class Batch:
    """device inputs of one batch call (junk behind every count) and outputs filled with 0xA5, one pair more than the call may touch"""
    def __init__(self, fe, cases, cap, seed=5, sets=None, iterations=None):
        rng = np.random.default_rng(seed)
        P = len(cases)
        self.P, self.cap, self.cases = P, cap, cases
        kp1 = rng.integers(0, 256, (P, cap, fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(P, cap)
        kp2 = rng.integers(0, 256, (P, cap, fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(P, cap)
        m12 = rng.integers(-5, cap + 5, (P, cap)).astype(np.int32)
        self.n1 = np.array([len(c["kp1"]) for c in cases], np.int32); self.n2 = np.array([len(c["kp2"]) for c in cases], np.int32)
        for p, c in enumerate(cases):
            kp1[p, :self.n1[p]] = keypoints(fe, c["kp1"], rng); kp2[p, :self.n2[p]] = keypoints(fe, c["kp2"], rng)
            m12[p, :self.n1[p]] = c["m12"]
        self.d = dict(kp1=dev(kp1), kp2=dev(kp2), n1=dev(self.n1), n2=dev(self.n2), m12=dev(m12), sets=None if sets is None else dev(np.ascontiguousarray(sets, np.int32)))
        self.res = torch.full(((P + 1) * fe.TWO_VIEW_RESULT_DTYPE.itemsize,), FILL, dtype=torch.uint8, device="cuda")
        self.inl = torch.full(((P + 1) * cap,), FILL, dtype=torch.uint8, device="cuda")
        self.fe = fe
        torch.cuda.synchronize()

    def launch(self, ctx, iterations, sigma, seed, stream=None, cap=None, npairs=None):
        ctx.two_view_ransac_batch_dev(self.d["kp1"], self.d["n1"], self.d["kp2"], self.d["n2"], self.cap if cap is None else cap, self.P if npairs is None else npairs,
                                      self.d["m12"], self.res, self.inl, d_sets=self.d["sets"], iterations=iterations, sigma=sigma, seed=seed, stream=stream)
        return self

    def results(self):
        return self.res.cpu().numpy().view(self.fe.TWO_VIEW_RESULT_DTYPE), self.inl.cpu().numpy().reshape(self.P + 1, self.cap)

    def untouched(self):
        res, inl = self.results()
        return bool((res.view(np.uint8) == FILL).all() and (inl == FILL).all())

    def check(self, want):
        res, inl = self.results()
        for p, w in enumerate(want):
            name = "%s as pair %d" % (self.cases[p]["name"], p)
            assert same_result(res[p], w["result"]), (name, res[p], w["result"])
            np.testing.assert_array_equal(inl[p, :self.n1[p]], w["inliers"], err_msg=name)
            assert (inl[p, self.n1[p]:] == FILL).all(), name            # rows [n1, cap) are not written
        assert (res[self.P:].view(np.uint8) == FILL).all() and (inl[self.P] == FILL).all()


def test_batch_of_two(fe, ctx):
    cs = tc.all_cases()
    want0, want1 = tc.expected(), tc.expected(tuple([1] * len(cs)))
    for c, w0, w1 in zip(cs, want0, want1):
        cap = max(len(c["kp1"]), len(c["kp2"]), 1) + 3
        sets = None if c["sets"] is None else np.stack([c["sets"], c["sets"]])
        b = Batch(fe, [c, c], cap, sets=sets).launch(ctx, c["iterations"], c["sigma"], c["seed"])
        ctx.synchronize()
        b.check([w0, w1])
        if c["sets"] is None and w0["result"]["nmatches"] >= 8:
            assert (w0["sets"] != w1["sets"]).any(), c["name"]           # pairs 0 and 1 draw different sets


def test_exact_capacity(fe, ctx):
    """nmatches == n1 == n2 == cap: no row behind the counts"""
    i = [c["name"] for c in tc.all_cases()].index("count_full_64")
    c = tc.all_cases()[i]
    b = Batch(fe, [c], 64).launch(ctx, c["iterations"], c["sigma"], c["seed"])
    ctx.synchronize()
    b.check([tc.expected()[i]])


def mixed_batch():
    """70 pairs under one iteration count, sigma and seed, the library drawing: every case's geometry, the first 27 twice"""
    cs = tc.all_cases()
    cs = [dict(c, sets=None, iterations=8, sigma=1.0, seed=77) for c in (cs + cs[:27])]
    assert len(cs) == 70
    return cs


def test_batch_of_70(fe, ctx):
    cs = mixed_batch()
    want = sim.run([dict(c, pair=p) for p, c in enumerate(cs)])
    res = [w["result"] for w in want]
    assert {int(r["model"]) for r in res} == {0, 1, 2} and any(r["model"] and r["best_it_h"] < 0 for r in res)       # skipped, H, F, and no homography above 0
    cap = max(max(len(c["kp1"]), len(c["kp2"])) for c in cs)
    st = torch.cuda.Stream()
    b = Batch(fe, cs, cap).launch(ctx, 8, 1.0, 77, stream=st.cuda_stream)
    st.synchronize()
    b.check(want)


def test_size_bound(fe, ctx):
    c = tc.all_cases()[[c["name"] for c in tc.all_cases()].index("count_63")]
    want = sim.run([c])[0]
    b = Batch(fe, [c], 4096).launch(ctx, c["iterations"], c["sigma"], c["seed"])
    ctx.synchronize()
    b.check([want])
    b = Batch(fe, [c], 4097)
    with pytest.raises(fe.SslamError) as e:
        b.launch(ctx, c["iterations"], c["sigma"], c["seed"])
    assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED
    ctx.synchronize()
    assert b.untouched()


def test_argument_errors(fe, ctx):
    c = tc.all_cases()[[c["name"] for c in tc.all_cases()].index("count_9")]
    b = Batch(fe, [c], 16)
    good = dict(d_kp1=b.d["kp1"], d_n1=b.d["n1"], d_kp2=b.d["kp2"], d_n2=b.d["n2"], cap=16, npairs=1, d_matches12=b.d["m12"], d_result=b.res, d_inliers=b.inl, d_sets=None,
                iterations=4, sigma=1.0, seed=0)
    bad = [dict(iterations=0), dict(iterations=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(cap=0), dict(cap=-4), dict(npairs=0), dict(npairs=-1),
           dict(d_kp1=None), dict(d_n1=None), dict(d_kp2=None), dict(d_n2=None), dict(d_matches12=None), dict(d_result=None), dict(d_inliers=None),
           dict(d_kp1=b.d["kp1"].data_ptr() + 2), dict(d_n2=b.d["n2"].data_ptr() + 1), dict(d_matches12=b.d["m12"].data_ptr() + 2), dict(d_result=b.res.data_ptr() + 1),
           dict(d_sets=b.d["m12"].data_ptr() + 1), dict(npairs=1 << 20, cap=4096)]
    for k in bad:
        with pytest.raises(fe.SslamError) as e:
            ctx.two_view_ransac_batch_dev(**dict(good, **k))
        assert e.value.code == fe.SSLAM_ERR_INVALID, k
    ctx.synchronize()
    assert b.untouched()
    kp = keypoints(fe, c["kp1"], np.random.default_rng(3))
    for k in (dict(iterations=0), dict(sigma=0.0), dict(sigma=-2.0)):
        with pytest.raises(fe.SslamError) as e:
            ctx.two_view_ransac(kp, kp, c["m12"], **k)
        assert e.value.code == fe.SSLAM_ERR_INVALID, k
    big = np.zeros(4097, fe.KP_DTYPE)
    with pytest.raises(fe.SslamError) as e:
        ctx.two_view_ransac(big, big, np.full(4097, -1, np.int32), iterations=1)
    assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED


def test_behind_search_for_initialization(fe, ctx):
    """the ICL frame against a copy shifted by (6, 4) pixels, twice in one batch: ORB on both, SearchForInitialization on the device, this call on its d_matches12"""
    gray = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icl_input_gray.npz"))["gray"]
    moved = np.ascontiguousarray(np.pad(gray, ((4, 0), (6, 0)), mode="edge")[:gray.shape[0], :gray.shape[1]])
    ex = fe.OrbExtractor(ctx, 1000, 1.2, 8, 20, 7)
    (kp1, d1), (kp2, d2) = ex(gray), ex(moved)
    ex.close()
    P, cap = 2, max(len(kp1), len(kp2)) + 7
    K1 = np.zeros((P, cap), fe.KP_DTYPE); K2 = np.zeros((P, cap), fe.KP_DTYPE); D1 = np.zeros((P, cap, 32), np.uint8); D2 = np.zeros((P, cap, 32), np.uint8)
    pm = np.zeros((P, cap, 2), np.float32)
    for p in range(P):
        K1[p, :len(kp1)] = kp1; K2[p, :len(kp2)] = kp2; D1[p, :len(kp1)] = d1; D2[p, :len(kp2)] = d2
        pm[p, :len(kp1), 0] = kp1["x"]; pm[p, :len(kp1), 1] = kp1["y"]
    g = dict(kp1=dev(K1), kp2=dev(K2), d1=dev(D1), d2=dev(D2), n1=dev(np.full(P, len(kp1), np.int32)), n2=dev(np.full(P, len(kp2), np.int32)), pm=dev(pm))
    m12 = torch.full((P, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    res = torch.full((P * fe.TWO_VIEW_RESULT_DTYPE.itemsize,), FILL, dtype=torch.uint8, device="cuda"); inl = torch.full((P * cap,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _p = lambda x: C.c_void_p(x.data_ptr())
    bounds = (C.c_float * 4)(0.0, 640.0, 0.0, 480.0)
    rc = fe.lib().sslam_orb_search_for_initialization_batch_dev(ctx.h, _p(g["kp1"]), _p(g["d1"]), _p(g["n1"]), _p(g["kp2"]), _p(g["d2"]), _p(g["n2"]), cap, P, _p(g["pm"]), _p(m12),
                                                                _p(nm), 100, C.c_float(0.9), 1, bounds, C.c_void_p(0))
    assert rc == 0, fe.lib().sslam_last_error()
    ctx.two_view_ransac_batch_dev(g["kp1"], g["n1"], g["kp2"], g["n2"], cap, P, m12, res, inl, iterations=200, sigma=1.0, seed=2026)      # same stream, no copy in between
    ctx.synchronize()
    m = m12.cpu().numpy(); got = res.cpu().numpy().view(fe.TWO_VIEW_RESULT_DTYPE); gi = inl.cpu().numpy().reshape(P, cap)
    assert nm.cpu().numpy()[0] >= 100                                        # what Tracking asks for before it initialises (src/Tracking.cc)
    xy = lambda k: np.stack([k["x"], k["y"]], 1)
    want = sim.run([dict(kp1=xy(kp1), kp2=xy(kp2), m12=m[p, :len(kp1)], sets=None, iterations=200, sigma=1.0, seed=2026, pair=p) for p in range(P)])
    for p in range(P):
        assert same_result(got[p], want[p]["result"]), (p, got[p], want[p]["result"])
        np.testing.assert_array_equal(gi[p, :len(kp1)], want[p]["inliers"])
        assert (gi[p, len(kp1):] == FILL).all()
    assert got[0]["model"] == 1 and got[0]["nmatches"] == nm.cpu().numpy()[0]      # a pure image shift is a homography
