"""GPU parity of sslam_sim3_ransac / sslam_sim3_ransac_batch_dev (Sim3Solver, reference src/Sim3Solver.cc: the RANSAC of LoopClosing::ComputeSim3) with the host model of
the same header: tests/sim3_sim.py runs csrc/sim3_math.h under g++.  Every comparison is bit for bit (a NaN equals a NaN), and through the testing tap it covers EVERY
iteration the reference's loop ran -- set, s12, R12, t12 and the count -- not only the best.  The cases are tests/sim3_cases.py's (what each reaches is shown in
tests/test_sim3_cases_cpu.py).

  test_single_call_and_every_hypothesis   every case, call after call on one state, through sslam_sim3_ransac and through sslam_testing_sim3_hypotheses
  test_batch_of_two                       every case as pairs 0 and 1 of a batch over a pool of two slots, call after call on the device-resident states: pair 0 equals the
                                          single call, pair 1 draws other sets; 0xA5 behind every count and behind the last pair
  test_batch_of_70                        one launch on a side stream: every case's geometry, one keyframe against 20 candidates, (a, b) beside (b, a), a pair of a slot with
                                          itself, two skipped pairs
  test_caps_and_size_bound                capacities on both sides of the dynamic-LDS opt-in and at the bound; 3073 is SSLAM_ERR_UNSUPPORTED with nothing written
  test_table_rebuilds_in_stream_order     calls that alternate between two parameter sets and two streams without a synchronise in between
  test_argument_errors                    every refused combination: SSLAM_ERR_INVALID, nothing enqueued, the outputs left alone
  test_behind_search_by_bow               sslam_orb_search_by_bow_keyframes_batch_dev -> this call on the ICL frame and the same points under a known similarity
  (the Python methods are what the tests call: they return the C ABI's bytes)"""
import ctypes as C
import os
import numpy as np
import pytest
import torch
import sim3_cases as tc
import sim3_sim as sim

pytestmark = pytest.mark.gpu

FILL = 0xA5
INTS = ("its_done", "best_inliers", "best_it", "n", "max_its", "found_it", "n_inliers", "no_more")


def same_floats(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_state(got, want):
    return all(int(got[k]) == int(want[k]) for k in INTS) and all(same_floats(got[k], want[k]) for k in ("s12", "R12", "t12"))


def keypoints(fe, octave, rng):
    """KP_DTYPE rows with the octaves given; the fields the call must not read hold junk"""
    kp = rng.integers(0, 256, (len(octave), fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(-1)
    kp["octave"] = octave
    return kp


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def params(c):
    return dict(fix_scale=c["fix_scale"], probability=c["probability"], min_inliers=c["min_inliers"], max_iterations=c["max_iterations"], seed=c["seed"])


def tap(fe, ctx, c, kp1, kp2, state, new_iterations, pair=0):
    it = c["max_iterations"]
    st = np.zeros(1, fe.SIM3_STATE_DTYPE); st[0] = state
    inl = np.zeros(len(kp1), np.uint8)
    sets = np.full((it, 3), -9, np.int32); mats = np.full((it, 13), -9, np.float32); counts = np.full(it, -9, np.int32)
    p = lambda a: None if a is None else C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    k1, k2 = c["kf1"], c["kf2"]
    hold = [np.ascontiguousarray(a) for a in (k1["x3dc"], k1["valid"], k1["K"], k2["x3dc"], k2["valid"], k2["K"], c["sigma2"], c["m12"])]
    cs = None if c["sets"] is None else np.ascontiguousarray(c["sets"], np.int32)
    rc = fe.testing_lib().sslam_testing_sim3_hypotheses(ctx.h, p(kp1), p(hold[0]), p(hold[1]), len(kp1), p(hold[2]), p(kp2), p(hold[3]), p(hold[4]), len(kp2), p(hold[5]),
                                                        p(hold[6]), len(hold[6]), p(hold[7]), int(c["fix_scale"]), C.c_double(c["probability"]), c["min_inliers"], it,
                                                        int(new_iterations), p(cs), C.c_uint32(c["seed"]), int(pair), p(st), p(inl), p(sets), p(mats), p(counts))
    assert rc == 0, fe.testing_lib().sslam_last_error()
    return st[0], inl, sets, mats, counts


def check_tap(name, got, want, max_iterations):
    st, inl, sets, mats, counts = got
    assert same_state(st, want["state"]), (name, st, want["state"])
    np.testing.assert_array_equal(inl, want["inliers"], err_msg=name)
    ran = np.zeros(max_iterations, bool); ran[want["its"]] = True
    np.testing.assert_array_equal(sets[ran], want["sets"], err_msg=name)
    np.testing.assert_array_equal(counts[ran], want["counts"], err_msg=name)
    for j, it in enumerate(want["its"]):
        assert same_floats(mats[it], want["mats"][j]), (name, it, mats[it], want["mats"][j])
    assert not sets[~ran].any() and not mats[~ran].any() and not counts[~ran].any(), name      # iterations this call did not run stay as the zero fill


def test_single_call_and_every_hypothesis(fe, ctx):
    rng = np.random.default_rng(1)
    for c, want in zip(tc.all_cases(), tc.expected()):
        kp1, kp2 = keypoints(fe, c["kf1"]["oct"], rng), keypoints(fe, c["kf2"]["oct"], rng)
        st = ts = None
        for new_its, w in zip(c["calls"], want["calls"]):
            st, inl = ctx.sim3_ransac(kp1, c["kf1"]["x3dc"], c["kf1"]["valid"], c["kf1"]["K"], kp2, c["kf2"]["x3dc"], c["kf2"]["valid"], c["kf2"]["K"], c["sigma2"], c["m12"],
                                      state=st, new_iterations=new_its, sets=c["sets"], **params(c))
            assert same_state(st, w["state"]), (c["name"], st, w["state"])
            np.testing.assert_array_equal(inl, w["inliers"], err_msg=c["name"])
            got = tap(fe, ctx, c, kp1, kp2, np.zeros(1, fe.SIM3_STATE_DTYPE)[0] if ts is None else ts, new_its)
            check_tap(c["name"], got, w, c["max_iterations"])
            ts = got[0]


class Pool:
    """a keyframe pool and a pair list on the device (junk behind every count), states and inlier rows of one pair more than the call may touch.
    slots: dicts of tests/sim3_cases.py's keyframes; pairs: (kf1, kf2, m12 int32 [n[kf1]] or None for a skipped pair)"""
    def __init__(self, fe, slots, pairs, cap, seed=5, sets=None, max_iterations=None):
        rng = np.random.default_rng(seed)
        S, P = len(slots), len(pairs)
        self.fe, self.slots, self.pairs, self.cap, self.S, self.P = fe, slots, pairs, cap, S, P
        kp = rng.integers(0, 256, (S, cap, fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(S, cap)
        kp["octave"] = rng.integers(0, tc.NLEVELS, (S, cap))      # in range behind the counts too: a row read there would count
        x = rng.normal(0, 3, (S, cap, 3)).astype(np.float32); valid = rng.integers(0, 2, (S, cap)).astype(np.uint8)
        K = np.zeros((S, 4), np.float32)
        self.n = np.array([len(s["oct"]) for s in slots], np.int32)
        for k, s in enumerate(slots):
            kp[k, :self.n[k]] = keypoints(fe, s["oct"], rng); x[k, :self.n[k]] = s["x3dc"]; valid[k, :self.n[k]] = s["valid"]; K[k] = s["K"]
        m12 = rng.integers(-5, cap + 5, (P, cap)).astype(np.int32)
        pr = np.zeros((P, 2), np.int32)
        st = np.zeros(P + 1, fe.SIM3_STATE_DTYPE)
        st.view(np.uint8)[-84:] = FILL
        for p, (a, b, m) in enumerate(pairs):
            pr[p] = (a, b)
            if m is None:
                st.view(np.uint8).reshape(P + 1, 84)[p] = FILL
            else:
                m12[p, :self.n[a]] = m
        self.d = dict(kp=dev(kp), x=dev(x), valid=dev(valid), n=dev(self.n), K=dev(K), m12=dev(m12), pairs=dev(pr), sets=None if sets is None else dev(np.ascontiguousarray(sets, np.int32)))
        self.state = dev(st)
        self.inl = torch.full(((P + 1) * cap,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def launch(self, ctx, new_iterations, stream=None, cap=None, **kw):
        ctx.sim3_ransac_batch_dev(self.d["kp"], self.d["x"], self.d["valid"], self.d["n"], self.cap if cap is None else cap, self.S, self.d["K"], tc.SIGMA2, self.d["pairs"], self.P,
                                  self.d["m12"], self.state, self.inl, d_sets=self.d["sets"], new_iterations=new_iterations, stream=stream, **kw)
        return self

    def results(self):
        return self.state.cpu().numpy().view(self.fe.SIM3_STATE_DTYPE), self.inl.cpu().numpy().reshape(self.P + 1, self.cap)

    def cases(self, **kw):
        """the pairs as cases for the sim (pair index included); None for a skipped pair"""
        return [None if m is None else dict(kf1=self.slots[a], kf2=self.slots[b], sigma2=tc.SIGMA2, m12=m, pair=p, sets=None, **kw) for p, (a, b, m) in enumerate(self.pairs)]

    def check(self, want, call=0):
        """want[p]: the sim's answer of pair p (its `call`-th call), None for a skipped pair"""
        st, inl = self.results()
        raw = st.view(np.uint8).reshape(self.P + 1, 84)
        for p, w in enumerate(want):
            a = self.pairs[p][0]
            if w is None:
                assert (int(st[p]["n"]), int(st[p]["max_its"]), int(st[p]["found_it"]), int(st[p]["n_inliers"]), int(st[p]["no_more"])) == (0, 0, -1, 0, 1), (p, st[p])
                assert (raw[p, :12] == FILL).all() and (raw[p, 32:] == FILL).all() and (inl[p] == FILL).all(), p      # the in/out words and the inlier row are not written
                continue
            w = w["calls"][call]
            assert same_state(st[p], w["state"]), (p, st[p], w["state"])
            np.testing.assert_array_equal(inl[p, :self.n[a]], w["inliers"], err_msg=str(p))
            assert (inl[p, self.n[a]:] == FILL).all(), p                                               # rows [n1, cap) are not written
        assert (raw[self.P] == FILL).all() and (inl[self.P] == FILL).all()

    def untouched(self, state0):
        st, inl = self.results()
        return bool((st.view(np.uint8) == state0).all() and (inl == FILL).all())


def test_batch_of_two(fe, ctx):
    cs = tc.all_cases()
    want0, want1 = tc.expected(), tc.expected(tuple([1] * len(cs)))
    for c, w0, w1 in zip(cs, want0, want1):
        cap = max(len(c["kf1"]["oct"]), len(c["kf2"]["oct"]), 1) + 3
        sets = None if c["sets"] is None else np.stack([c["sets"], c["sets"]])
        b = Pool(fe, [c["kf1"], c["kf2"]], [(0, 1, c["m12"]), (0, 1, c["m12"])], cap, sets=sets)
        for k, new_its in enumerate(c["calls"]):
            b.launch(ctx, new_its, **params(c))
            if k in (0, len(c["calls"]) - 1):
                ctx.synchronize()
                b.check([w0, w1], call=k)
        if c["sets"] is None and w0["n"] >= max(3, c["min_inliers"]):
            a, d = w0["calls"][0]["sets"], w1["calls"][0]["sets"]                                # (the two pairs may return at different iterations)
            k = min(len(a), len(d))
            assert (a[:k] != d[:k]).any(), c["name"]                                              # pairs 0 and 1 draw different sets


def mixed_pool(fe, cap=None):
    """every case's two keyframes as slots 2i, 2i + 1 and its matches as pair i; then slot 0 against 20 other slots over random matches, (b, a) beside (a, b), a slot
    against itself and two skipped pairs (a slot below 0, a slot at nkeyframes): 70 pairs"""
    cs = tc.all_cases()
    rng = np.random.default_rng(70)
    slots = [k for c in cs for k in (c["kf1"], c["kf2"])]
    pairs = [(2 * i, 2 * i + 1, c["m12"]) for i, c in enumerate(cs)]
    n = [len(s["oct"]) for s in slots]
    rand = lambda a, b: rng.integers(-1, n[b] + 1, n[a]).astype(np.int32)
    pairs += [(0, b, rand(0, b)) for b in range(1, 21)]
    back = np.full(n[3], -1, np.int32); m = cs[1]["m12"]; back[m[m >= 0]] = np.flatnonzero(m >= 0)
    pairs += [(3, 2, back), (6, 6, np.arange(n[6], dtype=np.int32)), (-1, 3, None), (4, len(slots), None)]
    pairs += [(2 * i, 2 * i + 1, cs[i]["m12"]) for i in range(70 - len(pairs))]
    assert len(pairs) == 70 and sum(p[2] is None for p in pairs) == 2
    return Pool(fe, slots, pairs, max(n) + 1 if cap is None else cap)


def test_batch_of_70(fe, ctx):
    b = mixed_pool(fe)
    kw = dict(fix_scale=False, probability=0.99, min_inliers=7, max_iterations=70, seed=77)
    cases = b.cases(calls=[5, 70], **kw)
    want = iter(sim.run([c for c in cases if c is not None]))
    want = [None if c is None else next(want) for c in cases]
    found = [w["calls"][1]["state"]["found_it"] for w in want if w is not None]
    assert min(found) == -1 and max(found) > 5 and any(w["n"] < 7 for w in want if w is not None)      # never, behind the first call, nothing iterated
    st = torch.cuda.Stream()
    b.launch(ctx, 5, stream=st.cuda_stream, **kw)
    st.synchronize()
    b.check(want, call=0)
    b.launch(ctx, 70, stream=st.cuda_stream, **kw)
    st.synchronize()
    b.check(want, call=1)


def test_caps_and_size_bound(fe, ctx):
    """48 bytes a row: 1000 rows stay below the 48 KB a kernel may have without asking, 1100 and 1400 (above 64 KB) need the opt-in, 3072 is the bound"""
    cs = [tc.all_cases()[[c["name"] for c in tc.all_cases()].index(n)] for n in ("count_129", "loop_closing")]
    kw = dict(fix_scale=False, probability=0.99, min_inliers=20, max_iterations=30, seed=3)
    pairs = [(0, 1, cs[0]["m12"]), (2, 3, cs[1]["m12"]), (3, 3, np.arange(len(cs[1]["kf2"]["oct"]), dtype=np.int32))]
    slots = [cs[0]["kf1"], cs[0]["kf2"], cs[1]["kf1"], cs[1]["kf2"]]
    want = None
    for cap in (1000, 1100, 1400, 3072):
        b = Pool(fe, slots, pairs, cap)
        if want is None:
            want = sim.run(b.cases(calls=[30], **kw))
        b.launch(ctx, 30, **kw)
        ctx.synchronize()
        b.check(want)
    b = Pool(fe, slots, pairs, 3073)
    s0 = b.results()[0].view(np.uint8).copy()
    with pytest.raises(fe.SslamError) as e:
        b.launch(ctx, 30, **kw)
    assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED
    ctx.synchronize()
    assert b.untouched(s0)
    big = np.zeros(3073, fe.KP_DTYPE)
    with pytest.raises(fe.SslamError) as e:
        ctx.sim3_ransac(big, np.ones((3073, 3), np.float32), None, tc.K1, big, np.ones((3073, 3), np.float32), None, tc.K2, tc.SIGMA2, np.full(3073, -1, np.int32))
    assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED


def test_table_rebuilds_in_stream_order(fe, ctx):
    """the table of mRansacMaxIts is the context's and is rebuilt when the parameters change: launches that alternate between two parameter sets and two streams, no
    synchronise in between, must each read their own table"""
    c = tc.all_cases()[[c["name"] for c in tc.all_cases()].index("loop_closing")]
    kws = [dict(fix_scale=False, probability=0.99, min_inliers=20, max_iterations=300, seed=9), dict(fix_scale=False, probability=0.9, min_inliers=40, max_iterations=12, seed=9)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pools, wants = [], []
    for k in range(6):
        b = Pool(fe, [c["kf1"], c["kf2"]], [(0, 1, c["m12"])] * 3, 96 + (k % 2), seed=k)
        pools.append(b); wants.append(sim.run(b.cases(calls=[300], **kws[k % 2])))
    for k, b in enumerate(pools):
        b.launch(ctx, 300, stream=streams[(k // 2) % 2].cuda_stream, **kws[k % 2])
    for s in streams:
        s.synchronize()
    for b, w in zip(pools, wants):
        b.check(w)
    assert wants[0][0]["calls"][0]["state"]["max_its"] == 293 and wants[1][0]["calls"][0]["state"]["max_its"] == 12


def test_argument_errors(fe, ctx):
    c = tc.all_cases()[[c["name"] for c in tc.all_cases()].index("count_min_plus_1")]
    b = Pool(fe, [c["kf1"], c["kf2"]], [(0, 1, c["m12"])], 16, sets=np.zeros((1, 4, 3), np.int32))
    s0 = b.results()[0].view(np.uint8).copy()
    good = dict(d_kp=b.d["kp"], d_x3dc=b.d["x"], d_valid=b.d["valid"], d_n=b.d["n"], cap=16, nkeyframes=2, d_K=b.d["K"], level_sigma2=tc.SIGMA2, d_pairs=b.d["pairs"], npairs=1,
                d_matches12=b.d["m12"], d_state=b.state, d_inliers=b.inl, fix_scale=False, probability=0.99, min_inliers=8, max_iterations=4, new_iterations=4, d_sets=None, seed=0)
    bad = [dict(d_kp=None), dict(d_x3dc=None), dict(d_n=None), dict(d_K=None), dict(level_sigma2=None, nlevels=8), dict(d_pairs=None), dict(d_matches12=None), dict(d_state=None),
           dict(d_inliers=None), dict(d_kp=b.d["kp"].data_ptr() + 2), dict(d_x3dc=b.d["x"].data_ptr() + 2), dict(d_n=b.d["n"].data_ptr() + 1), dict(d_K=b.d["K"].data_ptr() + 1),
           dict(d_pairs=b.d["pairs"].data_ptr() + 2), dict(d_matches12=b.d["m12"].data_ptr() + 2), dict(d_state=b.state.data_ptr() + 1), dict(d_sets=b.d["sets"].data_ptr() + 1),
           dict(cap=0), dict(cap=-3), dict(npairs=-1), dict(nkeyframes=-1), dict(nlevels=0), dict(nlevels=65), dict(nlevels=-1), dict(min_inliers=0), dict(min_inliers=-2),
           dict(max_iterations=0), dict(new_iterations=0), dict(new_iterations=-5), dict(probability=0.0), dict(probability=1.0), dict(probability=-0.5), dict(probability=1.5),
           dict(probability=float("nan")), dict(npairs=1 << 20, cap=2048), dict(nkeyframes=1 << 20, cap=2048), dict(d_sets=b.d["sets"], npairs=1 << 10, max_iterations=1 << 18)]
    for k in bad:
        with pytest.raises(fe.SslamError) as e:
            ctx.sim3_ransac_batch_dev(**dict(good, **k))
        assert e.value.code == fe.SSLAM_ERR_INVALID, k
    with pytest.raises(fe.SslamError) as e:
        fe._chk(fe.lib().sslam_sim3_ransac_batch_dev(None, *[C.c_void_p(0)] * 4, 16, 2, C.c_void_p(0), C.c_void_p(0), 8, C.c_void_p(0), 1, C.c_void_p(0), 0, C.c_double(0.99), 8, 4, 4,
                                                     C.c_void_p(0), C.c_uint32(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)))
    assert e.value.code == fe.SSLAM_ERR_INVALID
    ctx.sim3_ransac_batch_dev(**dict(good, npairs=0))                      # OK, and enqueues nothing
    ctx.synchronize()
    assert b.untouched(s0)
    kp1, kp2 = keypoints(fe, c["kf1"]["oct"], np.random.default_rng(3)), keypoints(fe, c["kf2"]["oct"], np.random.default_rng(4))
    a = (kp1, c["kf1"]["x3dc"], c["kf1"]["valid"], c["kf1"]["K"], kp2, c["kf2"]["x3dc"], c["kf2"]["valid"], c["kf2"]["K"], tc.SIGMA2, c["m12"])
    for k in (dict(min_inliers=0), dict(max_iterations=0), dict(new_iterations=0), dict(probability=1.0), dict(probability=0.0)):
        with pytest.raises(fe.SslamError) as e:
            ctx.sim3_ransac(*a, **k)
        assert e.value.code == fe.SSLAM_ERR_INVALID, k
    with pytest.raises(fe.SslamError) as e:
        ctx.sim3_ransac(kp1, c["kf1"]["x3dc"], None, c["kf1"]["K"], kp2, c["kf2"]["x3dc"], c["kf2"]["valid"], c["kf2"]["K"], tc.SIGMA2, c["m12"])      # one validity array only
    assert e.value.code == fe.SSLAM_ERR_INVALID


def test_behind_search_by_bow(fe, ctx):
    """ORB on the ICL frame; keyframe 1 holds its keypoints back-projected at a synthetic depth, keyframe 2 the same features in another row order with the same points under a
    known similarity; SearchByBoW between the two slots on the device (node ids: one node per 25 features), this call on its d_matches12 where it lies"""
    gray = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icl_input_gray.npz"))["gray"]
    ex = fe.OrbExtractor(ctx, 1000, 1.2, 8, 20, 7)
    kp, desc = ex(gray)
    ex.close()
    n = len(kp)
    rng = np.random.default_rng(2026)
    perm = rng.permutation(n)
    K = np.array([481.2, 480.0, 319.5, 239.5], np.float32)
    depth = 2.0 + 0.5 * (np.arange(n) % 7)
    X1 = np.stack([(kp["x"] - K[2]) / K[0] * depth, (kp["y"] - K[3]) / K[1] * depth, depth], 1)
    X2 = (((X1 - tc.T_TRUE) @ tc.R_TRUE) / tc.S_TRUE)[perm]
    node = (np.arange(n) // 25).astype(np.int32)
    cap = n + 5
    KP = np.zeros((2, cap), fe.KP_DTYPE); D = np.zeros((2, cap, 32), np.uint8); ND = np.full((2, cap), -1, np.int32); X = np.zeros((2, cap, 3), np.float32)
    KP[0, :n] = kp; KP[1, :n] = kp[perm]; D[0, :n] = desc; D[1, :n] = desc[perm]; ND[0, :n] = node; ND[1, :n] = node[perm]; X[0, :n] = X1; X[1, :n] = X2
    valid = np.ones((2, cap), np.uint8)
    g = dict(kp=dev(KP), desc=dev(D), node=dev(ND), valid=dev(valid), n=dev(np.full(2, n, np.int32)), x=dev(X), K=dev(np.stack([K, K])), pairs=dev(np.array([[0, 1], [1, 0]], np.int32)))
    m12 = torch.full((2, cap), -7, dtype=torch.int32, device="cuda"); m21 = torch.full((2, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    state = torch.zeros(2 * 84, dtype=torch.uint8, device="cuda"); inl = torch.full((2 * cap,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.search_by_bow_keyframes_batch_dev(g["kp"], g["desc"], g["node"], g["n"], cap, 2, g["pairs"], 2, m12, m21, nm, d_valid=g["valid"], nnratio=0.75, check_orientation=True)
    kw = dict(fix_scale=False, probability=0.99, min_inliers=20, max_iterations=300, seed=2026)
    ctx.sim3_ransac_batch_dev(g["kp"], g["x"], g["valid"], g["n"], cap, 2, g["K"], tc.SIGMA2, g["pairs"], 2, m12, state, inl, new_iterations=5, **kw)      # same stream, no copy in between
    ctx.synchronize()
    m = m12.cpu().numpy(); got = state.cpu().numpy().view(fe.SIM3_STATE_DTYPE); gi = inl.cpu().numpy().reshape(2, cap)
    assert nm.cpu().numpy().min() >= 20                                      # LoopClosing's own threshold (src/LoopClosing.cc:271)
    slot = [dict(oct=KP[k, :n]["octave"].astype(np.int32), valid=valid[k, :n], x3dc=X[k, :n], K=K) for k in (0, 1)]
    want = sim.run([dict(kf1=slot[a], kf2=slot[b], sigma2=tc.SIGMA2, m12=m[p, :n], pair=p, sets=None, calls=[5], **kw) for p, (a, b) in enumerate(((0, 1), (1, 0)))])
    for p in range(2):
        w = want[p]["calls"][0]
        assert same_state(got[p], w["state"]), (p, got[p], w["state"])
        np.testing.assert_array_equal(gi[p, :n], w["inliers"])
        assert (gi[p, n:] == FILL).all()
    assert got[0]["found_it"] >= 0 and got[0]["n_inliers"] > 20 and abs(got[0]["s12"] - tc.S_TRUE) < 1e-2 and np.abs(got[0]["R12"].reshape(3, 3) - tc.R_TRUE).max() < 1e-2
