"""GPU parity of sslam_pnp_ransac / sslam_pnp_ransac_batch_dev (PnPsolver, reference src/PnPsolver.cc: the RANSAC of Tracking::Relocalization) with the host model of the
same header: tests/pnp_sim.py runs csrc/pnp_math.h under g++.  Every comparison is bit for bit (a NaN equals a NaN), and through the testing tap it covers EVERY iteration
the reference's loop ran -- set, R, t, the count, the chosen N, rep_errors, betas, whether Refine ran and its count.  The cases are tests/pnp_cases.py's.

  test_single_call_and_every_hypothesis   every case, call after call on one state, through sslam_pnp_ransac and through sslam_testing_pnp_hypotheses
  test_batch_of_two                       every case as pairs 0 and 1 of a batch (NULL pair arrays), call after call on the device-resident states: pair 0 equals the single
                                          call, pair 1 draws other sets; 0xA5 behind every count and behind the last pair
  test_batch_of_70                        one launch on a side stream: one frame slot against 20 keyframe slots, given pair arrays, two skipped pairs
  test_caps_and_size_bound                capacities 1000 and 2048; 2049 is SSLAM_ERR_UNSUPPORTED with nothing written
  test_table_rebuilds_in_stream_order     calls that alternate between two parameter sets and two streams without a synchronise in between
  test_argument_errors                    every refused combination: SSLAM_ERR_INVALID, nothing enqueued, the outputs left alone
  test_behind_bow_transform_and_search_by_bow   the Relocalization chain on the ICL frame of tests/golden/icl_input_gray.npz
No test here sets a time limit of its own, as the older RANSAC tests do not: a launch is one wave per pair for at most 130 iterations, and the limit is that of whatever
runs the suite."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch
import pnp_cases as tc
import pnp_sim as sim

pytestmark = pytest.mark.gpu

FILL = 0xA5
INTS = ("its_done", "best_inliers", "best_it", "refine_ok", "n", "min_inliers", "max_its", "found", "found_it", "n_inliers", "no_more")
BOUND = 2048


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def same_state(got, want):
    return all(int(got[k]) == int(want[k]) for k in INTS) and all(same_bits(got[k], want[k]) for k in ("best_R", "best_t", "Tcw"))


@functools.lru_cache(maxsize=None)
def cases():
    B = tc.build()
    names = list(B)
    cs = [tc.public(B[n]) for n in names]
    return names, cs, sim.run(cs)


def keypoints(fe, c, rng):
    """KP_DTYPE rows with the case's points and octaves; the fields the call must not read hold junk"""
    kp = rng.integers(0, 256, (len(c["oct"]), fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(-1)
    kp["octave"] = c["oct"]; kp["x"] = c["pt"][:, 0]; kp["y"] = c["pt"][:, 1]
    return kp


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def params(c):
    return dict(probability=c["probability"], min_inliers=c["min_inliers"], max_iterations=c["max_iterations"], epsilon=c["epsilon"], th2=c["th2"], seed=c["seed"])


def tap_rows(c):
    return max(c["max_iterations"], 1) + sum(c["calls"]) + 1


def tap(fe, ctx, c, kp, state, new_iterations, pair=0):
    rows = tap_rows(c)
    st = np.zeros(1, fe.PNP_STATE_DTYPE); st[0] = state
    inl = np.zeros(len(kp), np.uint8)
    sets = np.full((rows, 4), -9, np.int32); poses = np.full((rows, 12), -9, np.float64); counts = np.full((rows, 4), -9, np.int32); trace = np.full((rows, 15), -9, np.float64)
    p = lambda a: None if a is None else C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    hold = [np.ascontiguousarray(c["K"], np.float32), np.ascontiguousarray(c["xw"], np.float32), np.ascontiguousarray(c["valid"], np.uint8),
            np.ascontiguousarray(c["sigma2"], np.float32), np.ascontiguousarray(c["assigned"], np.int32)]
    cs = None if c["sets"] is None else np.ascontiguousarray(c["sets"], np.int32)
    rc = fe.testing_lib().sslam_testing_pnp_hypotheses(ctx.h, p(kp), len(kp), p(hold[0]), p(hold[1]), p(hold[2]), len(hold[1]), p(hold[3]), len(hold[3]), p(hold[4]),
                                                       C.c_double(c["probability"]), c["min_inliers"], c["max_iterations"], C.c_float(c["epsilon"]), C.c_float(c["th2"]),
                                                       int(new_iterations), p(cs), 0 if cs is None else len(cs), C.c_uint32(c["seed"]), int(pair), p(st), p(inl), rows,
                                                       p(sets), p(poses), p(counts), p(trace))
    assert rc == 0, fe.testing_lib().sslam_last_error()
    return st[0], inl, sets, poses, counts, trace


def check_tap(name, got, want, rows):
    st, inl, sets, poses, counts, trace = got
    assert same_state(st, want["state"]), (name, st, want["state"])
    np.testing.assert_array_equal(inl, want["inliers"], err_msg=name)
    ran = np.zeros(rows, bool); ran[want["its"]] = True
    np.testing.assert_array_equal(sets[ran], want["sets"], err_msg=name)
    np.testing.assert_array_equal(counts[ran], want["counts"], err_msg=name)
    for j, it in enumerate(want["its"]):
        assert same_bits(poses[it], want["poses"][j]), (name, it, poses[it], want["poses"][j])
        assert same_bits(trace[it], want["trace"][j]), (name, it, trace[it], want["trace"][j])
    assert not sets[~ran].any() and not poses[~ran].any() and not counts[~ran].any() and not trace[~ran].any(), name      # iterations this call did not run stay zero


def test_single_call_and_every_hypothesis(fe, ctx):
    rng = np.random.default_rng(1)
    names, cs, wants = cases()
    for name, c, want in zip(names, cs, wants):
        kp = keypoints(fe, c, rng)
        st = ts = None
        for new_its, w in zip(c["calls"], want["calls"]):
            st, inl = ctx.pnp_ransac(kp, c["K"], c["xw"], c["valid"], c["sigma2"], c["assigned"], state=st, new_iterations=new_its, sets=c["sets"], **params(c))
            assert same_state(st, w["state"]), (name, st, w["state"])
            np.testing.assert_array_equal(inl, w["inliers"], err_msg=name)
            got = tap(fe, ctx, c, kp, np.zeros(1, fe.PNP_STATE_DTYPE)[0] if ts is None else ts, new_its)
            check_tap(name, got, w, tap_rows(c))
            ts = got[0]


class Pool:
    """frame slots, keyframe slots and a pair list on the device (junk behind every count), states and inlier rows of one pair more than the call may touch.
    frames / keyframes: cases (their frame side / keyframe side is used); pairs: (kf, f, assigned int32 [nf] or None for a skipped pair)"""
    def __init__(self, fe, frames, keyframes, pairs, cap, kfcap, seed=5, sets=None, null_pairs=False, all_valid=False):
        rng = np.random.default_rng(seed)
        F, Kn, P = len(frames), len(keyframes), len(pairs)
        self.fe, self.frames, self.keyframes, self.pairs, self.cap, self.kfcap, self.F, self.K, self.P = fe, frames, keyframes, pairs, cap, kfcap, F, Kn, P
        kp = rng.integers(0, 256, (F, cap, fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(F, cap)
        kp["octave"] = rng.integers(0, len(tc.SIGMA2), (F, cap))      # in range behind the counts too: a row read there would count
        fK = np.zeros((F, 4), np.float32)
        self.nf = np.array([len(c["oct"]) for c in frames], np.int32)
        for f, c in enumerate(frames):
            kp[f, :self.nf[f]] = keypoints(fe, c, rng); fK[f] = c["K"]
        xw = rng.normal(0, 3, (Kn, kfcap, 3)).astype(np.float32); valid = rng.integers(0, 2, (Kn, kfcap)).astype(np.uint8)
        self.nkf = np.array([len(c["xw"]) for c in keyframes], np.int32)
        for k, c in enumerate(keyframes):
            xw[k, :self.nkf[k]] = c["xw"]; valid[k, :self.nkf[k]] = 1 if all_valid else c["valid"]
        asg = rng.integers(-5, kfcap + 5, (P, cap)).astype(np.int32)
        pk = np.zeros(P, np.int32); pf = np.zeros(P, np.int32)
        st = np.zeros(P + 1, fe.PNP_STATE_DTYPE)
        st.view(np.uint8)[-192:] = FILL
        for p, (k, f, a) in enumerate(pairs):
            pk[p], pf[p] = k, f
            if a is None:
                st.view(np.uint8).reshape(P + 1, 192)[p] = FILL
            else:
                asg[p, :self.nf[f]] = a
        self.d = dict(kp=dev(kp), nf=dev(self.nf), fK=dev(fK), xw=dev(xw), valid=None if all_valid else dev(valid), nkf=dev(self.nkf), asg=dev(asg),
                      pk=None if null_pairs else dev(pk), pf=None if null_pairs else dev(pf), sets=None if sets is None else dev(np.ascontiguousarray(sets, np.int32)))
        self.nsets = 0 if sets is None else np.asarray(sets).shape[1]
        self.state = dev(st)
        self.inl = torch.full(((P + 1) * cap,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def launch(self, ctx, new_iterations, stream=None, cap=None, sigma2=None, **kw):
        d = self.d
        ctx.pnp_ransac_batch_dev(d["kp"], d["nf"], self.cap if cap is None else cap, self.F, d["fK"], d["xw"], d["valid"], d["nkf"], self.kfcap, self.K,
                                 tc.SIGMA2 if sigma2 is None else sigma2, d["pk"], d["pf"],
                                 self.P, d["asg"], self.state, self.inl, d_sets=d["sets"], nsets=self.nsets, new_iterations=new_iterations, stream=stream, **kw)
        return self

    def results(self):
        return self.state.cpu().numpy().view(self.fe.PNP_STATE_DTYPE), self.inl.cpu().numpy().reshape(self.P + 1, self.cap)

    def check(self, want, call=0, names=None):
        """want[p]: the sim's answer of pair p (its `call`-th call), None for a skipped pair"""
        st, inl = self.results()
        raw = st.view(np.uint8).reshape(self.P + 1, 192)
        for p, (k, f, a) in enumerate(self.pairs):
            tag = (p, None if names is None else names[p])
            if a is None:
                assert [int(st[p][x]) for x in ("n", "min_inliers", "max_its", "found", "found_it", "n_inliers", "no_more")] == [0, 0, 0, 0, -1, 0, 1], tag
                assert (raw[p, :16] == FILL).all() and (raw[p, 44:] == FILL).all() and (inl[p] == FILL).all(), tag      # nothing else of a skipped pair is written
                continue
            w = want[p]["calls"][call]
            assert same_state(st[p], w["state"]), (tag, st[p], w["state"])
            nf = self.nf[f]
            np.testing.assert_array_equal(inl[p, :nf], w["inliers"], err_msg=str(tag))
            assert (inl[p, nf:] == FILL).all(), tag
        assert (raw[self.P] == FILL).all() and (inl[self.P] == FILL).all()


def test_batch_of_two(fe, ctx):
    names, cs, wants = cases()
    for name, c, want in zip(names, cs, wants):
        c1 = dict(c, pair=1)
        w1 = sim.run_plain([c1])[0] if c["sets"] is None else want
        sets = None if c["sets"] is None else np.stack([c["sets"], c["sets"]])
        cap, kfcap = len(c["oct"]) + 3, len(c["xw"]) + 2
        pool = Pool(fe, [c, c], [c, c], [(0, 0, c["assigned"]), (1, 1, c["assigned"])], cap, kfcap, sets=sets, null_pairs=True)
        for call, new_its in enumerate(c["calls"]):
            pool.launch(ctx, new_its, sigma2=c["sigma2"], **params(c))
            torch.cuda.synchronize()
            pool.check([want, w1], call, names=[name, name])


def test_batch_of_70(fe, ctx):
    names, cs, wants = cases()
    drawn = [(n, c) for n, c in zip(names, cs) if c["sets"] is None and len(c["oct"]) > 0]
    name, frame = drawn[-1]      # the mixed scene: one frame slot ...
    rng = np.random.default_rng(7)
    keyframes, pairs, sim_cases = [], [], []
    nkf = len(frame["xw"])
    for k in range(20):      # ... against 20 keyframe slots: the frame's own map points under a permutation of the rows, every third slot with points of its own
        perm = rng.permutation(nkf)
        keyframes.append(dict(frame, xw=frame["xw"][perm] if k % 3 else rng.normal(0, 3, frame["xw"].shape).astype(np.float32), valid=frame["valid"][perm], _inv=np.argsort(perm)))
    P = 70
    for p in range(P):
        if p in (13, 64):
            pairs.append((20 if p == 13 else -1, 0, None)); sim_cases.append(None)
            continue
        k = int(rng.integers(0, 20))
        a = frame["assigned"].copy()
        ok = (a >= 0) & (a < nkf)
        a[ok] = keyframes[k]["_inv"][a[ok]]      # row r of the frame's own keyframe side sits at row inv[r] of slot k
        pairs.append((k, 0, a))
        sim_cases.append(dict(frame, xw=keyframes[k]["xw"], valid=keyframes[k]["valid"], assigned=a, pair=p, calls=[5]))
    cap, kfcap = len(frame["oct"]) + 7, len(frame["xw"]) + 5
    pool = Pool(fe, [frame], keyframes, pairs, cap, kfcap)
    live = [c for c in sim_cases if c is not None]
    answers = iter(sim.run(live))
    want = [None if c is None else next(answers) for c in sim_cases]
    side = torch.cuda.Stream()
    pool.launch(ctx, 5, stream=side.cuda_stream, **params(frame))
    side.synchronize()
    pool.check(want, 0)
    assert any(w is not None and w["calls"][0]["state"]["found"] == 1 for w in want)


def test_caps_and_size_bound(fe, ctx):
    names, cs, wants = cases()
    i = names.index("refine_fails_then_equal_then_best")
    c, want = cs[i], wants[i]
    sets = c["sets"][None]
    for cap in (1000, BOUND):
        pool = Pool(fe, [c], [c], [(0, 0, c["assigned"])], cap, len(c["xw"]), sets=sets)
        pool.launch(ctx, c["calls"][0], **params(c))
        torch.cuda.synchronize()
        pool.check([want], 0)
    pool = Pool(fe, [c], [c], [(0, 0, c["assigned"])], BOUND + 1, len(c["xw"]), sets=sets)
    with pytest.raises(fe.SslamError) as e:
        pool.launch(ctx, 5, **params(c))
    assert "exceeds the supported 2048" in str(e.value)
    torch.cuda.synchronize()
    st, inl = pool.results()
    assert not st.view(np.uint8)[:192].any() and (inl == FILL).all()      # nothing written


def test_table_rebuilds_in_stream_order(fe, ctx):
    names, cs, wants = cases()
    picks = [names.index("refine_fails_then_equal_then_best"), names.index("epsilon_above_min")]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pools = []
    for rep in range(3):
        for j, i in enumerate(picks):
            c = cs[i]
            pool = Pool(fe, [c], [c], [(0, 0, c["assigned"])], len(c["oct"]) + 1, len(c["xw"]), sets=c["sets"][None], seed=rep)
            pool.launch(ctx, c["calls"][0], stream=streams[(rep + j) % 2].cuda_stream, **params(c))      # another key than the call before it, no synchronise in between
            pools.append((pool, wants[i]))
    torch.cuda.synchronize()
    for pool, want in pools:
        pool.check([want], 0)


def test_argument_errors(fe, ctx):
    names, cs, wants = cases()
    c = cs[names.index("refine_at_0")]
    pool = Pool(fe, [c], [c], [(0, 0, c["assigned"])], len(c["oct"]), len(c["xw"]), sets=c["sets"][None])
    d = pool.d
    good = dict(d_f_kp=d["kp"], d_nf=d["nf"], cap=pool.cap, nframes=1, d_f_K=d["fK"], d_kf_xw=d["xw"], d_kf_valid=d["valid"], d_nkf=d["nkf"], kfcap=pool.kfcap, nkeyframes=1,
                level_sigma2=tc.SIGMA2, d_pair_kf=d["pk"], d_pair_f=d["pf"], npairs=1, d_assigned=d["asg"], d_state=pool.state, d_inliers=pool.inl, d_sets=d["sets"], nsets=pool.nsets,
                new_iterations=5, **params(c))
    off = lambda t, k: t.data_ptr() + k
    bad = [dict(d_f_kp=None), dict(d_nf=None), dict(d_f_K=None), dict(d_kf_xw=None), dict(d_nkf=None), dict(d_assigned=None), dict(d_state=None), dict(d_inliers=None),
           dict(level_sigma2=None), dict(nlevels=0), dict(nlevels=65), dict(probability=0.0), dict(probability=1.0), dict(probability=float("nan")), dict(min_inliers=0),
           dict(max_iterations=0), dict(new_iterations=0), dict(epsilon=0.0), dict(epsilon=1.0000001), dict(epsilon=float("nan")), dict(th2=0.0), dict(th2=-1.0),
           dict(th2=float("nan")), dict(cap=0), dict(kfcap=0), dict(npairs=-1), dict(nframes=-1), dict(nkeyframes=-1), dict(npairs=1 << 21, cap=1 << 10),
           dict(nframes=1 << 21, cap=1 << 10), dict(nkeyframes=1 << 21, kfcap=1 << 10), dict(npairs=1 << 14, nsets=1 << 14), dict(nsets=-1),
           dict(d_pair_kf=None, nkeyframes=2), dict(d_pair_f=None, nframes=2),
           dict(d_f_kp=off(d["kp"], 2)), dict(d_f_K=off(d["fK"], 2)), dict(d_kf_xw=off(d["xw"], 1)), dict(d_nf=off(d["nf"], 2)), dict(d_nkf=off(d["nkf"], 1)),
           dict(d_pair_kf=off(d["pk"], 2)), dict(d_pair_f=off(d["pf"], 2)), dict(d_assigned=off(d["asg"], 2)), dict(d_sets=off(d["sets"], 2)), dict(d_state=off(pool.state, 4))]
    before = pool.results()
    for b in bad:
        kw = dict(good, **b)
        with pytest.raises(fe.SslamError) as e:
            ctx.pnp_ransac_batch_dev(**kw)
        assert "invalid arguments" in str(e.value), b
    torch.cuda.synchronize()
    after = pool.results()
    assert np.array_equal(before[0].view(np.uint8), after[0].view(np.uint8)) and np.array_equal(before[1], after[1])
    ctx.pnp_ransac_batch_dev(**dict(good, npairs=0, d_pair_kf=None, d_pair_f=None, nframes=0, nkeyframes=0))      # nothing to do is no error
    ctx.pnp_ransac_batch_dev(**good)
    torch.cuda.synchronize()
    assert same_state(pool.results()[0][0], wants[names.index("refine_at_0")]["calls"][0]["state"])


def test_behind_bow_transform_and_search_by_bow(fe, ctx):
    """The Relocalization chain on the ICL frame: sslam_bow_transform_batch_dev -> sslam_orb_search_by_bow_batch_dev -> this call, on one stream with no copy in between.
    The keyframe slot holds the frame's own features in another row order; its world points are the keypoints back-projected at a synthetic depth under a known pose"""
    import os
    from synth import synthetic_vocab
    gray = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icl_input_gray.npz"))["gray"]
    ex = fe.OrbExtractor(ctx, 1000, 1.2, 8, 20, 7)
    kp, desc = ex(gray)
    ex.close()
    n = len(kp)
    rng = np.random.default_rng(2026)
    perm = rng.permutation(n)
    K = np.array([481.2, 480.0, 319.5, 239.5], np.float32)
    R, t = tc._pose(np.random.RandomState(3), 0.4)
    depth = 2.0 + 0.5 * (np.arange(n) % 7)
    Xc = np.stack([(kp["x"] - K[2]) / K[0] * depth, (kp["y"] - K[3]) / K[1] * depth, depth], 1)
    Xw = ((Xc - t) @ R).astype(np.float32)      # Xc = R Xw + t
    L, ptr, ch, nd, word, weight = synthetic_vocab(np.random.default_rng(5), k=10, L=4)
    voc = fe.Vocabulary(ctx, L, ptr, ch, nd, word, weight)
    cap = n + 5
    FKP = np.zeros((1, cap), fe.KP_DTYPE); KKP = np.zeros((1, cap), fe.KP_DTYPE); FD = np.zeros((1, cap, 32), np.uint8); KD = np.zeros((1, cap, 32), np.uint8)
    X = np.zeros((1, cap, 3), np.float32)
    FKP[0, :n] = kp; FD[0, :n] = desc; KKP[0, :n] = kp[perm]; KD[0, :n] = desc[perm]; X[0, :n] = Xw[perm]
    g = dict(fkp=dev(FKP), fd=dev(FD), kkp=dev(KKP), kd=dev(KD), x=dev(X), n=dev(np.full(1, n, np.int32)), K=dev(K[None]), valid=dev(np.ones((1, cap), np.uint8)))
    fnode = torch.full((cap,), -7, dtype=torch.int32, device="cuda"); knode = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    asg = torch.full((cap,), -7, dtype=torch.int32, device="cuda"); nm = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    state = torch.zeros(192, dtype=torch.uint8, device="cuda"); inl = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kw = dict(probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, seed=2026)      # Tracking's own parameters (src/Tracking.cc:2005)
    ctx.bow_transform_batch_dev(voc, g["fd"], g["n"], cap, 1, fnode, levelsup=2)
    ctx.bow_transform_batch_dev(voc, g["kd"], g["n"], cap, 1, knode, levelsup=2)
    ctx.search_by_bow_batch_dev(g["kkp"], g["kd"], knode, g["valid"], g["n"], cap, 1, g["fkp"], g["fd"], fnode, g["n"], cap, 1, 1, asg, nm, nnratio=0.75, check_orientation=True)
    ctx.pnp_ransac_batch_dev(g["fkp"], g["n"], cap, 1, g["K"], g["x"], g["valid"], g["n"], cap, 1, tc.SIGMA2, None, None, 1, asg, state, inl, new_iterations=5, **kw)
    ctx.synchronize()
    voc.close()
    a = asg.cpu().numpy(); got = state.cpu().numpy().view(fe.PNP_STATE_DTYPE)[0]; gi = inl.cpu().numpy()
    assert int(nm.cpu().numpy()[0]) >= 15                                     # Relocalization's own threshold (src/Tracking.cc:1997)
    c = dict(oct=kp["octave"].astype(np.int32), pt=np.stack([kp["x"], kp["y"]], 1).astype(np.float32), K=K, xw=Xw[perm], valid=np.ones(n, np.uint8), assigned=a[:n],
             sigma2=tc.SIGMA2, calls=[5], sets=None, pair=0, **kw)
    w = sim.run([c])[0]["calls"][0]
    assert same_state(got, w["state"]), (got, w["state"])
    np.testing.assert_array_equal(gi[:n], w["inliers"])
    assert (gi[n:] == FILL).all()
    true = np.hstack([R, t[:, None]]).ravel()
    assert got["found"] == 1 and got["n_inliers"] > 100 and np.abs(got["Tcw"].astype(np.float64) - true).max() < 1e-3
