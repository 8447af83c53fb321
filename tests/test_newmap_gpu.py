"""GPU parity of sslam_new_map_points* / sslam_new_map_lines* (the loop bodies of LocalMapping::CreateNewMapPoints and CreateNewMapLines2 with the first
UpdateNormalAndDepth / UpdateAverageDir, reference src/LocalMapping.cc:456-635 and :1005-1170) with the host model tests/newmap_sim.py (csrc/newmap_math.h compiled for the
host), whose own parity with the reference's lines is tests/test_newmap_ref_cpu.py.  Every comparison is bit for bit; a NaN equals a NaN (its sign and payload are the
processor's).  Rows past every count hold random bytes; the outputs hold 0xA5 before every call.

  test_point_cases_batch / test_line_cases_batch    every case of tests/newmap_cases.py as a pair with two slots of its own, the cases that share level tables in one launch;
                                                    rows at or past a count keep the fill; the free flags of created rows are cleared and no other
  test_point_cases_single_and_tap / test_line_...   every case through the single call and through the tap (the cosine and the homogeneous vectors)
  test_mixed_point_pairs / test_mixed_line_pairs    70 pairs of one pool in one launch: ragged counts, one keyframe against 20 neighbours, (a, b) beside (b, a), slots out of
                                                    range and kf1 == kf2 (count -1, every other word keeps the fill)
  test_point_rounds_on_one_stream                   three rounds of sslam_orb_search_for_triangulation_batch_dev + sslam_new_map_points_batch_dev on one stream with one
                                                    d_free and no synchronise in between = the host replay that updates the flags between rounds, != the one that does not
  test_line_rounds_on_one_stream                    one sslam_line_match_batch_dev, then three rounds of sslam_new_map_lines_batch_dev with d_lfree, likewise
  test_chain_on_image_features                      ORB and line features of the ICL frame and a shifted crop of it, made-up poses: d_matches12 and d_pairs are consumed where
                                                    the matchers left them
  test_argument_errors                              every refused argument is SSLAM_ERR_INVALID and leaves the outputs at the fill; npairs == 0 is SSLAM_OK"""
import ctypes as C
import os
import numpy as np
import pytest
import torch
import bow_batch_cases as bc
import newmap_cases as nc
import newmap_sim as sim
import pkg
import tri_batch_cases as tc

pytestmark = pytest.mark.gpu

FILL = 0xA5
SENT = np.frombuffer(bytes([FILL] * 4), np.int32)[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def filled(nbytes):
    return torch.full((int(nbytes),), FILL, dtype=torch.uint8, device="cuda")


def host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def same(a, b, msg):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (msg, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        np.testing.assert_array_equal(na, nb, err_msg=msg)
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        np.testing.assert_array_equal(a.view(u)[~na], b.view(u)[~nb], err_msg=msg)
    else:
        np.testing.assert_array_equal(a, b, err_msg=msg)


def keeps_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def kp_rows(fe, xy, octave):
    k = np.zeros(len(octave), fe.KP_DTYPE)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k["x"], k["y"], k["octave"], k["size"] = xy[:, 0], xy[:, 1], octave, 31
    return k


def kl_rows(fe, kl, octave):
    k = np.zeros(len(octave), fe.KL_DTYPE)
    kl = np.asarray(kl, np.float32).reshape(-1, 4)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"], k["octave"] = kl[:, 0], kl[:, 1], kl[:, 2], kl[:, 3], octave
    return k


def pair_rows(fe, pairs, medians=None):
    out = np.zeros(len(pairs), fe.NEWMAP_PAIR_DTYPE)
    for p, (a, b) in enumerate(pairs):
        out[p] = (a, b, 0.0 if medians is None else medians[p])
    return out


class PointCall:
    """one sslam_new_map_points_batch_dev: a pool of keyframes [(xy, octave)] with their poses, pairs [(kf1, kf2)] and per pair the matches12 row (None: junk);
    outputs with one pair more than the call may write"""
    def __init__(self, fe, kfs, poses, cap, pairs, m12s, with_free=True, seed=7, npairs=None):
        rng = np.random.default_rng(seed)
        S, P = len(kfs), len(pairs)
        self.cap, self.S, self.P, self.npairs = cap, S, P, P if npairs is None else npairs
        kp = bc.junk(rng, (S, cap), fe.KP_DTYPE); n = np.zeros(S, np.int32)
        self.free0 = bc.junk(rng, (S, cap), np.uint8)
        for k, (xy, oc) in enumerate(kfs):
            n[k] = len(oc); kp[k, :n[k]] = kp_rows(fe, xy, oc); self.free0[k, :n[k]] = 1
        m = bc.junk(rng, (P + 1, cap), np.int32)
        for p, row in enumerate(m12s):
            if row is not None: m[p, :len(row)] = row
        self.n = n
        self.d = dict(kp=dev(kp), n=dev(n), pose=dev(np.asarray(poses, np.float32)), pairs=dev(pair_rows(fe, list(pairs) + [(0, 1)])), m12=dev(m),
                      free=dev(self.free0) if with_free else None)
        R = (P + 1) * cap
        self.o = dict(x3d=filled(12 * R), stage=filled(R), normal=filled(12 * R), dist=filled(8 * R), nnew=filled(4 * (P + 1)))
        torch.cuda.synchronize()

    def launch(self, ctx, sf=nc.SF, sigma2=nc.SIGMA2, scale_factor=nc.SCALE_FACTOR, stream=None, **kw):
        a = dict(d_kp=self.d["kp"], d_n=self.d["n"], cap=self.cap, nkeyframes=self.S, d_pose=self.d["pose"], d_pairs=self.d["pairs"], npairs=self.npairs, d_matches12=self.d["m12"],
                 scale_factors=sf, level_sigma2=sigma2, scale_factor=scale_factor, d_x3d=self.o["x3d"], d_stage=self.o["stage"], d_normal=self.o["normal"], d_dist=self.o["dist"],
                 d_nnew=self.o["nnew"], d_free=self.d["free"], stream=stream)
        a.update(kw)
        ctx.new_map_points_batch_dev(**a)
        return self

    def results(self):
        P, cap = self.P + 1, self.cap
        r = dict(x3d=host(self.o["x3d"], np.float32, (P, cap, 3)), stage=host(self.o["stage"], np.uint8, (P, cap)), normal=host(self.o["normal"], np.float32, (P, cap, 3)),
                 dist=host(self.o["dist"], np.float32, (P, cap, 2)), nnew=host(self.o["nnew"], np.int32, (P,)))
        if self.d["free"] is not None: r["free"] = host(self.d["free"], np.uint8, (self.S, cap))
        return r

    def untouched(self):
        return all(keeps_fill(v) for k, v in self.results().items() if k != "free") and (self.d["free"] is None or (self.results()["free"] == self.free0).all())


POINT_OUT, LINE_OUT = ("x3d", "stage", "normal", "dist"), ("s3d", "e3d", "stage", "normal", "dist")


def check_pairs(res, wants, counts, keys, free0=None, clears=None):
    """pair p against wants[p] (the model's answer for its first counts[p] rows; None: a skipped pair), the fill everywhere else; free0 / clears: the flags before the call
    and [(slot, row)] of every created row's two features"""
    for p, w in enumerate(wants):
        if w is None:
            assert res["nnew"][p] == -1, (p, res["nnew"][p])
            assert all(keeps_fill(res[k][p]) for k in keys), p
            continue
        n = counts[p]
        for k in keys:
            same(res[k][p, :n], w[k], "pair %d %s" % (p, k))
            assert keeps_fill(res[k][p, n:]), (p, k)
        assert res["nnew"][p] == w["nnew"], (p, res["nnew"][p], w["nnew"])
    for k in keys:
        assert keeps_fill(res[k][len(wants):]), k
    assert keeps_fill(res["nnew"][len(wants):])
    if free0 is not None:
        want = free0.copy()
        for s, i in clears: want[s, i] = 0
        np.testing.assert_array_equal(res["free"], want)


def point_clears(pairs, m12s, wants):
    out = []
    for (a, b), m, w in zip(pairs, m12s, wants):
        if w is None: continue
        for i in np.nonzero(w["stage"] == 0)[0]: out += [(a, int(i)), (b, int(m[i]))]
    return out


def line_clears(pairs, lps, wants):
    out = []
    for (a, b), lp, w in zip(pairs, lps, wants):
        if w is None: continue
        for r in np.nonzero(w["stage"] == 0)[0]: out += [(a, int(lp[r, 0])), (b, int(lp[r, 1]))]
    return out


def groups(cases, keys):
    g = {}
    for c in cases:
        g.setdefault(tuple(np.asarray(c[k]).tobytes() for k in keys), []).append(c)
    return list(g.values())


@pytest.fixture(scope="module")
def model():
    cases = nc.all_cases()
    return {c["name"]: r for c, r in zip(cases, sim.run(list(cases)))}


def test_point_cases_batch(fe, ctx, model):
    ran = 0
    for grp in groups(nc.point_cases(), ("sf", "sigma2")):
        kfs = [k for c in grp for k in ((c["kp1"], c["oct1"]), (c["kp2"], c["oct2"]))]
        poses = [p for c in grp for p in (c["pose1"], c["pose2"])]
        pairs = [(2 * p, 2 * p + 1) for p in range(len(grp))]
        cap = max(len(k[1]) for k in kfs)
        assert cap <= 640
        call = PointCall(fe, kfs, poses, cap, pairs, [c["m12"] for c in grp]).launch(ctx, grp[0]["sf"], grp[0]["sigma2"], grp[0]["scale_factor"])
        ctx.synchronize()
        wants = [model[c["name"]] for c in grp]
        check_pairs(call.results(), wants, [len(c["oct1"]) for c in grp], POINT_OUT, call.free0, point_clears(pairs, [c["m12"] for c in grp], wants))
        ran += len(grp)
    assert ran == len(nc.point_cases()) >= 16


def test_point_cases_single_and_tap(fe, ctx, model):
    for c in nc.point_cases():
        w = model[c["name"]]
        for tap in (False, True):
            o = ctx.new_map_points(kp_rows(fe, c["kp1"], c["oct1"]), kp_rows(fe, c["kp2"], c["oct2"]), c["pose1"], c["pose2"], c["m12"], c["sf"], c["sigma2"], c["scale_factor"], tap=tap)
            for k in POINT_OUT + (("cos", "hom") if tap else ()):
                same(o[k], w[k], "%s %s tap=%d" % (c["name"], k, tap))
            assert o["nnew"] == w["nnew"], c["name"]


class LineCall:
    """one sslam_new_map_lines_batch_dev: a pool of keyframes [(kl, octave, fn)], pairs [(kf1, kf2)] with the neighbour's median depth, and per pair its rows of line pairs"""
    def __init__(self, fe, kfs, poses, lcap, pairs, medians, lps, free=None, seed=8, npairs=None):
        rng = np.random.default_rng(seed)
        S, P = len(kfs), len(pairs)
        self.lcap, self.S, self.P, self.npairs = lcap, S, P, P if npairs is None else npairs
        kl = bc.junk(rng, (S, lcap), fe.KL_DTYPE); fn = bc.junk(rng, (S, lcap, 3), np.float64); n = np.zeros(S, np.int32)
        self.free0 = None if free is None else bc.junk(rng, (S, lcap), np.uint8)
        for k, (rows, oc, f) in enumerate(kfs):
            n[k] = len(oc); kl[k, :n[k]] = kl_rows(fe, rows, oc); fn[k, :n[k]] = f
            if free is not None: self.free0[k, :n[k]] = 1 if free[k] is None else free[k]
        lp = bc.junk(rng, (P + 1, lcap, 2), np.int32); cnt = np.zeros(P + 1, np.int32)
        for p, rows in enumerate(lps):
            if rows is not None: cnt[p] = len(rows); lp[p, :len(rows)] = rows
        self.d = dict(kl=dev(kl), fn=dev(fn), n=dev(n), pose=dev(np.asarray(poses, np.float32)), pairs=dev(pair_rows(fe, list(pairs) + [(0, 1)], list(medians) + [1.0])), lp=dev(lp),
                      cnt=dev(cnt), free=None if free is None else dev(self.free0))
        R = (P + 1) * lcap
        self.o = dict(s3d=filled(12 * R), e3d=filled(12 * R), stage=filled(R), normal=filled(24 * R), dist=filled(8 * R), nnew=filled(4 * (P + 1)))
        torch.cuda.synchronize()

    def launch(self, ctx, sf=nc.SF, stream=None, **kw):
        a = dict(d_kl=self.d["kl"], d_linefn=self.d["fn"], d_nl=self.d["n"], lcap=self.lcap, nkeyframes=self.S, d_pose=self.d["pose"], d_pairs=self.d["pairs"], npairs=self.npairs,
                 d_line_pairs=self.d["lp"], d_line_npairs=self.d["cnt"], scale_factors=sf, d_s3d=self.o["s3d"], d_e3d=self.o["e3d"], d_stage=self.o["stage"],
                 d_normal=self.o["normal"], d_dist=self.o["dist"], d_nnew=self.o["nnew"], d_lfree=self.d["free"], stream=stream)
        a.update(kw)
        ctx.new_map_lines_batch_dev(**a)
        return self

    def results(self):
        P, c = self.P + 1, self.lcap
        r = dict(s3d=host(self.o["s3d"], np.float32, (P, c, 3)), e3d=host(self.o["e3d"], np.float32, (P, c, 3)), stage=host(self.o["stage"], np.uint8, (P, c)),
                 normal=host(self.o["normal"], np.float64, (P, c, 3)), dist=host(self.o["dist"], np.float32, (P, c, 2)), nnew=host(self.o["nnew"], np.int32, (P,)))
        if self.d["free"] is not None: r["free"] = host(self.d["free"], np.uint8, (self.S, c))
        return r

    def untouched(self):
        return all(keeps_fill(v) for k, v in self.results().items() if k != "free") and (self.d["free"] is None or (self.results()["free"] == self.free0).all())


def test_line_cases_batch(fe, ctx, model):
    ran = 0
    for with_free in (False, True):      # a NULL d_lfree (every line is free) and given flags are two launches: a call has one d_lfree
        for grp in groups([c for c in nc.line_cases() if (c["free1"] is not None) == with_free and not c.get("single_only")], ("sf",)):
            kfs = [k for c in grp for k in ((c["kl1"], c["loct1"], c["fn1"]), (c["kl2"], c["loct2"], c["fn2"]))]
            poses = [p for c in grp for p in (c["pose1"], c["pose2"])]
            pairs = [(2 * p, 2 * p + 1) for p in range(len(grp))]
            lcap = max(max(len(k[1]) for k in kfs), max(len(c["lp"]) for c in grp), 1)
            assert lcap <= 128
            free = [f for c in grp for f in (c["free1"], c["free2"])] if with_free else None
            call = LineCall(fe, kfs, poses, lcap, pairs, [c["median"] for c in grp], [c["lp"] for c in grp], free).launch(ctx, grp[0]["sf"])
            ctx.synchronize()
            wants = [model[c["name"]] for c in grp]
            check_pairs(call.results(), wants, [len(c["lp"]) for c in grp], LINE_OUT, call.free0, line_clears(pairs, [c["lp"] for c in grp], wants) if with_free else None)
            ran += len(grp)
    assert ran == len([c for c in nc.line_cases() if not c.get("single_only")]) >= 16


def test_line_cases_single_and_tap(fe, ctx, model):
    for c in nc.line_cases():
        if c["free1"] is not None and not c.get("single_only"): continue      # the single call has no flags
        w = model[c["name"]]
        if c["free1"] is not None:      # the case of 300 rows (the lanes' second turn) without its flags
            c = dict(c, free1=None, free2=None)
            w = sim.run([c])[0]
            assert len(w["stage"]) > 256 and (w["stage"][256:] == 0).any()
        for tap in (False, True):
            o = ctx.new_map_lines(kl_rows(fe, c["kl1"], c["loct1"]), c["fn1"], kl_rows(fe, c["kl2"], c["loct2"]), c["fn2"], c["pose1"], c["pose2"], c["median"], c["lp"], c["sf"], tap=tap)
            for k in LINE_OUT + (("cos", "hom") if tap else ()):
                same(o[k], w[k], "%s %s tap=%d" % (c["name"], k, tap))
            assert o["nnew"] == w["nnew"], c["name"]


def mixed_pairs(nkf, rng):
    """70 pairs: keyframe 0 against 20 neighbours, (a, b) beside (b, a), slots out of range, kf1 == kf2, the rest random"""
    pairs = [(0, k) for k in range(1, 21)] + [(7, 3), (3, 7), (11, 12), (12, 11), (-1, 3), (4, nkf), (nkf + 3, -2), (5, 5), (0, 0), (2, 9), (9, 2), (8, 4), (4, 8)]
    while len(pairs) < 70:
        a, b = (int(x) for x in rng.integers(0, nkf, 2))
        pairs.append((a, b))
    return pairs


def test_mixed_point_pairs(fe, ctx):
    P = nc.point_pool(5, nkf=24, cap=96)
    nkf = len(P["kp"])
    assert {0, 1, 63, 64, 65, 96} <= set(len(o) for o in P["oct"])
    pairs = mixed_pairs(nkf, np.random.default_rng(3))
    live = [0 <= a < nkf and 0 <= b < nkf and a != b for a, b in pairs]
    cases = [nc.pool_point_case(P, a, b) if ok else None for (a, b), ok in zip(pairs, live)]
    got = iter(sim.run([c for c in cases if c is not None]))
    wants = [next(got) if c is not None else None for c in cases]
    assert sum(w["nnew"] for w in wants if w) > 1000 and live.count(False) >= 5
    m12s = [None if c is None else c["m12"] for c in cases]
    call = PointCall(fe, list(zip(P["kp"], P["oct"])), P["poses"], 96, pairs, m12s).launch(ctx)
    ctx.synchronize()
    check_pairs(call.results(), wants, [0 if c is None else len(c["oct1"]) for c in cases], POINT_OUT, call.free0, point_clears(pairs, m12s, wants))


def test_mixed_line_pairs(fe, ctx):
    L = nc.line_pool(6, nkf=24, lcap=48)
    nkf = len(L["kl"])
    rng = np.random.default_rng(4)
    pairs = mixed_pairs(nkf, rng)
    cases, lps = [], []
    for a, b in pairs:
        if not (0 <= a < nkf and 0 <= b < nkf and a != b):
            cases.append(None); lps.append(None); continue
        m = nc.matches_by_id(L["ids"][a], L["ids"][b]); rows = np.nonzero(m >= 0)[0]
        lp = np.stack([rows, m[rows]], 1).astype(np.int32)[rng.permutation(len(rows))]
        cases.append(nc.pool_line_case(L, a, b, lp)); lps.append(lp)
    got = iter(sim.run([c for c in cases if c is not None]))
    wants = [next(got) if c is not None else None for c in cases]
    assert sum(w["nnew"] for w in wants if w) > 300
    call = LineCall(fe, list(zip(L["kl"], L["oct"], L["fn"])), L["poses"], 48, pairs, [L["median"]] * len(pairs), lps).launch(ctx)
    ctx.synchronize()
    check_pairs(call.results(), wants, [0 if lp is None else len(lp) for lp in lps], LINE_OUT)


S_ROUNDS, N_ROUNDS = 3, 3
neighbour = lambda s, r: s + 5 + 4 * r      # session s: keyframe s against keyframes s + 5, s + 9, s + 13 of a pool of 16


def point_rounds(fe, oracle, cap=96):
    """three sessions of one keyframe and three neighbours each in a pool of 16 keyframes, and the two host replays of their three rounds: SearchForTriangulation (the
    CPU oracle) then the host model, with and without the free flags updated between rounds -> (pool scene, sides, motions, rng, with_update, final flags, without)"""
    P = nc.point_pool(21, nkf=16, cap=cap, counts=[cap - (k % 5) for k in range(16)])
    rng = np.random.default_rng(22)
    D = rng.integers(0, 256, size=(len(P["X"]), 32), dtype=np.uint8)
    sides = [tc.side(kp_rows(fe, xy, oc), D[ids], ids % 16) for xy, oc, ids in zip(P["kp"], P["oct"], P["ids"])]
    mots = {}
    for s in range(S_ROUNDS):
        for r in range(N_ROUNDS):
            F, ex, ey = nc.f12_of(P["poses"][s], P["poses"][neighbour(s, r)])
            mots[s, r] = dict(F12=F, ex=ex, ey=ey)

    def replay(update):
        free = [s["free"].copy() for s in sides]
        rounds = []
        for r in range(N_ROUNDS):
            cases = []
            for s in range(S_ROUNDS):
                a, b = s, neighbour(s, r)
                m12, _ = tc.expect(oracle, tc.pair(dict(sides[a], free=free[a]), dict(sides[b], free=free[b]), mots[s, r]))
                cases.append(nc.point_case("round", P["poses"][a], P["poses"][b], P["kp"][a], P["oct"][a], P["kp"][b], P["oct"][b], m12, sf=tc.SCALE, sigma2=tc.SIGMA2))
            outs = sim.run(cases)
            if update:
                for s, (c, o) in enumerate(zip(cases, outs)):
                    for i in np.nonzero(o["stage"] == 0)[0]:
                        free[s][i] = 0; free[neighbour(s, r)][c["m12"][i]] = 0
            rounds.append((cases, outs))
        return rounds, free

    with_update, free_u = replay(True)
    without, _ = replay(False)
    lost = 0      # a match of round 2 that the creation of round 1 took away
    for s in range(S_ROUNDS):
        made = with_update[0][1][s]["stage"] == 0
        lost += int((made & (without[1][0][s]["m12"] >= 0) & (with_update[1][0][s]["m12"] < 0)).sum())
    assert lost >= 1 and sum(o["nnew"] for o in with_update[0][1]) > 50, (lost, [o["nnew"] for o in with_update[0][1]])
    return P, sides, mots, rng, with_update, free_u, without


def test_point_rounds_on_one_stream(fe, ctx, oracle):
    cap = 96
    P, sides, mots, rng, with_update, free_u, without = point_rounds(fe, oracle, cap)
    pool = tc.pack_pool(rng, sides, cap)
    d = {k: dev(pool[k]) for k in ("kp", "desc", "node", "free", "n")}
    d_pose = dev(P["poses"])
    tri = [dev(tc.pack_pairs([(mots[s, r], s, neighbour(s, r)) for s in range(S_ROUNDS)])) for r in range(N_ROUNDS)]
    nmp = [dev(pair_rows(fe, [(s, neighbour(s, r)) for s in range(S_ROUNDS)])) for r in range(N_ROUNDS)]
    R = S_ROUNDS * cap
    m12 = [filled(4 * R) for _ in range(N_ROUNDS)]; nm = [filled(4 * S_ROUNDS) for _ in range(N_ROUNDS)]
    o = [dict(x3d=filled(12 * R), stage=filled(R), normal=filled(12 * R), dist=filled(8 * R), nnew=filled(4 * S_ROUNDS)) for _ in range(N_ROUNDS)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for r in range(N_ROUNDS):      # six launches in stream order, no synchronise in between
        ctx.search_for_triangulation_batch_dev(d["kp"], d["desc"], d["node"], d["n"], cap, 16, tri[r], S_ROUNDS, tc.SCALE, tc.SIGMA2, m12[r], nm[r], d_free=d["free"], stream=st.cuda_stream)
        ctx.new_map_points_batch_dev(d["kp"], d["n"], cap, 16, d_pose, nmp[r], S_ROUNDS, m12[r], tc.SCALE, tc.SIGMA2, nc.SCALE_FACTOR, o[r]["x3d"], o[r]["stage"], o[r]["normal"],
                                     o[r]["dist"], o[r]["nnew"], d_free=d["free"], stream=st.cuda_stream)
    st.synchronize()
    differs = False
    for r in range(N_ROUNDS):
        gm = host(m12[r], np.int32, (S_ROUNDS, cap))
        res = dict(x3d=host(o[r]["x3d"], np.float32, (S_ROUNDS, cap, 3)), stage=host(o[r]["stage"], np.uint8, (S_ROUNDS, cap)), normal=host(o[r]["normal"], np.float32, (S_ROUNDS, cap, 3)),
                   dist=host(o[r]["dist"], np.float32, (S_ROUNDS, cap, 2)), nnew=host(o[r]["nnew"], np.int32, (S_ROUNDS,)))
        for s in range(S_ROUNDS):
            c, w = with_update[r][0][s], with_update[r][1][s]
            n1 = len(c["m12"])
            np.testing.assert_array_equal(gm[s, :n1], c["m12"], err_msg="round %d session %d" % (r, s))
            for k in POINT_OUT:
                same(res[k][s, :n1], w[k], "round %d session %d %s" % (r, s, k))
            assert res["nnew"][s] == w["nnew"]
            differs = differs or not np.array_equal(gm[s, :n1], without[r][0][s]["m12"])
    assert differs
    gf = host(d["free"], np.uint8, (16, cap))
    for k in range(16):
        np.testing.assert_array_equal(gf[k, :len(free_u[k])], free_u[k])
        np.testing.assert_array_equal(gf[k, len(free_u[k]):], pool["free"][k, len(free_u[k]):])


def line_match_batch(fe, ctx, d1, n1, d2, n2, cap, npairs, pairs, counts, stream):
    rc = fe.lib().sslam_line_match_batch_dev(ctx.h, C.c_void_p(d1.data_ptr()), C.c_void_p(n1.data_ptr()), C.c_void_p(d2.data_ptr()), C.c_void_p(n2.data_ptr()), cap, npairs,
                                             C.c_double(0.1), 0, C.c_void_p(pairs.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(stream or 0))
    assert rc == 0, rc


def test_line_rounds_on_one_stream(fe, ctx):
    lcap = 48
    L = nc.line_pool(31, nkf=16, lcap=lcap, nseg=52, counts=[lcap - (k % 4) for k in range(16)])
    rng = np.random.default_rng(32)
    D = rng.integers(0, 256, size=(52, 32), dtype=np.uint8)
    NP = S_ROUNDS * N_ROUNDS      # the matcher's pairs, round after round: pair r * S + s
    l1 = bc.junk(rng, (NP, lcap, 32), np.uint8); l2 = bc.junk(rng, (NP, lcap, 32), np.uint8); n1 = np.zeros(NP, np.int32); n2 = np.zeros(NP, np.int32)
    for r in range(N_ROUNDS):
        for s in range(S_ROUNDS):
            p, a, b = r * S_ROUNDS + s, s, neighbour(s, r)
            n1[p], n2[p] = len(L["ids"][a]), len(L["ids"][b])
            l1[p, :n1[p]] = D[L["ids"][a]]; l2[p, :n2[p]] = D[L["ids"][b]]
    call = LineCall(fe, list(zip(L["kl"], L["oct"], L["fn"])), L["poses"], lcap, [(0, 1)], [1.0], [None], free=[None] * 16)      # the pool, its flags and nothing else
    d_l1, d_n1, d_l2, d_n2 = dev(l1), dev(n1), dev(l2), dev(n2)
    d_lp, d_cnt = filled(8 * NP * lcap), filled(4 * NP)
    nmp = [dev(pair_rows(fe, [(s, neighbour(s, r)) for s in range(S_ROUNDS)], [L["median"]] * S_ROUNDS)) for r in range(N_ROUNDS)]
    R = S_ROUNDS * lcap
    o = [dict(s3d=filled(12 * R), e3d=filled(12 * R), stage=filled(R), normal=filled(24 * R), dist=filled(8 * R), nnew=filled(4 * S_ROUNDS)) for _ in range(N_ROUNDS)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    line_match_batch(fe, ctx, d_l1, d_n1, d_l2, d_n2, lcap, NP, d_lp, d_cnt, st.cuda_stream)
    for r in range(N_ROUNDS):
        ctx.new_map_lines_batch_dev(call.d["kl"], call.d["fn"], call.d["n"], lcap, 16, call.d["pose"], nmp[r], S_ROUNDS, d_lp.data_ptr() + 8 * r * R, d_cnt.data_ptr() + 4 * r * S_ROUNDS,
                                    nc.SF, o[r]["s3d"], o[r]["e3d"], o[r]["stage"], o[r]["normal"], o[r]["dist"], o[r]["nnew"], d_lfree=call.d["free"], stream=st.cuda_stream)
    st.synchronize()
    lp = host(d_lp, np.int32, (NP, lcap, 2)); cnt = host(d_cnt, np.int32, (NP,))
    assert (cnt > 20).all() and (cnt <= lcap).all()

    def replay(update):
        free = [np.ones(len(i), np.uint8) for i in L["ids"]]
        rounds = []
        for r in range(N_ROUNDS):
            cases = []
            for s in range(S_ROUNDS):
                p, a, b = r * S_ROUNDS + s, s, neighbour(s, r)
                cases.append(nc.pool_line_case(L, a, b, lp[p, :cnt[p]], free[a].copy(), free[b].copy()))
            outs = sim.run(cases)
            if update:
                for s, (c, w) in enumerate(zip(cases, outs)):
                    for row in np.nonzero(w["stage"] == 0)[0]:
                        free[s][c["lp"][row, 0]] = 0; free[neighbour(s, r)][c["lp"][row, 1]] = 0
            rounds.append((cases, outs))
        return rounds, free

    with_update, free_u = replay(True)
    without, _ = replay(False)
    lost = sum(int(((with_update[1][1][s]["stage"] == 2) & (without[1][1][s]["stage"] != 2)).sum()) for s in range(S_ROUNDS))
    assert lost >= 1 and sum(w["nnew"] for w in with_update[0][1]) > 20
    differs = False
    for r in range(N_ROUNDS):
        res = dict(s3d=host(o[r]["s3d"], np.float32, (S_ROUNDS, lcap, 3)), e3d=host(o[r]["e3d"], np.float32, (S_ROUNDS, lcap, 3)), stage=host(o[r]["stage"], np.uint8, (S_ROUNDS, lcap)),
                   normal=host(o[r]["normal"], np.float64, (S_ROUNDS, lcap, 3)), dist=host(o[r]["dist"], np.float32, (S_ROUNDS, lcap, 2)), nnew=host(o[r]["nnew"], np.int32, (S_ROUNDS,)))
        for s in range(S_ROUNDS):
            w, n = with_update[r][1][s], cnt[r * S_ROUNDS + s]
            for k in LINE_OUT:
                same(res[k][s, :n], w[k], "round %d session %d %s" % (r, s, k))
                assert keeps_fill(res[k][s, n:])
            assert res["nnew"][s] == w["nnew"]
            differs = differs or not np.array_equal(res["stage"][s, :n], without[r][1][s]["stage"])
    assert differs
    gf = call.results()["free"]
    for k in range(16):
        np.testing.assert_array_equal(gf[k, :len(free_u[k])], free_u[k])
        np.testing.assert_array_equal(gf[k, len(free_u[k]):], call.free0[k, len(free_u[k]):])


def test_chain_on_image_features(fe, ctx):
    gray = np.load(os.path.join(pkg.ROOT, "tests", "golden", "icl_input_gray.npz"))["gray"]
    dx, dy = 12, 8
    h, w = gray.shape[0] - dy, gray.shape[1] - dx
    imgs = [np.ascontiguousarray(gray[:h, :w]), np.ascontiguousarray(gray[dy:, dx:])]      # the frame and a crop of it shifted by (12, 8)
    poses = np.stack([nc.CAM1, nc.pose(nc.rot((0, 1, 0), 0.3), (0.25, 0.15, 0.0), nc.KA)])
    # points: both frames' features in one node, the image motion as F12
    ex = fe.OrbExtractor(ctx, 500, 1.2, 8, 20, 7)
    feats = [ex(im) for im in imgs]
    ex.close()
    cap = 640
    assert all(50 < len(kp) <= cap for kp, _ in feats)
    rng = np.random.default_rng(41)
    sides = [tc.side(kp, desc, np.zeros(len(kp), np.int32)) for kp, desc in feats]
    pool = tc.pack_pool(rng, sides, cap)
    d = {k: dev(pool[k]) for k in ("kp", "desc", "node", "free", "n")}
    mot = tc.motion(angle_deg=0.0, tx=-float(dx), ty=-float(dy))
    tri = dev(tc.pack_pairs([(mot, 0, 1)])); nmp = dev(pair_rows(fe, [(0, 1)])); d_pose = dev(poses)
    m12, nm = filled(4 * cap), filled(4)
    o = dict(x3d=filled(12 * cap), stage=filled(cap), normal=filled(12 * cap), dist=filled(8 * cap), nnew=filled(4))
    torch.cuda.synchronize()
    ctx.search_for_triangulation_batch_dev(d["kp"], d["desc"], d["node"], d["n"], cap, 2, tri, 1, tc.SCALE, tc.SIGMA2, m12, nm, d_free=d["free"])
    ctx.new_map_points_batch_dev(d["kp"], d["n"], cap, 2, d_pose, nmp, 1, m12, tc.SCALE, tc.SIGMA2, nc.SCALE_FACTOR, o["x3d"], o["stage"], o["normal"], o["dist"], o["nnew"], d_free=d["free"])
    ctx.synchronize()
    n1 = len(feats[0][0])
    gm = host(m12, np.int32, (cap,))[:n1]
    assert host(nm, np.int32, (1,))[0] == (gm >= 0).sum() > 30
    (kp1, _), (kp2, _) = feats
    c = nc.point_case("chain", poses[0], poses[1], np.stack([kp1["x"], kp1["y"]], 1), kp1["octave"], np.stack([kp2["x"], kp2["y"]], 1), kp2["octave"], gm, sf=tc.SCALE, sigma2=tc.SIGMA2)
    want = sim.run([c])[0]
    for k, dt, shape in (("x3d", np.float32, (cap, 3)), ("stage", np.uint8, (cap,)), ("normal", np.float32, (cap, 3)), ("dist", np.float32, (cap, 2))):
        got = host(o[k], dt, shape)
        same(got[:n1], want[k], "chain " + k)
        assert keeps_fill(got[n1:])
    assert host(o["nnew"], np.int32, (1,))[0] == want["nnew"]
    # lines
    lx = fe.LineExtractor(ctx, 128)
    lf = [lx(im) for im in imgs]
    lx.close()
    lcap = 128
    assert all(10 < len(kl) <= lcap for kl, _, _ in lf)
    call = LineCall(fe, [(np.stack([kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]], 1), kl["octave"], fn) for kl, _, fn in lf], poses, lcap, [(0, 1)], [2.0],
                    [None], free=[None, None])
    l1 = bc.junk(rng, (1, lcap, 32), np.uint8); l2 = bc.junk(rng, (1, lcap, 32), np.uint8)
    l1[0, :len(lf[0][1])] = lf[0][1]; l2[0, :len(lf[1][1])] = lf[1][1]
    d_l1, d_l2, d_n1, d_n2 = dev(l1), dev(l2), dev(np.array([len(lf[0][1])], np.int32)), dev(np.array([len(lf[1][1])], np.int32))
    d_lp, d_cnt = filled(8 * lcap), filled(4)
    torch.cuda.synchronize()
    line_match_batch(fe, ctx, d_l1, d_n1, d_l2, d_n2, lcap, 1, d_lp, d_cnt, None)
    call.launch(ctx, d_line_pairs=d_lp, d_line_npairs=d_cnt)
    ctx.synchronize()
    lp = host(d_lp, np.int32, (lcap, 2)); n = int(host(d_cnt, np.int32, (1,))[0])
    assert 5 < n <= lcap
    (ka, _, fa), (kb, _, fb) = lf
    rows = lambda kl: np.stack([kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]], 1)
    c = nc.line_case("chain", poses[0], poses[1], rows(ka), ka["octave"], fa, rows(kb), kb["octave"], fb, lp[:n], 2.0)
    want = sim.run([c])[0]
    res = call.results()
    for k in LINE_OUT:
        same(res[k][0, :n], want[k], "line chain " + k)
        assert keeps_fill(res[k][0, n:])
    assert res["nnew"][0] == want["nnew"]
    want_free = call.free0.copy()
    for r in np.nonzero(want["stage"] == 0)[0]:
        want_free[0, lp[r, 0]] = 0; want_free[1, lp[r, 1]] = 0
    np.testing.assert_array_equal(res["free"], want_free)


def test_argument_errors(fe, ctx):
    P = nc.point_pool(5, nkf=4, cap=32, counts=[32, 30, 31, 32])
    pairs = [(0, 1), (2, 3)]
    m12s = [nc.matches_by_id(P["ids"][a], P["ids"][b]) for a, b in pairs]
    mk = lambda: PointCall(fe, list(zip(P["kp"], P["oct"])), P["poses"], 32, pairs, m12s)
    off = lambda t, k: t.data_ptr() + k

    def refused(call, **kw):
        with pytest.raises(fe.SslamError) as e:
            call.launch(ctx, **kw)
        assert e.value.code == fe.SSLAM_ERR_INVALID, kw
        ctx.synchronize()
        assert call.untouched(), kw

    c = mk()
    for k in ("d_kp", "d_n", "d_pose", "d_pairs", "d_matches12", "d_x3d", "d_stage", "d_normal", "d_dist", "d_nnew", "scale_factors", "level_sigma2"):
        refused(c, **{k: None})
    for k, t in (("d_kp", c.d["kp"]), ("d_n", c.d["n"]), ("d_pose", c.d["pose"]), ("d_pairs", c.d["pairs"]), ("d_matches12", c.d["m12"]), ("d_x3d", c.o["x3d"]),
                 ("d_normal", c.o["normal"]), ("d_dist", c.o["dist"]), ("d_nnew", c.o["nnew"])):
        refused(c, **{k: off(t, 2)})
    for kw in (dict(cap=-1), dict(nkeyframes=-1), dict(npairs=-1), dict(nlevels=0), dict(nlevels=65), dict(cap=1 << 16, npairs=1 << 15), dict(cap=1 << 16, nkeyframes=1 << 15)):
        refused(c, **kw)
    c.launch(ctx, npairs=0); ctx.synchronize()
    assert c.untouched()
    c.launch(ctx, d_stage=off(c.o["stage"], 0)); ctx.synchronize()      # the call itself is fine
    assert (c.results()["nnew"][:2] > 0).all()

    L = nc.line_pool(6, nkf=4, lcap=16, counts=[16, 15, 16, 14])
    lps = []
    for a, b in pairs:
        m = nc.matches_by_id(L["ids"][a], L["ids"][b]); rows = np.nonzero(m >= 0)[0]
        lps.append(np.stack([rows, m[rows]], 1).astype(np.int32))
    c = LineCall(fe, list(zip(L["kl"], L["oct"], L["fn"])), L["poses"], 16, pairs, [L["median"]] * 2, lps, free=[None] * 4)
    for k in ("d_kl", "d_linefn", "d_nl", "d_pose", "d_pairs", "d_line_pairs", "d_line_npairs", "d_s3d", "d_e3d", "d_stage", "d_normal", "d_dist", "d_nnew", "scale_factors"):
        refused(c, **{k: None})
    for k, t, by in (("d_kl", c.d["kl"], 2), ("d_linefn", c.d["fn"], 4), ("d_nl", c.d["n"], 2), ("d_pose", c.d["pose"], 2), ("d_pairs", c.d["pairs"], 2), ("d_line_pairs", c.d["lp"], 2),
                     ("d_line_npairs", c.d["cnt"], 2), ("d_s3d", c.o["s3d"], 2), ("d_e3d", c.o["e3d"], 2), ("d_normal", c.o["normal"], 4), ("d_dist", c.o["dist"], 2), ("d_nnew", c.o["nnew"], 2)):
        refused(c, **{k: off(t, by)})
    for kw in (dict(lcap=-1), dict(nkeyframes=-1), dict(npairs=-1), dict(nlevels=0), dict(nlevels=65), dict(lcap=1 << 16, npairs=1 << 15)):
        refused(c, **kw)
    c.launch(ctx, npairs=0); ctx.synchronize()
    assert c.untouched()
    c.launch(ctx); ctx.synchronize()
    assert (c.results()["nnew"][:2] >= 0).all() and not keeps_fill(c.results()["stage"][0, :len(lps[0])])
