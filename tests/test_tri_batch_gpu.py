"""GPU parity of sslam_orb_search_for_triangulation_batch_dev: ORBmatcher::SearchForTriangulation for pairs of keyframe slots of one cap strided
device pool, enqueued on the caller's stream.  Every expectation is the CPU oracle's -- oracle.search_for_triangulation on the CSR lists
tests/tri_batch_cases.py builds from the node arrays (its reach is shown in tests/test_tri_batch_cases_cpu.py) -- and every comparison is exact; one
test checks that the library's single call agrees row for row.  Rows past every count hold random bytes, node ids, free flags and right coordinates
included; the outputs hold a sentinel before every call.

  test_ragged_batch            twelve slots of capacity 96 with counts 0 / 1 / 63 / 64 / 65 / 96, rows in no node, nodes on one side only; 27 pairs with
                               every combination of an empty and a non-empty side; only_stereo 0 / 1 x check_orientation 0 / 1
  test_against_the_single_call the same pairs through sslam_orb_search_for_triangulation on uploaded frames
  test_lane_loop_edges         one node of 1 / 63 / 64 / 65 / 129 keyframe-2 rows, the winner first, in the middle, last
  test_gates                   equal distances, a closer candidate off the epipolar line before / after the one that passes, distance 50 / 51, the
                               epipole gate and the epipolar gate on neighbouring floats, an all-zero F12, another F12 and epipole in every pair
  test_rotation                histograms that wrap, tie and drop their second maximum; neighbouring pairs with other dominant rotations
  test_pairs                   one keyframe against 20 neighbours, kf1 == kf2, swapped roles, slots out of range, npairs == 0
  test_counts_are_clamped      counts of -3 and capacity + 5
  test_null_free_and_uright    NULL d_free (every row free), NULL d_uright (monocular)
  test_size_bound              capacities 1024 / 1025 (the dynamic-LDS opt-in) and 1365 / 1366 (keyframe 2 leaves LDS), full slots
  test_streams_*               two calls back to back on a side stream; a call beside the synchronous single call
  test_argument_errors         SSLAM_ERR_INVALID leaves the outputs at the sentinel"""
import numpy as np
import pytest
import torch
import tri_batch_cases as tc
import bow_batch_cases as bc

pytestmark = pytest.mark.gpu

SENT = -77          # what the outputs hold before a call


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Call:
    """one matcher call: device inputs (kept alive) and sentinel-filled outputs, made by the constructor; launch() enqueues it.
    sides: the pool's slots; pairs: [(pair, kf1 slot, kf2 slot)] (the pair gives F12 and the epipole)"""
    def __init__(self, sides, cap, pairs, seed=99, n=None, npairs=None, with_free=True, with_uright=True):
        rng = np.random.default_rng(seed)
        P = tc.pack_pool(rng, sides, cap)
        self.cap, self.nk = cap, len(sides)
        self.npairs = len(pairs) if npairs is None else npairs
        self.d = {x: dev(P[x]) for x in ("kp", "desc", "node")}
        self.d["free"] = dev(P["free"]) if with_free else None; self.d["uright"] = dev(P["uright"]) if with_uright else None
        self.d["n"] = dev(P["n"] if n is None else np.asarray(n, np.int32))
        rows = tc.pack_pairs(list(pairs) + [(pairs[0][0], 0, 0)])          # one row more than the call may read
        self.pairs = dev(rows)
        out_rows = max(self.npairs, len(pairs)) + 1                       # one row more than the call may write
        self.m12 = torch.full((out_rows, cap), SENT, dtype=torch.int32, device="cuda"); self.nm = torch.full((out_rows,), SENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()          # the buffers were filled on torch's stream

    def launch(self, ctx, only_stereo=False, ori=True, stream=None):
        ctx.search_for_triangulation_batch_dev(self.d["kp"], self.d["desc"], self.d["node"], self.d["n"], self.cap, self.nk, self.pairs, self.npairs, tc.SCALE, tc.SIGMA2,
                                               self.m12, self.nm, d_free=self.d["free"], d_uright=self.d["uright"], only_stereo=only_stereo, check_orientation=ori,
                                               stream=stream)
        return self

    def results(self):
        """after a synchronise"""
        return self.m12.cpu().numpy(), self.nm.cpu().numpy()


def check(got, want, n1s, npairs=None):
    """matches12 rows and count of pair p against want[p] = (matches12, count), or None for a skipped pair (count 0, no row written); rows at or past
    keyframe 1's count and everything behind the last pair keep the sentinel"""
    m, nm = got
    for p, w in enumerate(want):
        if w is None:
            assert nm[p] == 0 and (m[p] == SENT).all(), p
            continue
        n1 = n1s[p]
        np.testing.assert_array_equal(m[p, :n1], w[0], err_msg="pair %d" % p)
        assert nm[p] == w[1], (p, nm[p], w[1])
        assert (m[p, n1:] == SENT).all(), p
    n = len(want) if npairs is None else npairs
    assert (m[n:] == SENT).all() and (nm[n:] == SENT).all()


def run_pool(ctx, oracle, sides, slots, cap, only_stereo=False, ori=True, mots=None, **kw):
    """pairs (kf1 slot, kf2 slot) of one pool in one call -> (got, want, cases)"""
    cases = [tc.pair(sides[a], sides[b], None if mots is None else mots[p], bool(only_stereo), bool(ori)) for p, (a, b) in enumerate(slots)]
    want = [tc.expect(oracle, c) for c in cases]
    call = Call(sides, cap, [(c, a, b) for c, (a, b) in zip(cases, slots)], **kw).launch(ctx, only_stereo, ori)
    ctx.synchronize()
    got = call.results()
    check(got, want, [len(c["s1"]["kp"]) for c in cases])
    return got, want, cases


def run_cases(ctx, oracle, cases, cap, only_stereo=False, ori=True):
    """independent pairs, each with two slots of its own (2 p, 2 p + 1), in one call -> (got, want)"""
    cs = [tc.with_flags(c, only_stereo, ori) for c in cases]
    want = [tc.expect(oracle, c) for c in cs]
    sides = [s for c in cs for s in (c["s1"], c["s2"])]
    call = Call(sides, cap, [(c, 2 * p, 2 * p + 1) for p, c in enumerate(cs)]).launch(ctx, only_stereo, ori)
    ctx.synchronize()
    got = call.results()
    check(got, want, [len(c["s1"]["kp"]) for c in cs])
    return got, want


def winner(c, m):
    r = int(m[c["q"]])
    return None if r < 0 else int(np.flatnonzero(c["cand"] == r)[0])


# ---- 1. a ragged batch
@pytest.fixture(scope="module")
def ragged():
    return tc.ragged_pool(np.random.default_rng(7700))


@pytest.mark.parametrize("ori", [0, 1])
@pytest.mark.parametrize("only_stereo", [0, 1])
def test_ragged_batch(ctx, oracle, ragged, only_stereo, ori):
    sides, slots = ragged
    got, want, cases = run_pool(ctx, oracle, sides, slots, tc.RAGGED_CAP, only_stereo, ori)
    assert sum(w[1] for w in want) > (60 if only_stereo else 300)


@pytest.mark.parametrize("only_stereo,ori", [(0, 1), (1, 0)])
def test_against_the_single_call(ctx, oracle, ragged, only_stereo, ori):
    sides, slots = ragged
    got, want, cases = run_pool(ctx, oracle, sides, slots, tc.RAGGED_CAP, only_stereo, ori)
    frames = {i: ctx.frame_upload(0, s["kp"], s["desc"], s["uright"]) for i, s in enumerate(sides) if len(s["kp"])}
    seen = 0
    for p, ((a, b), c) in enumerate(zip(slots, cases)):
        if a not in frames or b not in frames: continue
        pk, pf, ik, jf = bc.csr_from_nodes(c["s1"]["node"], c["s2"]["node"])
        m, n = frames[a].search_for_triangulation(frames[b], c["s1"]["free"], c["s2"]["free"], pk, pf, ik, jf, c["F12"], c["ex"], c["ey"], tc.SCALE, tc.SIGMA2,
                                                  bool(only_stereo), bool(ori))
        np.testing.assert_array_equal(m, got[0][p, :len(m)], err_msg="pair %d" % p); assert n == got[1][p]
        seen += 1
    assert seen >= 20
    for f in frames.values(): f.close()


# ---- 2. the lane loop's edges
def test_lane_loop_edges(ctx, oracle):
    L = tc.lane_cases(np.random.default_rng(7600))
    got, want = run_cases(ctx, oracle, [c for c, _ in L.values()], 160)
    for p, (name, (c, pos)) in enumerate(L.items()):
        assert winner(c, got[0][p]) == pos and got[1][p] == 1, name


# ---- 3. ties, the threshold chain and the two geometric gates; a different F12 and epipole per pair
def test_gates(ctx, oracle):
    G = {}
    G.update(tc.tie_cases(np.random.default_rng(7610))); G.update(tc.epipole_cases(np.random.default_rng(7620))); G.update(tc.epipolar_cases(np.random.default_rng(7630)))
    m0, m1 = tc.two_motions(np.random.default_rng(7640))
    cases = [c for c, _ in G.values()] + [m0, m1, tc.zero_F12(m0), m1, m0]
    assert len(set(c["F12"].tobytes() for c in cases)) >= 4 and len(set((c["ex"], c["ey"]) for c in cases)) >= 3
    got, want = run_cases(ctx, oracle, cases, 96)
    for p, (name, (c, stated)) in enumerate(G.items()):
        w = winner(c, got[0][p])
        assert ((w is not None) == stated) if isinstance(stated, bool) else (w == stated), (name, w, stated)
    k = len(G)
    assert got[1][k] > 20 and got[1][k + 1] > 20 and got[1][k + 2] == 0 and got[1][k + 3] == got[1][k + 1] and got[1][k + 4] == got[1][k]


# ---- 4. rotation
def test_rotation(ctx, oracle):
    R = tc.rot_pairs()
    names = list(R)
    assert names[-2:] == ["neighbour_0", "neighbour_90"]
    got, want = run_cases(ctx, oracle, list(R.values()), 64, ori=True)
    full = [len(c["rc"]["i1"]) for c in R.values()]
    assert all(w[1] < f for w, f in zip(want, full)) and want[-1][1] == want[-2][1] == 33
    got, want = run_cases(ctx, oracle, list(R.values()), 64, ori=False)
    assert [w[1] for w in want] == full


# ---- 5. pairs
@pytest.fixture(scope="module")
def neighbours():
    return tc.neighbours_pool(np.random.default_rng(7660))


def test_pairs(ctx, oracle, neighbours):
    sides = neighbours
    K = len(sides)
    assert K == 21
    # LocalMapping::CreateNewMapPoints: the new keyframe against 20 neighbours (every pair sees the same free flags), then itself, then swapped roles
    slots = [(0, k) for k in range(1, K)] + [(0, 0), (1, 0), (5, 5)]
    got, want, cases = run_pool(ctx, oracle, sides, slots, 64)
    assert min(w[1] for w in want[:20]) > 5 and len(set(w[0].tobytes() for w in want[:20])) == 20
    # slots out of range on either side, between pairs that are computed
    slots = [(0, 1), (-1, 1), (0, K), (K, 0), (0, 2), (1 << 30, 0), (0, -(1 << 31)), (0, 3)]
    cases = [tc.pair(sides[a], sides[b]) if 0 <= a < K and 0 <= b < K else None for a, b in slots]
    want = [tc.expect(oracle, c) if c is not None else None for c in cases]
    assert [w is None for w in want] == [False, True, True, True, False, True, True, False]
    call = Call(sides, 64, [(c or cases[0], a, b) for c, (a, b) in zip(cases, slots)]).launch(ctx); ctx.synchronize()
    check(call.results(), want, [len(c["s1"]["kp"]) if c is not None else 0 for c in cases])
    # no pair at all
    call = Call(sides, 64, [(cases[0], 0, 1)], npairs=0).launch(ctx); ctx.synchronize()
    check(call.results(), [], [], 0)


def test_counts_are_clamped(ctx, oracle, ragged):
    sides, _ = ragged
    w, m = sides[0], sides[1]                              # sides of 96 rows fill their slots
    cap = tc.RAGGED_CAP
    pool, n = [w, m, w, m], [-3, cap + 5, cap, cap + 5]
    empty = tc.cut(w, 0)
    slots = [(1, 0), (1, 2), (0, 1), (3, 2)]
    seen = [tc.pair(m, empty), tc.pair(m, w), tc.pair(empty, m), tc.pair(m, w)]
    want = [tc.expect(oracle, c) for c in seen]
    assert want[0][1] == 0 and want[1][1] > 10 and want[2][1] == 0
    call = Call(pool, cap, [(c, a, b) for c, (a, b) in zip(seen, slots)], n=n).launch(ctx); ctx.synchronize()
    check(call.results(), want, [cap, cap, 0, cap])


def test_null_free_and_uright(ctx, oracle, ragged):
    sides, slots = ragged
    all_free = [dict(s, free=np.ones(len(s["kp"]), np.uint8)) for s in sides]
    mono = [{k: v for k, v in s.items() if k != "uright"} for s in sides]
    got, want, _ = run_pool(ctx, oracle, all_free, slots, tc.RAGGED_CAP, with_free=False)
    plain = [tc.expect(oracle, tc.pair(sides[a], sides[b]))[1] for a, b in slots]
    assert sum(w[1] for w in want) > sum(plain)           # the flags of the pool did hold rows back
    got, want, _ = run_pool(ctx, oracle, mono, slots, tc.RAGGED_CAP, with_uright=False)
    assert sum(w[1] for w in want) > 300
    got, want, _ = run_pool(ctx, oracle, mono, slots, tc.RAGGED_CAP, only_stereo=True, with_uright=False)
    assert all(w[1] == 0 for w in want)
    got, want, _ = run_pool(ctx, oracle, [dict(s, free=np.ones(len(s["kp"]), np.uint8)) for s in mono], slots, tc.RAGGED_CAP, with_free=False, with_uright=False)
    assert sum(w[1] for w in want) > 300


# ---- 6. the size bounds of the plan
@pytest.mark.parametrize("cap", [tc.PLAIN_CAP, tc.PLAIN_CAP + 1, tc.LDS_CAP, tc.LDS_CAP + 1])
def test_size_bound(ctx, oracle, cap):
    """48 * 1024 bytes is the last launch without the dynamic-LDS opt-in, 48 * 1365 <= 64 KB the last capacity with keyframe 2 in LDS.  Two slots are
    full, two hold 200 rows; three rows per node"""
    assert tc.ROW_BYTES * tc.LDS_CAP <= tc.LDS_MAX < tc.ROW_BYTES * (tc.LDS_CAP + 1) and tc.ROW_BYTES * tc.PLAIN_CAP <= tc.LDS_DEFAULT < tc.ROW_BYTES * (tc.PLAIN_CAP + 1)
    sides = tc.full_pool(np.random.default_rng(8200 + cap), cap)
    got, want, _ = run_pool(ctx, oracle, sides, tc.FULL_PAIRS, cap)
    assert want[0][1] > 300 and want[3][1] > 40


# ---- 7. streams
@pytest.fixture(scope="module")
def two_calls(oracle):
    A = tc.neighbours_pool(np.random.default_rng(8300), nneigh=6, cap=100)
    B = tc.neighbours_pool(np.random.default_rng(8310), nneigh=4, cap=120)
    sa = [(0, k) for k in range(1, 7)]; sb = [(0, k) for k in range(1, 5)]
    ca = [tc.pair(A[a], A[b]) for a, b in sa]; cb = [tc.pair(B[a], B[b]) for a, b in sb]
    return dict(A=A, B=B, sa=sa, sb=sb, ca=ca, cb=cb, cap=128, wantA=[tc.expect(oracle, c) for c in ca], wantB=[tc.expect(oracle, c) for c in cb])


def test_streams_back_to_back(ctx, two_calls):
    t = two_calls
    s = torch.cuda.Stream()
    c1 = Call(t["A"], t["cap"], [(c, a, b) for c, (a, b) in zip(t["ca"], t["sa"])])
    c2 = Call(t["B"], t["cap"], [(c, a, b) for c, (a, b) in zip(t["cb"], t["sb"])], seed=98)
    c1.launch(ctx, stream=s.cuda_stream); c2.launch(ctx, stream=s.cuda_stream)
    s.synchronize()
    check(c1.results(), t["wantA"], [len(c["s1"]["kp"]) for c in t["ca"]]); check(c2.results(), t["wantB"], [len(c["s1"]["kp"]) for c in t["cb"]])
    assert min(w[1] for w in t["wantA"] + t["wantB"]) > 5


def test_streams_batch_beside_the_synchronous_call(ctx, two_calls):
    t = two_calls
    s = torch.cuda.Stream()
    c = t["cb"][1]
    pk, pf, ik, jf = bc.csr_from_nodes(c["s1"]["node"], c["s2"]["node"])
    f1 = ctx.frame_upload(0, c["s1"]["kp"], c["s1"]["desc"], c["s1"]["uright"]); f2 = ctx.frame_upload(0, c["s2"]["kp"], c["s2"]["desc"], c["s2"]["uright"])
    c1 = Call(t["A"], t["cap"], [(x, a, b) for x, (a, b) in zip(t["ca"], t["sa"])]).launch(ctx, stream=s.cuda_stream)
    m, n = f1.search_for_triangulation(f2, c["s1"]["free"], c["s2"]["free"], pk, pf, ik, jf, c["F12"], c["ex"], c["ey"], tc.SCALE, tc.SIGMA2, False, True)      # on the context stream
    s.synchronize()
    check(c1.results(), t["wantA"], [len(x["s1"]["kp"]) for x in t["ca"]])
    np.testing.assert_array_equal(m, t["wantB"][1][0]); assert n == t["wantB"][1][1]
    f1.close(); f2.close()


# ---- 8. argument errors
def test_argument_errors(fe, ctx, neighbours):
    sides = neighbours
    cases = [tc.pair(sides[0], sides[k]) for k in (1, 2, 3)]
    c = Call(sides, 64, [(x, 0, k) for x, k in zip(cases, (1, 2, 3))])
    base = dict(kp=c.d["kp"], desc=c.d["desc"], node=c.d["node"], n=c.d["n"], cap=64, nk=len(sides), pairs=c.pairs, npairs=3, sf=tc.SCALE, sg=tc.SIGMA2, m12=c.m12, nm=c.nm,
                free=c.d["free"], uright=c.d["uright"], nlevels=None)

    def call(ok=False, **kw):
        a = dict(base, **kw)
        args = (a["kp"], a["desc"], a["node"], a["n"], a["cap"], a["nk"], a["pairs"], a["npairs"], a["sf"], a["sg"], a["m12"], a["nm"])
        opt = dict(d_free=a["free"], d_uright=a["uright"], nlevels=a["nlevels"])
        if ok:
            return ctx.search_for_triangulation_batch_dev(*args, **opt)
        with pytest.raises(fe.SslamError) as e:
            ctx.search_for_triangulation_batch_dev(*args, **opt)
        assert e.value.code == fe.SSLAM_ERR_INVALID and "sslam_orb_search_for_triangulation_batch_dev" in str(e.value)
    for name in ("kp", "desc", "node", "n", "pairs", "m12", "nm"):
        call(**{name: None})
    p_ = fe._p
    assert fe.lib().sslam_orb_search_for_triangulation_batch_dev(None, p_(c.d["kp"]), p_(c.d["desc"]), p_(c.d["node"]), p_(c.d["free"]), p_(c.d["uright"]), p_(c.d["n"]), 64, len(sides),
                                                                 p_(c.pairs), 3, p_(tc.SCALE), p_(tc.SIGMA2), 8, 0, 1, p_(c.m12), p_(c.nm), None) == fe.SSLAM_ERR_INVALID      # no context
    call(sf=None, nlevels=8); call(sg=None)
    for name in ("cap", "nk", "npairs"):
        call(**{name: -1})
    call(cap=1 << 19)
    call(nlevels=0); call(nlevels=65); call(nlevels=-1)
    call(cap=1 << 18, npairs=1 << 13)                  # npairs * cap = 2^31
    call(desc=c.d["desc"].data_ptr() + 8); call(desc=c.d["desc"].data_ptr() + 4)          # descriptor rows are read as 16-byte words
    call(node=c.d["node"].data_ptr() + 2); call(nm=c.nm.data_ptr() + 1); call(pairs=c.pairs.data_ptr() + 2); call(uright=c.d["uright"].data_ptr() + 1)
    ctx.synchronize(); torch.cuda.synchronize()
    m, nm = c.results()
    assert (m == SENT).all() and (nm == SENT).all()
    assert fe.TRI_PAIR_DTYPE.itemsize == 52 and fe.TRI_PAIR_DTYPE == tc.pack_pairs([(cases[0], 0, 1)]).dtype
    call(ok=True); ctx.synchronize()                   # the same buffers are accepted once the arguments are valid
    assert (c.results()[1][:3] > 0).all() and c.results()[1][3] == SENT
    call(ok=True, nlevels=64, sf=np.concatenate([tc.SCALE, np.ones(56, np.float32)]), sg=np.concatenate([tc.SIGMA2, np.ones(56, np.float32)])); ctx.synchronize()      # the largest table
    assert (c.results()[1][:3] > 0).all()
