"""GPU parity of sslam_bow_transform_batch_dev and sslam_orb_search_by_bow_batch_dev: the vocabulary descent and SearchByBoW for frames in cap
strided device buffers, enqueued on the caller's stream.  Every expectation is the CPU oracle's: oracle.bow_transform, and oracle.search_by_bow on
the CSR lists tests/bow_batch_cases.py builds from the node arrays (its reach is shown in tests/test_bow_batch_cases_cpu.py); one assertion of the
ragged test and one of the end-to-end test check that the library's single call agrees too.  Rows past every count hold random bytes, node ids
and valid flags included; the outputs hold a sentinel before every call.

  test_ragged_batch          five pairs with counts from {0, 1, 63, 64, 65, 129, cap}, check_orientation 0 / 1, nnratio 0.9 / 0.75
  test_node_layouts          one node for everything, one feature per node, nodes of one side only, ids -1 / -5 / 0, ids near 2^30 and 2^31,
                             ids i * W (one wave owns every node) and consecutive ids (every wave walks)
  test_order_dependence      two and three keyframe rows after the same frame row, in both index orders; equal distances; best equal to second
  test_gates                 bestDist1 50 / 51, bestDist1 == nnratio * bestDist2, kf_valid 0
  test_rotation              rotations of 354..360 degrees, max2 < 0.1 * max1, equal features 90 degrees apart in neighbouring pairs
  test_pairs                 one frame slot against four keyframe slots, a repeated keyframe slot, slots out of range, identity, npairs == 0
  test_counts_are_clamped    counts of -3 and capacity + 7 on either side
  test_size_bound            frame capacities 1228 / 1229 (the dynamic-LDS opt-in) and 1638 / 1639 (the frame side leaves LDS), counts at and far below
  test_streams_*             two calls back to back on a side stream; a call beside the synchronous single call
  test_argument_errors       SSLAM_ERR_INVALID leaves the outputs at the sentinel
  test_descent               both vocabularies, levelsup 0 .. L + 1, counts 0 / 1 / 255 / 256 / 257 / cap / -3 / cap + 7, NULL word and weight
  test_descent_errors
  test_frontend_batch        FrontendBatch.search_by_bow on two extractions, B = 3"""
import os
import numpy as np
import pytest
import torch
import pkg
import bow_batch_cases as bc
from synth import synth_frame, warp_prev, synthetic_vocab

pytestmark = pytest.mark.gpu

SENT = -77          # what the outputs hold before a call


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Call:
    """one matcher call: device inputs (kept alive) and sentinel-filled outputs, made by the constructor; launch() enqueues it.
    pairs: [(keyframe slot, frame slot)], or None for the identity with NULL pair arrays"""
    def __init__(self, kf_sides, f_sides, kfcap, cap, pairs=None, seed=99, nkf=None, nf=None, npairs=None):
        rng = np.random.default_rng(seed)
        K, F = bc.pack_sides(rng, kf_sides, kfcap, True), bc.pack_sides(rng, f_sides, cap, False)
        self.kfcap, self.cap, self.nk, self.nfr = kfcap, cap, len(kf_sides), len(f_sides)
        self.npairs = (len(pairs) if pairs is not None else len(f_sides)) if npairs is None else npairs
        self.k = {x: dev(K[x]) for x in ("kp", "desc", "node", "valid")}; self.f = {x: dev(F[x]) for x in ("kp", "desc", "node")}
        self.k["n"] = dev(K["n"] if nkf is None else np.asarray(nkf, np.int32)); self.f["n"] = dev(F["n"] if nf is None else np.asarray(nf, np.int32))
        self.pk = self.pf = None
        if pairs is not None:
            self.pk = dev(np.array([p[0] for p in pairs] + [0], np.int32)); self.pf = dev(np.array([p[1] for p in pairs] + [0], np.int32))
        rows = max(self.npairs, len(pairs) if pairs is not None else 0, 1) + 1          # one row more than the call may write
        self.assigned = torch.full((rows, cap), SENT, dtype=torch.int32, device="cuda"); self.nm = torch.full((rows,), SENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()          # the buffers were filled on torch's stream

    def launch(self, ctx, nnratio=0.9, ori=True, stream=None):
        ctx.search_by_bow_batch_dev(self.k["kp"], self.k["desc"], self.k["node"], self.k["valid"], self.k["n"], self.kfcap, self.nk,
                                    self.f["kp"], self.f["desc"], self.f["node"], self.f["n"], self.cap, self.nfr, self.npairs, self.assigned, self.nm,
                                    d_pair_kf=self.pk, d_pair_f=self.pf, nnratio=nnratio, check_orientation=ori, stream=stream)
        return self

    def results(self):
        """after a synchronise"""
        return self.assigned.cpu().numpy(), self.nm.cpu().numpy()


def check(got, want, nfs, npairs=None):
    """assigned rows and count of pair p against want[p] = (assigned, count), or None for a skipped pair (count 0, no row written); rows at or past the
    frame's count and everything behind the last pair keep the sentinel"""
    a, nm = got
    for p, w in enumerate(want):
        if w is None:
            assert nm[p] == 0 and (a[p] == SENT).all(), p
            continue
        nf = nfs[p]
        np.testing.assert_array_equal(a[p, :nf], w[0], err_msg="pair %d" % p)
        assert nm[p] == w[1], (p, nm[p], w[1])
        assert (a[p, nf:] == SENT).all(), p
    n = len(want) if npairs is None else npairs
    assert (a[n:] == SENT).all() and (nm[n:] == SENT).all()


def run_identity(ctx, oracle, cases, kfcap, cap, nnratio, ori, seed=99):
    """the cases as pairs 0.. of one call with NULL pair arrays -> (got, want)"""
    cs = [dict(c, nnratio=nnratio, ori=ori) for c in cases]
    want = [bc.expect(oracle, c) for c in cs]
    call = Call([c["kf"] for c in cs], [c["f"] for c in cs], kfcap, cap, seed=seed).launch(ctx, nnratio, ori)
    ctx.synchronize()
    got = call.results()
    check(got, want, [len(c["f"]["kp"]) for c in cs])
    return got, want


# ---- 1. a ragged batch
CAP1 = 160
RAGGED_COUNTS = [(CAP1, CAP1), (0, 129), (63, 64), (65, 1), (129, 0)]


@pytest.fixture(scope="module")
def ragged():
    out = []
    for i, (nkf, nf) in enumerate(RAGGED_COUNTS):
        c = bc.from_bow_case(np.random.default_rng(8000 + i), 80)
        assert len(c["kf"]["kp"]) == CAP1 and len(c["f"]["kp"]) == CAP1
        out.append(bc.cut(c, nkf, nf))
    return out


@pytest.mark.parametrize("nnratio", [0.9, 0.75])
@pytest.mark.parametrize("ori", [0, 1])
def test_ragged_batch(ctx, oracle, ragged, ori, nnratio):
    got, want = run_identity(ctx, oracle, ragged, CAP1, CAP1, nnratio, bool(ori))
    assert want[0][1] > 40 and want[2][1] > 5 and want[1][1] == want[4][1] == 0
    # the single call on the first pair's CSR lists agrees as well
    c = ragged[0]
    pk, pf, ik, jf = bc.csr_from_nodes(c["kf"]["node"], c["f"]["node"])
    a, nm = ctx.search_by_bow(c["kf"]["kp"], c["kf"]["desc"], c["kf"]["valid"], c["f"]["kp"], c["f"]["desc"], pk, pf, ik, jf, nnratio, bool(ori))
    np.testing.assert_array_equal(a, got[0][0, :CAP1]); assert nm == got[1][0]


# ---- 2. node layouts
def test_node_layouts(ctx, oracle):
    L = bc.layout_cases(np.random.default_rng(7100))
    got, want = run_identity(ctx, oracle, list(L.values()), 150, 150, 0.9, True)
    assert all(w[1] > 5 for w in want)


# ---- 3. order dependence
def test_order_dependence(ctx, oracle):
    chains = [bc.chain_case(np.random.default_rng(7200 + m), m, rev) for m in (2, 3) for rev in (False, True)]
    cases = chains + [bc.tie_case(np.random.default_rng(7210), 0.9)]
    got, want = run_identity(ctx, oracle, cases, 48, 48, 0.9, True)
    for p, c in enumerate(chains):                        # the generator's promise, on the library's answer: the j-th visited chain row holds f_j
        krows, frows = c["chain"]
        assert [int(got[0][p, j]) for j in frows] == np.sort(krows).tolist()
    kr, fr = cases[4]["tie"]
    assert (got[0][4, fr] == -1).all()
    got, want = run_identity(ctx, oracle, [bc.tie_case(np.random.default_rng(7210), 1.2)], 48, 48, 1.2, True)
    assert got[0][0, fr[0]] == kr and got[0][0, fr[1]] == -1


# ---- 4. gates
def test_gates(ctx, oracle):
    T = bc.threshold_cases(np.random.default_rng(7300))
    for nnratio in (0.9, 0.75):
        names = [k for k, (c, _) in T.items() if c["nnratio"] == nnratio]
        got, want = run_identity(ctx, oracle, [T[k][0] for k in names], 16, 16, nnratio, True)
        for p, k in enumerate(names):
            kf_row, j1, _ = T[k][0]["th"]
            assert (got[0][p, j1] == kf_row) == T[k][1], k


# ---- 5. rotation
def test_rotation(ctx, oracle):
    c0, c1 = bc.rot_neighbours()
    cases = [bc.rot_case(np.random.default_rng(7400), [(30, 354, 360), (12, 95, 104), (8, 200, 209), (5, 230, 239)]), c0, c1,
             bc.rot_case(np.random.default_rng(7401), [(40, 30, 44), (3, 150, 160), (2, 230, 239)])]
    got, want = run_identity(ctx, oracle, cases, 64, 64, 0.9, True)
    assert [w[1] for w in want] == [50, 44, 44, 40]
    got, want = run_identity(ctx, oracle, cases, 64, 64, 0.9, False)
    assert [w[1] for w in want] == [55, 50, 50, 45]


# ---- 6. pairs
@pytest.fixture(scope="module")
def slots():
    """four keyframe sides and three frame sides over one set of node ids, so that any keyframe slot matches any frame slot"""
    rng = np.random.default_rng(8100)
    f_sides = [bc.node_pair(rng, rng.integers(0, 30, 4), rng.integers(0, 30, n))["f"] for n in (90, 70, 96)]
    kf_sides = []
    for i, n in enumerate((80, 96, 96, 66)):          # keyframe side i holds noisy copies of frame side i % 3
        f = f_sides[i % 3]
        node = rng.integers(0, 30, n).astype(np.int32)
        c = bc.node_pair(rng, node, f["node"])              # (its frame side is discarded: the copies below are of f itself)
        src = np.array([rng.choice(np.flatnonzero(f["node"] == nd)) if (f["node"] == nd).any() else -1 for nd in node])
        has = src >= 0
        c["kf"]["desc"][has] = bc.mc.flip_bits(rng, f["desc"][src[has]], 40); c["kf"]["kp"]["angle"][has] = f["kp"]["angle"][src[has]]
        kf_sides.append(c["kf"])
    return kf_sides, f_sides


def pair_want(oracle, slots, pairs, nnratio=0.9, ori=True):
    kf_sides, f_sides = slots
    return [bc.expect(oracle, bc.case(kf_sides[k], f_sides[f], nnratio, ori)) if 0 <= k < len(kf_sides) and 0 <= f < len(f_sides) else None for k, f in pairs]


def test_pairs(ctx, oracle, slots):
    kf_sides, f_sides = slots
    nfs = lambda pairs: [len(f_sides[f]["kp"]) if 0 <= f < 3 else 0 for _, f in pairs]
    # Relocalization: the one frame slot against four keyframe slots
    pairs = [(0, 0), (1, 0), (2, 0), (3, 0)]
    want = pair_want(oracle, slots, pairs)
    assert sum(w[1] for w in want) > 40
    c = Call(kf_sides, f_sides[:1], 96, 96, pairs).launch(ctx); ctx.synchronize()
    check(c.results(), want, nfs(pairs))
    # a repeated keyframe slot, a repeated frame slot, slots out of range on either side
    pairs = [(0, 0), (0, 1), (3, 0), (-1, 0), (4, 1), (2, 3), (0, -2), (0, 0), (1 << 30, 0)]
    want = pair_want(oracle, slots, pairs)
    assert [w is None for w in want] == [False, False, False, True, True, True, True, False, True] and want[0][1] > 10 and want[2][1] > 10
    c = Call(kf_sides, f_sides, 96, 96, pairs).launch(ctx); ctx.synchronize()
    check(c.results(), want, nfs(pairs))
    # identity on one side only: keyframe slot p against frame slot d_pair_f[p]
    c = Call(kf_sides[:3], f_sides, 96, 96, [(0, 2), (1, 0), (2, 1)]); c.pk = None
    c.launch(ctx); ctx.synchronize()
    check(c.results(), pair_want(oracle, slots, [(0, 2), (1, 0), (2, 1)]), [96, 90, 70])
    # identity with both arrays NULL
    c = Call(kf_sides[:3], f_sides, 96, 96).launch(ctx); ctx.synchronize()
    check(c.results(), pair_want(oracle, slots, [(0, 0), (1, 1), (2, 2)]), [90, 70, 96])
    # no pair at all
    c = Call(kf_sides, f_sides, 96, 96, [(0, 0)], npairs=0).launch(ctx); ctx.synchronize()
    check(c.results(), [], [], 0)


def test_counts_are_clamped(ctx, oracle, slots):
    kf_sides, f_sides = slots
    kf = [kf_sides[2], kf_sides[2], kf_sides[2], kf_sides[0]]; f = [f_sides[2], f_sides[2], f_sides[2], f_sides[0]]          # sides of 96 rows fill their slots
    nkf, nf = [96 + 7, -3, 96, 80], [96 + 7, 96, -3, 90]
    empty_kf = {k: v[:0] for k, v in kf_sides[2].items()}; empty_f = {k: v[:0] for k, v in f_sides[2].items()}
    seen = [bc.case(kf[0], f[0]), bc.case(empty_kf, f[1]), bc.case(kf[2], empty_f), bc.case(kf[3], f[3])]
    want = [bc.expect(oracle, c) for c in seen]
    assert want[0][1] > 10 and want[1][1] == 0 and want[2][1] == 0 and want[3][1] > 10
    c = Call(kf, f, 96, 96, nkf=nkf, nf=nf).launch(ctx); ctx.synchronize()
    check(c.results(), want, [96, 96, 0, 90])


# ---- 7. the size bound of the plan
@pytest.mark.parametrize("cap", [1228, 1229, bc.LDS_CAP, bc.LDS_CAP + 1])
def test_size_bound(ctx, oracle, cap):
    """40 * 1228 bytes is the last launch without the dynamic-LDS opt-in, 40 * 1638 = 64 KB the last frame capacity in LDS.  One pair fills both
    capacities (which differ: the strides are the sides' own), the other uses 200 rows; at most 3 rows per node"""
    assert bc.ROW_BYTES * bc.LDS_CAP <= bc.LDS_MAX < bc.ROW_BYTES * (bc.LDS_CAP + 1) and bc.ROW_BYTES * 1228 <= 48 * 1024 < bc.ROW_BYTES * 1229
    rng = np.random.default_rng(8200 + cap)
    kfcap = cap + 3
    full = bc.node_pair(rng, rng.permutation(kfcap) // 3, rng.permutation(cap) // 3)
    small = bc.node_pair(rng, 5000 + rng.permutation(200) // 2, 5000 + rng.permutation(200) // 3)
    cases = [full, small]
    want = [bc.expect(oracle, c) for c in cases]
    assert want[0][1] > 300 and want[1][1] > 40
    c = Call([x["kf"] for x in cases], [x["f"] for x in cases], kfcap, cap).launch(ctx); ctx.synchronize()
    check(c.results(), want, [cap, 200])


# ---- 8. streams
@pytest.fixture(scope="module")
def two_calls(oracle):
    A = [bc.from_bow_case(np.random.default_rng(8300 + i), 40 + 5 * i) for i in range(4)]
    B = [bc.node_pair(np.random.default_rng(8310 + i), np.random.default_rng(8320 + i).integers(0, 20, 100 + 9 * i), np.random.default_rng(8330 + i).integers(0, 20, 120 - 7 * i))
         for i in range(3)]
    cap = 130
    assert max(len(c[s]["kp"]) for c in A + B for s in ("kf", "f")) <= cap
    return dict(A=A, B=B, cap=cap, wantA=[bc.expect(oracle, c) for c in A], wantB=[bc.expect(oracle, c) for c in B])


def test_streams_back_to_back(ctx, two_calls):
    t = two_calls
    s = torch.cuda.Stream()
    c1 = Call([c["kf"] for c in t["A"]], [c["f"] for c in t["A"]], t["cap"], t["cap"])
    c2 = Call([c["kf"] for c in t["B"]], [c["f"] for c in t["B"]], t["cap"], t["cap"], seed=98)
    c1.launch(ctx, stream=s.cuda_stream); c2.launch(ctx, stream=s.cuda_stream)
    s.synchronize()
    check(c1.results(), t["wantA"], [len(c["f"]["kp"]) for c in t["A"]]); check(c2.results(), t["wantB"], [len(c["f"]["kp"]) for c in t["B"]])


def test_streams_batch_beside_the_synchronous_call(ctx, two_calls):
    t = two_calls
    s = torch.cuda.Stream()
    c = t["B"][1]
    pk, pf, ik, jf = bc.csr_from_nodes(c["kf"]["node"], c["f"]["node"])
    c1 = Call([x["kf"] for x in t["A"]], [x["f"] for x in t["A"]], t["cap"], t["cap"]).launch(ctx, stream=s.cuda_stream)
    a, nm = ctx.search_by_bow(c["kf"]["kp"], c["kf"]["desc"], c["kf"]["valid"], c["f"]["kp"], c["f"]["desc"], pk, pf, ik, jf, 0.9, True)      # on the context stream
    s.synchronize()
    check(c1.results(), t["wantA"], [len(x["f"]["kp"]) for x in t["A"]])
    np.testing.assert_array_equal(a, t["wantB"][1][0]); assert nm == t["wantB"][1][1]


# ---- 9. argument errors
def test_argument_errors(fe, ctx, slots):
    kf_sides, f_sides = slots
    c = Call(kf_sides[:3], f_sides, 96, 96, [(0, 0), (1, 1), (2, 2)])
    base = dict(kf_kp=c.k["kp"], kf_desc=c.k["desc"], kf_node=c.k["node"], kf_valid=c.k["valid"], nkf=c.k["n"], kfcap=96, nk=3,
                f_kp=c.f["kp"], f_desc=c.f["desc"], f_node=c.f["node"], nf=c.f["n"], cap=96, nfr=3, npairs=3, assigned=c.assigned, nm=c.nm, pk=c.pk, pf=c.pf)

    def call(ok=False, **kw):
        a = dict(base, **kw)
        args = (a["kf_kp"], a["kf_desc"], a["kf_node"], a["kf_valid"], a["nkf"], a["kfcap"], a["nk"], a["f_kp"], a["f_desc"], a["f_node"], a["nf"], a["cap"], a["nfr"],
                a["npairs"], a["assigned"], a["nm"])
        if ok:
            return ctx.search_by_bow_batch_dev(*args, d_pair_kf=a["pk"], d_pair_f=a["pf"])
        with pytest.raises(fe.SslamError) as e:
            ctx.search_by_bow_batch_dev(*args, d_pair_kf=a["pk"], d_pair_f=a["pf"])
        assert e.value.code == fe.SSLAM_ERR_INVALID
    for name in ("kf_kp", "kf_desc", "kf_node", "kf_valid", "nkf", "f_kp", "f_desc", "f_node", "nf", "assigned", "nm"):
        call(**{name: None})
    for name in ("kfcap", "cap", "nk", "nfr", "npairs"):
        call(**{name: -1})
    call(kfcap=1 << 19); call(cap=1 << 19)
    call(kf_desc=c.k["desc"].data_ptr() + 8); call(f_desc=c.f["desc"].data_ptr() + 4)          # descriptor rows are read as 16-byte words
    call(kf_node=c.k["node"].data_ptr() + 2); call(nm=c.nm.data_ptr() + 1); call(pk=c.pk.data_ptr() + 2)
    call(pk=None, nk=4, kf_kp=c.k["kp"]); call(pf=None, nfr=2); call(pk=None, pf=None, npairs=2)      # identity needs that side's slot count to equal npairs
    ctx.synchronize(); torch.cuda.synchronize()
    a, nm = c.results()
    assert (a == SENT).all() and (nm == SENT).all()
    call(ok=True); ctx.synchronize()                   # the same buffers are accepted once the arguments are valid
    assert (c.results()[1][:3] >= 0).all()


# ---- 10. the descent
VOCABS = {"k10_L4": (5, 10, 4), "k3_L2": (6, 3, 2)}


@pytest.fixture(scope="module", params=sorted(VOCABS))
def vocab(request, fe, ctx):
    seed, k, L = VOCABS[request.param]
    arrays = synthetic_vocab(np.random.default_rng(seed), k=k, L=L)
    voc = fe.Vocabulary(ctx, *arrays)
    yield arrays, voc
    voc.close()


def test_descent(ctx, oracle, vocab):
    (L, ptr, ch, nd, word, weight), voc = vocab
    cap = 300
    counts = [0, 1, 255, 256, 257, cap, -3, cap + 7]
    real = [min(max(c, 0), cap) for c in counts]
    B = len(counts)
    rng = np.random.default_rng(8400 + L)
    desc = bc.mc.rand_desc(rng, B * cap).reshape(B, cap, 32)          # rows past a count stay random
    for f, n in enumerate(real):
        m = n // 3
        if m: desc[f, :m] = nd[rng.integers(1, len(nd), m)]           # exact node descriptors: distance-0 ties between equal children are decided by order
    d_desc, d_n = dev(desc), dev(np.array(counts, np.int32))
    for levelsup in range(L + 2):
        want = [oracle.bow_transform(L, ptr, ch, nd, word, weight, desc[f, :n], levelsup) for f, n in enumerate(real)]
        for with_word, with_weight in ((True, True), (False, False)) if levelsup in (0, 2) else ((True, True),):
            w = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda"); v = torch.full((B, cap), float(SENT), dtype=torch.float64, device="cuda")
            n_ = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.bow_transform_batch_dev(voc, d_desc, d_n, cap, B, n_, w if with_word else None, v if with_weight else None, levelsup=levelsup)
            ctx.synchronize()
            w, v, n_ = w.cpu().numpy(), v.cpu().numpy(), n_.cpu().numpy()
            for f, n in enumerate(real):
                ow, ov, on = want[f]
                np.testing.assert_array_equal(n_[f, :n], on)
                assert (n_[f, n:] == SENT).all()
                if with_word:
                    np.testing.assert_array_equal(w[f, :n], ow); np.testing.assert_array_equal(v[f, :n].view(np.uint64), ov.view(np.uint64))      # weights as bit patterns
                assert (w[f, n if with_word else 0:] == SENT).all() and (v[f, n if with_weight else 0:] == float(SENT)).all()
        if levelsup >= L: assert all((on == 0).all() for _, _, on in want)             # the word lies above the level asked for
        elif levelsup == 0: assert len(np.unique(np.concatenate([on for _, _, on in want]))) > (30 if L == 4 else 4)
    # the single call agrees, and a frame count of zero frames enqueues nothing
    sw, sv, sn = voc.transform(desc[5], 2 if L == 4 else 1)
    ow, ov, on = oracle.bow_transform(L, ptr, ch, nd, word, weight, desc[5], 2 if L == 4 else 1)
    np.testing.assert_array_equal(sw, ow); np.testing.assert_array_equal(sn, on)
    n_ = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda"); torch.cuda.synchronize()
    ctx.bow_transform_batch_dev(voc, d_desc, d_n, cap, 0, n_); ctx.bow_transform_batch_dev(voc, d_desc, d_n, 0, B, n_); ctx.synchronize()
    assert (n_.cpu().numpy() == SENT).all()


def test_descent_errors(fe, ctx, vocab):
    _, voc = vocab
    cap, B = 64, 2
    d_desc = dev(bc.mc.rand_desc(np.random.default_rng(1), B * cap + 1)); d_n = dev(np.array([64, 10], np.int32))
    node = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda"); w = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(voc=voc, desc=d_desc, n=d_n, cap=cap, B=B, node=node, levelsup=4):
        with pytest.raises(fe.SslamError) as e:
            ctx.bow_transform_batch_dev(voc, desc, n, cap, B, node, w, None, levelsup=levelsup)
        assert e.value.code == fe.SSLAM_ERR_INVALID
    call(voc=None); call(desc=None); call(n=None); call(node=None); call(cap=-1); call(B=-1)
    call(cap=1 << 16, B=1 << 15)                       # nframes * cap = 2^31
    call(desc=d_desc.data_ptr() + 8)                   # not 16-byte aligned
    ctx.synchronize(); torch.cuda.synchronize()
    assert (node.cpu().numpy() == SENT).all() and (w.cpu().numpy() == SENT).all()
    ctx.bow_transform_batch_dev(voc, d_desc, d_n, cap, B, node, w, None); ctx.synchronize()
    assert (node.cpu().numpy()[1, :10] >= 0).all() and (node.cpu().numpy()[1, 10:] == SENT).all()


# ---- 11. the pipeline's method
def test_frontend_batch(fe, ctx, oracle):
    pipeline = pkg._load("sslam_pipeline", os.path.join(pkg.PKG_DIR, "pipeline.py"))
    w, h, B, levelsup = 320, 240, 3, 2
    L, ptr, ch, nd, word, weight = synthetic_vocab(np.random.default_rng(5), k=10, L=4)
    weight = np.where(weight > 0, weight, 1.0)           # no stopped words: host compute_bow drops their features from the FeatureVector, the node arrays keep them
    voc = fe.Vocabulary(ctx, L, ptr, ch, nd, word, weight)
    cur = [synth_frame(8500 + i, w, h, nshapes=14 + 5 * i, nstrokes=4 + 2 * i) for i in range(B)]
    prev = [warp_prev(c) for c in cur]
    pipe = pipeline.FrontendBatch(fe, ctx, w, h, B, 500, 100, "cuda:0", with_lines=False)
    assert not hasattr(pipe, "_bow")                     # nothing held for the matcher until it is used
    pipe.extract(torch.from_numpy(np.stack(prev)).cuda(), "prev"); pipe.extract(torch.from_numpy(np.stack(cur)).cuda(), "cur")
    rng = np.random.default_rng(8500)
    valid = (rng.random((B, pipe.cap)) < 0.9).astype(np.uint8)
    a, nm = pipe.search_by_bow(voc, torch.from_numpy(valid).cuda(), nnratio=0.7, check_orientation=True, levelsup=levelsup)
    torch.cuda.synchronize()
    assert a.shape == (B, pipe.cap) and nm.shape == (B,)
    a, nm = a.cpu().numpy(), nm.cpu().numpy()
    for i in range(B):
        side = {}
        for tag in ("prev", "cur"):
            f = pipe.feat[tag]
            n = int(f["n"][i].item())
            kp = f["kp"][i, :n].cpu().numpy().view(np.uint8).reshape(n, -1).copy().view(fe.KP_DTYPE).reshape(-1); d = f["desc"][i, :n].cpu().numpy()
            side[tag] = bc.side(kp, d, oracle.bow_transform(L, ptr, ch, nd, word, weight, d, levelsup)[2], valid[i, :n])
        c = bc.case(side["prev"], side["cur"], 0.7, True)
        oa, on = bc.expect(oracle, c)                      # oracle descent + oracle matcher
        nf = len(c["f"]["kp"])
        assert on > 20 and nf > 100, (i, on, nf)
        np.testing.assert_array_equal(a[i, :nf], oa); assert nm[i] == on
        # host compute_bow's FeatureVectors fed to the single call
        fv1, fv2 = voc.compute_bow(c["kf"]["desc"], levelsup)[1], voc.compute_bow(c["f"]["desc"], levelsup)[1]
        shared = sorted(set(fv1) & set(fv2))
        pk = np.cumsum([0] + [len(fv1[k]) for k in shared]).astype(np.int32); pf = np.cumsum([0] + [len(fv2[k]) for k in shared]).astype(np.int32)
        ik = np.array(sum((fv1[k] for k in shared), []), np.int32); jf = np.array(sum((fv2[k] for k in shared), []), np.int32)
        sa, sn = ctx.search_by_bow(c["kf"]["kp"], c["kf"]["desc"], c["kf"]["valid"], c["f"]["kp"], c["f"]["desc"], pk, pf, ik, jf, 0.7, True)
        np.testing.assert_array_equal(sa, a[i, :nf]); assert sn == nm[i]
    a2, nm2 = pipe.search_by_bow(voc, None, nnratio=0.7, levelsup=levelsup)          # every prev keypoint valid; the pipeline's own buffers again
    torch.cuda.synchronize()
    assert a2.data_ptr() == pipe._bow["assigned"].data_ptr() and (nm2.cpu().numpy() >= nm).all()
    pipe.close(); voc.close()
