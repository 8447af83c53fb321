"""GPU parity of sslam_orb_search_by_bow_keyframes_batch_dev: ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) for pairs of slots of one
device-resident keyframe pool, enqueued on the caller's stream.  Every expectation is the CPU oracle's search_by_bow_keyframes on the CSR lists
tests/bow_kf_batch_cases.py builds from the node arrays (its reach is shown in tests/test_bow_kf_batch_cases_cpu.py); every comparison is exact.  Rows
past every count hold random bytes, node ids and validity flags included; the outputs hold a sentinel before every call, and every check also holds
d_matches21 against the inverse of d_matches12 and d_nmatches against the number of rows >= 0.

  test_ragged_batch          counts {0, 1, 2, 63, 64, 65, 127, 128, 129, cap} on both sides, nnratio 0.75 / 0.9, with and without the rotation check; the
                             single call sslam_orb_search_by_bow_keyframes on the same node arrays' CSR lists agrees row for row
  test_every_case            validity, chains, gates, rotation (bins, 10 % rule, bin edges, operand order), node layouts: at both ratios, with and without
                             the check, and at the ratios the gate cases are made for
  test_valid_null            d_valid == NULL
  test_pairs                 one keyframe against 20 candidates, (a, b) beside (b, a), kf1 == kf2, slots out of range and negative, npairs == 0
  test_counts_are_clamped    counts of -3 and cap + 7
  test_forms_and_bounds      caps 1228 / 1229 (the dynamic-LDS opt-in) and 1638 / 1639 (keyframe 2 leaves the LDS): the same rows from every cap
  test_streams_*             two calls on two streams; a call beside the synchronous single call
  test_argument_errors       every SSLAM_ERR_INVALID rule leaves the outputs at the sentinel
  test_end_to_end            batch extractor -> sslam_undistort_keypoints_batch_dev (k1 = 0) -> sslam_bow_transform_batch_dev -> the new call"""
import numpy as np
import pytest
import torch
import bow_batch_cases as bc
import bow_kf_batch_cases as kc
from synth import synth_frame, warp_prev, synthetic_vocab

pytestmark = pytest.mark.gpu

SENT = -77          # what the outputs hold before a call


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Call:
    """one matcher call: the pool on the device (kept alive) and sentinel-filled outputs, made by the constructor; launch() enqueues it.
    pairs: [(kf1 slot, kf2 slot)]"""
    def __init__(self, sides, cap, pairs, seed=99, n=None, npairs=None):
        rng = np.random.default_rng(seed)
        P = kc.pack_pool(rng, sides, cap)
        self.cap, self.nk = cap, len(sides)
        self.npairs = len(pairs) if npairs is None else npairs
        self.d = {x: dev(P[x]) for x in ("kp", "desc", "node", "valid")}
        self.n = dev(P["n"] if n is None else np.asarray(n, np.int32))
        self.pairs = dev(np.array(list(pairs) + [(0, 0)], np.int32).reshape(-1, 2))          # one pair more than the call may read
        rows = max(self.npairs, len(pairs), 1) + 1                                           # one row more than the call may write
        self.m12 = torch.full((rows, cap), SENT, dtype=torch.int32, device="cuda"); self.m21 = torch.full((rows, cap), SENT, dtype=torch.int32, device="cuda")
        self.nm = torch.full((rows,), SENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()          # the buffers were filled on torch's stream

    def launch(self, ctx, nnratio=0.75, ori=True, stream=None, valid=True):
        ctx.search_by_bow_keyframes_batch_dev(self.d["kp"], self.d["desc"], self.d["node"], self.n, self.cap, self.nk, self.pairs, self.npairs,
                                              self.m12, self.m21, self.nm, d_valid=self.d["valid"] if valid else None, nnratio=nnratio,
                                              check_orientation=ori, stream=stream)
        return self

    def results(self):
        """after a synchronise"""
        return self.m12.cpu().numpy(), self.m21.cpu().numpy(), self.nm.cpu().numpy()


def check(got, want, counts, npairs=None):
    """the rows and count of pair p against want[p] = (matches12, matches21, count), or None for a skipped pair (count 0, no row written); counts[p] =
    (n1, n2).  Rows at or past a count and everything behind the last pair keep the sentinel; matches21 is the inverse of matches12 and the count the
    number of rows >= 0, whatever the oracle says"""
    m12, m21, nm = got
    for p, w in enumerate(want):
        if w is None:
            assert nm[p] == 0 and (m12[p] == SENT).all() and (m21[p] == SENT).all(), p
            continue
        n1, n2 = counts[p]
        assert (m12[p, n1:] == SENT).all() and (m21[p, n2:] == SENT).all(), p
        np.testing.assert_array_equal(m21[p, :n2], kc.inverse(m12[p, :n1], n2), err_msg="pair %d: matches21 is not the inverse of matches12" % p)
        assert nm[p] == (m12[p, :n1] >= 0).sum() == (m21[p, :n2] >= 0).sum(), p
        np.testing.assert_array_equal(m12[p, :n1], w[0], err_msg="pair %d" % p)
        np.testing.assert_array_equal(m21[p, :n2], w[1], err_msg="pair %d" % p)
        assert nm[p] == w[2], (p, nm[p], w[2])
    n = len(want) if npairs is None else npairs
    assert (m12[n:] == SENT).all() and (m21[n:] == SENT).all() and (nm[n:] == SENT).all()


def counts_of(cases):
    return [(len(c["k1"]["kp"]), len(c["k2"]["kp"])) for c in cases]


def run_cases(ctx, oracle, cases, cap, nnratio, ori, seed=99, valid=True):
    """the cases as pairs (2p, 2p + 1) of one pool and one call -> (got, want)"""
    want = [kc.expect(oracle, c, nnratio, ori) for c in cases]
    sides, pairs = kc.pool_of_cases(cases)
    call = Call(sides, cap, pairs, seed=seed).launch(ctx, nnratio, ori, valid=valid)
    ctx.synchronize()
    got = call.results()
    check(got, want, counts_of(cases))
    return got, want


# ---- 1. a ragged batch
@pytest.fixture(scope="module")
def ragged():
    return kc.ragged_cases()


@pytest.mark.parametrize("nnratio", [0.75, 0.9])
@pytest.mark.parametrize("ori", [0, 1])
def test_ragged_batch(ctx, oracle, ragged, ori, nnratio):
    got, want = run_cases(ctx, oracle, ragged, kc.RAGGED_CAP, nnratio, bool(ori))
    assert want[0][2] > 40 and want[1][2] == want[2][2] == 0 and min(w[2] for w in want[5:]) > 10
    # the single call on every pair's CSR lists agrees row for row
    for p, c in enumerate(ragged):
        n1, n2 = len(c["k1"]["kp"]), len(c["k2"]["kp"])
        p1, p2, i1, i2 = bc.csr_from_nodes(c["k1"]["node"], c["k2"]["node"])
        if n1 == 0 or n2 == 0 or len(p1) == 1: continue
        m, nm = ctx.search_by_bow_keyframes(c["k1"]["kp"], c["k1"]["desc"], c["k1"]["valid"], c["k2"]["kp"], c["k2"]["desc"], c["k2"]["valid"], p1, p2, i1, i2,
                                            nnratio, bool(ori))
        np.testing.assert_array_equal(m, got[0][p, :n1], err_msg="pair %d" % p); assert nm == got[2][p]


# ---- 2. every crafted case
@pytest.fixture(scope="module")
def crafted():
    out = {"valid_" + k: v[0] for k, v in kc.validity_cases(np.random.default_rng(9250)).items()}
    out.update({k: v[0] for k, v in kc.chain_cases().items()})
    out.update({"gate_" + k: v[0] for k, v in kc.gate_cases().items()})
    out.update({"rot_" + k: v[0] for k, v in kc.rot_cases().items()})
    out.update({"edge_" + k: v[0] for k, v in kc.rot_edge_cases().items()})
    out.update({"layout_" + k: v for k, v in kc.layout_cases(np.random.default_rng(9600)).items()})
    return out


@pytest.mark.parametrize("nnratio,ori", [(0.75, 1), (0.75, 0), (0.9, 1), (0.9, 0), (0.15, 1), (1.2, 1)])
def test_every_case(ctx, oracle, crafted, nnratio, ori):
    names = sorted(crafted)
    cases = [crafted[k] for k in names]
    got, want = run_cases(ctx, oracle, cases, 150, nnratio, bool(ori))
    nm = dict(zip(names, (w[2] for w in want)))
    assert sum(nm.values()) > 300
    ans = lambda k: {p: (int(np.flatnonzero(crafted[k]["rows"][1] == got[0][names.index(k), i])[0]) if got[0][names.index(k), i] >= 0 else -1)
                     for p, i in enumerate(crafted[k]["rows"][0])}
    if (nnratio, ori) == (0.75, 1):      # the generators' promises, on the library's answer
        assert [ans("gate_dist_%d" % d)[0] for d in (49, 50, 51)] == [0, -1, -1] and ans("gate_ratio_30_40")[0] == -1 and ans("gate_ratio_29_40")[0] == 0
        assert ans("valid_k1_invalid_would_win") == {0: -1, 1: 0} and ans("valid_k2_invalid_best") == {0: 1} and ans("valid_k2_invalid_second") == {0: 0}
        assert ans("taken_second") == {0: 0, 1: 1} and ans("gate_tie_fails")[0] == -1
        assert [nm["rot_" + k] for k in ("three_bins", "four_bins", "six_bins", "tenth_second_stays", "tenth_both_go", "operand_order")] == [36, 50, 34, 44, 40, 22]
    if nnratio == 0.15: assert ans("gate_single_38")[0] == 0 and ans("gate_single_39")[0] == -1
    if nnratio == 1.2: assert ans("gate_tie_lower_index")[0] == 1


def test_valid_null(ctx, oracle, ragged):
    """d_valid == NULL: every row of both sides is valid"""
    cases = [dict(c, k1=kc.with_valid(c["k1"]), k2=kc.with_valid(c["k2"])) for c in ragged[:1] + ragged[5:8]]
    flagged = [kc.expect(oracle, c) for c in ragged[:1] + ragged[5:8]]
    got, want = run_cases(ctx, oracle, cases, kc.RAGGED_CAP, 0.75, True, valid=False)          # the pool still holds the flags; the call is not given them
    assert any(not np.array_equal(w[0], f[0]) for w, f in zip(want, flagged))


# ---- 3. pair lists
@pytest.fixture(scope="module")
def pool():
    return kc.pool_sides(np.random.default_rng(9700), (90, 70, 96) + tuple(40 + 3 * i for i in range(19)))      # 22 slots: slot 0 and 21 others


def pair_want(oracle, pool, pairs, nnratio=0.75, ori=True):
    return [kc.expect(oracle, kc.case(pool[a], pool[b], nnratio, ori)) if 0 <= a < len(pool) and 0 <= b < len(pool) else None for a, b in pairs]


def pair_counts(pool, pairs):
    return [(len(pool[a]["kp"]), len(pool[b]["kp"])) if 0 <= a < len(pool) and 0 <= b < len(pool) else (0, 0) for a, b in pairs]


def test_pairs(ctx, oracle, pool):
    # one loop closure: the current keyframe against 20 candidates in one call
    pairs = [(0, k) for k in range(1, 21)]
    want = pair_want(oracle, pool, pairs)
    assert min(w[2] for w in want) > 3 and len({w[0].tobytes() for w in want}) == 20
    c = Call(pool, 96, pairs).launch(ctx); ctx.synchronize()
    check(c.results(), want, pair_counts(pool, pairs))
    # (a, b) beside (b, a), kf1 == kf2, a repeated pair, slots out of range and negative
    pairs = [(1, 2), (2, 1), (0, 0), (2, 2), (-1, 0), (0, 22), (22, 0), (0, -2), (1, 2), (1 << 30, 1), (21, 0)]
    want = pair_want(oracle, pool, pairs)
    assert [w is None for w in want] == [False, False, False, False, True, True, True, True, False, True, False]
    assert not np.array_equal(want[0][0], want[1][1]) and want[2][2] > 40
    c = Call(pool, 96, pairs).launch(ctx); ctx.synchronize()
    check(c.results(), want, pair_counts(pool, pairs))
    # no pair at all
    c = Call(pool, 96, [(0, 1)], npairs=0).launch(ctx); ctx.synchronize()
    check(c.results(), [], [], 0)


def test_counts_are_clamped(ctx, oracle, pool):
    sides = [pool[2], pool[2], pool[2], pool[0]]          # pool[2] fills its slot of 96 rows
    n = [96 + 7, -3, 96, 90]
    empty = {k: v[:0] for k, v in pool[2].items()}
    pairs = [(0, 2), (1, 2), (2, 1), (3, 0), (0, 3)]
    seen = [kc.case(pool[2], pool[2]), kc.case(empty, pool[2]), kc.case(pool[2], empty), kc.case(pool[0], pool[2]), kc.case(pool[2], pool[0])]
    want = [kc.expect(oracle, c) for c in seen]
    assert want[0][2] > 40 and want[1][2] == 0 and want[2][2] == 0 and want[3][2] > 10
    c = Call(sides, 96, pairs, n=n).launch(ctx); ctx.synchronize()
    check(c.results(), want, [(96, 96), (0, 96), (96, 0), (90, 96), (96, 90)])


# ---- 4. both forms, and the bounds of the plan
def test_forms_and_bounds(ctx, oracle, ragged, pool):
    """40 * 1228 bytes is the last launch without the dynamic-LDS opt-in, 40 * 1638 the last capacity with keyframe 2 in LDS; a few dozen to 160 live
    rows per slot, the same pool at every capacity: the same rows from every form"""
    assert kc.ROW_BYTES * kc.LDS_CAP <= kc.LDS_MAX < kc.ROW_BYTES * (kc.LDS_CAP + 1) and kc.ROW_BYTES * kc.OPT_IN_CAP <= 48 * 1024 < kc.ROW_BYTES * (kc.OPT_IN_CAP + 1)
    chains = kc.chain_cases()
    cases = [ragged[0], ragged[8], ragged[9], chains["chain_3_rev"][0], chains["taken_second"][0], kc.case(pool[0], pool[1]), kc.case(pool[2], pool[2])]
    want = [kc.expect(oracle, c) for c in cases]
    assert want[0][2] > 40 and want[6][2] > 40
    sides, pairs = kc.pool_of_cases(cases)
    pairs = pairs + [(1, 0), (99, 0)]                      # the first pair the other way round, and a skipped pair
    want = want + [kc.expect(oracle, kc.case(cases[0]["k2"], cases[0]["k1"])), None]
    counts = counts_of(cases) + [counts_of(cases)[0][::-1], (0, 0)]
    seen = {}
    for cap in (kc.OPT_IN_CAP, kc.OPT_IN_CAP + 1, kc.LDS_CAP, kc.LDS_CAP + 1):
        c = Call(sides, cap, pairs, seed=cap).launch(ctx); ctx.synchronize()
        got = c.results()
        check(got, want, counts)
        seen[cap] = [(got[0][p, :n1].copy(), got[1][p, :n2].copy(), got[2][p]) for p, (n1, n2) in enumerate(counts)]
    for cap in seen:
        for a, b in zip(seen[cap], seen[kc.LDS_CAP]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # one slot filled to the first capacity past the LDS: every row of the global-memory form's strides is walked
    cap = kc.LDS_CAP + 1
    rng = np.random.default_rng(9800)
    full = kc.node_pair(rng, rng.permutation(cap) // 3, rng.permutation(cap) // 3)
    w = kc.expect(oracle, full)
    assert w[2] > 300
    c = Call([full["k1"], full["k2"]], cap, [(0, 1), (1, 0)]).launch(ctx); ctx.synchronize()
    check(c.results(), [w, kc.expect(oracle, kc.case(full["k2"], full["k1"]))], [(cap, cap), (cap, cap)])


# ---- 5. streams
@pytest.fixture(scope="module")
def two_calls(oracle, pool):
    pa = [(0, 1), (1, 2), (2, 0), (3, 3)]; pb = [(2, 1), (0, 2), (1, 1)]
    return dict(pa=pa, pb=pb, wantA=pair_want(oracle, pool, pa), wantB=pair_want(oracle, pool, pb, 0.9, False))


def test_streams_two_calls_on_two_streams(ctx, pool, two_calls):
    t = two_calls
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c1 = Call(pool, 96, t["pa"]); c2 = Call(pool, 96, t["pb"], seed=98)
    c1.launch(ctx, stream=s1.cuda_stream); c2.launch(ctx, 0.9, False, stream=s2.cuda_stream)
    s1.synchronize(); s2.synchronize()
    check(c1.results(), t["wantA"], pair_counts(pool, t["pa"])); check(c2.results(), t["wantB"], pair_counts(pool, t["pb"]))


def test_streams_batch_beside_the_synchronous_call(ctx, oracle, pool, two_calls):
    t = two_calls
    s = torch.cuda.Stream()
    a, b = pool[0], pool[2]
    p1, p2, i1, i2 = bc.csr_from_nodes(a["node"], b["node"])
    c1 = Call(pool, 96, t["pa"]).launch(ctx, stream=s.cuda_stream)
    m, nm = ctx.search_by_bow_keyframes(a["kp"], a["desc"], a["valid"], b["kp"], b["desc"], b["valid"], p1, p2, i1, i2, 0.75, True)      # on the context stream
    s.synchronize()
    check(c1.results(), t["wantA"], pair_counts(pool, t["pa"]))
    w = kc.expect(oracle, kc.case(a, b))
    np.testing.assert_array_equal(m, w[0]); assert nm == w[2]


# ---- 6. argument errors
def test_argument_errors(fe, ctx, pool):
    c = Call(pool[:3], 96, [(0, 1), (1, 2), (2, 0)])
    base = dict(kp=c.d["kp"], desc=c.d["desc"], node=c.d["node"], valid=c.d["valid"], n=c.n, cap=96, nk=3, pairs=c.pairs, npairs=3, m12=c.m12, m21=c.m21, nm=c.nm)

    def call(ok=False, **kw):
        a = dict(base, **kw)
        args = (a["kp"], a["desc"], a["node"], a["n"], a["cap"], a["nk"], a["pairs"], a["npairs"], a["m12"], a["m21"], a["nm"])
        if ok:
            return ctx.search_by_bow_keyframes_batch_dev(*args, d_valid=a["valid"])
        with pytest.raises(fe.SslamError) as e:
            ctx.search_by_bow_keyframes_batch_dev(*args, d_valid=a["valid"])
        assert e.value.code == fe.SSLAM_ERR_INVALID
    for name in ("kp", "desc", "node", "n", "pairs", "m12", "m21", "nm"):
        call(**{name: None})
    for name in ("cap", "nk", "npairs"):
        call(**{name: -1})
    call(cap=1 << 19)
    call(cap=1 << 16, npairs=1 << 15)                                                     # npairs * cap = 2^31
    call(desc=c.d["desc"].data_ptr() + 8)                                                 # descriptor rows are read as 16-byte words
    for name, buf in (("kp", c.d["kp"]), ("node", c.d["node"]), ("n", c.n), ("pairs", c.pairs), ("m12", c.m12), ("m21", c.m21), ("nm", c.nm)):
        call(**{name: buf.data_ptr() + 2})
    with pytest.raises(fe.SslamError) as e:                                               # a NULL context
        fe._chk(fe.lib().sslam_orb_search_by_bow_keyframes_batch_dev(None, fe._p(c.d["kp"]), fe._p(c.d["desc"]), fe._p(c.d["node"]), fe._p(c.d["valid"]), fe._p(c.n), 96, 3,
                                                                    fe._p(c.pairs), 3, fe.C.c_float(0.75), 1, fe._p(c.m12), fe._p(c.m21), fe._p(c.nm), None))
    assert e.value.code == fe.SSLAM_ERR_INVALID
    ctx.synchronize(); torch.cuda.synchronize()
    m12, m21, nm = c.results()
    assert (m12 == SENT).all() and (m21 == SENT).all() and (nm == SENT).all()
    call(ok=True, npairs=0); ctx.synchronize()                                            # no pair: SSLAM_OK, nothing enqueued
    assert (c.results()[2] == SENT).all()
    call(ok=True); ctx.synchronize()                                                      # the same buffers are accepted once the arguments are valid
    assert (c.results()[2][:3] > 0).all() and c.results()[2][3] == SENT


# ---- 7. end to end through the pool, as a caller fills it
def test_end_to_end(fe, ctx, oracle):
    w, h, B, levelsup = 320, 240, 4, 2
    L, ptr, ch, nd, word, weight = synthetic_vocab(np.random.default_rng(5), k=10, L=4)
    voc = fe.Vocabulary(ctx, L, ptr, ch, nd, word, weight)
    cur = [synth_frame(9900 + i, w, h, nshapes=16 + 4 * i, nstrokes=5 + i) for i in range(B // 2)]
    frames = np.stack([f for c in cur for f in (warp_prev(c), c)])                         # slots 2i, 2i + 1: two views of one scene
    ex = fe.OrbExtractor(ctx, 500, 1.2, 8, 20, 7)
    cap = ex.cap
    d_img = torch.from_numpy(frames).cuda()
    d_kp = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda"); d_kpun = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda"); d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_node = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(9900)
    valid = (rng.random((B, cap)) < 0.9).astype(np.uint8)
    d_valid = torch.from_numpy(valid).cuda()
    pairs = [(1, 0), (0, 1), (3, 2), (1, 2), (2, 2)]
    d_pairs = torch.from_numpy(np.array(pairs, np.int32)).cuda()
    m12 = torch.full((len(pairs), cap), SENT, dtype=torch.int32, device="cuda"); m21 = torch.full((len(pairs), cap), SENT, dtype=torch.int32, device="cuda")
    nm = torch.full((len(pairs),), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cam = fe.Camera(260.0, 260.0, 160.0, 120.0, 0.0, 0.0, 0.0, 0.0, 0.0)                   # k1 = 0: mvKeysUn = mvKeys
    ex.extract_batch_dev(d_img, w, h, w, w * h, B, d_kp, d_desc, d_n, cap)
    ctx.undistort_keypoints_batch_dev(cam, d_kp, d_n, B, cap, d_kpun)
    ctx.bow_transform_batch_dev(voc, d_desc, d_n, cap, B, d_node, levelsup=levelsup)
    ctx.search_by_bow_keyframes_batch_dev(d_kpun, d_desc, d_node, d_n, cap, B, d_pairs, len(pairs), m12, m21, nm, d_valid=d_valid, nnratio=0.75, check_orientation=True)
    ctx.synchronize()
    n = d_n.cpu().numpy()
    kp = d_kpun.cpu().numpy().view(fe.KP_DTYPE).reshape(B, cap); desc = d_desc.cpu().numpy().reshape(B, cap, 32)
    sides = [bc.side(kp[i, :n[i]].copy(), desc[i, :n[i]], oracle.bow_transform(L, ptr, ch, nd, word, weight, desc[i, :n[i]], levelsup)[2], valid[i, :n[i]]) for i in range(B)]
    node = d_node.cpu().numpy()
    for i in range(B):
        np.testing.assert_array_equal(node[i, :n[i]], sides[i]["node"]); assert (node[i, n[i]:] == SENT).all()
    want = [kc.expect(oracle, kc.case(sides[a], sides[b])) for a, b in pairs]
    assert n.min() > 100 and want[0][2] >= 20 and want[2][2] >= 20 and want[3][2] < 20, (n, [x[2] for x in want])      # LoopClosing's own threshold: two views of one scene pass it, two scenes do not
    check((m12.cpu().numpy(), m21.cpu().numpy(), nm.cpu().numpy()), want, [(n[a], n[b]) for a, b in pairs])
    ex.close(); voc.close()
