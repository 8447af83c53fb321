"""Inputs of the batch SearchByBoW tests (tests/test_bow_batch_gpu.py, tests/test_bow_batch_cases_cpu.py): pairs of a keyframe side and a frame
side, each a dict(kp, desc, node[, valid]) of per-feature arrays -- the node ARRAY is what sslam_orb_search_by_bow_batch_dev takes -- built from
match_cases.rand_desc, flip_bits and bow_case.  csr_from_nodes() turns two node arrays into the CSR lists FeatureVector::addFeature(node[i], i)
would give (shared ids >= 0 ascending, ascending feature index inside a node), which is what oracle.search_by_bow takes: every expectation of
the two test files is expect() = helper + CPU oracle.  Every generator is a pure function of its numpy Generator."""
import numpy as np
import match_cases as mc
from oracle_lib import KP_DTYPE

W = 8               # waves per pair of k_search_bow_batch (csrc/match_plan.h BATCH_WAVES): wave w owns the nodes with id % W == w
ROW_BYTES = 40      # LDS bytes per frame row (BOW_BATCH_ROW_BYTES)
LDS_MAX = 64 * 1024
LDS_CAP = LDS_MAX // ROW_BYTES          # 1638: the last row capacity whose frame side sits in LDS
TH_LOW = 50


# ---- helper + oracle
def csr_from_nodes(node_kf, node_f):
    """-> (ptr_kf, ptr_f, idx_kf, idx_f) over the node ids >= 0 present on both sides, ascending; feature indices ascending inside a node"""
    node_kf = np.asarray(node_kf, np.int64); node_f = np.asarray(node_f, np.int64)
    shared = np.intersect1d(node_kf[node_kf >= 0], node_f[node_f >= 0])
    pk, pf, ik, jf = [0], [0], [], []
    for nd in shared:
        a = np.flatnonzero(node_kf == nd); b = np.flatnonzero(node_f == nd)
        ik += a.tolist(); jf += b.tolist(); pk.append(len(ik)); pf.append(len(jf))
    return np.array(pk, np.int32), np.array(pf, np.int32), np.array(ik, np.int32), np.array(jf, np.int32)


def expect(oracle, c):
    """(assigned[nf], nmatches) of one pair: the CPU oracle on the CSR lists of the two node arrays"""
    kf, f = c["kf"], c["f"]
    nf = len(f["kp"])
    pk, pf, ik, jf = csr_from_nodes(kf["node"], f["node"])
    if nf == 0 or len(kf["kp"]) == 0 or len(pk) == 1:
        return np.full(nf, -1, np.int32), 0
    return oracle.search_by_bow(kf["kp"], kf["desc"], kf["valid"], f["kp"], f["desc"], pk, pf, ik, jf, c["nnratio"], c["ori"])


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def order_free(c):
    """per keyframe row: (best, second) frame rows of its node by (distance, index) with NOTHING taken -- what a matcher that ignores the chain sees;
    -1 where there is none"""
    kf, f = c["kf"], c["f"]
    out = np.full((len(kf["kp"]), 2), -1, np.int64)
    for i in range(len(kf["kp"])):
        if kf["node"][i] < 0: continue
        js = np.flatnonzero(f["node"] == kf["node"][i])
        if len(js) == 0: continue
        d = np.array([hamming(kf["desc"][i], f["desc"][j]) for j in js])
        o = np.lexsort((js, d))
        out[i, 0] = js[o[0]]
        if len(js) > 1: out[i, 1] = js[o[1]]
    return out


def second_choices(c, assigned):
    """keyframe rows that were matched to their order-free SECOND candidate (an earlier row of the node took the first)"""
    of = order_free(c)
    return [int(i) for j, i in enumerate(assigned) if i >= 0 and of[i, 1] == j and of[i, 0] != j]


def lost_first_choice(c, assigned):
    """valid keyframe rows whose order-free best candidate lies within TH_LOW but went to an EARLIER keyframe row: the rows an order-free matcher gets wrong"""
    of = order_free(c)
    kf, f = c["kf"], c["f"]
    return [i for i in range(len(kf["kp"])) if kf["valid"][i] and of[i, 0] >= 0 and 0 <= assigned[of[i, 0]] < i
            and hamming(kf["desc"][i], f["desc"][of[i, 0]]) <= TH_LOW]


# ---- building blocks
def _kp(rng, n):
    kp = np.zeros(n, KP_DTYPE)
    kp["x"] = rng.uniform(20, 620, n); kp["y"] = rng.uniform(20, 460, n); kp["octave"] = rng.integers(0, 4, n); kp["angle"] = rng.uniform(0, 360, n); kp["size"] = 31
    return kp


def _flip(row, bits):
    out = row.copy()
    bits = np.asarray(bits, np.int64)
    np.bitwise_xor.at(out, bits >> 3, (1 << (bits & 7)).astype(np.uint8))
    return out


def side(kp, desc, node, valid=None):
    s = dict(kp=kp, desc=np.ascontiguousarray(desc, np.uint8), node=np.asarray(node, np.int32))
    if valid is not None: s["valid"] = np.asarray(valid, np.uint8)
    return s


def case(kf, f, nnratio=0.9, ori=True, **extra):
    return dict(kf=kf, f=f, nnratio=nnratio, ori=ori, **extra)


def cut(c, nkf, nf):
    """the pair with the first nkf keyframe rows and the first nf frame rows"""
    return dict(c, kf={k: v[:nkf].copy() for k, v in c["kf"].items()}, f={k: v[:nf].copy() for k, v in c["f"].items()})


def from_bow_case(rng, nnodes, ids=None, p_valid=0.9):
    """match_cases.bow_case (1..3 features of each frame per node, keyframe rows noisy copies of their node's frame rows) as node arrays;
    ids[nd] = the id of bow_case's node nd (default nd)"""
    b = mc.bow_case(rng, nnodes)
    ids = np.arange(nnodes) if ids is None else np.asarray(ids)
    n1, n2 = len(b["kp1"]), len(b["kp2"])
    node1 = np.zeros(n1, np.int32); node2 = np.zeros(n2, np.int32)
    for nd in range(nnodes):
        node1[b["idx1"][b["ptr1"][nd]:b["ptr1"][nd + 1]]] = ids[nd]; node2[b["idx2"][b["ptr2"][nd]:b["ptr2"][nd + 1]]] = ids[nd]
    return case(side(b["kp1"], b["d1"], node1, rng.random(n1) < p_valid), side(b["kp2"], b["d2"], node2))


def node_pair(rng, node_kf, node_f, max_flips=40, p_valid=0.9, nnratio=0.9, ori=True):
    """a pair with the given node arrays: frame rows random, a keyframe row a noisy copy (descriptor, angle) of a random frame row of its node
    where the frame has one (so rows of a crowded node contend for the same frame rows), random otherwise"""
    node_kf = np.asarray(node_kf, np.int32); node_f = np.asarray(node_f, np.int32)
    nkf, nf = len(node_kf), len(node_f)
    fkp = _kp(rng, nf); fd = mc.rand_desc(rng, nf)
    kkp = _kp(rng, nkf); kd = mc.rand_desc(rng, nkf)
    src = np.full(nkf, -1, np.int64)
    for i in range(nkf):
        js = np.flatnonzero(node_f == node_kf[i])
        if len(js): src[i] = js[rng.integers(0, len(js))]
    has = src >= 0
    if has.any():
        kd[has] = mc.flip_bits(rng, fd[src[has]], max_flips)
        kkp["angle"][has] = (fkp["angle"][src[has]] + rng.normal(0, 8, int(has.sum()))) % 360
    return case(side(kkp, kd, node_kf, rng.random(nkf) < p_valid), side(fkp, fd, node_f), nnratio, ori)


# ---- node layouts
def layout_cases(rng):
    """name -> pair.  Sizes are small: one workgroup of W waves per pair, and 150 rows are three ballots of keyframe rows and three strides of frame rows"""
    n = 150
    out = {}
    out["one_node"] = node_pair(rng, np.full(n, 7), np.full(100, 7))                                # the whole frame is one chain; more keyframe rows than frame rows
    out["one_feature_per_node"] = node_pair(rng, rng.permutation(n), rng.permutation(n))
    out["one_side_only"] = node_pair(rng, rng.integers(0, 40, n), rng.integers(20, 60, n))           # ids 0..19 keyframe only, 40..59 frame only
    out["minus_one_and_zero"] = node_pair(rng, rng.choice([-1, 0, -5], n), rng.choice([-1, 0, -5], n))    # -1 and -5 on BOTH sides: in no node, never matched
    out["near_2_30"] = node_pair(rng, (1 << 30) - 1 - rng.integers(0, 30, n), (1 << 30) - 1 - rng.integers(0, 30, n))
    out["max_id"] = node_pair(rng, 0x7FFFFFFF - rng.integers(0, 9, n), 0x7FFFFFFF - rng.integers(0, 9, n))
    out["one_wave"] = node_pair(rng, W * rng.integers(0, 25, n), W * rng.integers(0, 25, n))          # ids i * W: every node belongs to wave 0
    out["all_waves"] = node_pair(rng, rng.integers(0, 25, n), rng.integers(0, 25, n))                 # consecutive ids: every wave walks
    return out


# ---- order dependence
def chain_case(rng, m, reverse=False, filler=40):
    """m (2 or 3) keyframe rows of ONE node whose best candidate is the same frame row f0; the node has m frame rows f0, f1, f2 at 0 / 20 / 30 bits from
    a base descriptor, keyframe row i lies i + 1 bits from it (all on disjoint bits: d(k_i, f_j) = i + 1 + (0, 20, 30)[j]).  In index order k_0 takes
    f0, k_1 its second choice f1, k_2 the last one f2; reverse=True puts the keyframe rows in the opposite index order, and then the row k_2 takes f0.
    The chain rows are scattered among `filler` rows of other nodes on each side.  -> pair with chain=(kf rows of k_0.., frame rows of f_0..)"""
    assert m in (2, 3)
    base = mc.rand_desc(rng, 1)[0]
    perm = rng.permutation(256)
    fdesc = [base, _flip(base, perm[0:20]), _flip(base, perm[20:50])][:m]
    kdesc = [_flip(base, perm[100 + 10 * i:100 + 10 * i + i + 1]) for i in range(m)]
    nid = 3 * W + 5
    nkf, nf = filler + m, filler + m
    c = node_pair(rng, rng.integers(100, 120, nkf), rng.integers(100, 120, nf), p_valid=1.0)
    krows = np.sort(rng.choice(nkf, m, replace=False)); frows = np.sort(rng.choice(nf, m, replace=False))
    korder = krows[::-1] if reverse else krows
    for i in range(m):
        c["kf"]["desc"][korder[i]] = kdesc[i]; c["kf"]["node"][korder[i]] = nid; c["kf"]["valid"][korder[i]] = 1
        c["f"]["desc"][frows[i]] = fdesc[i]; c["f"]["node"][frows[i]] = nid
        c["kf"]["kp"]["angle"][korder[i]] = 77.0; c["f"]["kp"]["angle"][frows[i]] = 77.0      # whoever takes whom, the rotation is 0: the fillers' own bin
    c["chain"] = (korder, frows)
    return c


def tie_case(rng, nnratio):
    """one keyframe row, two frame rows of its node at the SAME distance 12 (different bits), a third at 40.  nnratio 1.2: the ratio test passes
    (12 < 1.2 * 12) and the lower frame index wins (first strictly smaller distance); nnratio 0.9: best equals second, the ratio test fails"""
    base = mc.rand_desc(rng, 1)[0]
    perm = rng.permutation(256)
    c = node_pair(rng, rng.integers(100, 110, 21), rng.integers(100, 110, 23), p_valid=1.0, nnratio=nnratio)
    kr = 9; fr = [4, 15, 20]
    c["kf"]["desc"][kr] = base; c["kf"]["node"][kr] = 5
    for j, bits in zip(fr, (perm[0:12], perm[12:24], perm[24:64])):
        c["f"]["desc"][j] = _flip(base, bits); c["f"]["node"][j] = 5
    c["tie"] = (kr, fr)
    return c


# ---- gates
def threshold_case(rng, d1, d2=None, nnratio=0.9, valid=1):
    """one keyframe row (index 3) and, in its node, a frame row (index 6) at exactly d1 bits and -- where d2 is given -- another (index 2) at exactly d2;
    the other rows are of other nodes"""
    base = mc.rand_desc(rng, 1)[0]
    perm = rng.permutation(256)
    c = node_pair(rng, rng.integers(100, 110, 8), rng.integers(100, 110, 9), p_valid=1.0, nnratio=nnratio)
    c["kf"]["desc"][3] = base; c["kf"]["node"][3] = 2 * W + 1; c["kf"]["valid"][3] = valid
    c["f"]["desc"][6] = _flip(base, perm[:d1]); c["f"]["node"][6] = 2 * W + 1
    if d2 is not None:
        c["f"]["desc"][2] = _flip(base, perm[256 - d2:]); c["f"]["node"][2] = 2 * W + 1
    c["th"] = (3, 6, 2)
    return c


def threshold_cases(rng):
    """name -> (pair, the frame row 6 is matched to keyframe row 3).  0.75 * 40 = 30 exactly in float, so 30 against 40 sits on the ratio's equality (strict: no match)"""
    return {"dist_50": (threshold_case(rng, 50), True), "dist_51": (threshold_case(rng, 51), False),
            "ratio_equal": (threshold_case(rng, 30, 40, nnratio=0.75), False), "ratio_below": (threshold_case(rng, 29, 40, nnratio=0.75), True),
            "kf_invalid": (threshold_case(rng, 10, valid=0), False)}


# ---- rotation
def rot_case(rng, groups, nnratio=0.9, turn=0.0):
    """one keyframe row and one frame row per node, close descriptors (every pair matches); groups = [(count, rot_lo, rot_hi)]: keyframe angle =
    frame angle + U(rot_lo, rot_hi) + turn (mod 360) -- the rotation SearchByBoW bins.  Rows are shuffled."""
    n = sum(g[0] for g in groups)
    fkp = _kp(rng, n); fd = mc.rand_desc(rng, n)
    rot = np.concatenate([rng.uniform(lo, hi, cnt) for cnt, lo, hi in groups]).astype(np.float32)
    fkp["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    pk = rng.permutation(n)          # keyframe row i is the copy of frame row pk[i]
    kkp = _kp(rng, n); kkp["angle"] = ((fkp["angle"][pk] + rot[pk] + np.float32(turn)) % np.float32(360)).astype(np.float32)
    kd = mc.flip_bits(rng, fd[pk], 10)
    nodes_f = rng.permutation(n).astype(np.int32) + 1
    return case(side(kkp, kd, nodes_f[pk], np.ones(n)), side(fkp, fd, nodes_f), nnratio, True)


def rot_neighbours():
    """two pairs of equal features whose keyframe angles are 90 degrees apart (neighbouring pairs of one launch: the histogram is per pair)"""
    g = [(20, 10, 14), (14, 100, 104), (10, 190, 194), (6, 280, 284)]
    return rot_case(np.random.default_rng(7402), g), rot_case(np.random.default_rng(7402), g, turn=90.0)


# ---- packing: slots of `cap` rows, junk past every count
def junk(rng, shape, dtype):
    dt = np.dtype(dtype)
    return rng.integers(0, 256, size=int(np.prod(shape)) * dt.itemsize, dtype=np.uint8).view(dt).reshape(shape)


def pack_sides(rng, sides, cap, with_valid):
    """[S, cap] buffers of the sides, rows at or past a side's count random bytes (node ids and valid flags included) -> dict(kp, desc, node[, valid], n)"""
    S = len(sides)
    P = dict(kp=junk(rng, (S, cap), KP_DTYPE), desc=junk(rng, (S, cap, 32), np.uint8), node=junk(rng, (S, cap), np.int32), n=np.zeros(S, np.int32))
    if with_valid: P["valid"] = junk(rng, (S, cap), np.uint8)
    for i, s in enumerate(sides):
        n = len(s["kp"])
        assert n <= cap, (i, n, cap)
        P["kp"][i, :n] = s["kp"]; P["desc"][i, :n] = s["desc"]; P["node"][i, :n] = s["node"]; P["n"][i] = n
        if with_valid: P["valid"][i, :n] = s["valid"]
    return P


# ---- the reference's own SearchByBoW takes the node arrays directly; it files a NEGATIVE id under (unsigned)id, so for it the rows "in no node" get
# ids of their own that no other row has (the same thing said in its terms)
def ref_nodes(c):
    kn = c["kf"]["node"].astype(np.int32).copy(); fn = c["f"]["node"].astype(np.int32).copy()
    assert max(kn.max(initial=0), fn.max(initial=0)) < 0x7F000000 or (kn >= 0).all() and (fn >= 0).all()
    neg = np.flatnonzero(kn < 0); kn[neg] = 0x7F000000 + neg
    neg = np.flatnonzero(fn < 0); fn[neg] = 0x7F800000 + neg
    return kn, fn
