"""Inputs of the keyframe-to-keyframe batch SearchByBoW tests (tests/test_bow_kf_batch_gpu.py, tests/test_bow_kf_batch_cases_cpu.py): pairs of two
keyframe sides k1 (pKF1, the side the result is indexed by) and k2 (pKF2, the candidates), each a dict(kp, desc, node, valid) of per-feature arrays
-- the node ARRAY is what sslam_orb_search_by_bow_keyframes_batch_dev takes.  Built on bow_batch_cases (node_pair, csr_from_nodes, pack_sides) and
rot_cases; expect() = csr_from_nodes + the CPU oracle's search_by_bow_keyframes, and every expectation of the two test files comes from it.
The crafted cases put a handful of rows with descriptors at EXACT distances into a node of their own, among filler rows of other nodes: a
descriptor is a base row with a set of bits flipped, the sets are disjoint slices of one permutation, so d(a, b) = |bits(a) xor bits(b)|.
Every generator is a pure function of its numpy Generator."""
import numpy as np
import match_cases as mc
import bow_batch_cases as bc
import rot_cases as rc

W = bc.W                    # waves per pair (csrc/match_plan.h BATCH_WAVES): wave w owns the nodes with id % W == w
ROW_BYTES = bc.ROW_BYTES    # LDS bytes per keyframe-2 row: the kernel reuses BOW_BATCH_ROW_BYTES (descriptor, node id, one state word)
LDS_MAX = bc.LDS_MAX
LDS_CAP = bc.LDS_CAP        # 1638: the last row capacity whose keyframe 2 sits in LDS
OPT_IN_CAP = 48 * 1024 // ROW_BYTES      # 1228: the last row capacity without the dynamic-LDS opt-in
TH_LOW = 50
NODE = 3 * W + 5            # the crafted rows' node (wave 5)


# ---- helper + oracle
def case(k1, k2, nnratio=0.75, ori=True, **extra):
    return dict(k1=k1, k2=k2, nnratio=nnratio, ori=ori, **extra)


def with_valid(s, valid=None):
    n = len(s["kp"])
    return dict(s, valid=np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8))


def from_bc(c, valid2=None, **kw):
    """a pair of bow_batch_cases (keyframe, frame) as (k1, k2); valid2: keyframe 2's flags (default: all valid)"""
    return case(with_valid(c["kf"], c["kf"].get("valid")), with_valid(c["f"], valid2), kw.pop("nnratio", c["nnratio"]), kw.pop("ori", c["ori"]), **kw)


def inverse(m12, n2):
    m21 = np.full(n2, -1, np.int32)
    i1 = np.flatnonzero(m12 >= 0)
    m21[m12[i1]] = i1
    return m21


def expect(oracle, c, nnratio=None, ori=None):
    """(matches12[n1], matches21[n2], nmatches) of one pair: the CPU oracle on the CSR lists of the two node arrays, and the inverse of its rows"""
    k1, k2 = c["k1"], c["k2"]
    n1, n2 = len(k1["kp"]), len(k2["kp"])
    nnratio = c["nnratio"] if nnratio is None else nnratio
    ori = c["ori"] if ori is None else ori
    p1, p2, i1, i2 = bc.csr_from_nodes(k1["node"], k2["node"])
    if n1 == 0 or n2 == 0 or len(p1) == 1:
        return np.full(n1, -1, np.int32), np.full(n2, -1, np.int32), 0
    m12, nm = oracle.search_by_bow_keyframes(k1["kp"], k1["desc"], k1["valid"], k2["kp"], k2["desc"], k2["valid"], p1, p2, i1, i2, nnratio, ori)
    assert nm == int((m12 >= 0).sum())
    return m12, inverse(m12, n2), nm


def order_free(c):
    """per VALID keyframe-1 row: its best valid keyframe-2 row of the node by (distance, index) with NOTHING taken, gates applied -- what a matcher
    that ignores the chain answers; -1 where there is none"""
    k1, k2 = c["k1"], c["k2"]
    out = np.full(len(k1["kp"]), -1, np.int32)
    for i in range(len(k1["kp"])):
        if k1["node"][i] < 0 or not k1["valid"][i]: continue
        js = np.flatnonzero((k2["node"] == k1["node"][i]) & (k2["valid"] != 0))
        if len(js) == 0: continue
        d = np.array([bc.hamming(k1["desc"][i], k2["desc"][j]) for j in js])
        o = np.lexsort((js, d))
        d2 = d[o[1]] if len(js) > 1 else 256
        if d[o[0]] < TH_LOW and np.float32(d[o[0]]) < np.float32(c["nnratio"]) * np.float32(d2): out[i] = js[o[0]]
    return out


def cut(c, n1, n2):
    """the pair with the first n1 keyframe-1 rows and the first n2 keyframe-2 rows"""
    return dict(c, k1={k: v[:n1].copy() for k, v in c["k1"].items()}, k2={k: v[:n2].copy() for k, v in c["k2"].items()})


def node_pair(rng, node1, node2, p_valid=0.9, nnratio=0.75, ori=True, max_flips=40):
    """bow_batch_cases.node_pair with validity flags on both sides"""
    c = bc.node_pair(rng, node1, node2, max_flips=max_flips, p_valid=p_valid, nnratio=nnratio, ori=ori)
    return from_bc(c, rng.random(len(c["f"]["kp"])) < p_valid)


# ---- ragged counts: both sides around the 64-row ballot step and the lane loop
RAGGED_CAP = 160
RAGGED_COUNTS = [(160, 160), (0, 129), (129, 0), (1, 2), (2, 1), (63, 64), (64, 65), (65, 63), (127, 128), (128, 129), (129, 127)]


def ragged_cases():
    """pairs of 160 rows per side over 40 nodes (about four rows of a node per side: chains everywhere), cut to RAGGED_COUNTS"""
    out = []
    for i, (n1, n2) in enumerate(RAGGED_COUNTS):
        rng = np.random.default_rng(9200 + i)
        out.append(cut(node_pair(rng, rng.integers(0, 40, RAGGED_CAP), rng.integers(0, 40, RAGGED_CAP)), n1, n2))
    return out


# ---- crafted rows
class Bits:
    """disjoint bit sets: take(n) hands out the next n positions of one permutation of 0..255"""
    def __init__(self, rng):
        self.perm = rng.permutation(256); self.at = 0

    def take(self, n):
        assert self.at + n <= 256
        out = self.perm[self.at:self.at + n]; self.at += n
        return out


def flip(row, *bitsets):
    out = row
    for b in bitsets: out = bc._flip(out, b)
    return out


def craft(rng, kdesc, fdesc, kvalid=None, fvalid=None, nnratio=0.75, ori=True, filler=40, reverse=False, **extra):
    """a pair of `filler` rows of other nodes (ids 100..119, all valid) per side, with the given descriptors as additional rows of node NODE at random
    positions: kdesc[i] at keyframe-1 row rows[0][i], fdesc[j] at keyframe-2 row rows[1][j], both ascending (reverse=True: kdesc in descending row
    order).  Every crafted row has the angle 77, so whoever takes whom the rotation is 0, the fillers' own bin."""
    m1, m2 = len(kdesc), len(fdesc)
    c = node_pair(rng, rng.integers(100, 120, filler + m1), rng.integers(100, 120, filler + m2), p_valid=1.0, nnratio=nnratio, ori=ori)
    krows = np.sort(rng.choice(filler + m1, m1, replace=False)); frows = np.sort(rng.choice(filler + m2, m2, replace=False))
    if reverse: krows = krows[::-1].copy()
    kvalid = [1] * m1 if kvalid is None else kvalid; fvalid = [1] * m2 if fvalid is None else fvalid
    for rows, s, desc, valid in ((krows, c["k1"], kdesc, kvalid), (frows, c["k2"], fdesc, fvalid)):
        for r, d, v in zip(rows, desc, valid):
            s["desc"][r] = d; s["node"][r] = NODE; s["valid"][r] = v; s["kp"]["angle"][r] = 77.0
    return dict(c, rows=(krows, frows), **extra)


def dist_table(c):
    """d[i][j] between the crafted rows"""
    krows, frows = c["rows"]
    return [[bc.hamming(c["k1"]["desc"][i], c["k2"]["desc"][j]) for j in frows] for i in krows]


# ---- validity
def validity_cases(rng):
    """name -> (pair, {crafted k1 position: crafted k2 position or -1} the matcher must answer, which (side, position) to make valid for the twin, the twin's answer)"""
    out = {}
    base = mc.rand_desc(rng, 1)[0]; B = Bits(rng)
    # an invalid keyframe-1 row (the earlier index) whose descriptor would win f0: the valid row behind it takes f0
    out["k1_invalid_would_win"] = (craft(rng, [flip(base, B.take(5)), flip(base, B.take(10))], [base, flip(base, B.take(45))], kvalid=[0, 1]),
                                   {0: -1, 1: 0}, ("k1", 0), {0: 0, 1: -1})
    base = mc.rand_desc(rng, 1)[0]; B = Bits(rng)
    # an invalid keyframe-2 row that would be the best: the match goes to the next one (20 < 0.75 * 40)
    out["k2_invalid_best"] = (craft(rng, [base], [flip(base, B.take(5)), flip(base, B.take(20)), flip(base, B.take(40))], fvalid=[0, 1, 1]),
                              {0: 1}, ("k2", 0), {0: 0})
    base = mc.rand_desc(rng, 1)[0]; B = Bits(rng)
    # an invalid keyframe-2 row that would be the SECOND best: 20 < 0.75 * 40 holds, 20 < 0.75 * 22 would not
    out["k2_invalid_second"] = (craft(rng, [base], [flip(base, B.take(20)), flip(base, B.take(22)), flip(base, B.take(40))], fvalid=[1, 0, 1]),
                                {0: 0}, ("k2", 1), {0: -1})
    return out


def set_valid(c, side, pos):
    """the twin of a crafted pair with one crafted row made valid"""
    t = dict(c, k1={k: v.copy() for k, v in c["k1"].items()}, k2={k: v.copy() for k, v in c["k2"].items()})
    t[side]["valid"][c["rows"][0 if side == "k1" else 1][pos]] = 1
    return t


# ---- order dependence inside a node
def chain_case(rng, m, reverse=False, last=30):
    """m (2 or 3) keyframe-1 rows whose best candidate is the same keyframe-2 row f0: d(k_i, f_j) = i + 1 + (0, 20, last)[j].  In index order k_0 takes
    f0, k_1 its second choice f1 (22 < 0.75 * 32), k_2 the last one; reverse=True puts the keyframe-1 rows in the opposite index order.  last=24 with
    m=2 and three candidates: the later row's second choice fails the ratio (22 < 0.75 * 26 is false)"""
    base = mc.rand_desc(rng, 1)[0]; B = Bits(rng)
    nf = 3 if last != 30 else m
    fdesc = [base, flip(base, B.take(20)), flip(base, B.take(last))][:nf]
    kdesc = [flip(base, B.take(i + 1)) for i in range(m)]
    return craft(rng, kdesc, fdesc, reverse=reverse)


def taken_second_case(rng):
    """k_0 takes f0 (2 against 24).  For k_1 the candidates are f1 at 10, f0 at 12, f2 at 40: with f0 free the ratio fails (10 < 0.75 * 12 is false), with f0
    taken -- skipped before its distance is looked at -- the second best is f2 and the match is made"""
    base = mc.rand_desc(rng, 1)[0]; B = Bits(rng)
    s0, s1, s2, s3 = B.take(2), B.take(12), B.take(10), B.take(40)
    return craft(rng, [flip(base, s0), flip(base, s1)], [base, flip(base, s1, s2), flip(base, s1, s3)])


def chain_cases():
    """name -> (pair, crafted k2 position per crafted k1 position IN INDEX ORDER of keyframe 1)"""
    r = lambda k: np.random.default_rng(9300 + k)
    return {"chain_2_fwd": (chain_case(r(0), 2), [0, 1]), "chain_2_rev": (chain_case(r(0), 2, True), [0, 1]),
            "chain_3_fwd": (chain_case(r(1), 3), [0, 1, 2]), "chain_3_rev": (chain_case(r(1), 3, True), [0, 1, 2]),
            "chain_2_second_fails": (chain_case(r(2), 2, last=24), [0, -1]),
            "taken_second": (taken_second_case(r(3)), [0, 1])}


# ---- the gates on neighbouring integers
def gate_case(rng, dists, nnratio=0.75, fvalid=None):
    """one keyframe-1 row and keyframe-2 rows of its node at exactly dists[j] bits (ascending index)"""
    base = mc.rand_desc(rng, 1)[0]; B = Bits(rng)
    return craft(rng, [base], [flip(base, B.take(d)) for d in dists], nnratio=nnratio, fvalid=fvalid, filler=12)


def gate_cases():
    """name -> (pair, crafted k2 position the one crafted k1 row is matched to, or -1)"""
    r = lambda k: np.random.default_rng(9400 + k)
    return {"dist_49": (gate_case(r(0), [49]), 0), "dist_50": (gate_case(r(1), [50]), -1), "dist_51": (gate_case(r(2), [51]), -1),
            "ratio_30_40": (gate_case(r(3), [30, 40]), -1), "ratio_29_40": (gate_case(r(4), [29, 40]), 0),
            # no second candidate: bestDist2 = 256, and 0.15f * 256 = 38.4 separates 38 from 39
            "single_38": (gate_case(r(5), [38], nnratio=0.15), 0), "single_39": (gate_case(r(6), [39], nnratio=0.15), -1),
            # equal best distances at two indices: the lower index is the best, the equal second fails the ratio below 1 and passes it above
            "tie_fails": (gate_case(r(7), [40, 12, 12]), -1), "tie_lower_index": (gate_case(r(7), [40, 12, 12], nnratio=1.2), 1)}


def as_frame_pair(c):
    """the pair in bow_batch_cases' shape (keyframe -> frame matcher: no flags on side 2, gate <=)"""
    return bc.case(c["k1"], {k: v for k, v in c["k2"].items() if k != "valid"}, c["nnratio"], c["ori"])


# ---- rotation
def rot_group_case(rng, groups, nnratio=0.75):
    """one keyframe-1 row and one keyframe-2 row per node, close descriptors (every pair matches); groups = [(count, rot)]: keyframe-1 angle =
    keyframe-2 angle + rot (mod 360), all multiples of 0.25 and away from bin edges.  Rows are shuffled; pk[i] = the keyframe-2 row of keyframe-1 row i"""
    n = sum(g[0] for g in groups)
    kp2 = bc._kp(rng, n); d2 = mc.rand_desc(rng, n)
    kp2["angle"] = rng.integers(0, 1440, n) * 0.25
    group = rng.permutation(np.repeat(np.arange(len(groups)), [g[0] for g in groups]))      # of keyframe-2 row j
    rot = np.array([groups[g][1] for g in group], np.float32)
    pk = rng.permutation(n)
    kp1 = bc._kp(rng, n); kp1["angle"] = (kp2["angle"][pk] + rot[pk]) % np.float32(360)
    d1 = mc.flip_bits(rng, d2[pk], 10)
    node2 = rng.permutation(n).astype(np.int32) + 1
    ones = np.ones(n, np.uint8)
    return case(bc.side(kp1, d1, node2[pk], ones), bc.side(kp2, d2, node2, ones), nnratio, True, pk=pk, group1=group[pk])


def swap_angles(c):
    """the pair whose matched rows carry each other's angles: what a matcher that bins kp2.angle - kp1.angle sees"""
    t = dict(c, k1=dict(c["k1"], kp=c["k1"]["kp"].copy()), k2=dict(c["k2"], kp=c["k2"]["kp"].copy()))
    t["k1"]["kp"]["angle"] = c["k2"]["kp"]["angle"][c["pk"]]
    t["k2"]["kp"]["angle"][c["pk"]] = c["k1"]["kp"]["angle"]
    return t


def rot_cases():
    """name -> (pair, matches without the check, groups the check prunes).  bin = round(rot / 30); the second and third bin go when they hold less than
    0.1f * max (4 < 0.1f * 40 is false in float: 4 stays, 3 goes)"""
    r = lambda k: np.random.default_rng(9500 + k)
    out = {"three_bins": (rot_group_case(r(0), [(20, 40), (10, 100), (6, 190)]), 36, []),
           "four_bins": (rot_group_case(r(1), [(30, 40), (12, 100), (8, 190), (5, 280)]), 55, [3]),
           "six_bins": (rot_group_case(r(2), [(9, 40), (14, 100), (7, 130), (11, 190), (5, 250), (3, 310)]), 49, [2, 4, 5]),
           "tenth_second_stays": (rot_group_case(r(3), [(40, 40), (4, 100), (3, 190)]), 47, [2]),
           "tenth_both_go": (rot_group_case(r(4), [(40, 40), (3, 100), (3, 190)]), 46, [1, 2]),
           # three bins tie for the second place: the first two bin INDICES stay.  With kp1 - kp2 the groups sit in bins 1, 3, 6, 9 and the last goes; with
           # the operands swapped they sit in bins 11, 9, 6, 3 and the group of bin 9 -- group 1 -- goes instead
           "operand_order": (rot_group_case(r(5), [(10, 40), (6, 100), (6, 190), (6, 280)]), 28, [3])}
    return out


def rot_edge_cases():
    """rot_cases' bin-edge families (rot = 15 exactly, [345, 360) -> bin 12, the 10 % boundary, ties, the bin-30 wrap) as keyframe pairs, all rows valid
    -> name -> (pair, rot_cases' own case)"""
    out = {}
    for name, c in rc.all_cases().items():
        n = len(c["kp1"])
        ones = np.ones(n, np.uint8)
        out[name] = (case(bc.side(c["kp1"], c["d1"], c["node1"], ones), bc.side(c["kp2"], c["d2"], c["node2"], ones), 0.75, True), c)
    return out


# ---- node layouts
def layout_cases(rng):
    n = 150
    out = {}
    out["one_node"] = node_pair(rng, np.full(n, 7), np.full(100, 7))                                 # one wave does all the work, one long chain
    out["negative_ids"] = node_pair(rng, rng.choice([-1, 0, -5, 3], n), rng.choice([-1, 0, -5, 3], n))     # -1 and -5 on BOTH sides: in no node
    out["one_side_only"] = node_pair(rng, rng.integers(0, 40, n), rng.integers(20, 60, n))            # ids 0..19 keyframe 1 only, 40..59 keyframe 2 only
    out["one_wave"] = node_pair(rng, 3 + W * rng.integers(0, 25, n), 3 + W * rng.integers(0, 25, n))  # ids 3 + i * W: every node belongs to wave 3
    out["all_waves"] = node_pair(rng, rng.integers(0, 25, n), rng.integers(0, 25, n))
    out["near_1e6"] = node_pair(rng, 1000000 - rng.integers(0, 30, n), 1000000 - rng.integers(0, 30, n))
    return out


# ---- a pool for pair lists: any slot matches any other
def pool_sides(rng, counts, nnodes=30, p_valid=0.9):
    """keyframe sides over one set of node ids that all derive from one set of `nnodes * 3` source descriptors (a row is a noisy copy of a source of
    its node), so that any two slots -- and a slot with itself -- match"""
    src_node = np.repeat(np.arange(nnodes), 3).astype(np.int32)
    src_desc = mc.rand_desc(rng, len(src_node)); src_angle = rng.uniform(0, 360, len(src_node))
    sides = []
    for n in counts:
        s = rng.integers(0, len(src_node), n)
        kp = bc._kp(rng, n); kp["angle"] = (src_angle[s] + rng.normal(0, 8, n)) % 360
        sides.append(bc.side(kp, mc.flip_bits(rng, src_desc[s], 24), src_node[s], rng.random(n) < p_valid))
    return sides


# ---- packing: one pool of slots of `cap` rows, junk past every count (node ids and validity flags included)
def pack_pool(rng, sides, cap):
    return bc.pack_sides(rng, sides, cap, True)


def pool_of_cases(cases):
    """the pairs' sides as slots 2p (k1) and 2p + 1 (k2) -> (sides, pairs)"""
    sides, pairs = [], []
    for p, c in enumerate(cases):
        sides += [c["k1"], c["k2"]]; pairs.append((2 * p, 2 * p + 1))
    return sides, pairs


# ---- the reference's own SearchByBoW files a NEGATIVE id under (unsigned)id: for it the rows "in no node" get ids of their own that no other row has
def ref_nodes(c):
    return bc.ref_nodes(dict(kf=c["k1"], f=c["k2"]))
