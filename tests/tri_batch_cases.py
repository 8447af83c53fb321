"""Inputs of the batch SearchForTriangulation tests (tests/test_tri_batch_gpu.py, tests/test_tri_batch_cases_cpu.py): keyframe sides, each a
dict(kp, desc, node, free[, uright]) of per-feature arrays -- the node ARRAY is what sslam_orb_search_for_triangulation_batch_dev takes -- and pairs
dict(s1, s2, F12, ex, ey, only_stereo, ori) of a query side and a candidate side.  bow_batch_cases.csr_from_nodes() turns the two node arrays into the
CSR lists FeatureVector::addFeature(node[i], i) would give, which is what oracle.search_for_triangulation takes: every expectation of the two test
files is expect() = helper + CPU oracle.  The gate cases pick their numbers with the matcher's own float expressions (epi_ok, epipole_rejects), one
float32 operation at a time.  Every generator is a pure function of its numpy Generator."""
import numpy as np
import match_cases as mc
import bow_batch_cases as bc
import rot_cases
from oracle_lib import KP_DTYPE

W = 8                                   # waves per pair of k_tri_search_batch (csrc/match_plan.h BATCH_WAVES)
ROW_BYTES = 48                          # LDS bytes per keyframe-2 row (TRI_BATCH_ROW_BYTES)
LDS_MAX = 64 * 1024                     # BATCH_LDS_MAX
LDS_DEFAULT = 48 * 1024                 # DYNAMIC_LDS_DEFAULT_MAX
LDS_CAP = LDS_MAX // ROW_BYTES          # 1365: the last row capacity whose keyframe 2 sits in LDS
PLAIN_CAP = LDS_DEFAULT // ROW_BYTES    # 1024: the last row capacity without the dynamic-LDS opt-in
TH_LOW = 50
NLEVELS = 8
SCALE = (np.float32(1.2) ** np.arange(NLEVELS)).astype(np.float32)      # pKF2->mvScaleFactors
SIGMA2 = (SCALE * SCALE).astype(np.float32)                            # pKF2->mvLevelSigma2
f32 = np.float32


# ---- the image motion: F12 = ([e]x H)^T puts the epipolar line of a keyframe-1 keypoint through H * keypoint (and through the epipole e)
def motion(angle_deg=1.5, tx=-3.0, ty=2.0, epipole=mc.TRI_EPIPOLE):
    """-> dict(H, Hinv, F12 [3, 3] float32, ex, ey); the defaults are match_cases.tri_F12 / TRI_EPIPOLE"""
    a = np.deg2rad(angle_deg); cx, cy = 319.5, 239.5
    H = np.array([[np.cos(a), np.sin(a), cx + tx - cx * np.cos(a) - cy * np.sin(a)],
                  [-np.sin(a), np.cos(a), cy + ty + cx * np.sin(a) - cy * np.cos(a)], [0, 0, 1.0]])
    ex, ey = epipole
    E = np.array([[0, -1.0, ey], [1.0, 0, -ex], [-ey, ex, 0]])
    F12 = (E @ H).T
    return dict(H=H, Hinv=np.linalg.inv(H), F12=(F12 / np.abs(F12).max()).astype(np.float32), ex=float(f32(ex)), ey=float(f32(ey)))


def back(mot, x2, y2):
    """where a keyframe-1 keypoint lies whose epipolar line passes through (x2, y2) of image 2"""
    p = mot["Hinv"] @ np.stack([np.asarray(x2, np.float64), np.asarray(y2, np.float64), np.ones(np.shape(x2))])
    return (p[0] / p[2]).astype(np.float32), (p[1] / p[2]).astype(np.float32)


# ---- the matcher's two geometric gates in its own float arithmetic (src/ORBmatcher.cc:757-763, :140-157)
def epipole_rejects(ex, ey, x2, y2, scale):
    """two monocular keypoints: the candidate is skipped when it lies closer than sqrt(100 * scale) to the epipole (strict <)"""
    dx = f32(ex) - f32(x2); dy = f32(ey) - f32(y2)
    return bool(f32(f32(dx * dx) + f32(dy * dy)) < f32(f32(100) * f32(scale)))


def epi_dsqr(F12, x1, y1, x2, y2):
    F = np.asarray(F12, np.float32).reshape(9); x1, y1, x2, y2 = f32(x1), f32(y1), f32(x2), f32(y2)
    la = f32(f32(f32(x1 * F[0]) + f32(y1 * F[3])) + F[6]); lb = f32(f32(f32(x1 * F[1]) + f32(y1 * F[4])) + F[7]); lc = f32(f32(f32(x1 * F[2]) + f32(y1 * F[5])) + F[8])
    num = f32(f32(f32(la * x2) + f32(lb * y2)) + lc); den = f32(f32(la * la) + f32(lb * lb))
    return None if den == 0 else f32(f32(num * num) / den)


def epi_ok(F12, x1, y1, x2, y2, sigma2):
    d = epi_dsqr(F12, x1, y1, x2, y2)
    return d is not None and float(d) < 3.84 * float(f32(sigma2))


def bisect(pred, lo, hi, steps=60):
    """float32 (lo, hi) as close as bisection brings them with pred(lo) true and pred(hi) false"""
    lo, hi = f32(lo), f32(hi)
    assert pred(lo) and not pred(hi)
    for _ in range(steps):
        mid = f32((float(lo) + float(hi)) / 2)
        if mid == lo or mid == hi: break
        if pred(mid): lo = mid
        else: hi = mid
    return lo, hi


# ---- helper + oracle
def side(kp, desc, node, free=None, uright=None):
    s = dict(kp=kp, desc=np.ascontiguousarray(desc, np.uint8), node=np.asarray(node, np.int32),
             free=np.ones(len(kp), np.uint8) if free is None else np.asarray(free, np.uint8))
    if uright is not None: s["uright"] = np.asarray(uright, np.float32)
    return s


def pair(s1, s2, mot=None, only_stereo=False, ori=True, **extra):
    mot = mot or motion()
    return dict(s1=s1, s2=s2, F12=mot["F12"], ex=mot["ex"], ey=mot["ey"], only_stereo=only_stereo, ori=ori, **extra)


def cut(s, n):
    """the side's first n rows"""
    return {k: v[:n].copy() for k, v in s.items()}


def expect(oracle, c):
    """(matches12[n1], nmatches) of one pair: the CPU oracle on the CSR lists of the two node arrays"""
    s1, s2 = c["s1"], c["s2"]
    n1 = len(s1["kp"])
    pk, pf, ik, jf = bc.csr_from_nodes(s1["node"], s2["node"])
    if n1 == 0 or len(s2["kp"]) == 0 or len(pk) == 1:
        return np.full(n1, -1, np.int32), 0
    return oracle.search_for_triangulation(s1["kp"], s1["desc"], s1.get("uright"), s1["free"], s2["kp"], s2["desc"], s2.get("uright"), s2["free"], pk, pf, ik, jf,
                                           c["F12"], c["ex"], c["ey"], SCALE, SIGMA2, c["only_stereo"], c["ori"])


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


# ---- building blocks
def _kp(rng, n):
    kp = np.zeros(n, KP_DTYPE)
    kp["x"] = rng.uniform(20, 620, n); kp["y"] = rng.uniform(20, 460, n); kp["octave"] = rng.integers(0, 4, n); kp["angle"] = rng.uniform(0, 360, n); kp["size"] = 31
    return kp


def _stereo(rng, kp, p):
    return np.where(rng.random(len(kp)) < p, kp["x"] - 5, -1).astype(np.float32)


def world(rng, node, p_free=0.9, p_stereo=0.5):
    """a candidate side with the given node ids: random keypoints and descriptors, mixed free flags and right coordinates"""
    n = len(node)
    kp = _kp(rng, n)
    return side(kp, mc.rand_desc(rng, n), node, rng.random(n) < p_free, _stereo(rng, kp, p_stereo))


def moved(rng, w, node, mot=None, max_flips=40, p_free=0.9, p_stereo=0.5):
    """a query side with the given node ids for the candidate side w: a row is a noisy copy (descriptor, angle, level) of a random row of its node in w
    where w has one, placed where `mot` maps it onto that row (0.3 px of noise), random otherwise"""
    mot = mot or motion()
    node = np.asarray(node, np.int32); n = len(node)
    kp = _kp(rng, n); d = mc.rand_desc(rng, n)
    src = np.full(n, -1, np.int64)
    for i in range(n):
        js = np.flatnonzero(w["node"] == node[i]) if node[i] >= 0 else []
        if len(js): src[i] = js[rng.integers(0, len(js))]
    has = src >= 0
    if has.any():
        s = src[has]
        d[has] = mc.flip_bits(rng, w["desc"][s], max_flips)
        x, y = back(mot, w["kp"]["x"][s], w["kp"]["y"][s])
        kp["x"][has] = x + rng.normal(0, 0.3, len(s)); kp["y"][has] = y + rng.normal(0, 0.3, len(s))
        kp["octave"][has] = w["kp"]["octave"][s]; kp["angle"][has] = (w["kp"]["angle"][s] + rng.normal(0, 8, len(s))) % 360
    return side(kp, d, node, rng.random(n) < p_free, _stereo(rng, kp, p_stereo))


def from_bow_case(rng, nnodes):
    """match_cases.bow_case (1..3 features of each keyframe per node, keyframe-1 rows moved noisy copies of their node's keyframe-2 rows) as node arrays"""
    c = bc.from_bow_case(rng, nnodes)
    k1, k2 = c["kf"], c["f"]
    return pair(side(k1["kp"], k1["desc"], k1["node"], rng.random(len(k1["kp"])) < 0.9, _stereo(rng, k1["kp"], 0.3)),
                side(k2["kp"], k2["desc"], k2["node"], rng.random(len(k2["kp"])) < 0.9, _stereo(rng, k2["kp"], 0.3)))


# ---- 1. the ragged pool: slots of one capacity whose counts sit on the lane loop's edges
RAGGED_CAP = 96


def ragged_pool(rng):
    """-> (sides[12], pairs [(kf1 slot, kf2 slot)]).  Even slots are candidate sides cut from one world of 96 rows over 30 nodes, odd slots query sides
    moved from it: an (odd, even) pair matches; every other combination is legal and matches little or nothing"""
    cap = RAGGED_CAP
    w = world(rng, rng.integers(0, 30, cap))
    m = moved(rng, w, rng.integers(0, 30, cap))
    none = moved(rng, w, rng.choice([-1, -5, -(1 << 31)], 70))                      # every row in no node
    half = moved(rng, w, np.where(rng.random(80) < 0.5, -1, rng.integers(0, 30, 80)))
    apart = world(rng, 1000 + rng.integers(0, 30, 80))                             # node ids no other slot has
    empty = cut(w, 0)
    sides = [w, m, cut(w, 64), cut(m, 65), cut(w, 65), cut(m, 63), empty, none, apart, half, cut(w, 1), cut(m, 1)]
    pairs = [(1, 0), (3, 0), (5, 0), (9, 0), (1, 2), (3, 2), (5, 2), (1, 4), (3, 4), (5, 4), (9, 4), (9, 2),      # query side against candidate side
             (11, 0), (1, 10), (11, 10), (7, 0), (1, 8),                                                        # one row; no node; nodes on one side only
             (6, 0), (1, 6), (6, 6), (6, 10), (11, 6),                                                          # an empty side: either, both
             (0, 1), (2, 3), (1, 1), (0, 0), (3, 5)]                                                            # swapped roles, kf1 == kf2, two query sides
    return sides, pairs


def with_flags(c, only_stereo, ori):
    return dict(c, only_stereo=bool(only_stereo), ori=bool(ori))


# ---- 2. one query against chosen candidates
QNODE = 21


def query_case(rng, cands, mot=None, xy1=None, q_ur=-1.0, nfill=7, only_stereo=False, ori=True):
    """side 1: nfill rows of other nodes and ONE query row of node QNODE; side 2: nfill + 2 rows of other nodes and the candidates -- dicts
    (bits: descriptor distance to the query, None for an unrelated descriptor; xy: position in image 2; octave; ur; free) -- of node QNODE, in the given
    order at ascending scattered rows.  The query lies at xy1, by default where its epipolar line passes through the first candidate.
    -> pair with q = the query's row, cand = the candidates' rows"""
    mot = mot or motion()
    n1, n2 = nfill + 1, nfill + 2 + len(cands)
    q = int(rng.integers(0, n1)); rows = np.sort(rng.choice(n2, len(cands), replace=False))
    kp1 = _kp(rng, n1); kp2 = _kp(rng, n2)
    d1 = mc.rand_desc(rng, n1); d2 = mc.rand_desc(rng, n2)
    node1 = rng.integers(100, 110, n1).astype(np.int32); node2 = rng.integers(100, 110, n2).astype(np.int32)
    ur1 = np.full(n1, -1, np.float32); ur2 = np.full(n2, -1, np.float32); free2 = np.ones(n2, np.uint8)
    base = d1[q]; perm = rng.permutation(256); used = 0
    node1[q] = QNODE; ur1[q] = q_ur; kp1["angle"][q] = 40.0
    for r, c in zip(rows, cands):
        node2[r] = QNODE
        if c.get("bits") is not None:
            d2[r] = bc._flip(base, perm[used:used + c["bits"]]); used += c["bits"]
            assert used <= 256
        kp2["x"][r], kp2["y"][r] = c.get("xy", (300.0, 200.0)); kp2["octave"][r] = c.get("octave", 0); kp2["angle"][r] = 40.0
        ur2[r] = c.get("ur", -1.0); free2[r] = c.get("free", 1)
    if xy1 is None:
        x, y = back(mot, kp2["x"][rows[0]], kp2["y"][rows[0]]); xy1 = (float(x), float(y))
    kp1["x"][q], kp1["y"][q] = xy1
    return pair(side(kp1, d1, node1, None, ur1), side(kp2, d2, node2, free2, ur2), mot, only_stereo, ori, q=q, cand=rows)


def lane_cases(rng):
    """name -> (pair, candidate position that wins): one node holding 1, 63, 64, 65 or 129 keyframe-2 rows, all on the epipolar line, one of them 5 bits
    from the query -- the first, a middle or the last"""
    out = {}
    for m in (1, 63, 64, 65, 129):
        for pos in sorted({0, m // 2, m - 1}):
            out["lane_%d_%d" % (m, pos)] = (query_case(rng, [dict(bits=5 if k == pos else None) for k in range(m)], nfill=10), pos)
    return out


def off_line(mot, xy, px):
    """xy moved px pixels along the normal of the epipolar line through it"""
    x1, y1 = back(mot, xy[0], xy[1])
    F = mot["F12"].astype(np.float64)
    la = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]; lb = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
    nrm = np.hypot(la, lb)
    return (float(xy[0] + px * la / nrm), float(xy[1] + px * lb / nrm))


def tie_cases(rng):
    """name -> (pair, candidate position that wins or None).  Equal distances: the LAST candidate wins (`dist > bestDist` lets an equal one through).  A
    closer candidate 30 px off the epipolar line never becomes bestDist, so it stops nothing, before or after the one that passes.  TH_LOW is inclusive"""
    mot = motion(); on = (300.0, 200.0); off = off_line(mot, on, 30.0)
    return {"tie_2": (query_case(rng, [dict(bits=12), dict(bits=12)]), 1),
            "tie_3": (query_case(rng, [dict(bits=12), dict(bits=12), dict(bits=12), dict(bits=40)]), 2),
            "closer_fails_before": (query_case(rng, [dict(bits=5, xy=off), dict(bits=20, xy=on)], xy1=tuple(float(v) for v in back(mot, *on))), 1),
            "closer_fails_after": (query_case(rng, [dict(bits=20, xy=on), dict(bits=5, xy=off)], xy1=tuple(float(v) for v in back(mot, *on))), 0),
            "dist_50": (query_case(rng, [dict(bits=50)]), 0), "dist_51": (query_case(rng, [dict(bits=51)]), None),
            "not_free": (query_case(rng, [dict(bits=5, free=0), dict(bits=30)]), 1)}


EPIPOLE_IN_IMAGE = (330.0, 210.0)


def epipole_cases(rng):
    """name -> (pair, matched).  The epipole lies in the image; the candidate sits on the row of the epipole at the last float x whose squared distance is
    still < 100 * scale[octave] (inside: skipped when both keypoints are monocular) or the first that is not (outside); the query lies where its epipolar
    line passes through the candidate.  With a right coordinate on either side the gate is not applied"""
    mot = motion(epipole=EPIPOLE_IN_IMAGE); ex, ey = mot["ex"], mot["ey"]
    out = {}
    for octave in (0, 3):
        inside, outside = bisect(lambda x: epipole_rejects(ex, ey, x, ey, SCALE[octave]), ex + 1.0, ex + 40.0)
        assert np.nextafter(inside, f32(1e9)) == outside
        for name, x, kw, matched in (("inside", inside, {}, False), ("outside", outside, {}, True), ("inside_stereo1", inside, dict(q_ur=7.0), True),
                                     ("inside_stereo2", inside, dict(ur=7.0), True)):
            cand = dict(bits=9, xy=(float(x), float(ey)), octave=octave, ur=kw.get("ur", -1.0))
            out["epipole_oct%d_%s" % (octave, name)] = (query_case(rng, [cand], mot, q_ur=kw.get("q_ur", -1.0)), matched)
    return out


def epipolar_cases(rng):
    """name -> (pair, matched): the candidate is moved off the query's epipolar line until dsqr crosses 3.84 * sigma2[octave]; below = the last offset
    that passes, above = the first that does not (bisection on the float32 y coordinate, the matcher's own expression)"""
    mot = motion(); on = (300.0, 200.0)
    x1, y1 = back(mot, *on)
    out = {}
    for octave in (0, 2):
        ok = lambda y: epi_ok(mot["F12"], x1, y1, on[0], y, SIGMA2[octave])
        below, above = bisect(ok, on[1], on[1] + 60.0)
        assert below > on[1] + 0.5
        for name, y, matched in (("below", below, True), ("above", above, False)):
            out["epipolar_oct%d_%s" % (octave, name)] = (query_case(rng, [dict(bits=9, xy=(on[0], float(y)), octave=octave)], mot, xy1=(float(x1), float(y1))), matched)
    return out


def zero_F12(c):
    """the pair under an all-zero F12: den == 0 for every query, nothing matches"""
    return dict(c, F12=np.zeros((3, 3), np.float32))


def two_motions(rng, n=80, nodes=25):
    """two pairs over the SAME candidate side whose query sides were moved by different motions (and carry different epipoles): each matches under its own
    F12 and (almost) nothing under the other's"""
    w = world(rng, rng.integers(0, nodes, n), p_stereo=0.0)
    out = []
    for mot in (motion(), motion(-2.5, 6.0, -4.0, (2600.0, -150.0))):
        out.append(pair(moved(rng, w, rng.integers(0, nodes, n), mot, p_stereo=0.0), w, mot))
    return out


# ---- 3. rotation: the histogram shapes of rot_cases (side 1 = keyframe 1), and two neighbouring pairs whose dominant rotations differ
ROT_NAMES = ("wrap_345_360", "both_dropped", "ties", "boundary")


def rot_pair(c, turn=0.0):
    kp1 = c["kp1"].copy()
    kp1["angle"] = ((kp1["angle"] + f32(turn)) % f32(360)).astype(np.float32)
    return pair(side(kp1, c["d1"], c["node1"]), side(c["kp2"], c["d2"], c["node2"]), rc=c)


def rot_pairs():
    """name -> pair; `neighbour_0` / `neighbour_90` are the boundary case and the same features with keyframe-1 angles turned by 90 degrees: alone each
    loses its group of 2 (bins 3, 6, 9 -> 30, 3, 2 and 6, 9, 12 | 0); histograms added over both (3: 30, 6: 33, 9: 5) would keep bin 9 in the first"""
    cs = rot_cases.all_cases()
    out = {name: rot_pair(cs[name]) for name in ROT_NAMES}
    out["neighbour_0"] = rot_pair(cs["boundary"]); out["neighbour_90"] = rot_pair(cs["boundary"], 90.0)
    return out


# ---- 4. CreateNewMapPoints: one new keyframe against its neighbours
def neighbours_pool(rng, nneigh=20, cap=64):
    """-> sides[1 + nneigh]: slot 0 the query side, slots 1.. candidate sides -- the world the query side was moved from, each with its own descriptor
    noise, free flags, right coordinates and count"""
    w = world(rng, rng.integers(0, 20, cap - 4))
    sides = [moved(rng, w, rng.integers(0, 20, cap - 2), max_flips=20)]
    for k in range(nneigh):
        n = int(rng.integers(cap // 2, cap - 3))
        s = cut(w, n)
        s["desc"] = mc.flip_bits(rng, s["desc"], 25); s["free"] = (rng.random(n) < 0.85).astype(np.uint8); s["uright"] = _stereo(rng, s["kp"], 0.4)
        sides.append(s)
    return sides


# ---- 5. both forms of the kernel: a pool of full slots
def full_pool(rng, cap):
    """-> sides: a candidate side and a query side of `cap` rows (three rows per node) and a small pair of 200 rows over other nodes"""
    w = world(rng, rng.permutation(cap) // 3)
    m = moved(rng, w, rng.permutation(cap) // 3)
    w2 = world(rng, 5000 + rng.permutation(200) // 3)
    return [w, m, w2, moved(rng, w2, 5000 + rng.permutation(200) // 2)]


FULL_PAIRS = [(1, 0), (0, 1), (1, 1), (3, 2), (3, 0)]


# ---- packing: slots of `cap` rows, junk past every count
def pack_pool(rng, sides, cap):
    """[S, cap] buffers of the sides, rows at or past a side's count random bytes (node ids, free flags and right coordinates included)
    -> dict(kp, desc, node, free, uright, n); a side without right coordinates is monocular (-1)"""
    S = len(sides)
    P = dict(kp=bc.junk(rng, (S, cap), KP_DTYPE), desc=bc.junk(rng, (S, cap, 32), np.uint8), node=bc.junk(rng, (S, cap), np.int32),
             free=bc.junk(rng, (S, cap), np.uint8), uright=bc.junk(rng, (S, cap), np.float32), n=np.zeros(S, np.int32))
    for i, s in enumerate(sides):
        n = len(s["kp"])
        assert n <= cap, (i, n, cap)
        P["kp"][i, :n] = s["kp"]; P["desc"][i, :n] = s["desc"]; P["node"][i, :n] = s["node"]; P["free"][i, :n] = s["free"]; P["n"][i] = n
        P["uright"][i, :n] = s["uright"] if "uright" in s else -1.0
    return P


def pack_pairs(cases_and_slots):
    """[(pair, kf1 slot, kf2 slot)] -> rows of sslam_tri_pair (frontend.TRI_PAIR_DTYPE)"""
    dt = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("F12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4")])
    out = np.zeros(len(cases_and_slots), dt)
    for p, (c, a, b) in enumerate(cases_and_slots):
        out[p] = (a, b, np.asarray(c["F12"], np.float32).reshape(9), c["ex"], c["ey"])
    return out


# ---- the reference's own SearchForTriangulation takes the node arrays directly; it files a NEGATIVE id under (unsigned)id, so for it the rows "in no
# node" get ids of their own that no other row has (bow_batch_cases.ref_nodes)
def ref_nodes(c):
    return bc.ref_nodes(dict(kf=dict(node=c["s1"]["node"]), f=dict(node=c["s2"]["node"])))
