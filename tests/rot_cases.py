"""Inputs of the rotation-consistency tests (tests/test_rot_gpu.py, tests/test_rot_cases_cpu.py): two frames of N + EXTRA features whose matches are
forced -- pair k has the same random descriptor in both frames, every other descriptor is random (about 128 bits from anything) -- and whose angles are
chosen per pair, so that the rotation histogram of the check every matcher ends with (rotation bin, 30 bins, ComputeThreeMaxima, prune) is the one
the case names.  Side 1 is the side whose angle comes first in `rot = angle1 - angle2`: F1 of SearchForInitialization, the queries of SearchByProjection,
the keyframe of SearchByBoW, keyframe 1 of SearchForTriangulation.  A side-1 feature sits where the image motion of match_cases.tri_F12 puts its
partner, so the pair passes the windows of the first two and the epipolar gate of the last; every feature is of level 0.  All angles and rotations are
multiples of 0.25, so angle1 - angle2 is exact in float and a case lands on the bin boundary it aims at.
Every generator is a pure function of its numpy Generator."""
import numpy as np
import match_cases as mc
import bow_batch_cases as bc
from oracle_lib import KP_DTYPE

HISTO_LENGTH = 30
EXTRA = 8          # features per frame without a partner

# name -> (groups [(matches, rot_lo, rot_hi)], histogram {bin: matches}, groups the check prunes).  bin = round(rot / 30): the reference's factor is
# 1 / HISTO_LENGTH, not HISTO_LENGTH / 360, so angles of [0, 360) use the bins 0 .. 12
SPECS = {
    # 3 < 0.1f * 30 is false: the second bin stays, the third (2) goes -- exactly on the 10 % boundary
    "boundary": ([(30, 85, 95), (3, 175, 185), (2, 265, 275)], {3: 30, 6: 3, 9: 2}, [2]),
    "both_dropped": ([(30, 85, 95), (2, 175, 185), (2, 265, 275)], {3: 30, 6: 2, 9: 2}, [1, 2]),
    # ties: a later bin needs strictly more, so the first three bin indices stay
    "ties": ([(10, 25, 35), (10, 115, 125), (10, 205, 215), (10, 295, 305)], {1: 10, 4: 10, 7: 10, 10: 10}, [3]),
    # rot in [345, 360) rounds to 12 (not to HISTO_LENGTH): a bin of its own, which ties with bin 0 for the third place and loses it; folded into bin 0
    # the two groups would hold 12 and nothing would be pruned
    "wrap_345_360": ([(6, 345, 359.75), (6, 0, 14), (20, 85, 95), (9, 175, 185)], {12: 6, 0: 6, 3: 20, 6: 9}, [0]),
    # bin == HISTO_LENGTH -> 0 needs rot in [885, 915), which no two angles of [0, 360) give: side 1 carries angles up to 1275 here.  The group joins the
    # one of bin 0, which takes the third place with 12 and pushes bin 9 out
    "wrap_bin_30": ([(6, 885, 914.75), (6, 0, 14), (20, 85, 95), (13, 175, 185), (7, 265, 275)], {0: 12, 3: 20, 6: 13, 9: 7}, [4]),
    # rot = 15: 15 * (1.0f / 30) is 0.5 exactly and roundf takes it to 1 (half away from zero; half-to-even would fold the group into bin 0, whose 13 would
    # then stay and nothing would be pruned)
    "half": ([(8, 15, 15), (5, 0, 14), (20, 85, 95), (9, 175, 185)], {1: 8, 0: 5, 3: 20, 6: 9}, [1]),
}


def rot_bin(angle1, angle2):
    """the reference's bin in float arithmetic; C's round() is half away from zero"""
    rot = (np.asarray(angle1, np.float32) - np.asarray(angle2, np.float32)).astype(np.float32)
    rot = np.where(rot < 0, rot + np.float32(360), rot).astype(np.float32)
    x = (rot * (np.float32(1) / np.float32(HISTO_LENGTH))).astype(np.float32)
    b = np.floor(x.astype(np.float64) + 0.5).astype(np.int64)
    return np.where(b == HISTO_LENGTH, 0, b)


def make(rng, name):
    """-> dict(kp1, d1, node1, kp2, d2, node2, i1[M], i2[M] (pair k = side-1 row i1[k], side-2 row i2[k]), group[M], hist, pruned[M] (bool), name)"""
    groups, hist, pruned_groups = SPECS[name]
    M = sum(g[0] for g in groups); n = M + EXTRA
    group = rng.permutation(np.repeat(np.arange(len(groups)), [g[0] for g in groups]))
    rot = np.array([rng.choice(np.arange(groups[g][1], groups[g][2] + 0.125, 0.25)) for g in group], np.float32)
    i1 = rng.permutation(n)[:M]; i2 = rng.permutation(n)[:M]
    kp1 = np.zeros(n, KP_DTYPE); kp2 = np.zeros(n, KP_DTYPE)
    for kp in (kp1, kp2):
        kp["x"] = rng.uniform(60, 580, n); kp["y"] = rng.uniform(60, 420, n); kp["size"] = 31; kp["angle"] = rng.integers(0, 720, n) * 0.5
    Hinv = np.linalg.inv(mc._tri_motion()[0])
    p1 = Hinv @ np.stack([kp2["x"][i2], kp2["y"][i2], np.ones(M)]).astype(np.float64)
    kp1["x"][i1] = p1[0] / p1[2]; kp1["y"][i1] = p1[1] / p1[2]
    a1 = kp2["angle"][i2] + rot
    kp1["angle"][i1] = np.where(rot < 360, a1 % np.float32(360), a1)
    d1 = mc.rand_desc(rng, n); d2 = mc.rand_desc(rng, n)
    d1[i1] = d2[i2]
    # vocabulary nodes: one per pair; the features without a partner share nodes too (and stay unmatched: their descriptors are unrelated)
    node1 = np.zeros(n, np.int32); node2 = np.zeros(n, np.int32)
    node1[i1] = node2[i2] = 1 + rng.permutation(M)
    node1[np.setdiff1d(np.arange(n), i1)] = node2[np.setdiff1d(np.arange(n), i2)] = 500 + np.arange(EXTRA)
    return dict(name=name, kp1=kp1, d1=d1, node1=node1, kp2=kp2, d2=d2, node2=node2, i1=i1, i2=i2, group=group, hist=hist, pruned=np.isin(group, pruned_groups))


def all_cases():
    return {name: make(np.random.default_rng(9100 + k), name) for k, name in enumerate(SPECS)}


# ---- what each matcher takes
def prev_matched(c):
    return np.stack([c["kp1"]["x"], c["kp1"]["y"]], axis=1).astype(np.float32)


def queries(c, radius=20.0):
    """side 1 as the queries of SearchByProjection(CurrentFrame, LastFrame) (mode 1): no level window, every projection observed"""
    q = np.zeros(len(c["kp1"]), mc.PQ_DTYPE)
    q["u"] = c["kp1"]["x"]; q["v"] = c["kp1"]["y"]; q["radius"] = radius; q["min_level"] = 0; q["max_level"] = -1; q["angle"] = c["kp1"]["angle"]
    q["ur"] = -1; q["valid"] = 1; q["obs_positive"] = 1
    return q


def bow_pair(c):
    """the two sides as a pair of bow_batch_cases (node arrays; csr_from_nodes gives the lists of the single calls)"""
    n = len(c["kp1"])
    return bc.case(bc.side(c["kp1"], c["d1"], c["node1"], np.ones(n)), bc.side(c["kp2"], c["d2"], c["node2"]), 0.9, True)


# ---- what each matcher has to answer: want_12 indexed by side 1 (SearchForInitialization, SearchByBoW of two keyframes, SearchForTriangulation),
# want_21 by side 2 (SearchByProjection, SearchByBoW of a keyframe and a frame); `gone` is what a pruned match leaves (-1, SearchByProjection -2)
def want_12(c, ori):
    m = np.full(len(c["kp1"]), -1, np.int32)
    keep = ~c["pruned"] if ori else np.ones(len(c["i1"]), bool)
    m[c["i1"][keep]] = c["i2"][keep]
    return m, int(keep.sum())


def want_21(c, ori, gone=-1):
    a = np.full(len(c["kp2"]), -1, np.int32)
    a[c["i2"]] = c["i1"]
    if ori: a[c["i2"][c["pruned"]]] = gone
    return a, int((~c["pruned"]).sum()) if ori else len(c["i1"])
