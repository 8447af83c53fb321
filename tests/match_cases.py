"""Synthetic matcher inputs for tests/test_match_sizes_gpu.py and tests/test_match_cases_cpu.py: keypoints, keylines, queries and
descriptors built directly (no image extraction), sized to cross the thresholds at which csrc/match.hip picks another kernel, LDS
layout or grid.  Every generator is a pure function of its numpy Generator."""
import numpy as np
from oracle_lib import KP_DTYPE, KL_DTYPE

PQ_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("u2", "<f4"), ("v2", "<f4"), ("radius", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                     ("angle", "<f4"), ("ur", "<f4"), ("valid", "<i4"), ("obs_positive", "<i4")])      # sslam_proj_query (include/sslam_frontend.h)

CLUSTER = 12          # features and identical queries per cluster: more than PROJ_K = 8 (csrc/match_ordered.h)
# (features, ordinary queries) of the projection cases: the frame in LDS (n <= 2048), features in global memory, commit LDS beyond 48 KB
# (8 n + 64 bytes: n > 6136), and the one-wave kernel beyond 8192 features (slow per query: fewer ordinary queries)
PROJ_SIZES = [(600, 300), (2100, 300), (6200, 300), (8200, 40)]
BOW_NODES, BOW_SEED = 4096 + 50, 4146


def proj_seed(n, kind, mode):
    return 1000 * n + 10 * kind + mode


def rand_desc(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def flip_bits(rng, d, max_flips):
    """every row of d with 0 .. max_flips - 1 distinct random bits flipped"""
    out = d.copy()
    for i in range(len(out)):
        k = int(rng.integers(0, max_flips))
        if k:
            b = rng.choice(256, size=k, replace=False)
            np.bitwise_xor.at(out[i], b >> 3, (1 << (b & 7)).astype(np.uint8))
    return out


def _flip_exact(rng, row, k):
    """row with exactly k bits flipped"""
    out = row.copy()
    b = rng.choice(256, size=k, replace=False)
    np.bitwise_xor.at(out, b >> 3, (1 << (b & 7)).astype(np.uint8))
    return out


# ---- A. projection matcher: clusters that exhaust the per-query top-8 list
def cluster_case(rng, n, kind=0, C=30, nq_extra=300):
    """n features (kind 0: keypoints, 1: keylines) and the queries of a window search in which the ordered commit must re-scan.

    C clusters of 12 features, each cluster inside the window of 12 consecutive IDENTICAL queries (same window, descriptor q_c,
    obs_positive = 1, valid = 1).  Feature j of a cluster has q_c with exactly j bits flipped (distances 0..11, all distinct) and its
    level alternates between the two levels the query admits, so best and second-best never share a level (mode 0's ratio test never
    applies).  By construction query k of a cluster takes feature k; from the 8th (mode 1) / 7th (mode 0) query on, every entry of the
    query's top-8 list is taken while 12 candidates exist.  The remaining features are padding away from every cluster window, with
    nq_extra ordinary jittered queries on them (some obs_positive = 0, some valid = 0) and 10 % initial occupancy on the padding only.

    -> dict(feats, desc, q, qdesc, occ, uright, cfeat[C, 12], cquery[C, 12])"""
    assert n >= C * CLUSTER + 50 and C <= 30
    npad = n - C * CLUSTER
    centres = np.array([(60.0 + 100.0 * (c % 6), 60.0 + 90.0 * (c // 6)) for c in range(C)], np.float32)      # 6 x 5 lattice, 90+ px apart
    pos = np.zeros((n, 2), np.float32)
    # padding: at least 30 px (Chebyshev) from every cluster centre; cluster features within 5 px, cluster windows 12 px, padding windows <= 14 px + 3 px jitter
    k = 0
    while k < npad:
        p = np.stack([rng.uniform(8, 632, 2 * npad), rng.uniform(8, 472, 2 * npad)], axis=1).astype(np.float32)
        far = (np.abs(p[:, None, :] - centres[None, :, :]).max(axis=2) >= 30).all(axis=1)
        p = p[far][: npad - k]
        pos[k:k + len(p)] = p; k += len(p)
    slots = rng.permutation(n)                                   # where each feature sits in the frame: clusters scattered over the index range
    pad_idx = np.sort(slots[:npad]); cfeat = slots[npad:].reshape(C, CLUSTER)
    pos[pad_idx] = pos[:npad].copy()
    desc = rand_desc(rng, n)
    octave = rng.integers(0, 8, n).astype(np.int32)
    angle = rng.uniform(0, 360, n).astype(np.float32)
    qc = rand_desc(rng, C)
    cang = rng.uniform(0, 360, C).astype(np.float32)
    for c in range(C):
        for j in range(CLUSTER):
            f = cfeat[c, j]
            pos[f] = centres[c] + rng.uniform(-5, 5, 2).astype(np.float32)
            desc[f] = _flip_exact(rng, qc[c], j)
            octave[f] = (1 + (j & 1)) if kind == 0 else (j & 1)
            angle[f] = cang[c]
    occ = np.zeros(n, np.uint8); occ[pad_idx] = rng.random(npad) < 0.10
    uright = np.where(rng.random(n) < 0.3, pos[:, 0] - rng.uniform(0, 40, n), -1).astype(np.float32)

    # queries: a few ordinary ones first (so the clusters do not start on a multiple of 64), the clusters, the rest of the ordinary ones
    nq = C * CLUSTER + nq_extra
    lead = min(17, nq_extra)
    q = np.zeros(nq, PQ_DTYPE); qdesc = np.zeros((nq, 32), np.uint8)
    cquery = (lead + np.arange(C * CLUSTER)).reshape(C, CLUSTER)
    ext = np.concatenate([np.arange(lead), np.arange(lead + C * CLUSTER, nq)])
    src = pad_idx[rng.integers(0, npad, nq_extra)]               # the padding feature an ordinary query aims at
    jit = rng.normal(0, 1.0, (nq_extra, 2)).clip(-3, 3).astype(np.float32)
    qdesc[ext] = flip_bits(rng, desc[src], 20)
    q["valid"][ext] = rng.random(nq_extra) < 0.9
    q["obs_positive"][ext] = rng.random(nq_extra) < 0.7
    if kind == 0:
        q["u"][ext] = pos[src, 0] + jit[:, 0]; q["v"][ext] = pos[src, 1] + jit[:, 1]
        q["radius"][ext] = rng.uniform(8, 14, nq_extra)
        o = octave[src]
        q["min_level"][ext] = o - 1; q["max_level"][ext] = np.where(rng.random(nq_extra) < 0.3, -1, o + 1)
        q["min_level"][ext] = np.where(q["max_level"][ext] < 0, o, q["min_level"][ext])          # the forward window [o, inf)
        q["angle"][ext] = (angle[src] + rng.normal(0, 12, nq_extra)) % 360
        q["ur"][ext] = np.where(uright[src] > 0, uright[src] + rng.normal(0, 6, nq_extra), q["u"][ext] - 10)
        for c in range(C):
            qi = cquery[c]
            q["u"][qi] = centres[c, 0]; q["v"][qi] = centres[c, 1]; q["radius"][qi] = 12.0
            q["min_level"][qi] = 1; q["max_level"][qi] = 2; q["angle"][qi] = cang[c]
            q["ur"][qi] = centres[c, 0] - 20.0
            uright[cfeat[c]] = np.where(np.arange(CLUSTER) % 3 == 0, pos[cfeat[c], 0] - 20.0, -1)      # a third pass the stereo gate (|du| <= 5 < radius), the rest have no right coordinate
            qdesc[qi] = qc[c]
        q["valid"][cquery] = 1; q["obs_positive"][cquery] = 1
        feats = np.zeros(n, KP_DTYPE)
        feats["x"] = pos[:, 0]; feats["y"] = pos[:, 1]; feats["size"] = 31; feats["angle"] = angle; feats["octave"] = octave
        feats["response"] = rng.uniform(10, 100, n); feats["class_id"] = -1
    else:
        # keylines: GetLinesInArea takes a line when its midpoint lies within `radius` of the query's midpoint and
        # (slope of the projected segment) - angle <= radius * 0.01, in index order
        half = np.stack([rng.uniform(6, 25, n), rng.uniform(-20, 20, n)], axis=1).astype(np.float32)      # half extent; x part > 0: no vertical segment
        feats = np.zeros(n, KL_DTYPE)
        feats["pt_x"] = pos[:, 0]; feats["pt_y"] = pos[:, 1]; feats["octave"] = np.where(np.isin(np.arange(n), cfeat), octave, 0); feats["class_id"] = np.arange(n)
        feats["startPointX"] = pos[:, 0] - half[:, 0]; feats["startPointY"] = pos[:, 1] - half[:, 1]
        feats["endPointX"] = pos[:, 0] + half[:, 0]; feats["endPointY"] = pos[:, 1] + half[:, 1]
        for a, b in (("sPointInOctaveX", "startPointX"), ("sPointInOctaveY", "startPointY"), ("ePointInOctaveX", "endPointX"), ("ePointInOctaveY", "endPointY")): feats[a] = feats[b]
        feats["lineLength"] = 2 * np.hypot(half[:, 0], half[:, 1]); feats["numOfPixels"] = feats["lineLength"].astype(np.int32); feats["size"] = 1; feats["response"] = 0.5
        slope = ((feats["startPointY"] - feats["endPointY"]) / (feats["startPointX"] - feats["endPointX"])).astype(np.float32)
        feats["angle"] = slope + rng.uniform(-0.2, 0.4, n).astype(np.float32)                    # ordinary lines: the slope gate passes for most, fails for some
        q["u"][ext] = feats["startPointX"][src] + jit[:, 0]; q["v"][ext] = feats["startPointY"][src] + jit[:, 1]
        q["u2"][ext] = feats["endPointX"][src] + jit[:, 0]; q["v2"][ext] = feats["endPointY"][src] + jit[:, 1]
        q["radius"][ext] = rng.uniform(8, 14, nq_extra); q["min_level"][ext] = -1; q["max_level"][ext] = 0
        for c in range(C):
            qi = cquery[c]
            q["u"][qi] = centres[c, 0] - 15; q["v"][qi] = centres[c, 1] - 6; q["u2"][qi] = centres[c, 0] + 15; q["v2"][qi] = centres[c, 1] + 6      # midpoint = the centre, slope 0.4
            q["radius"][qi] = 12.0; q["min_level"][qi] = 0; q["max_level"][qi] = 1
            feats["angle"][cfeat[c]] = np.float32(0.4) + np.float32(0.5)                          # slope - angle = -0.5 <= 0.12: the gate passes
            qdesc[qi] = qc[c]
        q["valid"][cquery] = 1; q["obs_positive"][cquery] = 1
        uright = None
    return dict(feats=feats, desc=desc, q=q, qdesc=qdesc, occ=occ, uright=uright, cfeat=cfeat, cquery=cquery)


def proj_params(kind, mode):
    """(nnratio, th_dist, check_orientation) of the cluster tests: the reference's values; the rotation check is on where it exists (keypoints, mode 1)"""
    if kind == 1: return 0.6, 100, True
    return (0.8, 100, True) if mode == 0 else (0.9, 100, True)


def clusters_taken_in_order(case, assigned):
    """the generator's promise: feature j of every cluster went to query j of that cluster"""
    return bool((assigned[case["cfeat"]] == case["cquery"]).all())


# ---- B. grid caps
def fuse_case(rng, kind, n, nq):
    """n features of a keyframe and nq Fuse queries aimed at them"""
    if kind == 0:
        feats = np.zeros(n, KP_DTYPE)
        feats["x"] = rng.uniform(8, 632, n); feats["y"] = rng.uniform(8, 472, n); feats["octave"] = rng.integers(0, 4, n); feats["angle"] = rng.uniform(0, 360, n); feats["size"] = 31
        fx, fy = feats["x"], feats["y"]
    else:
        feats = np.zeros(n, KL_DTYPE)
        feats["pt_x"] = rng.uniform(30, 610, n); feats["pt_y"] = rng.uniform(30, 450, n); feats["octave"] = rng.integers(0, 2, n)
        hx = rng.uniform(6, 25, n).astype(np.float32); hy = rng.uniform(-20, 20, n).astype(np.float32)
        feats["startPointX"] = feats["pt_x"] - hx; feats["startPointY"] = feats["pt_y"] - hy; feats["endPointX"] = feats["pt_x"] + hx; feats["endPointY"] = feats["pt_y"] + hy
        feats["angle"] = (hy / hx) + rng.uniform(-0.2, 0.4, n).astype(np.float32)
    desc = rand_desc(rng, n)
    uright = np.where(rng.random(n) < 0.4, (feats["x"] if kind == 0 else feats["pt_x"]) - rng.uniform(0, 40, n), -1).astype(np.float32)
    src = rng.integers(0, n, nq)
    q = np.zeros(nq, PQ_DTYPE)
    qdesc = flip_bits(rng, desc[src], 20)
    jit = rng.normal(0, 1.0, (nq, 2)).astype(np.float32)
    o = feats["octave"][src]
    if kind == 0:
        sc = (1.2 ** np.arange(8)).astype(np.float32)
        q["u"] = fx[src] + jit[:, 0]; q["v"] = fy[src] + jit[:, 1]; q["radius"] = 3.0 * sc[o]
        q["ur"] = np.where(uright[src] >= 0, uright[src] + rng.normal(0, 1.0, nq), q["u"] - 10)
        pred = o + rng.integers(0, 2, nq)
    else:
        q["u"] = feats["startPointX"][src] + jit[:, 0]; q["v"] = feats["startPointY"][src] + jit[:, 1]
        q["u2"] = feats["endPointX"][src] + jit[:, 0]; q["v2"] = feats["endPointY"][src] + jit[:, 1]
        q["radius"] = np.where(rng.random(nq) < 0.5, 15.0, 24.0)
        pred = o + rng.integers(0, 2, nq)
    q["min_level"] = pred - 1; q["max_level"] = pred
    q["valid"] = rng.random(nq) < 0.95; q["obs_positive"] = 1
    return dict(feats=feats, desc=desc, uright=uright if kind == 0 else None, q=q, qdesc=qdesc)


def distinctive_case(rng, nsets):
    """nsets observation sets of 0..6 noisy copies of one descriptor each -> (desc, ptr)"""
    sizes = rng.integers(0, 7, nsets)
    sizes[-19:] = rng.integers(2, 7, 19)                         # the sets behind the grid cap are not empty
    sets = []
    for m in sizes:
        base = np.repeat(rand_desc(rng, 1), m, axis=0)
        if m: base = base ^ np.packbits(rng.random((m, 256)) < rng.uniform(0.02, 0.3, (m, 1)), axis=1)
        sets.append(base)
    return np.concatenate(sets), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# the rigid image motion of the existing triangulation test: F12 = ([e]x H)^T puts the epipolar line of a keyframe-1 keypoint through H * keypoint
TRI_EPIPOLE = (-2000.0, 300.0)


def _tri_motion():
    a = np.deg2rad(1.5); cx, cy = 319.5, 239.5
    H = np.array([[np.cos(a), np.sin(a), cx - 3.0 - cx * np.cos(a) - cy * np.sin(a)],
                  [-np.sin(a), np.cos(a), cy + 2.0 + cx * np.sin(a) - cy * np.cos(a)], [0, 0, 1.0]])
    ex, ey = TRI_EPIPOLE
    E = np.array([[0, -1.0, ey], [1.0, 0, -ex], [-ey, ex, 0]])
    F12 = (E @ H).T
    return H, (F12 / np.abs(F12).max()).astype(np.float32)


def tri_F12():
    return _tri_motion()[1]


def bow_case(rng, nnodes):
    """Two frames filed under nnodes shared vocabulary nodes, 1..3 features of each frame per node (2 * nnodes features per frame in
    all), every feature under exactly one node (disjoint lists: the multi-workgroup launch).  A keyframe-1 feature is a noisy copy of one
    of its node's frame-2 features (descriptor, angle, and the position moved back through the image motion of tri_F12, so that the pair
    passes the epipolar test of SearchForTriangulation).
    -> dict(kp1, d1, kp2, d2, ptr1, ptr2, idx1, idx2, node_of_2[n2])"""
    def counts():
        c = np.full(nnodes, 2, np.int64)
        sw = rng.permutation(nnodes)[: 2 * (nnodes // 3)]
        c[sw[: len(sw) // 2]] = 1; c[sw[len(sw) // 2:]] = 3
        return c
    c1, c2 = counts(), counts()
    n1, n2 = int(c1.sum()), int(c2.sum())
    ptr1 = np.concatenate([[0], np.cumsum(c1)]).astype(np.int32); ptr2 = np.concatenate([[0], np.cumsum(c2)]).astype(np.int32)
    # feature numbers: a random permutation, ascending inside a node (as DBoW2 fills a node's list)
    idx1 = rng.permutation(n1).astype(np.int32); idx2 = rng.permutation(n2).astype(np.int32)
    for nd in range(nnodes):
        idx1[ptr1[nd]:ptr1[nd + 1]].sort(); idx2[ptr2[nd]:ptr2[nd + 1]].sort()
    kp2 = np.zeros(n2, KP_DTYPE)
    kp2["x"] = rng.uniform(20, 620, n2); kp2["y"] = rng.uniform(20, 460, n2); kp2["octave"] = rng.integers(0, 4, n2); kp2["angle"] = rng.uniform(0, 360, n2); kp2["size"] = 31
    d2 = rand_desc(rng, n2)
    Hinv = np.linalg.inv(_tri_motion()[0])
    kp1 = np.zeros(n1, KP_DTYPE); d1 = np.zeros((n1, 32), np.uint8)
    node_of_2 = np.zeros(n2, np.int32)
    srcs = np.zeros(n1, np.int64)
    for nd in range(nnodes):
        node_of_2[idx2[ptr2[nd]:ptr2[nd + 1]]] = nd
        srcs[idx1[ptr1[nd]:ptr1[nd + 1]]] = idx2[ptr2[nd] + rng.integers(0, c2[nd], c1[nd])]
    p2 = np.stack([kp2["x"][srcs], kp2["y"][srcs], np.ones(n1)], axis=0).astype(np.float64)
    p1 = Hinv @ p2
    kp1["x"] = p1[0] / p1[2] + rng.normal(0, 0.3, n1); kp1["y"] = p1[1] / p1[2] + rng.normal(0, 0.3, n1)
    kp1["octave"] = kp2["octave"][srcs]; kp1["angle"] = (kp2["angle"][srcs] + rng.normal(0, 8, n1)) % 360; kp1["size"] = 31
    d1 = flip_bits(rng, d2[srcs], 40)
    return dict(kp1=kp1, d1=d1, kp2=kp2, d2=d2, ptr1=ptr1, ptr2=ptr2, idx1=idx1, idx2=idx2, node_of_2=node_of_2)


# ---- C. line matcher
LINE_BATCH_COUNTS = [(0, 5), (5, 0), (5, 1), (1, 2), (2, 2), (3, 7), (4, 4), (5, 9), (255, 300), (256, 256), (257, 100), (511, 512), (513, 40),
                     (1023, 1024), (1024, 1100), (1025, 1100), (1100, 3)]


def line_descriptors(rng, n1, n2, style):
    """(query, train) LBD-like descriptors.  style 0: queries are noisy copies of train rows (up to 59 flipped bits), 40 % of them
    replaced by unrelated rows; 1: both sides drawn
    from four distinct rows (heavy ties in both medians, zero gaps); 2: independent random rows"""
    if style == 1:
        four = rand_desc(rng, 4)
        return four[rng.integers(0, 4, n1)].copy(), four[rng.integers(0, 4, n2)].copy()
    t = rand_desc(rng, n2)
    if style == 0 and n1 and n2:
        q = flip_bits(rng, t[rng.integers(0, n2, n1)], 60)
        stray = rng.random(n1) < 0.4                              # no counterpart: gaps near 0 next to the copies' large ones, so the MAD gate separates and 0.5 / 0.1 differ
        q[stray] = rand_desc(rng, int(stray.sum()))
        return q, t
    return rand_desc(rng, n1), t


def line_batch_case(rng, cap=1100):
    """-> (l1[P, cap, 32], l2[P, cap, 32], n1[P], n2[P]); rows past a pair's counts hold junk"""
    P = len(LINE_BATCH_COUNTS)
    l1 = rand_desc(rng, P * cap).reshape(P, cap, 32); l2 = rand_desc(rng, P * cap).reshape(P, cap, 32)
    for p, (a, b) in enumerate(LINE_BATCH_COUNTS):
        qd, td = line_descriptors(rng, a, b, p % 3)
        l1[p, :a] = qd; l2[p, :b] = td
    return l1, l2, np.array([a for a, _ in LINE_BATCH_COUNTS], np.int32), np.array([b for _, b in LINE_BATCH_COUNTS], np.int32)


# ---- D. SearchForInitialization
def sfi_pair(rng, n1, n2, lvl0):
    """One frame pair in the style of test_search_for_initialization_contention: F1 keypoints are jittered copies of F2 keypoints with
    flipped descriptor bits, half of them in runs of four that want the same F2 keypoint.  lvl0 = share of level-0 keypoints (only
    those take part); an F1 keypoint has the level of the F2 keypoint it copies.  -> (kp1, d1, kp2, d2)"""
    kp2 = np.zeros(n2, KP_DTYPE); kp1 = np.zeros(n1, KP_DTYPE)
    d2 = rand_desc(rng, n2)
    if n2 == 0 or n1 == 0:
        return kp1, rand_desc(rng, n1), kp2, d2
    kp2["x"] = rng.uniform(5, 635, n2); kp2["y"] = rng.uniform(5, 475, n2)
    kp2["octave"] = (rng.random(n2) >= lvl0).astype(np.int32) * rng.integers(1, 8, n2); kp2["angle"] = rng.uniform(0, 360, n2); kp2["size"] = 31
    src = rng.integers(0, n2, n1)
    runs = n1 // 2
    src[:runs] = np.repeat(rng.integers(0, n2, (runs + 3) // 4), 4)[:runs]      # contended runs first, scattered keypoints behind
    kp1["x"] = kp2["x"][src] + rng.uniform(-3, 3, n1); kp1["y"] = kp2["y"][src] + rng.uniform(-3, 3, n1)
    kp1["octave"] = kp2["octave"][src]; kp1["angle"] = (kp2["angle"][src] + rng.normal(0, 8, n1)) % 360; kp1["size"] = 31
    d1 = flip_bits(rng, d2[src], 25)
    return kp1, d1, kp2, d2
