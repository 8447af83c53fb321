"""Candidate lists for the ORB tail (k_octree, k_describe: csrc/orb.hip) -- what tests/test_orb_tail_gpu.py injects through sslam_testing_orb_tail and
tests/test_orb_tail_cases_cpu.py checks, from the oracle's trace alone, to reach what each case is named after.  Everything is seeded.  A candidate is x, y, score with
x, y relative to the level's minBorder (16), a list is in arrival order, and no two candidates of a list are closer than Chebyshev distance 2 (what 3x3 NMS allows).
An octree case is one level (nlevels = 1, so N == nfeatures); where a case depends on N, the generator scans N on the CPU and the CPU test asserts the outcome."""
import functools
import numpy as np
from synth import synth_frame, noise_frame

MINB = 16                # csrc/orb.hip: minBorder; a level's detection range is W x H = (w - 32) x (h - 32)
PR = 21                  # k_describe's patch radius
SPLIT_ONE_PASS = 64      # k_octree divides a node of up to 64 candidates in one pass

IMAGES = {
    "noise160": (160, 120, lambda: noise_frame(21, w=160, h=120)),
    "synth160": (160, 120, lambda: synth_frame(22, w=160, h=120)),
    "noise199": (199, 151, lambda: noise_frame(23, w=199, h=151)),
    "synth199": (199, 151, lambda: synth_frame(24, w=199, h=151)),
    "noise192": (192, 144, lambda: noise_frame(25, w=192, h=144)),          # width == pitch
    "noise400": (400, 100, lambda: noise_frame(26, w=400, h=100)),          # five root strips, hX = 73.6
}


@functools.lru_cache(maxsize=None)
def image(name):
    img = IMAGES[name][2]()
    assert img.shape == (IMAGES[name][1], IMAGES[name][0]) and img.dtype == np.uint8
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------------------------------------------------------- level geometry (build_plan, csrc/orb.hip)
def _round_half_away(v):
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


@functools.lru_cache(maxsize=None)
def levels(w, h, nlevels, scale=1.2):
    """the pyramid levels as build_plan lays them out: dicts of w, h, pitch, W, H, cells [(x0, y0, x1, y1)], cand_cap, nIni, hX"""
    out = []
    s = np.float32(1.0)
    for l in range(nlevels):
        if l: s = np.float32(np.float64(s) * np.float64(np.float32(scale)))
        inv = np.float32(1.0) / s
        lw, lh = int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))
        max_bx, max_by = lw - 19 + 3, lh - 19 + 3
        W, H = max_bx - MINB, max_by - MINB
        cells = []
        ncols, nrows = int(np.float32(W) / np.float32(30)), int(np.float32(H) / np.float32(30))
        if ncols > 0 and nrows > 0:
            wc, hc = int(np.ceil(np.float32(W) / ncols)), int(np.ceil(np.float32(H) / nrows))
            for i in range(nrows):
                iy = MINB + i * hc
                if iy >= max_by - 3: continue
                my = min(iy + hc + 6, max_by)
                for j in range(ncols):
                    ix = MINB + j * wc
                    if ix >= max_bx - 6: continue
                    mx = min(ix + wc + 6, max_bx)
                    c = (ix + 3, iy + 3, mx - 3, my - 3)
                    if c[2] > c[0] and c[3] > c[1]: cells.append(c)
        cap = sum(((c[2] - c[0] + 1) // 2) * ((c[3] - c[1] + 1) // 2) for c in cells)
        nini = _round_half_away(np.float32(W) / np.float32(H)) if W > 0 and H > 0 and cells else 0
        out.append(dict(w=lw, h=lh, pitch=(lw + 63) & ~63, W=W, H=H, cells=tuple(cells), cand_cap=cap, nIni=nini, hX=float(np.float32(W) / np.float32(nini)) if nini else 0.0, scale=float(s)))
    return tuple(out)


def quotas(oracle, nfeatures, nlevels):
    return [int(v) for v in oracle.orb_params(nfeatures, 1.2, nlevels)[1]]


def interior(kx, ky, L):
    """k_describe's choice of the aligned staging path, restated from its condition"""
    ax = (kx - PR) & ~3
    return kx - PR >= 0 and ky - PR >= 0 and ky + PR < L["h"] and kx + PR < L["w"] and ax + 48 <= L["pitch"]


def fails_only_pitch(kx, ky, L):
    return kx - PR >= 0 and ky - PR >= 0 and ky + PR < L["h"] and kx + PR < L["w"] and ((kx - PR) & ~3) + 48 > L["pitch"]


def delta(kx):
    return ((kx - PR) & 3) - 2


# ---------------------------------------------------------------------------------------------------------------- list builders
def check_spacing(cand, W, H):
    """inside the level, scores 1..255, Chebyshev distance >= 2 between any two"""
    c = np.asarray(cand, np.int64).reshape(-1, 3)
    assert ((c[:, 0] >= 0) & (c[:, 0] < W) & (c[:, 1] >= 0) & (c[:, 1] < H) & (c[:, 2] >= 1) & (c[:, 2] <= 255)).all()
    occ = np.zeros((H + 2, W + 2), np.int32)
    for dy in (0, 1):          # 2 x 2 stamps overlap exactly when two candidates are closer than distance 2
        for dx in (0, 1):
            np.add.at(occ, (c[:, 1] + dy, c[:, 0] + dx), 1)
    assert occ.max(initial=0) <= 1, "two candidates closer than Chebyshev distance 2"
    return True


def scatter(seed, W, H, n, lo=1, hi=255):
    """n random positions at Chebyshev distance >= 2, scores uniform in [lo, hi], in the order they were drawn"""
    rng = np.random.Generator(np.random.PCG64(seed))
    occ = np.zeros((H + 2, W + 2), bool)
    out = []
    while len(out) < n:
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        if occ[y:y + 3, x:x + 3].any(): continue
        occ[y + 1, x + 1] = True
        out.append((x, y, int(rng.integers(lo, hi + 1))))
    return np.array(out, np.int32).reshape(-1, 3)


def lattice(W, H):
    """every second pixel of every second row of the range FAST reaches (3 pixels inside the detection range): raster order"""
    ys, xs = np.meshgrid(np.arange(3, H - 3, 2), np.arange(3, W - 3, 2), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size, np.int64)], axis=1).astype(np.int32)


def with_scores(cand, seed, lo=1, hi=255):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.array(cand, np.int32); c[:, 2] = rng.integers(lo, hi + 1, len(c))
    return c


def raster(cand, cell=30):
    """cell-raster-like arrival: cells of 30 x 30 in row-major order, raster order inside a cell -- the order k_fast_cells' cells give"""
    c = np.asarray(cand, np.int32)
    return c[np.lexsort((c[:, 0], c[:, 1], c[:, 0] // cell, c[:, 1] // cell))]


def shuffled(cand, seed):
    c = np.asarray(cand, np.int32)
    return c[np.random.Generator(np.random.PCG64(seed)).permutation(len(c))]


def _halves(n, depth):
    """the box boundaries k_octree / DivideNode reach after `depth` halvings of [0, n): half = ceil(extent / 2)"""
    b = [(0, n)]
    for _ in range(depth):
        nb = []
        for a, e in b:
            m = a + (e - a + 1) // 2
            nb += [(a, m), (m, e)]
        b = nb
    return b


CLUSTER = ((2, 0), (4, 0), (2, 2), (4, 2))       # a cluster of 1..4 candidates inside its box: in the 8-wide depth-4 boxes of a 128 x 88 level the next halving (at x0 + 4) parts its columns


def clusters(seed, W, H, sizes, depth=4, lo=1, hi=255):
    """one cluster of sizes[i] candidates in each of len(sizes) distinct depth-`depth` boxes (seeded choice), a list in box-raster order: at that depth the quadtree holds exactly one
    node per cluster, and the nodes of more than one candidate are the clusters of size > 1"""
    rng = np.random.Generator(np.random.PCG64(seed))
    bx, by = _halves(W, depth), _halves(H, depth)
    assert all(e - a >= 5 for a, e in bx) and all(e - a >= (4 if max(sizes) > 2 else 3) for a, e in by) and len(sizes) <= len(bx) * len(by)
    pick = np.sort(rng.permutation(len(bx) * len(by))[:len(sizes)])
    sz = rng.permutation(np.asarray(sizes))
    out = []
    for p, n in zip(pick, sz):
        x0, y0 = bx[p % len(bx)][0], by[p // len(bx)][0]
        out += [(x0 + dx, y0 + dy, int(rng.integers(lo, hi + 1))) for dx, dy in CLUSTER[:n]]
    return np.array(out, np.int32).reshape(-1, 3)


def find_n(oracle, cand, W, H, pred, candidates=None):
    """the first N (scanned on the CPU) for which the oracle's trace satisfies pred(trace, N)"""
    for N in (candidates if candidates is not None else range(2, len(cand) + 3)):
        if pred(oracle.distribute_octtree(cand, W, H, N)[1], N): return N
    raise AssertionError("no N reaches the outcome")


def _case(name, img, N, cand):
    w, h = IMAGES[img][:2]
    L = levels(w, h, 1)[0]
    cand = np.ascontiguousarray(cand, np.int32).reshape(-1, 3)
    assert check_spacing(cand, L["W"], L["H"]) and len(cand) <= L["cand_cap"], name
    return dict(name=name, img=img, N=int(N), cand=cand, W=L["W"], H=L["H"])


# ---------------------------------------------------------------------------------------------------------------- octree cases
SORT_TARGETS = (1, 2, 63, 64, 65, 128, 129)
NODE_SIZES = (64, 65, 128, 129)
STRIP_EDGES = (73, 147, 220, 294)        # (int)(hX * r), r = 1..4, of the 400 x 100 level (hX = 73.6, W = 368)


@functools.lru_cache(maxsize=None)
def octree_cases(oracle):
    """name -> case (dict: img, N, cand, W, H); the CPU test states what each must reach"""
    import oracle_lib as ol
    C = {}
    W, H = 128, 88          # noise160 / synth160

    def add(name, img, N, cand): C[name] = _case(name, img, N, cand)

    # ---- ends
    pts = scatter(101, W, H, 400)
    for k in (0, 1, 2):
        N = find_n(oracle, pts, W, H, lambda t, N, k=k: t["end"] == ol.END_SECOND_BREAK and t["final_nodes"] == N + k, range(8, 400))
        add("end_break_N+%d" % k, "noise160", N, pts)
    add("end_round_without_break", "noise160", find_n(oracle, pts, W, H, lambda t, N: t["rounds2_no_break"] >= 1, range(8, 400)), pts)
    add("end_first_phase_N", "synth160", 3, pts)
    add("end_first_phase_no_growth", "synth160", 200, scatter(102, W, H, 50))
    add("end_N0", "noise160", 0, pts)
    add("end_N1", "noise160", 1, pts)
    add("end_N1_one_candidate", "noise160", 1, pts[:1])
    # ---- sort sizes: K clusters of two among single candidates give a first sorted list of exactly K entries; the triple leaves a list of one for the next round,
    # the quadruple a list of two
    for K in (63, 64, 65, 128, 129):
        c = clusters(200 + K, W, H, [2] * K + [1] * 40)
        add("sort_%d" % K, "noise160", find_n(oracle, c, W, H, lambda t, N, K=K: K in t["sorted"]), c)
    c = clusters(210, W, H, [2] * 30 + [3] + [1] * 30)
    add("sort_1", "noise160", find_n(oracle, c, W, H, lambda t, N: 1 in t["sorted"]), c)
    c = clusters(211, W, H, [2] * 30 + [4] + [1] * 30)
    add("sort_2", "noise160", find_n(oracle, c, W, H, lambda t, N: 2 in t["sorted"]), c)
    W9, H9 = 167, 119       # noise199
    c = clusters(212, W9, H9, [2] * 300 + [1] * 100, depth=5)
    add("sort_300", "noise199", find_n(oracle, c, W9, H9, lambda t, N: max(t["sorted"], default=0) > 256), c)
    # ---- ties: every sorted entry of one size (the clusters of two), all responses equal, the maximal response twice in a node; each in two arrival orders
    c = clusters(220, W, H, [2] * 100 + [1] * 20)
    N = find_n(oracle, c, W, H, lambda t, N: t["max_all_equal"] >= 100 and t["end"] == ol.END_SECOND_BREAK)
    add("tie_sizes_raster", "noise160", N, raster(c)); add("tie_sizes_shuffled", "noise160", N, shuffled(c, 221))
    c = scatter(222, W, H, 500, lo=77, hi=77)
    add("tie_all_responses_raster", "synth160", 150, raster(c)); add("tie_all_responses_shuffled", "synth160", 150, shuffled(c, 223))
    c = scatter(224, W, H, 600, lo=1, hi=3)
    add("tie_max_twice_raster", "noise160", 120, raster(c)); add("tie_max_twice_shuffled", "noise160", 120, shuffled(c, 225))
    # ---- node sizes: the root holds exactly n candidates; a division of more than 64 that leaves classes empty; the dense lattice
    for n in NODE_SIZES:
        add("node_%d" % n, "synth160", n // 2, scatter(230 + n, W, H, n))
    left = scatter(240, W // 2 - 2, H, 150)          # everything left of the root's middle: classes UR and BR stay empty in a chunked division
    add("node_chunked_empty_class", "noise160", 60, left)
    add("node_dense_lattice", "noise160", 1000, with_scores(lattice(W, H), 241))
    add("node_dense_lattice_199", "synth199", 777, shuffled(with_scores(lattice(W9, H9), 242), 243))
    # ---- roots: five strips
    Ws, Hs = 368, 68
    edge = [(x, y, 1 + (7 * i + 3 * j) % 255) for i, e in enumerate((0,) + STRIP_EDGES + (Ws,)) for j, (x, y) in enumerate(((e - 2, 10 + 4 * i), (e, 20 + 4 * i), (e + 2, 30 + 4 * i))) if 0 <= x < Ws]
    fill = [tuple(p) for p in scatter(250, Ws, Hs, 300) if all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 2 for q in edge)]
    add("roots_strip_edges", "noise400", 150, np.array(edge + fill, np.int32))
    add("roots_strip_edges_only", "noise400", 40, np.array(edge, np.int32))

    def strips(seed, counts):          # counts[r] candidates in strip r, strictly inside it
        out = []
        for r, n in enumerate(counts):
            a = (0,) + STRIP_EDGES + (Ws,)
            s = scatter(seed + r, a[r + 1] - a[r] - 4, Hs, n)
            s[:, 0] += a[r] + 2
            out.append(s)
        return np.concatenate(out)
    add("roots_empty_first_middle_last", "noise400", 60, strips(260, (0, 1, 0, 100, 0)))
    add("roots_one_and_many", "noise400", 200, shuffled(strips(270, (90, 1, 70, 0, 130)), 271))
    add("roots_N_below_strips", "noise400", 3, strips(280, (20, 20, 20, 20, 20)))
    return C


# ---------------------------------------------------------------------------------------------------------------- multi-level lists
def _level_scatter(seed, Ls, frac, lo=1, hi=255):
    return [scatter(seed + 17 * l, L["W"], L["H"], int(frac * L["cand_cap"]), lo, hi) if L["cand_cap"] else np.zeros((0, 3), np.int32) for l, L in enumerate(Ls)]


BATCH_FRAMES, BATCH_LEVELS, BATCH_NFEAT = 73, 3, 150


@functools.lru_cache(maxsize=None)
def batch_case():
    """73 frames x 3 levels on 160 x 120: every (frame, level) list different, some empty (frame 0 all empty, an empty level between full ones in every 5th frame)"""
    Ls = levels(160, 120, BATCH_LEVELS)
    rng = np.random.Generator(np.random.PCG64(300))
    cands = []
    for f in range(BATCH_FRAMES):
        per = []
        for l, L in enumerate(Ls):
            n = int(rng.integers(1, 500))
            if f == 0 or (f % 5 == 1 and l == 1) or (f % 7 == 2 and l == 2) or (f % 11 == 3 and l == 0): n = 0
            per.append(scatter(1000 + 10 * f + l, L["W"], L["H"], n))
        cands.append(per)
    images = np.stack([noise_frame(400 + f, w=160, h=120) for f in range(BATCH_FRAMES)])
    return dict(images=images, cands=cands, nfeatures=BATCH_NFEAT, nlevels=BATCH_LEVELS, cap=BATCH_NFEAT + 40)


BORDER = 12
BORDER_PHASES = 4          # x % 4, y % 4: sixteen frames, each a lattice of spacing 4
BORDER_NFEAT = 1500


@functools.lru_cache(maxsize=None)
def border_case(img):
    """every position within 12 pixels of a border of the detection range, on each of 3 levels, dealt over 16 frames by (x % 4, y % 4); distinct responses; the level
    quotas exceed the counts, so every candidate survives"""
    w, h = IMAGES[img][:2]
    Ls = levels(w, h, 3)
    cands = []
    for ph in range(BORDER_PHASES * BORDER_PHASES):
        px, py = ph % BORDER_PHASES, ph // BORDER_PHASES
        per = []
        for L in Ls:
            ys, xs = np.meshgrid(np.arange(py, L["H"], BORDER_PHASES), np.arange(px, L["W"], BORDER_PHASES), indexing="ij")
            xs, ys = xs.ravel(), ys.ravel()
            m = (xs < BORDER) | (xs >= L["W"] - BORDER) | (ys < BORDER) | (ys >= L["H"] - BORDER)
            xs, ys = xs[m], ys[m]
            per.append(np.stack([xs, ys, 1 + (np.arange(len(xs)) * 37 + 11 * ph) % 255], axis=1).astype(np.int32))
        cands.append(per)
    images = np.stack([image(img)] * len(cands))
    return dict(images=images, cands=cands, nfeatures=BORDER_NFEAT, nlevels=3, cap=BORDER_NFEAT + 40)


RAMPS = ("const", "+x", "-x", "+y", "-y", "+x+y", "-x-y", "+x-y", "-x+y")


@functools.lru_cache(maxsize=None)
def moments_case():
    """a constant image and the eight exact ramps (160 x 120, one level): IC_Angle's moments are zero, on an axis or on a diagonal"""
    h, w = 120, 160
    y, x = np.mgrid[0:h, 0:w]
    ry = h - 1 - y
    imgs = [np.full((h, w), 128), x, 255 - x, y, 255 - y, (x + y) // 2, 255 - (x + y) // 2, (x + ry) // 2, 255 - (x + ry) // 2]
    images = np.stack(imgs).astype(np.uint8)
    L = levels(w, h, 1)[0]
    c = scatter(500, L["W"], L["H"], 60)
    c[0, 2], c[1, 2] = 1, 255                     # the extreme scores
    c[2:, 2] = 2 + np.arange(len(c) - 2) * 4      # distinct
    return dict(images=images, cands=[[c]] * len(imgs), nfeatures=100, nlevels=1, cap=140)


@functools.lru_cache(maxsize=None)
def cap_case():
    """one frame, 3 levels (199 x 151 synthetic), lists of which everything survives; the caps are set from the level counts by the tests"""
    Ls = levels(199, 151, 3)
    cands = [scatter(600 + l, L["W"], L["H"], 40 + 10 * l) for l, L in enumerate(Ls)]
    for l, c in enumerate(cands): c[:, 2] = 1 + (np.arange(len(c)) * 5 + l) % 255
    cands[0][0, 2], cands[0][1, 2] = 1, 255
    return dict(images=image("synth199")[None], cands=[cands], nfeatures=400, nlevels=3)


BIG_N = 2000


@functools.lru_cache(maxsize=None)
def big_lds_case():
    """N = 2000 on one level with more than 4000 candidates: k_octree's dynamic LDS passes 64 KB.  199 x 151 holds 4617 candidates"""
    L = levels(199, 151, 1)[0]
    c = shuffled(with_scores(lattice(L["W"], L["H"]), 700), 701)[:4200]
    return _case("big_lds", "noise199", BIG_N, c)


def octree_lds_bytes(nfeat_per_level, Ls):
    """the dynamic LDS of the k_octree launch, restated: 16 * NCp2 + 4 * (maxCellsLevel + 1) + 20 * NC with NC = the largest level's node capacity + 4"""
    nc = max(max(n + 3, 4 * max(L["nIni"], 1) + 1) for n, L in zip(nfeat_per_level, Ls)) + 4
    p2 = 1
    while p2 < nc: p2 <<= 1
    return 16 * p2 + 4 * (max(len(L["cells"]) for L in Ls) + 1) + 20 * nc, nc


def pack(cands, nlevels):
    """per-frame, per-level lists -> (cand[nframes][nlevels][nmax][3], ncand[nframes][nlevels])"""
    nmax = max(1, max(len(c) for per in cands for c in per))
    cand = np.zeros((len(cands), nlevels, nmax, 3), np.int32); nc = np.zeros((len(cands), nlevels), np.int32)
    for f, per in enumerate(cands):
        assert len(per) == nlevels
        for l, c in enumerate(per):
            cand[f, l, :len(c)] = c; nc[f, l] = len(c)
    return cand, nc
