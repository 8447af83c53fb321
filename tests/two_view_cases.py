"""Inputs of the two-view RANSAC tests (tests/test_two_view_gpu.py, tests/test_two_view_cases_cpu.py): frame pairs for sslam_two_view_ransac, each a dict(name, kp1, kp2
(float32 [n, 2]: the undistorted pt.x, pt.y), m12 (int32 [n1]), sets (None: the library draws; or int32 [iterations, 8]), iterations, sigma, seed).  Every expectation of
the two test files is tests/two_view_sim.py's: csrc/two_view_math.h on the host.  That each case reaches what its name says is shown in test_two_view_cases_cpu.py.
The cases that sit on a float boundary (gates, order) are found by search with the sim itself, once per process.  Every generator is a pure function of its seed."""
import functools
import numpy as np
import two_view_ref as ref
import two_view_sim as sim

f32 = np.float32
W, H = 640.0, 480.0
H_TRUE = np.array([[1.02, 0.03, 5.0], [-0.02, 0.98, -3.0], [1e-5, -2e-5, 1.0]])
K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])


def planar(p1):
    x = np.c_[p1, np.ones(len(p1))] @ H_TRUE.T
    return x[:, :2] / x[:, 2:]


def two_layer(p1, rng):
    """points at depths 4 and 9 seen from a second camera that moved sideways and turned: no homography explains both layers"""
    d = np.where(rng.random(len(p1)) < 0.5, 4.0, 9.0)
    X = (np.c_[p1, np.ones(len(p1))] @ np.linalg.inv(K).T) * d[:, None]
    a = np.deg2rad(2.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    x = (X @ R.T + np.array([0.6, 0.05, 0.1])) @ K.T
    return x[:, :2] / x[:, 2:]


def make(name, seed, n1, n2, nm, scene="planar", noise=0.3, outliers=0.0, iterations=8, sigma=1.0, sets=None, holes="spread", descending=False):
    """n1 / n2 keypoints, nm of frame 1's matched to distinct keypoints of frame 2 that sit where `scene` puts them (+ noise, a fraction `outliers` anywhere).
    holes: where the unmatched rows of frame 1 are -- "spread", "ends" (first and last row unmatched) or "middle" (first and last row matched)"""
    rng = np.random.default_rng(seed)
    assert nm <= n1 and nm <= n2
    kp1 = rng.uniform([20, 20], [W - 20, H - 20], (n1, 2))
    kp2 = rng.uniform([20, 20], [W - 20, H - 20], (n2, 2))
    if holes == "ends":
        assert nm <= n1 - 2
        rows1 = 1 + np.sort(rng.permutation(n1 - 2)[:nm])
    elif holes == "middle":
        assert 2 <= nm
        rows1 = np.r_[0, 1 + np.sort(rng.permutation(n1 - 2)[:nm - 2]), n1 - 1] if n1 > 2 else np.arange(nm)
    else:
        rows1 = np.sort(rng.permutation(n1)[:nm])
    rows2 = rng.permutation(n2)[:nm]
    if descending:
        rows2 = np.sort(rows2)[::-1]
    if nm:
        moved = {"planar": lambda p: planar(p), "two_layer": lambda p: two_layer(p, rng), "random": lambda p: rng.uniform([20, 20], [W - 20, H - 20], p.shape)}[scene](kp1[rows1])
        moved = moved + rng.normal(0, noise, moved.shape)
        out = rng.random(nm) < outliers
        moved[out] = rng.uniform([20, 20], [W - 20, H - 20], (int(out.sum()), 2))
        kp2[rows2] = moved
    m12 = np.full(n1, -1, np.int32)
    m12[rows1] = rows2
    return dict(name=name, kp1=kp1.astype(f32), kp2=kp2.astype(f32), m12=m12, sets=None if sets is None else np.asarray(sets, np.int32), iterations=iterations,
                sigma=float(sigma), seed=seed & 0xFFFF)


def drawn_sets(rng, iterations, nm):
    return np.stack([rng.permutation(nm)[:8] for _ in range(iterations)]).astype(np.int32)


def nmatches(c):
    return int(((c["m12"] >= 0) & (c["m12"] < len(c["kp2"]))).sum())


# ---- sizes
def count_cases():
    """match counts 0, 7 (skipped), 8 (every set a permutation), 9, 63 / 64 / 65, 255 / 256 / 257; n1 != n2, holes at the first and last row or not, descending keypoint-2
    indices; nmatches == n1 == n2 (what the single call makes its capacity)"""
    out = []
    for k, nm in enumerate((0, 7, 8, 9, 63, 64, 65, 255, 256, 257)):
        out.append(make("count_%d" % nm, 100 + k, nm + 2 + k % 3, nm + 6 + k % 2, nm, iterations=4 if nm > 200 else 8, holes=("ends", "spread", "middle")[k % 3] if nm >= 2 else "spread",
                        descending=k % 2 == 1))
    out.append(make("count_full_64", 120, 64, 64, 64, iterations=8))
    out.append(make("count_0_of_0", 121, 0, 5, 0, iterations=3))
    out.append(make("count_no_frame2", 122, 9, 0, 0, iterations=3))
    return out


def iteration_cases():
    """1, 63 / 64 / 65 (one lane per iteration), 200 (the reference's count), 257 (lanes take more than one); the library draws the sets"""
    return [make("iterations_%d" % it, 200 + k, 50, 47, 40, iterations=it, outliers=0.2) for k, it in enumerate((1, 63, 64, 65, 200, 257))]


def sigma_cases():
    return [make("sigma_%s" % str(s).replace(".", "_"), 300, 90, 90, 80, noise=0.8, iterations=16, sigma=s, outliers=0.1) for s in (1.0, 2.5)]


def scene_cases():
    """a plane (model 1) and two depth layers (model 2), 200 drawn iterations each"""
    return [make("scene_planar", 400, 140, 150, 120, "planar", iterations=200, outliers=0.1), make("scene_two_layer", 401, 140, 150, 120, "two_layer", iterations=200, outliers=0.1)]


def seed_cases():
    """the library's own draw, three seeds"""
    return [dict(make("seeds_%d" % s, 500, 70, 66, 60, iterations=32, outliers=0.2), seed=s) for s in (0, 1, 0xDEADBEEF)]


# ---- selection
def tie_case():
    """the same set at iterations 3 and 7, all inliers of the plane; every other set holds four random correspondences: the two share the best score and 3 wins"""
    c = make("tie_3_7", 600, 60, 60, 48, iterations=10, noise=0.05)
    rng = np.random.default_rng(601)
    rows, idx = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
    bad = rng.permutation(len(rows))[:16]                       # these matches become outliers
    for r in bad:
        c["kp2"][c["m12"][idx[r]]] = rng.uniform([20, 20], [W - 20, H - 20], 2).astype(f32)
    good = np.setdiff1d(np.arange(len(rows)), bad)
    sets = np.stack([np.r_[rng.permutation(bad)[:4], rng.permutation(good)[:4]] for _ in range(10)])
    sets[3] = sets[7] = rng.permutation(good)[:8]
    c["sets"] = sets.astype(np.int32)
    return c


def no_winner_case():
    """random correspondences under a sigma so small that no term is ever added: both scores stay 0, best_it -1, zero matrices"""
    return make("no_winner", 700, 40, 40, 30, "random", iterations=12, sigma=1e-7)


def invalid_set_case():
    """injected sets with an index of -1, nmatches and a large one: those iterations score 0 and cannot win"""
    c = make("invalid_sets", 710, 40, 42, 30, iterations=6)
    sets = drawn_sets(np.random.default_rng(711), 6, 30)
    sets[0, 2] = -1; sets[2, 7] = 30; sets[5, 0] = 1 << 30
    c["sets"] = sets
    return c


# ---- degenerate sets
DEGENERATE_SETS = ("column", "good", "twin", "slant", "column", "other")      # what iteration it of degenerate_case() holds


def degenerate_case():
    """Frame 1's keypoints sit on integer pixels whose x sum to 300 * n1, so Normalize's meanX is exactly 300.  The sets by iteration (DEGENERATE_SETS):
    column   eight matches at x = 300 in frame 1: eight collinear points whose normalised u1 is exactly 0.  Columns 0, 3 and 6 of A vanish, the null vector is e0, Hn has one
             non-zero element, H21i two zero rows: its determinant is exactly 0, H12i the zero matrix, w2in1inv = 1 / 0 and the score NaN
    good     eight inliers of the plane
    twin     a set with two matches at one pixel in both frames (ORB does put keypoints of two octaves on one pixel)
    slant    eight collinear points on a slanted line
    other    another set of inliers"""
    n = 60
    rng = np.random.default_rng(801)
    c = make("degenerate", 800, n, n, 50, iterations=len(DEGENERATE_SETS), noise=0.05)
    kp1 = np.round(c["kp1"].astype(np.float64))
    rows, idx = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
    order = rng.permutation(len(rows))
    column, twin, slant, good, other = order[:8], order[8:16], order[16:24], order[24:32], order[32:40]
    for k, r in enumerate(column):
        kp1[idx[r]] = (300, 40 + 50 * k)
    for k, r in enumerate(slant):
        kp1[idx[r]] = (50 + 60 * k, 40 + 45 * k)
    kp1[idx[twin[1]]] = kp1[idx[twin[0]]]
    free = np.setdiff1d(np.arange(n), np.r_[idx[column], idx[slant], idx[twin[:2]]])
    d = int(300 * n - kp1[:, 0].sum())                 # spread what is missing over the other keypoints, a pixel at a time
    for k in range(abs(d)):
        kp1[free[k % len(free)], 0] += np.sign(d)
    assert kp1[:, 0].sum() == 300 * n and kp1[:, 0].min() >= 0
    kp2 = c["kp2"].astype(np.float64)
    moved = planar(kp1[idx]) + rng.normal(0, 0.05, (len(idx), 2))
    kp2[c["m12"][idx]] = moved
    kp2[c["m12"][idx[twin[1]]]] = kp2[c["m12"][idx[twin[0]]]]
    c["kp1"], c["kp2"] = kp1.astype(f32), kp2.astype(f32)
    sets = dict(column=column, good=good, twin=twin, slant=slant, other=np.r_[other[:4], good[:4]])
    c["sets"] = np.stack([sets[k] for k in DEGENERATE_SETS]).astype(np.int32)
    return c


# ---- gates: a match whose chi-square sits at the threshold of CheckHomography / CheckFundamental
GATES = (("h", 0), ("h", 1), ("f", 0), ("f", 1))


def _gate_base(seed, swap):
    """swap: frame 2 of the generator becomes frame 1.  Along y the plane's image is a little smaller in the generator's frame 2 (H_TRUE: 0.98), so of a match's two transfer
    errors the one measured in frame 1 is the larger and its term crosses the threshold first; swapped, the term measured in frame 2 does"""
    c = make("gate", seed, 30, 30, 24, iterations=1, noise=0.05)
    if swap:
        back = np.full(len(c["kp2"]), -1, np.int32)
        i = np.flatnonzero(c["m12"] >= 0)
        back[c["m12"][i]] = i
        c = dict(c, kp1=c["kp2"], kp2=c["kp1"], m12=back)
    c["sets"] = np.arange(8, dtype=np.int32)[None]
    return c


def _gate_chi(c, model, term, row):
    r = sim.run_plain([c])[0]
    rows, _ = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
    chi = ref.homography_terms(r["mats"][0, 1], r["mats"][0, 2], rows, c["sigma"]) if model == "h" else ref.fundamental_terms(r["mats"][0, 4], rows, c["sigma"])
    return chi[row, term]


@functools.lru_cache(maxsize=None)
def gate_cases():
    """for H and F, first-image and second-image term: three copies of one pair that differ in ONE coordinate of one match (not in the set) by one float each, the middle one
    the last float whose chi-square does not exceed the threshold.  Moving a keypoint moves Normalize's sums too, so every probe is a full run of the sim."""
    out = []
    for g, (model, term) in enumerate(GATES):
        c = _gate_base(900 + g, swap=(model, term) == ("h", 1))      # H's second term measures in frame 2; F's two cross apart as they are
        rows, idx = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
        row = 15
        th = ref.TH_H if model == "h" else ref.TH_F
        kp, at = "kp2", c["m12"][idx[row]]            # keypoint 2 moves along y

        def with_y(y):
            d = dict(c, kp1=c["kp1"].copy(), kp2=c["kp2"].copy())
            d[kp][at, 1] = y
            return d
        lo = c[kp][at, 1]                              # an inlier
        hi = f32(lo + 6)                               # six pixels off: outside every gate at sigma 1
        assert _gate_chi(with_y(lo), model, term, row) <= th < _gate_chi(with_y(hi), model, term, row)
        while np.nextafter(lo, f32(np.inf)) < hi:      # bisection over the floats between
            mid = f32((f32(lo) + f32(hi)) / 2)
            if _gate_chi(with_y(mid), model, term, row) <= th:
                lo = mid
            else:
                hi = mid
        for tag, y in (("below", np.nextafter(lo, f32(-np.inf))), ("at", lo), ("above", hi)):
            out.append(dict(with_y(y), name="gate_%s%d_%s" % (model, term + 1, tag), gate=(model, term, row, int(idx[row]))))
    return out


# ---- order: the winner depends on the order of the score's sum
def other_order_scores(c, r, model):
    """the scores of every iteration of sim result r with the same terms summed in reverse: float32 [iterations]"""
    rows, _ = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
    out = []
    for it in range(c["iterations"]):
        if model == "h":
            terms, _ = ref.score_terms(ref.homography_terms(r["mats"][it, 1], r["mats"][it, 2], rows, c["sigma"]), ref.TH_H, ref.TH_H)
        else:
            terms, _ = ref.score_terms(ref.fundamental_terms(r["mats"][it, 4], rows, c["sigma"]), ref.TH_F, ref.TH_SCORE)
        out.append(ref.sum_in_order(terms[::-1]))
    return np.array(out, f32)


@functools.lru_cache(maxsize=None)
def order_case():
    """64 iterations on a plane seen almost without noise (0.005 pixels): every set gives nearly the same homography, the scores lie a few floats apart, and the winner in
    match order is another iteration than the winner of the same terms summed in reverse.  Found by search over the seed."""
    for seed in range(1000, 1040):
        c = make("order", seed, 70, 70, 60, iterations=64, noise=0.005)
        c["sets"] = drawn_sets(np.random.default_rng(seed), 64, 60)
        r = sim.run_plain([c])[0]
        rev = other_order_scores(c, r, "h")
        if ref.select(rev)[1] != r["result"]["best_it_h"] and ref.select(rev)[0] != r["result"]["score_h"]:
            return c
    raise AssertionError("no seed gives an order-dependent winner")


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = count_cases() + iteration_cases() + sigma_cases() + scene_cases() + seed_cases() + [tie_case(), no_winner_case(), invalid_set_case(), degenerate_case()] + \
        list(gate_cases()) + [order_case()]
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


@functools.lru_cache(maxsize=None)
def expected(pairs=None):
    """the sim's answers for all_cases(), case p run as pair pairs[p] (None: pair 0 = the single call)"""
    cs = all_cases()
    return sim.run([dict(c, pair=0 if pairs is None else pairs[p]) for p, c in enumerate(cs)])


# ---- solver inputs: the A matrices of ComputeH21 / ComputeF21 (:259-286, :301-319) for one set, in float32 as the reference fills them
def system_matrices(c, set8):
    p1, _ = ref.normalize(c["kp1"]); p2, _ = ref.normalize(c["kp2"])
    _, idx = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
    AH, AF = np.zeros((16, 9), f32), np.zeros((8, 9), f32)
    for i, s in enumerate(set8):
        u1, v1 = p1[idx[s]]; u2, v2 = p2[c["m12"][idx[s]]]
        AH[2 * i] = [0, 0, 0, -u1, -v1, -1, f32(v2 * u1), f32(v2 * v1), v2]
        AH[2 * i + 1] = [u1, v1, 1, 0, 0, 0, f32(-u2 * u1), f32(-u2 * v1), -u2]
        AF[i] = [f32(u2 * u1), f32(u2 * v1), u2, f32(v2 * u1), f32(v2 * v1), v2, u1, v1, 1]
    return AH, AF


def random_systems(n=1000, seed=4242):
    """n sets on exact, noisy and random correspondences: cases of 8 .. 12 matches with ten injected sets each"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n // 10):
        nm = 8 + k % 5
        c = make("system_%d" % k, seed + k, nm + 3, nm + 2, nm, scene=("planar", "two_layer", "random")[k % 3], noise=(0.0, 0.5)[(k // 3) % 2], iterations=10)
        c["sets"] = drawn_sets(rng, 10, nm)
        out.append(c)
    return out
