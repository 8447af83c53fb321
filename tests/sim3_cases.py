"""Inputs of the Sim3Solver tests (tests/test_sim3_gpu.py, tests/test_sim3_cases_cpu.py): keyframe pairs for sslam_sim3_ransac in the format tests/sim3_sim.py states,
each a pure function of its seed.  Every expectation of the two test files is tests/sim3_sim.py's: csrc/sim3_math.h on the host.  That each case reaches what its name says
is shown in test_sim3_cases_cpu.py.  The cases that sit on a float boundary (gates) are found by search with the sim itself, once per process.  Every case is kept at the
smallest size that reaches its edge: a dozen or two correspondences unless the name says otherwise."""
import functools
import numpy as np
import sim3_ref as ref
import sim3_sim as sim

f32 = np.float32
K1 = np.array([500.0, 500.0, 320.0, 240.0], f32)
K2 = np.array([520.0, 510.0, 315.0, 245.0], f32)      # two cameras in every pair
NLEVELS = 8
SIGMA2 = np.array([1.44 ** l for l in range(NLEVELS)]).astype(f32)      # mvLevelSigma2 at scale factor 1.2


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); t = np.deg2rad(deg)
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * ax + (1 - np.cos(t)) * ax @ ax


S_TRUE, R_TRUE, T_TRUE = 1.25, rot([0.2, 1.0, 0.1], 14.0), np.array([0.4, -0.1, 0.3])      # X1 = s R X2 + t


def make(name, seed, n1, n2, nm, outliers=0.25, noise=0.002, holes="spread", min_inliers=6, max_iterations=40, calls=(40,), fix_scale=False, probability=0.99, sets=None,
         octaves=None):
    """n1 / n2 rows, nm of keyframe 1's matched to distinct rows of keyframe 2 whose map points are the same points under (S_TRUE, R_TRUE, T_TRUE) (+ noise in metres; a
    fraction `outliers` of them anywhere).  holes: where the unmatched rows of keyframe 1 are -- "spread", "ends" or "middle" (first and last row matched)."""
    rng = np.random.default_rng(seed)
    assert nm <= n1 and nm <= n2
    s_true = 1.0 if fix_scale else S_TRUE

    def cloud(n):
        return np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 8, n)]
    x1, x2 = cloud(n1), cloud(n2)
    if holes == "ends":
        rows1 = 1 + np.sort(rng.permutation(n1 - 2)[:nm])
    elif holes == "middle":
        rows1 = np.r_[0, 1 + np.sort(rng.permutation(n1 - 2)[:nm - 2]), n1 - 1]
    else:
        rows1 = np.sort(rng.permutation(n1)[:nm])
    rows2 = rng.permutation(n2)[:nm]
    moved = ((x1[rows1] - T_TRUE) @ R_TRUE) / s_true + rng.normal(0, noise, (nm, 3))      # R^T (X1 - t) / s
    out = rng.random(nm) < outliers
    moved[out] = cloud(int(out.sum()))
    x2[rows2] = moved
    m12 = np.full(n1, -1, np.int32); m12[rows1] = rows2
    oc = (lambda n: rng.integers(0, NLEVELS, n)) if octaves is None else (lambda n: np.full(n, octaves))
    kf1 = dict(oct=oc(n1).astype(np.int32), valid=np.ones(n1, np.uint8), x3dc=x1.astype(f32), K=K1)
    kf2 = dict(oct=oc(n2).astype(np.int32), valid=np.ones(n2, np.uint8), x3dc=x2.astype(f32), K=K2)
    return dict(name=name, kf1=kf1, kf2=kf2, sigma2=SIGMA2, m12=m12, fix_scale=bool(fix_scale), probability=probability, min_inliers=min_inliers, max_iterations=max_iterations,
                calls=list(calls), sets=None if sets is None else np.asarray(sets, np.int32), seed=seed & 0xFFFF, outlier=out, rows1=rows1)


def good_and_bad(c):
    """positions in the correspondence list of the matches made as inliers / as outliers (every row of make() is a correspondence unless a case filters some afterwards)"""
    return np.flatnonzero(~c["outlier"]), np.flatnonzero(c["outlier"])


def triple_sets(rng, good, bad, max_iterations, good_at=()):
    """sets whose iterations hold one outlier each (two inliers + one outlier: a hypothesis nothing agrees with) except `good_at`, which hold three inliers"""
    sets = np.stack([np.r_[rng.permutation(good)[:2], rng.permutation(bad)[:1]] for _ in range(max_iterations)])
    for it in good_at:
        sets[it] = rng.permutation(good)[:3]
    return sets.astype(np.int32)


# ---- sizes
def count_cases():
    """N = min_inliers - 1 (nothing iterated), min_inliers (one iteration that can never return), min_inliers + 1; 63 / 64 / 65 / 129 correspondences with n1 no multiple of
    64 and the unmatched rows at the ends or in the middle (min_inliers = N - 1 with outliers among them: every allowed iteration is walked)"""
    out = [make("count_min_minus_1", 10, 12, 11, 7, min_inliers=8, outliers=0.0), make("count_min", 11, 12, 13, 8, min_inliers=8, outliers=0.0),
           make("count_min_plus_1", 12, 12, 13, 9, min_inliers=8, outliers=0.0)]
    for k, n in enumerate((63, 64, 65, 129)):
        out.append(make("count_%d" % n, 20 + k, n + 3 + k, n + 5, n, holes=("ends", "middle")[k % 2], min_inliers=n - 1, max_iterations=12, calls=(12,), probability=1 - 1e-10))
    out.append(make("count_0", 29, 5, 4, 0))
    out.append(make("count_2_drawn", 28, 4, 4, 2, min_inliers=1, outliers=0.0, max_iterations=3, calls=(3,)))      # fewer than three: nothing can be drawn
    return out


FILTERED = dict(valid1=(2, 9), valid2=(5,), past_n2=(7,), negative=(11,), octave1=(13,), octave2=(14, 15))      # positions among the 20 matched rows of filter_case()


def filter_case():
    """20 matched rows of which FILTERED names those the constructor drops: valid1 = 0, valid2 = 0, m >= n2, m < -1, an octave of nlevels or -1"""
    c = make("filtered", 30, 24, 26, 20, min_inliers=5, outliers=0.0, max_iterations=10, calls=(10,))
    r1 = c["rows1"]; m = c["m12"]
    for p in FILTERED["valid1"]:
        c["kf1"]["valid"][r1[p]] = 0
    for p in FILTERED["valid2"]:
        c["kf2"]["valid"][m[r1[p]]] = 0
    m[r1[FILTERED["past_n2"][0]]] = 26
    m[r1[FILTERED["negative"][0]]] = -3
    c["kf1"]["oct"][r1[FILTERED["octave1"][0]]] = NLEVELS
    c["kf2"]["oct"][m[r1[FILTERED["octave2"][0]]]] = -1
    c["kf2"]["oct"][m[r1[FILTERED["octave2"][1]]]] = NLEVELS + 40
    return c


# ---- where iterate returns
RETURNS = (("return_at_0", 100, (0,), (100,)), ("return_at_63", 100, (63,), (100,)), ("return_at_64", 100, (64,), (100,)), ("return_at_last_below_64", 40, (39,), (40,)),
           ("return_at_last_64", 64, (63,), (64,)), ("return_at_last_above_64", 70, (69,), (70,)), ("never_below_64", 40, (), (40,)), ("never_64", 64, (), (64,)),
           ("never_above_64", 100, (), (60, 60)))


def return_cases():
    """30 correspondences, 21 made as inliers: injected sets hold an outlier each except at the named iteration.  mRansacMaxIts is max_iterations here (122 for N = 30 and
    min_inliers = 10 caps nothing below it): below, equal to and above 64"""
    out = []
    for k, (name, mi, at, calls) in enumerate(RETURNS):
        c = make(name, 40, 33, 34, 30, outliers=0.3, min_inliers=10, max_iterations=mi, calls=calls)
        good, bad = good_and_bad(c)
        c["sets"] = triple_sets(np.random.default_rng(400 + k), good, bad, mi, at)
        out.append(c)
    return out


def count_rule_cases():
    """16 correspondences, G of them exact inliers.  equal: min_inliers = G, the good sets at iterations 3 and 7 count exactly G and do not return, 7 replaces 3 as the
    best.  above: min_inliers = G - 1, the same sets, iteration 3 returns"""
    out = []
    for name, below in (("count_equal_min", 0), ("count_above_min", 1)):
        c = make(name, 50, 18, 19, 16, outliers=0.25, noise=0.0, max_iterations=10, calls=(10,), probability=1 - 1e-10)
        good, bad = good_and_bad(c)
        c["min_inliers"] = len(good) - below
        c["sets"] = triple_sets(np.random.default_rng(500), good, bad, 10, (3, 7))
        out.append(c)
    return out


def resume_cases():
    """the library's own draw on 40 correspondences: one call of 30 iterations, 30 calls of one, calls of 5 (LoopClosing's), each carried on until the solver has no more;
    min_inliers = 33 never returns (a probability of 1 - 1e-10 gives it 28 iterations), min_inliers = 12 returns and is resumed behind every return"""
    out = []
    for tag, mi, pr in (("never", 33, 1 - 1e-10), ("returns", 12, 0.99)):
        for pat, calls in (("once", [30] * 14), ("ones", [1] * 34), ("fives", [5] * 14)):
            out.append(make("resume_%s_%s" % (tag, pat), 60, 44, 45, 40, outliers=0.4, min_inliers=mi, max_iterations=30, calls=calls, probability=pr))
    return out


def parameter_cases():
    """fix_scale on and off on one geometry and three seeds of the draw (min_inliers = N - 1 with outliers: every allowed iteration is walked, none returns); LoopClosing's
    parameters (0.99, 20, 300, 5 iterations a call) on 80 correspondences; 130 drawn iterations (three rounds of the kernel) that never return"""
    out = [make("fix_scale_%d" % f, 70, 30, 30, 26, fix_scale=bool(f), min_inliers=25, max_iterations=20, calls=(20,), probability=1 - 1e-10) for f in (0, 1)]
    out += [dict(make("seed_%d" % s, 71, 30, 31, 24, min_inliers=23, max_iterations=16, calls=(16,), probability=1 - 1e-10), seed=s) for s in (0, 1, 0xDEADBEEF)]
    out.append(make("loop_closing", 72, 90, 88, 80, outliers=0.5, min_inliers=20, max_iterations=300, calls=(5, 5, 5, 5)))
    out.append(make("drawn_130", 73, 44, 43, 40, outliers=0.6, min_inliers=20, max_iterations=130, calls=(130,), probability=1 - 1e-10))
    return out


DEGENERATE_SETS = ("collinear", "good", "identity", "z0", "other")      # what iteration it of degenerate_case() holds


def degenerate_case():
    """20 exact correspondences; by iteration (DEGENERATE_SETS): three collinear points; a good set; three points that have the
    SAME coordinates in both keyframes (M is symmetric, the eigenvector is (1, 0, 0, 0) exactly, v = 0: the reference divides 0 by 0 and R12 is NaN); a set with a point at
    z = 0 in keyframe 1 (its own image point is not finite; the solve is); another good set.  Seven of the 20 are no inliers of the true transform and min_inliers is 19:
    nothing returns and every set is walked (a probability of 1 - 1e-10 allows 12 iterations)"""
    c = make("degenerate", 80, 22, 22, 20, outliers=0.0, noise=0.0, min_inliers=19, max_iterations=len(DEGENERATE_SETS), calls=(len(DEGENERATE_SETS),), probability=1 - 1e-10)
    r1, m = c["rows1"], c["m12"]
    x1, x2 = c["kf1"]["x3dc"], c["kf2"]["x3dc"]
    for k, p in enumerate((0, 1, 2)):
        x1[r1[p]] = f32([-1 + k, 0.5 * k, 4 + 0.25 * k]); x2[m[r1[p]]] = f32([k, 0, 5 + k])      # both sides on a line
    for p in (6, 7, 8):
        x2[m[r1[p]]] = x1[r1[p]]
    x1[r1[9]][2] = 0
    c["sets"] = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 12, 13], [14, 15, 16]], np.int32)
    return c


def twin_case():
    """an injected set that names one correspondence twice (two equal points: no draw of the reference gives it, d_sets may), then a good one"""
    c = make("twin_set", 81, 14, 14, 12, outliers=0.0, noise=0.0, min_inliers=11, max_iterations=2, calls=(2,), probability=1 - 1e-10)
    c["kf2"]["x3dc"][c["m12"][c["rows1"][0]]] += f32(1.0)      # one outlier: the good set counts 11 and does not return
    c["sets"] = np.array([[4, 4, 5], [1, 2, 3]], np.int32)
    return c


def invalid_set_case():
    """injected sets with an index of -1, N and a large one beside valid ones: those iterations never become the best"""
    c = make("invalid_sets", 90, 24, 25, 22, outliers=0.3, min_inliers=17, max_iterations=6, calls=(6,), probability=1 - 1e-10)
    rng = np.random.default_rng(91)
    sets = np.stack([rng.permutation(22)[:3] for _ in range(6)]).astype(np.int32)
    sets[0, 1] = -1; sets[2, 2] = 22; sets[5, 0] = 1 << 30
    c["sets"] = sets
    return c


# ---- gates: a correspondence whose error sits at the gate of CheckInliers (:356, a strict <)
GATES = (("err1", 0), ("err2", 1), ("size_t", 0))


def _gate_base(which):
    """16 exact correspondences, one injected good set, one iteration.  The probed correspondence sits at octave 1 (sigma2 = 1.44: the gate is 13) on the side whose gate
    is probed and at octave 7 on the other (gate 118: far away)"""
    c = make("gate", 95, 16, 16, 16, outliers=0.0, noise=0.0, min_inliers=16, max_iterations=1, calls=(1,), octaves=2)      # N == min_inliers: one iteration, no return
    c["sets"] = np.array([[0, 1, 2]], np.int32)
    row = 9
    c["kf1"]["oct"][c["rows1"][row]] = 1 if which == 0 else 7
    c["kf2"]["oct"][c["m12"][c["rows1"][row]]] = 7 if which == 0 else 1
    return c, row


def _gate_probe(c, row, which, y):
    """the pair with the y of the probed point in keyframe 2 set to y: (case, its error on the probed side by tests/sim3_ref.py from the sim's hypothesis, the sim's mark)"""
    d = dict(c, kf2=dict(c["kf2"], x3dc=c["kf2"]["x3dc"].copy()))
    d["kf2"]["x3dc"][c["m12"][c["rows1"][row]], 1] = y
    r = sim.run_plain([d])[0]["calls"][0]
    _, _, X1, X2, p1, p2, e1, e2 = ref.correspondences(d)
    err = ref.errors(r["mats"][0, 0], r["mats"][0, 1:10], r["mats"][0, 10:13], X1, X2, p1, p2, K1, K2)[which]
    return d, err[row], int(r["marks"][0, row])


@functools.lru_cache(maxsize=None)
def gate_cases():
    """err1 / err2: two copies of one pair that differ in ONE coordinate by one float, the error on the probed side below the gate of 13 in the first and at or above it in
    the second.  size_t: one copy whose error lies between 13 and 9.210 * 1.44 = 13.26: an outlier, because the gate is a size_t"""
    out = []
    for name, which in GATES:
        c, row = _gate_base(which)
        at = c["m12"][c["rows1"][row]]
        lo = c["kf2"]["x3dc"][at, 1]
        hi = f32(lo + 0.2)                        # some 15 pixels off
        assert _gate_probe(c, row, which, lo)[2] == 1 and _gate_probe(c, row, which, hi)[2] == 0
        if name == "size_t":
            for _ in range(60):                   # bisection on the error itself towards the middle of (13, 13.26)
                mid = f32((f32(lo) + f32(hi)) / 2)
                d, e, mark = _gate_probe(c, row, which, mid)
                if 13.05 < e < 13.2:
                    out.append(dict(d, name="gate_size_t", gate=(which, row)))
                    break
                lo, hi = (mid, hi) if e < 13.1 else (lo, mid)
            else:
                raise AssertionError("no error between 13 and 13.26 found")
            continue
        while np.nextafter(lo, f32(np.inf)) < hi:
            mid = f32((f32(lo) + f32(hi)) / 2)
            if _gate_probe(c, row, which, mid)[2]:
                lo = mid
            else:
                hi = mid
        for tag, y in (("below", lo), ("above", hi)):
            out.append(dict(_gate_probe(c, row, which, y)[0], name="gate_%s_%s" % (name, tag), gate=(which, row)))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = count_cases() + [filter_case()] + return_cases() + count_rule_cases() + resume_cases() + parameter_cases() + [degenerate_case(), twin_case(), invalid_set_case()] + list(gate_cases())
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


@functools.lru_cache(maxsize=None)
def expected(pairs=None):
    """the sim's answers for all_cases(), case p run as pair pairs[p] (None: pair 0 = the single call)"""
    cs = all_cases()
    return sim.run([dict(c, pair=0 if pairs is None else pairs[p]) for p, c in enumerate(cs)])
