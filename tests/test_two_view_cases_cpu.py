"""CPU side of the two-view RANSAC (sslam_two_view_ransac; Initializer::Initialize's model selection, reference src/Initializer.cc:55-118, :155-497, :784-830): that the
cases of tests/two_view_cases.py reach what their names say, and that the host build of csrc/two_view_math.h (tests/two_view_sim.py: two g++ builds, one under the
sanitizers, which must answer alike) agrees bit for bit
  - with tests/two_view_ref.py, an independent numpy restatement of the reference-owned parts (Normalize, CheckHomography, CheckFundamental, the draw, the selection), and
  - with tests/golden/two_view_ref.npz, recorded results of the reference's OWN Normalize / CheckHomography / CheckFundamental (tests/golden/make_two_view_ref.py)
on every case and every iteration, and that decision D15's solver delivers what a float SVD is entitled to."""
import os
import numpy as np
import two_view_cases as tc
import two_view_ref as ref
import two_view_sim as sim

f32 = np.float32
EPS32 = float(np.finfo(f32).eps)


def case(name):
    cs = tc.all_cases()
    i = [c["name"] for c in cs].index(name)
    return cs[i], tc.expected()[i]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    a = np.ascontiguousarray(a, f32); b = np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def test_match_counts_and_layouts():
    want = {"count_%d" % n: n for n in (0, 7, 8, 9, 63, 64, 65, 255, 256, 257)}
    seen = set()
    for c, r in zip(tc.all_cases(), tc.expected()):
        nm = tc.nmatches(c)
        assert r["result"]["nmatches"] == nm
        assert (r["result"]["model"] == 0) == (nm < 8)
        if nm < 8:
            assert r["result"]["best_it_h"] == -1 and r["result"]["best_it_f"] == -1 and not r["inliers"].any() and not r["result"]["H21"].any() and not r["sets"].any()
        if c["name"] in want:
            assert nm == want[c["name"]] and len(c["kp1"]) != len(c["kp2"])
            m = c["m12"]
            seen.add(("ends" if nm and m[0] < 0 and m[-1] < 0 else "middle" if nm and m[0] >= 0 and m[-1] >= 0 else "other",
                      bool(nm > 2 and (np.diff(m[m >= 0]) < 0).all())))
    assert {s[0] for s in seen} >= {"ends", "middle"} and {s[1] for s in seen} == {True, False}      # -1 at the first and last row; keypoint-2 indices descending
    c, r = case("count_8")
    assert all(sorted(s) == list(range(8)) for s in r["sets"])                                         # eight matches: every set a permutation
    c, r = case("count_full_64")
    assert len(c["kp1"]) == len(c["kp2"]) == r["result"]["nmatches"] == 64
    assert sorted({c["iterations"] for c in tc.iteration_cases()}) == [1, 63, 64, 65, 200, 257]
    assert {c["sigma"] for c in tc.sigma_cases()} == {1.0, 2.5}
    assert max(len(c["kp1"]) for c in tc.all_cases()) <= 260 and max(c["iterations"] for c in tc.all_cases()) <= 257


def test_sigma_moves_the_gates():
    (c1, r1), (c2, r2) = case("sigma_1_0"), case("sigma_2_5")
    assert (c1["kp1"] == c2["kp1"]).all() and (r1["sets"] == r2["sets"]).all() and same(r1["mats"], r2["mats"])
    assert (r2["scores"] >= r1["scores"]).all() and (r2["scores"] > r1["scores"]).any() and r2["inliers"].sum() > r1["inliers"].sum()


def test_tie_goes_to_the_first():
    c, r = case("tie_3_7")
    assert (c["sets"][3] == c["sets"][7]).all()
    for k, key in ((0, "best_it_h"), (1, "best_it_f")):
        s = r["scores"][:, k]
        assert bits(s[3]) == bits(s[7]) and s[3] == s.max() and (np.delete(s, [3, 7]) < s[3]).all()
        assert r["result"][key] == 3
    assert same(r["result"]["H21"], r["mats"][3, 1]) and same(r["result"]["F21"], r["mats"][3, 4])


def test_no_winner():
    c, r = case("no_winner")
    res = r["result"]
    assert res["nmatches"] == 30 and not r["scores"].any() and r["mats"][:, :5].any()
    assert res["best_it_h"] == -1 and res["best_it_f"] == -1 and not res["H21"].any() and not res["F21"].any() and not r["inliers"].any()
    assert res["score_h"] == 0 and res["score_f"] == 0 and np.isnan(res["rh"]) and res["model"] == 2      # 0 / 0 is not > 0.40: the reference would go on to ReconstructF


def test_invalid_sets_never_win():
    c, r = case("invalid_sets")
    for it in (0, 2, 5):
        assert not r["mats"][it].any() and not r["scores"][it].any()
    for it in (1, 3, 4):
        assert (r["scores"][it] > 0).all()
    assert r["result"]["best_it_h"] in (1, 3, 4) and r["result"]["best_it_f"] in (1, 3, 4)


def test_degenerate_sets():
    c, r = case("degenerate")
    assert r["norm"][0] == 300 and tc.DEGENERATE_SETS == ("column", "good", "twin", "slant", "column", "other")
    rows, _ = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
    for it in (0, 4):                                       # eight collinear points at the mean x: a singular H21i
        assert (rows[c["sets"][it], 0] == 300).all()
        Hn, H21, H12 = r["mats"][it, :3]
        assert np.count_nonzero(Hn) == 1 and not H21[3:].any() and not H12.any()
        assert np.isnan(r["scores"][it, 0])
    assert np.isfinite(r["scores"][[1, 2, 3, 5]]).all()
    # the NaN at iteration 0 loses to the finite iteration 1, and the NaN at iteration 4 does not displace it
    assert r["result"]["best_it_h"] == 1 and r["scores"][1, 0] > r["scores"][[2, 3, 5], 0].max() and np.isfinite(r["result"]["score_h"])
    tw = rows[c["sets"][2]]
    assert (tw[0] == tw[1]).all() and len({tuple(x) for x in tw}) == 7                      # two matches at one pixel in both frames
    sl = rows[c["sets"][3], :2].astype(np.float64)
    assert np.linalg.matrix_rank(np.c_[sl, np.ones(8)]) == 2                                # collinear


def test_gates():
    cs = {c["name"]: (c, r) for c, r in zip(tc.all_cases(), tc.expected()) if "gate" in c}
    assert len(cs) == 12
    for model, term in tc.GATES:
        th = ref.TH_H if model == "h" else ref.TH_F
        chi, inl, score = [], [], []
        for tag in ("below", "at", "above"):
            c, r = cs["gate_%s%d_%s" % (model, term + 1, tag)]
            _, _, row, kp1row = c["gate"]
            rows, idx = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
            assert idx[row] == kp1row and row not in c["sets"][0]
            t = ref.homography_terms(r["mats"][0, 1], r["mats"][0, 2], rows, c["sigma"]) if model == "h" else ref.fundamental_terms(r["mats"][0, 4], rows, c["sigma"])
            chi.append(t[row, term])
            assert t[row, 1 - term] <= th                      # the other term of the match stays inside: the bit is this gate's
            inl.append(int(r["inliers"][kp1row]) >> (0 if model == "h" else 1) & 1)
            terms, _ = ref.score_terms(t, th, ref.TH_SCORE)
            score.append(r["scores"][0, 0 if model == "h" else 1])
            assert bits(ref.sum_in_order(terms)) == bits(score[-1])                          # the score holds the term exactly while the gate is open
            assert len(terms) == 2 * len(rows) - (tag == "above")
        assert chi[0] <= chi[1] <= th < chi[2], (model, term, chi)                           # they straddle the threshold ...
        assert inl == [1, 1, 0], (model, term, inl)                                          # ... and the bit follows
        a, b = [cs["gate_%s%d_%s" % (model, term + 1, tag)][0] for tag in ("at", "above")]
        d = np.flatnonzero(bits(np.r_[a["kp1"].ravel(), a["kp2"].ravel()]) != bits(np.r_[b["kp1"].ravel(), b["kp2"].ravel()]))
        assert len(d) == 1                                                                  # one coordinate, one float apart
        x, y = np.r_[a["kp1"].ravel(), a["kp2"].ravel()][d[0]], np.r_[b["kp1"].ravel(), b["kp2"].ravel()][d[0]]
        assert np.nextafter(x, f32(np.inf)) == y


def test_order_of_the_sum_decides_the_winner():
    c, r = case("order")
    rev = tc.other_order_scores(c, r, "h")
    fwd = np.array([ref.check_homography(r["mats"][it, 1], r["mats"][it, 2], ref.match_rows(c["kp1"], c["kp2"], c["m12"])[0], c["sigma"])[0] for it in range(c["iterations"])], f32)
    assert same(fwd, r["scores"][:, 0])                                                     # match order is the sim's order
    best_rev, it_rev = ref.select(rev)
    assert it_rev != r["result"]["best_it_h"] and bits(best_rev) != bits(r["result"]["score_h"])
    assert ref.select(fwd) == (r["result"]["score_h"], r["result"]["best_it_h"])


def test_scenes():
    assert case("scene_planar")[1]["result"]["model"] == 1 and case("scene_planar")[1]["result"]["rh"] > 0.40
    assert case("scene_two_layer")[1]["result"]["model"] == 2 and case("scene_two_layer")[1]["result"]["rh"] < 0.40


def test_generated_sets():
    cs = tc.seed_cases() + tc.iteration_cases()
    r0 = sim.run([dict(c, pair=0) for c in cs]); r1 = sim.run([dict(c, pair=1) for c in cs])
    assert len({c["seed"] for c in tc.seed_cases()}) == 3
    for c, a, b in zip(cs, r0, r1):
        nm = tc.nmatches(c)
        for pair, r in ((0, a), (1, b)):
            for it, s in enumerate(r["sets"]):
                assert len(set(s)) == 8 and s.min() >= 0 and s.max() < nm
                randi = [ref.hash32(c["seed"], pair, it, j) % (nm - j) for j in range(8)]
                assert ref.draw(nm, randi) == list(s), (c["name"], pair, it)                  # the swap-with-back of :93-108 fed with the same integers
        assert (a["sets"] != b["sets"]).any()
    a, b, d = [r["sets"] for r in r0[:3]]
    assert (a != b).any() and (a != d).any() and (b != d).any()                              # the seed matters


def test_selection_and_result_follow_the_reference():
    for c, r in zip(tc.all_cases(), tc.expected()):
        if r["result"]["model"] == 0:
            continue
        res = r["result"]
        for k, (s, it, m) in enumerate((("score_h", "best_it_h", 1), ("score_f", "best_it_f", 4))):
            best, at = ref.select(r["scores"][:, k])
            assert bits(best) == bits(res[s]) and at == res[it], c["name"]
            assert same(res["H21" if k == 0 else "F21"], r["mats"][at, m] if at >= 0 else np.zeros(9, f32))
        rh, model = ref.model(res["score_h"], res["score_f"])
        assert same(rh, res["rh"]) and model == res["model"], c["name"]


def test_solver_is_as_good_as_a_float_svd():
    """D15's solver on every set of every case and 1 000 more (exact, noisy and random correspondences): with h the unit vector the sim returns, in float64 against LAPACK,
    |A h| <= sigma_min(A) + eps32 |A|_F -- what a float SVD, the reference's precision, is entitled to -- and the smallest singular value of Fn <= eps32 |Fn|_F.
    Fpre is the null vector of ComputeF21's A; Hn of ComputeH21's."""
    extra = tc.random_systems()
    cases = list(tc.all_cases()) + extra
    res = list(tc.expected()) + sim.run(extra)
    n, worst = 0, 0.0
    for c, r in zip(cases, res):
        if r["result"]["model"] == 0:
            continue
        for it in range(c["iterations"]):
            if not r["mats"][it].any():
                continue                     # an invalid injected set
            AH, AF = tc.system_matrices(c, r["sets"][it])
            for A, h in ((AH, r["mats"][it, 0]), (AF, r["mats"][it, 5])):
                A = A.astype(np.float64); h = h.astype(np.float64)
                assert abs(np.linalg.norm(h) - 1) < 4 * EPS32
                smin = np.linalg.svd(A, compute_uv=False)[-1] if A.shape[0] >= 9 else 0.0        # eight rows: a null vector exists
                fro = np.linalg.norm(A)
                excess = (np.linalg.norm(A @ h) - smin) / fro
                worst = max(worst, excess)
                assert excess <= EPS32, (c["name"], it, excess)
            Fn = r["mats"][it, 3].astype(np.float64).reshape(3, 3)
            assert np.linalg.svd(Fn, compute_uv=False)[-1] <= EPS32 * np.linalg.norm(Fn), (c["name"], it)
            n += 1
    assert n >= 1000 + 500
    print("solver: %d sets, worst (|A h| - sigma_min) / |A|_F = %.3g" % (n, worst))


def test_reference_fixture():
    """the reference's own Normalize, CheckHomography and CheckFundamental (tests/golden/two_view_ref.npz) == the sim == tests/two_view_ref.py, bit for bit, no case left out"""
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_view_ref.npz"))
    assert ":334-497" in str(fx["meta"]) and ":784-830" in str(fx["meta"]) and "-ffp-contract=off" in str(fx["meta"])
    cs = tc.all_cases()
    assert list(fx["names"]) == [c["name"] for c in cs]
    for c, r in zip(cs, tc.expected()):
        n = c["name"]
        assert same(fx[n + "/kp1"], c["kp1"]) and same(fx[n + "/kp2"], c["kp2"]) and (fx[n + "/m12"] == c["m12"]).all() and fx[n + "/sigma"] == f32(c["sigma"])
        assert same(fx[n + "/mats"], r["mats"][:, [1, 2, 4]]), n                               # the matrices the reference was run with are today's
        # Normalize: the reference's T elements = the sim's (sX, sY, -meanX sX, -meanY sY); its points = the numpy restatement's
        for f, kp, o in ((1, c["kp1"], 0), (2, c["kp2"], 4)):
            meanX, sX, meanY, sY = r["norm"][o:o + 4]
            with np.errstate(all="ignore"):
                assert same(fx[n + "/T%d" % f], np.array([sX, sY, f32(f32(-meanX) * sX), f32(f32(-meanY) * sY)], f32)), n
                pts, T = ref.normalize(kp)
                assert same(fx[n + "/pn%d" % f], pts) and same(fx[n + "/T%d" % f], [T[0, 0], T[1, 1], T[0, 2], T[1, 2]]), n
                assert same(fx[n + "/pn%d" % f], np.stack([(kp[:, 0] - meanX) * sX, (kp[:, 1] - meanY) * sY], 1).astype(f32)), n      # what the sim feeds its solves
        if r["result"]["model"] == 0:
            assert not fx[n + "/mats"].any()
            continue
        rows, idx = ref.match_rows(c["kp1"], c["kp2"], c["m12"])
        for it in range(c["iterations"]):
            if not r["mats"][it].any():             # an injected set with an index out of range: the library's own rule, nothing of the reference's to compare
                assert n == "invalid_sets" and not r["scores"][it].any()
                continue
            assert same(fx[n + "/scores"][it], r["scores"][it]), (n, it)
            sh, ih = ref.check_homography(r["mats"][it, 1], r["mats"][it, 2], rows, c["sigma"])
            sf, jf = ref.check_fundamental(r["mats"][it, 4], rows, c["sigma"])
            assert same([sh, sf], fx[n + "/scores"][it]), (n, it)
            assert (fx[n + "/inliers"][it] == ih.astype(np.uint8) + 2 * jf.astype(np.uint8)).all(), (n, it)
        # the winners' inlier vectors are the result's bytes
        for k, key in ((0, "best_it_h"), (1, "best_it_f")):
            at = r["result"][key]
            got = np.zeros(len(rows), np.uint8) if at < 0 else (fx[n + "/inliers"][at] >> k) & 1
            assert ((r["inliers"][idx] >> k) & 1 == got).all() and not r["inliers"][np.setdiff1d(np.arange(len(c["kp1"])), idx)].any(), (n, key)
