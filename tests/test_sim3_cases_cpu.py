"""CPU side of the Sim3Solver RANSAC (sslam_sim3_ransac; reference src/Sim3Solver.cc, LoopClosing::ComputeSim3's solver): that the cases of tests/sim3_cases.py reach
what their names say, and that the host build of csrc/sim3_math.h (tests/sim3_sim.py: two g++ builds, one under the sanitizers, which must answer alike) agrees bit for bit
  - with tests/sim3_ref.py, an independent numpy restatement (the constructor, SetRansacParameters, the draw, ComputeSim3 around the eigenvector, CheckInliers, Project,
    iterate's control flow), and
  - with tests/golden/sim3_ref.npz, recorded results of the reference's OWN SetRansacParameters / iterate / CheckInliers / Project / FromCameraToImage and of its N11 .. N44
    lines (tests/golden/make_sim3_ref.py)
on every case, every call and every iteration; that decision D16's eigenvector and rotation are what LAPACK and the literal atan2 + Rodrigues path give; and that the
library exports the new entry points."""
import math
import os
import subprocess
import numpy as np
import sim3_cases as tc
import sim3_ref as ref
import sim3_sim as sim

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGEN_BOUND = 2e-15      # measured 3.44e-16 over the 942 separated solves of the cases; the margin over it is the 5.7 x D15's solver test has over its own worst


def case(name):
    cs = tc.all_cases()
    i = [c["name"] for c in cs].index(name)
    return cs[i], tc.expected()[i]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    a = np.ascontiguousarray(a, f32); b = np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def solved(c, r):
    """(call, j) of every iteration whose set was solved (all indices in range)"""
    return [(k, j) for k, cl in enumerate(r["calls"]) for j in range(len(cl["its"])) if cl["counts"][j] >= 0]


def test_sim_equals_the_numpy_restatement():
    n_hyp = 0
    for c, r in zip(tc.all_cases(), tc.expected()):
        name = c["name"]
        i1, i2, X1, X2, p1, p2, e1, e2 = ref.correspondences(c)
        N = len(i1)
        assert r["n"] == N and (r["idx1"] == i1).all(), name
        assert same(r["img"], np.c_[p1, p2, e1, e2].reshape(N, 6)), name
        maxits = ref.max_its(c["probability"], c["min_inliers"], c["max_iterations"], N) if N >= c["min_inliers"] else 0
        state = (0, 0, -1)
        for cl, new_its in zip(r["calls"], c["calls"]):
            st = cl["state"]
            for j, it in enumerate(cl["its"]):
                s = cl["sets"][j]
                if c["sets"] is not None:
                    assert (s == c["sets"][it]).all(), (name, it)
                elif N >= 3:
                    assert ref.draw(N, [ref.hash32(c["seed"], 0, int(it), k) % (N - k) for k in range(3)]) == list(s), (name, it)
                if cl["counts"][j] < 0:
                    assert not cl["mats"][j].any() and not cl["marks"][j].any() and (c["sets"] is None or (s < 0).any() or (s >= N).any()), (name, it)
                    continue
                Pr1, Pr2, O1, O2, ne = ref.n_entries(X1[s].T, X2[s].T)
                assert same(ne, cl["nent"][j]), (name, it)
                R = ref.rotation_closed_form(cl["q"][j])
                assert same(R.reshape(9), cl["mats"][j, 1:10]), (name, it)
                sc, t = ref.finish_sim3(Pr1, Pr2, O1, O2, R, c["fix_scale"])
                assert same(sc, cl["mats"][j, 0]) and same(t, cl["mats"][j, 10:13]), (name, it)
                inl = ref.check_inliers(sc, R, t, X1, X2, p1, p2, e1, e2, c["kf1"]["K"], c["kf2"]["K"])
                assert (inl.astype(np.uint8) == cl["marks"][j]).all() and inl.sum() == cl["counts"][j], (name, it)
                n_hyp += 1
            if N < c["min_inliers"]:
                assert len(cl["its"]) == 0 and st["no_more"] == 1 and st["max_its"] == 0 and st["found_it"] == -1 and not cl["inliers"].any(), name
                continue
            first = int(cl["its"][0]) if len(cl["its"]) else state[0]
            assert first == state[0], name
            its_done, best, best_it, found, n_in, no_more = ref.iterate(list(cl["counts"]), first, state, c["min_inliers"], maxits, new_its)
            assert (st["its_done"], st["best_inliers"], st["best_it"], st["found_it"], st["n_inliers"], st["no_more"], st["max_its"], st["n"]) == \
                (its_done, best, best_it, found, n_in, no_more, maxits, N), (name, st)
            assert its_done - first == len(cl["its"]), name
            if best_it >= first:
                assert same(np.r_[st["s12"], st["R12"], st["t12"]], cl["mats"][best_it - first]), name
            want = np.zeros(len(c["m12"]), np.uint8)
            if found >= 0:
                want[i1[cl["marks"][found - first] == 1]] = 1
            assert (cl["inliers"] == want).all(), name
            state = (its_done, best, best_it)
    assert n_hyp > 900


def test_reference_fixture():
    """the reference's own functions (tests/golden/sim3_ref.npz) == the sim, bit for bit; no case left out but those the reference's draw cannot run"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "sim3_ref.npz"))
    meta = str(fx["meta"])
    assert all(s in meta for s in (":114-138", ":140-207", ":340-364", ":382-403", ":405-423", ":251-260", ":319-336", "-ffp-contract=off", "none left out"))
    left_out = ("count_2_drawn", "twin_set", "invalid_sets")
    cs = [(c, r) for c, r in zip(tc.all_cases(), tc.expected()) if c["name"] not in left_out]
    assert list(fx["names"]) == [c["name"] for c, _ in cs] and len(cs) == len(tc.all_cases()) - 3
    for c, r in cs:
        n = c["name"]
        assert same(fx[n + "/img"], r["img"][:, :4]), n                                      # FromCameraToImage
        if r["n"] >= c["min_inliers"]:
            assert fx[n + "/max_its"] == r["calls"][0]["state"]["max_its"], n             # SetRansacParameters
        counts = np.concatenate([cl["counts"] for cl in r["calls"]]); marks = np.concatenate([cl["marks"] for cl in r["calls"]])
        assert (fx[n + "/counts"] == counts).all() and (fx[n + "/marks"] == marks).all(), n   # CheckInliers + Project on every iteration
        nent = np.concatenate([cl["nent"] for cl in r["calls"]])
        assert same(fx[n + "/nent"].astype(f32), nent) and (fx[n + "/nent"].astype(f32).astype(np.float64) == fx[n + "/nent"]).all(), n      # :251-260: float sums
        for k, cl in enumerate(r["calls"]):                                                  # iterate
            st = cl["state"]
            ret, n_in, no_more, its_done, best = fx[n + "/calls"][k]
            assert (ret, n_in, no_more, its_done, best) == (st["found_it"], st["n_inliers"], st["no_more"], st["its_done"], st["best_inliers"]), (n, k)
            assert (fx[n + "/inliers"][k] == cl["inliers"]).all(), (n, k)
            if st["best_it"] >= 0:
                assert same(fx[n + "/best"][k], np.r_[st["s12"], st["R12"], st["t12"]]), (n, k)


def test_counts_and_filters():
    assert [case(n)[1]["n"] for n in ("count_min_minus_1", "count_min", "count_min_plus_1", "count_63", "count_64", "count_65", "count_129", "count_0")] == [7, 8, 9, 63, 64, 65, 129, 0]
    assert case("count_min_minus_1")[0]["min_inliers"] == 8
    st = case("count_min_minus_1")[1]["calls"][0]["state"]
    assert (st["its_done"], st["no_more"], st["max_its"]) == (0, 1, 0)
    st = case("count_min")[1]["calls"][0]["state"]
    assert (st["its_done"], st["max_its"], st["best_inliers"], st["found_it"], st["no_more"]) == (1, 1, 8, -1, 1)      # all eight agree and it still cannot return
    assert case("count_min_plus_1")[1]["calls"][0]["state"]["found_it"] == 0
    seen = set()
    for n in (63, 64, 65, 129):
        c, r = case("count_%d" % n)
        assert len(c["m12"]) % 64 != 0 and len(r["calls"][0]["its"]) >= 7 and r["calls"][0]["state"]["found_it"] == -1
        seen.add((bool(c["m12"][0] < 0 and c["m12"][-1] < 0), bool(c["m12"][0] >= 0 and c["m12"][-1] >= 0 and (c["m12"] < 0).any())))
    assert seen == {(True, False), (False, True)}                                            # unmatched rows at the ends; in the middle
    c, r = case("filtered")
    dropped = sorted(p for v in tc.FILTERED.values() for p in v)
    assert (r["idx1"] == np.delete(c["rows1"], dropped)).all() and r["n"] == 20 - len(dropped) == 12
    c, r = case("count_2_drawn")
    st = r["calls"][0]["state"]
    assert (r["calls"][0]["counts"] == -1).all() and (st["its_done"], st["best_it"], st["best_inliers"], st["no_more"]) == (3, -1, 0, 1)


def test_return_positions():
    for name, mi, at, calls in tc.RETURNS:
        c, r = case(name)
        st = r["calls"][-1]["state"]
        assert st["max_its"] == mi and r["n"] == 30
        allc = np.concatenate([cl["counts"] for cl in r["calls"]])
        if at:
            assert st["found_it"] == at[0] and st["its_done"] == at[0] + 1 and st["no_more"] == 0 and st["n_inliers"] > 10 and (allc[:-1] <= 10).all() and r["calls"][-1]["inliers"].sum() == st["n_inliers"]
        else:
            assert st["found_it"] == -1 and st["no_more"] == 1 and st["its_done"] == mi and (allc <= 10).all() and len(allc) == mi and not r["calls"][-1]["inliers"].any()
            assert len(set(allc.tolist())) > 1 and st["best_it"] == np.flatnonzero(allc == allc.max())[-1]      # the best moves, and sits at the last of the equal maxima
    assert {m for _, m, _, _ in tc.RETURNS} >= {40, 64, 70, 100}


def test_count_rules():
    c, r = case("count_equal_min")
    cl = r["calls"][0]; st = cl["state"]; G = c["min_inliers"]
    assert cl["counts"][3] == cl["counts"][7] == G == cl["counts"].max() and st["found_it"] == -1 and len(cl["its"]) == 10
    assert st["best_it"] == 7 and not same(cl["mats"][3], cl["mats"][7]) and same(np.r_[st["s12"], st["R12"], st["t12"]], cl["mats"][7])      # the later of two equal counts
    c2, r2 = case("count_above_min")
    st2 = r2["calls"][0]["state"]
    assert c2["min_inliers"] == G - 1 and st2["found_it"] == 3 and st2["n_inliers"] == G and r2["calls"][0]["inliers"].sum() == G


def test_resume():
    for tag in ("never", "returns"):
        runs = [case("resume_%s_%s" % (tag, p)) for p in ("once", "ones", "fives")]
        finals = [r["calls"][-1]["state"] for _, r in runs]
        for st in finals:
            assert st["no_more"] == 1 and st["its_done"] == st["max_its"] >= 28
        for st in finals[1:]:
            assert st.tobytes() == finals[0].tobytes()                                        # the same solver after any split into calls
        rets = [[int(cl["state"]["found_it"]) for cl in r["calls"] if cl["state"]["found_it"] >= 0] for _, r in runs]
        assert rets[0] == rets[1] == rets[2] and (len(rets[0]) >= 3) == (tag == "returns")  # and the same returns, resumed behind each
        allc = [np.concatenate([cl["counts"] for cl in r["calls"]]) for _, r in runs]
        assert (allc[0] == allc[1]).all() and (allc[0] == allc[2]).all()
    _, r = case("resume_returns_fives")
    b = [int(cl["state"]["best_inliers"]) for cl in r["calls"]]
    assert b == sorted(b)                                                                   # best_inliers stays raised behind a return


def test_gates():
    K1, K2 = tc.K1, tc.K2
    for name, which in tc.GATES:
        tags = ("",) if name == "size_t" else ("_below", "_above")
        errs, marks, ys = [], [], []
        for tag in tags:
            c, r = case("gate_%s%s" % (name, tag))
            w, row = c["gate"]
            _, _, X1, X2, p1, p2, e1, e2 = ref.correspondences(c)
            m = r["calls"][0]["mats"][0]
            e = ref.errors(m[0], m[1:10], m[10:13], X1, X2, p1, p2, K1, K2)
            assert (e1[row], e2[row]) == ((13, 118) if which == 0 else (118, 13)) and e[1 - which][row] < 100      # the other side's gate is far
            errs.append(e[which][row]); marks.append(int(r["calls"][0]["marks"][0, row])); ys.append(c["kf2"]["x3dc"][c["m12"][c["rows1"][row]], 1])
            assert row not in c["sets"][0] and r["calls"][0]["counts"][0] == 15 + marks[-1]
        if name == "size_t":
            assert 13 < errs[0] < 13.26 and marks == [0] and f32(9.210 * 1.44) > 13.26 - 1e-3      # inside 9.210 * sigma2 and still an outlier
        else:
            assert errs[0] < 13 <= errs[1] and marks == [1, 0] and np.nextafter(ys[0], f32(np.inf)) == ys[1]      # one float apart, a strict <


def test_parameters_and_degenerate_sets():
    (c0, r0), (c1, r1) = case("fix_scale_0"), case("fix_scale_1")
    assert (r0["calls"][0]["sets"] == r1["calls"][0]["sets"]).all() and len(r0["calls"][0]["its"]) >= 10
    assert (r1["calls"][0]["mats"][:, 0] == 1).all() and (np.abs(r0["calls"][0]["mats"][:, 0] - 1) > 1e-3).all()
    assert (c0["kf1"]["K"] != c0["kf2"]["K"]).all()
    sets = [case("seed_%d" % s)[1]["calls"][0]["sets"] for s in (0, 1, 0xDEADBEEF)]
    assert (sets[0] != sets[1]).any() and (sets[0] != sets[2]).any() and (sets[1] != sets[2]).any()
    for s in sets:
        assert all(len(set(x)) == 3 for x in s.tolist())
    c, r = case("loop_closing")
    assert (c["probability"], c["min_inliers"], c["max_iterations"], c["calls"]) == (0.99, 20, 300, [5, 5, 5, 5]) and r["calls"][0]["state"]["max_its"] == 293
    c, r = case("drawn_130")
    assert len(r["calls"][0]["its"]) == 130 and r["calls"][0]["state"]["found_it"] == -1 and r["calls"][0]["state"]["best_it"] > 64
    c, r = case("degenerate")
    cl = r["calls"][0]
    assert tc.DEGENERATE_SETS == ("collinear", "good", "identity", "z0", "other") and len(cl["its"]) == 5 and cl["state"]["found_it"] == -1
    _, _, X1, X2, p1, p2, _, _ = ref.correspondences(c)
    assert np.linalg.matrix_rank(X1[c["sets"][0]].astype(np.float64) - X1[c["sets"][0][0]].astype(np.float64)) == 1                            # collinear
    assert (X1[c["sets"][2]] == X2[c["sets"][2]]).all() and (cl["q"][2] == [1, 0, 0, 0]).all() and np.isnan(cl["mats"][2]).all() and cl["counts"][2] == 0   # v == 0: NaN, no inlier
    assert X1[9, 2] == 0 and not np.isfinite(p1[9]).all() and np.isfinite(cl["mats"][3]).all() and cl["marks"][:, 9].sum() == 0                # z = 0
    assert cl["counts"][1] == cl["counts"][4] == 13
    c, r = case("twin_set")
    cl = r["calls"][0]
    assert c["sets"][0][0] == c["sets"][0][1] and cl["counts"][0] >= 0 and cl["counts"][1] == 11 and cl["state"]["best_it"] == 1
    c, r = case("invalid_sets")
    cl = r["calls"][0]
    assert list(cl["counts"] < 0) == [True, False, True, False, False, True] and cl["state"]["best_it"] in (1, 3, 4) and len(cl["its"]) == 6
    assert max(len(c["m12"]) for c in tc.all_cases()) <= 140 and max(c["max_iterations"] for c in tc.all_cases()) <= 300


def test_iteration_table():
    """mRansacMaxIts by the libm formula for every N the cases' capacities allow, through the sim (which calls the header's ransac_max_its), and the values DESIGN.md lists beside D16"""
    t = [ref.max_its(0.99, 20, 300, N) for N in range(20, 140)]
    assert t[:10] == [1, 3, 4, 5, 6, 7, 8, 9, 11, 12] and t[80 - 20] == 293 and t[81 - 20:] == [300] * (140 - 81)
    base = tc.make("table", 1, 1, 1, 0)
    for prob, mi, mx in ((0.99, 20, 300), (0.99, 6, 300), (1 - 1e-10, 8, 40), (0.5, 1, 7)):
        cs = []
        for N in range(0, 140):
            k = dict(oct=np.zeros(N, np.int32), valid=np.ones(N, np.uint8), x3dc=np.ones((N, 3), f32), K=tc.K1)
            cs.append(dict(base, kf1=k, kf2=k, m12=np.arange(N, dtype=np.int32), probability=prob, min_inliers=mi, max_iterations=mx, calls=[1]))
        for N, r in enumerate(sim.run_plain(cs)):
            st = r["calls"][0]["state"]
            assert st["n"] == N and st["max_its"] == (0 if N < mi else ref.max_its(prob, mi, mx, N)), (prob, mi, mx, N)
            if N >= mi and N != mi:
                eps = f32(f32(mi) / f32(N))
                assert st["max_its"] == max(1, min(math.ceil(math.log(1 - prob) / math.log(1 - math.pow(float(eps), 3))), mx))


def test_eigenvector_and_rotation():
    """D16 on every solved set of every case.  eigen: the Jacobi eigenvector against numpy.linalg.eigh of the same float entries in float64, up to sign, where the largest
    eigenvalue is separated (gap > 1e-6 of the spectrum's width): |q - q_lapack|_inf x gap / width <= EIGEN_BOUND (an eigenvector is determined to rounding / gap), q is a
    unit vector and |N q - lambda_max q| <= 1e-13 max(1, |lambda|) on every solve.  rodrigues: the closed form against the
    literal atan2 + Rodrigues path in float64 from the same eigenvector: both are exact to double rounding before the one rounding to float, so an element differs by at
    most one float ulp."""
    worst, n, differing, elements = 0.0, 0, 0, 0
    for c, r in zip(tc.all_cases(), tc.expected()):
        for k, j in solved(c, r):
            cl = r["calls"][k]
            q = cl["q"][j]
            if not np.isfinite(q).all() or not np.isfinite(cl["nent"][j]).all():
                continue
            A = ref.n_matrix(cl["nent"][j])
            w, V = np.linalg.eigh(A)
            assert abs(np.linalg.norm(q) - 1) < 1e-14
            assert np.linalg.norm(A @ q - w[-1] * q) <= 1e-13 * max(1.0, np.abs(w).max()), (c["name"], j)      # an eigenvector of the largest eigenvalue, whatever the gap
            if w[-1] - w[-2] > 1e-6 * (w[-1] - w[0]):
                v = V[:, -1] * np.sign(V[:, -1] @ q)
                worst = max(worst, np.abs(v - q).max() * (w[-1] - w[-2]) / (w[-1] - w[0]))
                n += 1
            if (q[1:] == 0).all():
                assert np.isnan(cl["mats"][j, 1:10]).all()
                continue
            lit = ref.rotation_literal(q)
            got = cl["mats"][j, 1:10].reshape(3, 3)
            lit32 = lit.astype(f32)
            ulp = np.abs(np.nextafter(lit32, f32(np.inf)) - lit32)
            d = np.abs(got.astype(np.float64) - lit32.astype(np.float64))
            assert (d <= ulp).all(), (c["name"], j, got, lit32)
            differing += int((bits(got) != bits(lit32)).sum()); elements += 9
    print("eigen: %d separated solves, worst gap-weighted |q - q_lapack|_inf = %.3g; rotation: %d of %d elements differ from the literal path by one ulp"
          % (n, worst, differing, elements))
    assert n > 900 and worst <= EIGEN_BOUND


def test_the_library_exports_the_entry_points(fe):
    lib = os.path.join(ROOT, "structure-slam-pointline_amd", "lib")
    syms = lambda p: subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib, p)], capture_output=True, text=True, check=True).stdout.split()
    prod, test = syms("libsslam_frontend.so"), syms("libsslam_frontend_testing.so")
    for s in ("sslam_sim3_ransac", "sslam_sim3_ransac_batch_dev"):
        assert s in prod and s in test and s + "(" in open(os.path.join(ROOT, "include", "sslam_frontend.h")).read()
    assert "sslam_testing_sim3_hypotheses" in test and "sslam_testing_sim3_hypotheses" not in prod
    assert "sslam_testing_sim3_hypotheses(" in open(os.path.join(ROOT, "include", "sslam_testing.h")).read()
    assert callable(getattr(fe.Context, "sim3_ransac", None)) and callable(getattr(fe.Context, "sim3_ransac_batch_dev", None)) and fe.SIM3_STATE_DTYPE.itemsize == 84
    assert fe.lib().sslam_abi_version() == 1
