"""CPU suite of the PnP RANSAC (csrc/pnp_math.h through its host model tests/sim/pnp_sim.cpp, plain and under -fsanitize=address,undefined): what every case of
tests/pnp_cases.py reaches, the host model against the reference's own code (tests/golden/pnp_ref.npz, recorded by tests/golden/make_pnp_ref.py) and against the
independent numpy / LAPACK restatement tests/pnp_ref.py, pnp_plan, the iteration table, the parameter rules and the layout of sslam_pnp_state.

Against the fixture: bit for bit.  The fixture's leaves are decision D17's, so every bit between them is the reference's own arithmetic and control flow.

Against pnp_ref.py: every integer and boolean outcome of every case whose sets converge in both models (tests/pnp_cases.py chooses them by each model's own rep_error),
the chosen N aside -- on four exact points the three rep_errors are rounding noise wherever more than one solve arrives, and their order is no property of the solver.
Poses within four times the largest deviation measured over those cases: MINIMAL_DEV for four-point hypotheses, REFINED_DEV for Refine's Tcw.  LOOSE
names the cases compared on what does not depend on a hypothesis' pose (N, the table's entries, the sets drawn, the iterations and which of them had a usable set): the
library's draws and the coplanar and repeated-point sets need not converge, and the gate case puts a gate on one model's own float."""
import os
import subprocess
import numpy as np
import pytest
import pkg
import pnp_cases as tc
import pnp_ref as ref
import pnp_sim as sim

# The largest deviations measured between the host model and pnp_ref.py over the converged sets of the cases outside LOOSE; asserted at four times these.
MINIMAL_DEV = 8.0e-6      # R and t entries (double) of the four-point hypotheses whose chosen solve converged
REFINED_DEV = 1.34e-7     # Tcw entries (float) of the refined returns (found == 1)
LOOSE = tc.DRAWN + tc.BASIS_DEPENDENT + ("gate_neighbours",)
FIELDS = ("its_done", "best_inliers", "best_it", "refine_ok", "found", "found_it", "n_inliers", "no_more")


@pytest.fixture(scope="module")
def answers():
    B = tc.build()
    names = list(B)
    cs = [tc.public(B[n]) for n in names]
    return names, cs, sim.run(cs), [ref.run(c) for c in cs]


def _by(answers, name):
    names, cs, got, want = answers
    i = names.index(name)
    return cs[i], got[i], want[i]


def test_host_model_equals_reference_model(answers):
    names, cs, got, want = answers
    dev_min = dev_ref = 0.0
    for name, c, g, w in zip(names, cs, got, want):
        assert (g["n"], g["min_inliers"], g["max_its"]) == (w["n"], w["min_inliers"], w["max_its"]), name
        np.testing.assert_array_equal(g["idx"], w["idx"], err_msg=name)
        assert g["max_err"].tobytes() == w["max_err"].tobytes(), name
        loose = name in LOOSE
        for a, b in zip(g["calls"], w["calls"]):
            if loose:      # the two loops may return at different iterations: the sets of the iterations the host model ran, from the reference model's draw
                drawn = ref.sets_of(c, g["n"], [int(i) for i in a["its"]])
                np.testing.assert_array_equal(a["sets"], np.array([x[0] for x in drawn], np.int32).reshape(len(drawn), 4), err_msg=name)
                assert [bool(x) for x in a["counts"][:, 0] >= 0] == [x[1] for x in drawn], name
                continue
            np.testing.assert_array_equal(a["its"], np.array(b["its"], np.int64), err_msg=name)
            np.testing.assert_array_equal(a["counts"][:, [0, 2, 3]], b["counts"][:, [0, 2, 3]], err_msg=name)
            assert [int(a["state"][f]) for f in FIELDS] == [int(b[f]) for f in FIELDS], name
            np.testing.assert_array_equal(a["inliers"], b["inliers"], err_msg=name)
            ok = (a["counts"][:, 0] >= 0) & (a["trace"][:, :3].min(1) < tc.CONVERGED)      # the hypotheses of the chosen sets; others never ran
            if ok.any():
                dev_min = max(dev_min, float(np.abs(a["poses"][ok] - b["poses"][ok]).max()))
            if a["state"]["found"] == 1:
                dev_ref = max(dev_ref, float(np.abs(a["state"]["Tcw"].astype(np.float64) - b["Tcw"].astype(np.float64)).max()))
    print("largest deviation from the reference model: minimal %.3e, refined %.3e" % (dev_min, dev_ref))
    assert dev_min <= 4 * MINIMAL_DEV, dev_min
    assert dev_ref <= 4 * REFINED_DEV, dev_ref


def test_host_model_equals_the_reference_fixture(answers):
    """tests/golden/pnp_ref.npz: the reference's own SetRansacParameters, add_correspondence / compute_pose / CheckInliers per set, and iterate with Refine per call"""
    names, cs, got, want = answers
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_ref.npz"))
    used, left = [str(x) for x in fx["names"]], [str(x) for x in fx["left_out"]]
    assert sorted(used + left) == sorted(names) and len(used) >= 20
    hyps = 0
    for name in used:
        c, g, _ = _by(answers, name)
        assert fx[name + "/params"].tolist() == [g["min_inliers"], g["max_its"]], name
        ncalls = len(fx[name + "/calls"])
        calls = g["calls"][:ncalls]
        sets = np.concatenate([x["sets"] for x in calls])
        np.testing.assert_array_equal(sets, fx[name + "/sets"], err_msg=name + ": the case has changed since the fixture was recorded; run tests/golden/make_pnp_ref.py")
        poses = np.concatenate([x["poses"] for x in calls]); counts = np.concatenate([x["counts"][:, 0] for x in calls]); marks = np.concatenate([x["marks"] for x in calls])
        assert poses.tobytes() == fx[name + "/poses"].tobytes(), name      # mRi, mti of every iteration, bit for bit
        np.testing.assert_array_equal(counts, fx[name + "/counts"], err_msg=name)
        np.testing.assert_array_equal(marks, np.unpackbits(fx[name + "/marks"], axis=1)[:, :g["n"]], err_msg=name)
        hyps += len(counts)
        inl = np.unpackbits(fx[name + "/inliers"], axis=1)[:, :len(c["oct"])]
        for k, x in enumerate(calls):
            st = x["state"]
            returned, n_inliers, no_more, its, best = fx[name + "/calls"][k].tolist()
            assert (int(st["found"] != 0), int(st["n_inliers"]), int(st["no_more"]), int(st["its_done"]), int(st["best_inliers"])) == (returned, n_inliers, no_more, its, best), (name, k)
            assert int(st["found"]) == (0 if not returned else 2 if no_more else 1), (name, k)      # :226-236 leaves bNoMore false, :244-253 sets it
            assert st["Tcw"].tobytes() == fx[name + "/tcw"][k].tobytes(), (name, k)
            np.testing.assert_array_equal(x["inliers"], inl[k], err_msg=name)
    assert hyps > 500


def test_refined_pose_of_a_noise_free_scene(answers):
    c, g, w = _by(answers, "refine_at_0")
    R, t = tc.build()["refine_at_0"]["_poses"][0]
    true = np.hstack([R, t[:, None]]).ravel()
    own = np.abs(w["calls"][0]["Tcw"].astype(np.float64) - true).max()
    got = np.abs(g["calls"][0]["state"]["Tcw"].astype(np.float64) - true).max()
    print("refined Tcw against the true pose: host model %.3e, reference model %.3e" % (got, own))
    assert g["calls"][0]["state"]["found"] == 1 and got <= 4 * max(own, np.finfo(np.float32).eps)


def test_what_the_cases_reach(answers):
    names, cs, got, want = answers
    st = lambda name, call=0: _by(answers, name)[1]["calls"][call]["state"]
    calls = lambda name: _by(answers, name)[1]["calls"]
    for it, name in ((0, "refine_at_0"), (63, "refine_at_63"), (64, "refine_at_64")):
        assert (st(name)["found"], st(name)["found_it"], st(name)["n_inliers"], st(name)["no_more"]) == (1, it, 30, 0), name
    a = calls("refine_fails_then_equal_then_best")      # max_iterations 8: the first call runs them all unless it returns
    assert a[0]["counts"][:6, 0].tolist() == [12, 15, 15, 12, 15, 30] and a[0]["counts"][:6, 2:].tolist() == [[0, 0], [1, 15], [1, 15], [0, 0], [1, 15], [1, 30]]      # Refine fails thrice (refined count == min_inliers), then succeeds
    assert (a[0]["state"]["found"], a[0]["state"]["found_it"], a[0]["state"]["best_it"], a[0]["state"]["refine_ok"]) == (1, 5, 5, 1)
    assert (a[1]["state"]["found"], a[1]["state"]["found_it"], a[1]["state"]["no_more"]) == (2, 5, 1)      # nothing qualifies after the return: the best at exhaustion
    assert _by(answers, "refine_fails_then_equal_then_best")[1]["n"] == 57 and len(_by(answers, "refine_fails_then_equal_then_best")[0]["oct"]) == 67      # every filtered kind, twice
    a = calls("resume_after_refined_return")
    assert [(x["state"]["found"], x["state"]["found_it"], x["state"]["best_it"], int(x["counts"][-1, 0])) for x in a] == [(1, 1, 1, 30), (1, 3, 1, 15), (1, 5, 1, 30), (1, 6, 1, 15)]      # after a refined return: returns at the next qualifying iteration, a lower or an equal count, no new best
    a = calls("exhaustion_with_best")
    assert [(x["state"]["found"], x["state"]["found_it"], x["state"]["no_more"], x["state"]["n_inliers"]) for x in a] == [(2, 1, 1, 15)] * 3      # counts 15 at 1 and 3: the first stays the best
    assert [len(x["its"]) for x in a] == [6, 5, 5] and a[0]["inliers"].sum() == 15 and a[0]["counts"][:, 0].tolist() == [12, 15, 12, 15, 12, 12]
    a = calls("exhaustion_without_best")
    assert [(x["state"]["found"], x["state"]["no_more"], int(x["inliers"].sum())) for x in a] == [(0, 1, 0)] * 2 and not a[0]["state"]["Tcw"].any()
    a = calls("max_its_below_5")
    assert a[0]["state"]["max_its"] == 3 and len(a[0]["its"]) == 5 and (a[0]["state"]["found"], a[0]["state"]["found_it"]) == (2, 3)      # new_iterations governs
    assert (a[1]["state"]["found"], a[1]["state"]["found_it"]) == (1, 6)
    for m in (63, 64, 65, 129):
        a = calls("max_its_%d" % m)
        assert a[0]["state"]["max_its"] == m and len(a[0]["its"]) == m and (a[0]["state"]["found"], a[0]["state"]["found_it"]) == (2, m - 1), m
        assert len(a[1]["its"]) == 5 and a[1]["state"]["its_done"] == m + 5
    a = calls("past_nsets_and_out_of_range")
    assert a[0]["counts"][1:3, 0].tolist() == [-1, -1] and (a[0]["counts"][4:, 0] == -1).all() and not a[0]["poses"][1].any() and a[0]["state"]["found"] == 2
    for name, n in (("n_0", 0), ("n_3", 3), ("n_min_minus_1", 14)):
        g = _by(answers, name)[1]
        assert g["n"] == n and g["max_its"] == 0 and all(x["state"]["no_more"] == 1 and x["state"]["found"] == 0 and len(x["its"]) == 0 for x in g["calls"]), name
    for name, n in (("n_4_is_min", 4), ("n_is_min_drawn", 15), ("n_63_drawn", 63), ("n_64_drawn", 64), ("n_65_drawn", 65)):
        g = _by(answers, name)[1]
        assert g["n"] == n == g["min_inliers"] and g["max_its"] == 1 and [len(x["its"]) for x in g["calls"]] == _by(answers, name)[0]["calls"], name      # min_inliers == N: one iteration, then new_iterations
        assert all((x["counts"][:, 3] <= n).all() and x["state"]["found"] in (0, 2) for x in g["calls"]), name      # Refine cannot exceed min_inliers == N
    assert (_by(answers, "epsilon_above_min")[1]["min_inliers"], _by(answers, "epsilon_at_min")[1]["min_inliers"], _by(answers, "epsilon_below_min")[1]["min_inliers"]) == (30, 30, 20)
    assert calls("epsilon_above_min")[0]["counts"][:2, 2].tolist() == [0, 0] and calls("epsilon_below_min")[0]["counts"][0].tolist()[2:] == [1, 20]
    g = _by(answers, "mixed_drawn")[1]
    assert any(x["state"]["found"] == 1 for x in g["calls"])
    chosen = np.concatenate([x["counts"][:, 1] & 255 for g in got for x in g["calls"]])
    assert all((chosen == n).any() for n in (1, 2, 3))      # each of N = 1, 2, 3 is chosen
    # gates on neighbouring floats: row A's gate IS its error2 under the first hypothesis (the strict < leaves it out), row B's gate is the next float above its error2
    A, B, eA, eB = tc.build()["gate_neighbours"]["_gate_rows"]
    g = _by(answers, "gate_neighbours")[1]
    assert g["max_err"][A] == np.float32(eA) and g["max_err"][B] == np.nextafter(np.float32(eB), np.float32(np.inf)) and eA > 0 and eB > 0
    first = g["calls"][0]
    assert first["marks"][0, A] == 0 and first["marks"][0, B] == 1 and first["counts"][0, 0] == 29 and first["marks"][0].sum() == 29
    # the branches of the solves (pnp::REACH_*): the det < 0 flip, the pcs[2] < 0 sign change, b4[0] < 0, and a dropped singular value of CC (every coplanar set)
    reach = lambda gg: np.bitwise_or.reduce(np.concatenate([x["counts"][:, 1] >> 8 for x in gg["calls"]] + [np.zeros(1, np.int32)]))
    every = np.bitwise_or.reduce([reach(gg) for name, gg in zip(names, got) if name != "coplanar"])
    assert every & 1 and every & 2 and every & 4
    co = _by(answers, "coplanar")[1]
    assert all(x["counts"][:, 1].min() >> 8 & 8 for x in co["calls"])      # every coplanar four-point set: a zero control-point scale


def test_plan():
    P = {cap: sim.plan(cap) for cap in (1, 1000, 2000, 2048, 2049)}
    fixed = 8 * (78 + 144) * 64 + 256
    for cap, p in P.items():
        assert p == dict(rowBytes=24, ldsBytes=24 * cap + fixed, ldsOptIn=1, threads=64, maxCap=2048), cap
    assert P[2048]["ldsBytes"] + 256 <= 160 * 1024 < 24 * 3072 + fixed      # the bound fits the compute unit's LDS beside the static words; the next step of 1024 rows does not
    assert P[2048]["maxCap"] >= 2000      # the c2 configuration extracts 2000 keypoints


def test_table():
    for probability, mi, mx, eps, cap in ((0.99, 10, 300, 0.5, 130), (0.999, 4, 50, 0.05, 70), (0.5, 50, 7, 1.0, 120)):
        T = sim.table(probability, mi, mx, eps, cap)
        want = np.array([ref.ransac_params(probability, mi, mx, eps, n) for n in range(cap + 1)], np.int64)
        np.testing.assert_array_equal(T, want)
        assert (T[:, 1][np.arange(cap + 1) < T[:, 0]] == 0).all() and (T[:, 1][np.arange(cap + 1) >= T[:, 0]] >= 1).all()


def test_parameter_rules():
    assert sim.params_ok() == (True, True)
    nan = float("nan")
    for bad in (dict(has_sigma=0), dict(nlevels=0), dict(nlevels=65), dict(probability=0.0), dict(probability=1.0), dict(probability=nan), dict(min_inliers=0),
                dict(max_iterations=0), dict(new_iterations=0), dict(epsilon=0.0), dict(epsilon=np.nextafter(np.float32(1), np.float32(2))), dict(epsilon=nan), dict(th2=0.0),
                dict(th2=-1.0), dict(th2=nan)):
        assert sim.params_ok(**bad) == (False, True), bad
    for good in (dict(nlevels=1), dict(nlevels=64), dict(probability=1e-9), dict(probability=1 - 1e-9), dict(min_inliers=1, max_iterations=1, new_iterations=1), dict(epsilon=1.0),
                 dict(epsilon=1e-30), dict(th2=1e-30)):
        assert sim.params_ok(**good) == (True, True), good
    for bad in (dict(npairs=-1), dict(cap=0), dict(kfcap=0), dict(nframes=-1), dict(nkeyframes=-1), dict(npairs=1 << 21, cap=1 << 10), dict(nframes=1 << 21, cap=1 << 10),
                dict(nkeyframes=1 << 21, kfcap=1 << 10), dict(has_sets=1, npairs=1 << 14, nsets=1 << 14), dict(has_sets=1, nsets=-1)):
        assert sim.params_ok(**bad) == (True, False), bad
    for good in (dict(npairs=(1 << 21) - 1, cap=1 << 10), dict(has_sets=1, npairs=(1 << 14) - 1, nsets=1 << 14), dict(npairs=1 << 14, nsets=1 << 14), dict(npairs=0, nframes=0, nkeyframes=0)):
        assert sim.params_ok(**good) == (True, True), good


def test_state_layout_matches_the_header(tmp_path):
    fe = pkg.frontend()
    names = [n for n in fe.PNP_STATE_DTYPE.names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sslam_frontend.h"\nint main(void) {\n    printf("%zu", sizeof(sslam_pnp_state));\n' +
                   "".join('    printf(" %%zu", offsetof(sslam_pnp_state, %s));\n' % n for n in names) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(pkg.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [192] + [fe.PNP_STATE_DTYPE.fields[n][1] for n in names]
