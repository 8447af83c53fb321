"""The inputs of tests/test_bow_batch_gpu.py reach what they are meant to reach, shown on the CPU with helper + oracle (tests/bow_batch_cases.py):
the chain cases differ from an order-free evaluation, the threshold cases land on 50 / 51 and on the ratio's equality, the rotation cases prune,
the node layouts hold what their names say.  Where the reference's own SearchByBoW was built (oracle/_ref/libref_slices.so), it agrees with
helper + oracle on every case: it takes the node arrays directly."""
import ctypes as C
import os
import numpy as np
import pytest
import bow_batch_cases as bc
import match_cases as mc

SLICES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_slices.so")


def all_cases():
    """name -> pair: every generator of the case module at the seeds the GPU test uses"""
    out = {}
    out.update({"layout_" + k: v for k, v in bc.layout_cases(np.random.default_rng(7100)).items()})
    for m in (2, 3):
        for rev in (False, True):
            out["chain_%d_%s" % (m, "rev" if rev else "fwd")] = bc.chain_case(np.random.default_rng(7200 + m), m, rev)
    out["tie_wins"] = bc.tie_case(np.random.default_rng(7210), 1.2); out["tie_fails"] = bc.tie_case(np.random.default_rng(7210), 0.9)
    out.update({"th_" + k: v[0] for k, v in bc.threshold_cases(np.random.default_rng(7300)).items()})
    out["rot_wrap"] = bc.rot_case(np.random.default_rng(7400), [(30, 354, 360), (12, 95, 104), (8, 200, 209), (5, 230, 239)])
    out["rot_small_second"] = bc.rot_case(np.random.default_rng(7401), [(40, 30, 44), (3, 150, 160), (2, 230, 239)])
    out["bow_case"] = bc.from_bow_case(np.random.default_rng(7500), 60)
    out["bow_case_cut"] = bc.cut(out["bow_case"], 65, 63)
    return out


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def test_csr_helper():
    pk, pf, ik, jf = bc.csr_from_nodes([5, -1, 3, 5, 9, 3, 0], [3, 3, 7, -1, 5, 0, 0])
    assert pk.tolist() == [0, 1, 3, 5] and pf.tolist() == [0, 2, 4, 5]          # nodes 0, 3, 5; 9 and 7 are on one side only, -1 is no node
    assert ik.tolist() == [6, 2, 5, 0, 3] and jf.tolist() == [5, 6, 0, 1, 4]
    assert bc.csr_from_nodes([-1, -1], [-1])[0].tolist() == [0]


def test_chain_cases_differ_from_an_order_free_evaluation(oracle):
    for m in (2, 3):
        res = {}
        for rev in (False, True):
            c = bc.chain_case(np.random.default_rng(7200 + m), m, rev)
            krows, frows = c["chain"]
            a, nm = bc.expect(oracle, c)
            of = bc.order_free(c)
            assert (of[krows, 0] == frows[0]).all()                                # every chain row wants f0
            d = [[bc.hamming(c["kf"]["desc"][krows[i]], c["f"]["desc"][frows[j]]) for j in range(m)] for i in range(m)]
            assert d == [[i + 1 + (0, 20, 30)[j] for j in range(m)] for i in range(m)]
            walk = np.sort(krows)                                                  # the order the matcher visits them in
            assert [int(a[frows[j]]) for j in range(m)] == walk.tolist()            # the j-th visited row gets f_j
            took_second = bc.second_choices(c, a)
            assert int(walk[1]) in took_second and int(walk[0]) not in took_second
            res[rev] = int(np.flatnonzero(frows == np.flatnonzero(a == krows[0])[0])[0])      # which f_j the descriptor k_0 (krows[0] holds it) ends on
        assert res == {False: 0, True: m - 1}                                      # k_0 takes f0 when it comes first, the last frame row when it comes last


def test_tie_cases(oracle):
    c = bc.tie_case(np.random.default_rng(7210), 1.2)
    kr, fr = c["tie"]
    d = [bc.hamming(c["kf"]["desc"][kr], c["f"]["desc"][j]) for j in fr]
    assert d == [12, 12, 40]
    a, _ = bc.expect(oracle, c)
    assert a[fr[0]] == kr and a[fr[1]] == -1                                       # equal distances: the lower frame index wins
    c = bc.tie_case(np.random.default_rng(7210), 0.9)
    a, _ = bc.expect(oracle, c)
    assert (a[fr] == -1).all()                                                     # best equal to second: the ratio test fails


def test_threshold_cases_land_on_the_gates(oracle):
    T = bc.threshold_cases(np.random.default_rng(7300))
    dist = {}
    for name, (c, matched) in T.items():
        k, j1, j2 = c["th"]
        d1 = bc.hamming(c["kf"]["desc"][k], c["f"]["desc"][j1])
        d2 = bc.hamming(c["kf"]["desc"][k], c["f"]["desc"][j2]) if c["f"]["node"][j2] == c["kf"]["node"][k] else None
        dist[name] = (d1, d2)
        a, _ = bc.expect(oracle, c)
        assert (a[j1] == k) == matched, name
    assert dist == {"dist_50": (50, None), "dist_51": (51, None), "ratio_equal": (30, 40), "ratio_below": (29, 40), "kf_invalid": (10, None)}
    assert bc.TH_LOW == 50 and np.float32(0.75) * np.float32(40) == np.float32(30)    # the equality is exact in float


def test_rotation_cases_prune(cases, oracle):
    c = cases["rot_wrap"]
    a, nm = bc.expect(oracle, c)
    plain, nplain = bc.expect(oracle, dict(c, ori=False))
    assert nplain == 55 and (plain >= 0).all()
    # three bins survive: 354..360 degrees (30 matches; with factor 1 / 30 they round to bin 12 and 360 itself would wrap to 0), 95..104 (bin 3), 200..209 (bin 7)
    assert nm == 50 and ((plain >= 0) & (a < 0)).sum() == 5
    c = cases["rot_small_second"]
    a, nm = bc.expect(oracle, c)
    assert nm == 40                                                                # max2 = 3 < 0.1 * 40: only the first bin survives
    # equal features under keyframe angles 90 degrees apart (bins 0, 3, 6, 9 -> 3, 6, 9, 0): each pair alone loses its group of 6; histograms added
    # over the two pairs (26, 34, 24, 16) would lose bin 9 instead, which is the second pair's group of 10
    c0, c1 = bc.rot_neighbours(); a0, n0 = bc.expect(oracle, c0); a1, n1 = bc.expect(oracle, c1)
    assert n0 == n1 == 44 and np.array_equal(c0["f"]["desc"], c1["f"]["desc"]) and np.array_equal(a0, a1)
    rot = lambda c, a: [(float(c["kf"]["kp"]["angle"][i]) - float(c["f"]["kp"]["angle"][j])) % 360 for j, i in enumerate(a) if i >= 0]
    assert sorted(set(int(round(r / 30)) % 12 for r in rot(c0, a0))) == [0, 3, 6] and sorted(set(int(round(r / 30)) % 12 for r in rot(c1, a1))) == [3, 6, 9]


def test_layout_cases_hold_what_their_names_say(cases, oracle):
    L = {k[7:]: v for k, v in cases.items() if k.startswith("layout_")}
    W = bc.W
    a, nm = bc.expect(oracle, L["one_node"])
    assert nm > 40 and len(bc.lost_first_choice(L["one_node"], a)) > 10            # one long chain with contention
    assert bc.expect(oracle, L["one_feature_per_node"])[1] > 60
    c = L["one_side_only"]
    a, nm = bc.expect(oracle, c)
    assert nm > 20 and (a[c["f"]["node"] >= 40] == -1).all() and not np.isin(np.flatnonzero(c["kf"]["node"] < 20), a).any()
    c = L["minus_one_and_zero"]
    a, nm = bc.expect(oracle, c)
    assert (c["kf"]["node"] == -1).sum() > 20 and (c["f"]["node"] == -1).sum() > 20 and nm > 5
    assert (a[c["f"]["node"] < 0] == -1).all() and (c["kf"]["node"][a[a >= 0]] == 0).all()
    for name in ("near_2_30", "max_id"):
        assert bc.expect(oracle, L[name])[1] > 20 and L[name]["kf"]["node"].min() >= (1 << 30) - 40
    assert (L["one_wave"]["kf"]["node"] % W == 0).all() and (L["one_wave"]["f"]["node"] % W == 0).all() and bc.expect(oracle, L["one_wave"])[1] > 20
    assert len(np.unique(L["all_waves"]["kf"]["node"] % W)) == W and bc.expect(oracle, L["all_waves"])[1] > 20


def test_bow_case_as_node_arrays(oracle):
    """from_bow_case's node arrays give back bow_case's own CSR lists"""
    rng = np.random.default_rng(7500)
    b = mc.bow_case(np.random.default_rng(7500), 60)
    c = bc.from_bow_case(rng, 60)
    pk, pf, ik, jf = bc.csr_from_nodes(c["kf"]["node"], c["f"]["node"])
    for got, want in ((pk, b["ptr1"]), (pf, b["ptr2"]), (ik, b["idx1"]), (jf, b["idx2"])):
        np.testing.assert_array_equal(got, want)
    assert bc.expect(oracle, c)[1] > 40


@pytest.mark.skipif(not os.path.exists(SLICES), reason="oracle/_ref/libref_slices.so was not built (the reference tree is absent)")
def test_reference_agrees_on_every_case(cases, oracle):
    R = C.CDLL(SLICES)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for name, c in cases.items():
        for ori in (c["ori"], False):
            cc = dict(c, ori=ori)
            want, nwant = bc.expect(oracle, cc)
            kf, f = c["kf"], c["f"]
            kn, fn = bc.ref_nodes(c)
            nkf, nf = len(kf["kp"]), len(f["kp"])
            out = np.full(max(nf, 1), -7, np.int32)
            valid = np.ascontiguousarray(kf["valid"], np.uint8)
            nr = R.ref_search_by_bow(p(np.ascontiguousarray(kf["kp"])), p(kf["desc"]), nkf, p(kn), p(valid), p(np.ascontiguousarray(f["kp"])), p(f["desc"]), nf, p(fn),
                                     C.c_float(c["nnratio"]), int(ori), p(out))
            np.testing.assert_array_equal(out[:nf], want, err_msg=name)
            assert nr == nwant, (name, ori, nr, nwant)
