"""The inputs of tests/test_rot_gpu.py reach what they are meant to reach, shown on the CPU with the oracle alone (tests/rot_cases.py): without the
rotation check every forced pair is matched and nothing else, the rotation bins of those matches form the histogram the case names, and with the
check the oracle removes exactly the groups the case names -- in every matcher that has the check.  A GPU pass on these cases cannot be vacuous."""
import numpy as np
import pytest
import bow_batch_cases as bc
import match_cases as mc
import rot_cases as rc


@pytest.fixture(scope="module")
def cases():
    return rc.all_cases()


def test_bin_arithmetic():
    f = np.float32
    assert f(15) * (f(1) / f(30)) == f(0.5)                                         # the `half` case sits on the boundary exactly
    assert rc.rot_bin(15, 0) == 1 and rc.rot_bin(14.75, 0) == 0                      # roundf: half away from zero
    assert rc.rot_bin(0, 15) == 12 and rc.rot_bin(359.75, 0) == 12                   # [345, 360) is bin 12, not HISTO_LENGTH
    assert rc.rot_bin(885, 0) == 0 and rc.rot_bin(884.75, 0) == 29 and rc.rot_bin(1274.5, 359.75) == 0      # bin 30 wraps to 0
    assert f(0.1) * f(30) == f(3)                                                    # `boundary`: 3 < 0.1f * 30 is false in float as well


@pytest.mark.parametrize("name", list(rc.SPECS))
def test_cases_build_their_histograms(cases, oracle, name):
    c = cases[name]
    groups, hist, pruned_groups = rc.SPECS[name]
    M = len(c["i1"]); npruned = sum(groups[g][0] for g in pruned_groups)
    assert 40 <= len(c["kp1"]) == len(c["kp2"]) <= 60 and M == sum(hist.values()) and int(c["pruned"].sum()) == npruned > 0
    pm = rc.prev_matched(c)
    # SearchForInitialization without the check: the forced pairs and nothing else; their rotation bins are the histogram
    m12, _, n = oracle.search_for_initialization(c["kp1"], c["d1"], c["kp2"], c["d2"], pm, 100, 0.9, False)
    np.testing.assert_array_equal(m12, rc.want_12(c, False)[0]); assert n == M
    i1 = np.flatnonzero(m12 >= 0)
    bins = rc.rot_bin(c["kp1"]["angle"][i1], c["kp2"]["angle"][m12[i1]])
    assert {int(b): int(k) for b, k in zip(*np.unique(bins, return_counts=True))} == hist
    # with the check: exactly the named groups go
    m12, pmo, n = oracle.search_for_initialization(c["kp1"], c["d1"], c["kp2"], c["d2"], pm, 100, 0.9, True)
    np.testing.assert_array_equal(m12, rc.want_12(c, True)[0]); assert n == M - npruned
    # the other matchers agree, check off and on
    q = rc.queries(c)
    b = rc.bow_pair(c)
    pk, pf, ik, jf = bc.csr_from_nodes(c["node1"], c["node2"])
    ones1 = np.ones(len(c["kp1"]), np.uint8); ones2 = np.ones(len(c["kp2"]), np.uint8); ur = np.full(len(c["kp1"]), -1, np.float32)
    sc = oracle.orb_params()[0].astype(np.float32); sg = (sc * sc).astype(np.float32)
    ex, ey = mc.TRI_EPIPOLE
    for ori in (False, True):
        a, n = oracle.search_by_projection(0, 1, c["kp2"], c["d2"], q, c["d1"], None, None, 0.9, 100, ori)
        np.testing.assert_array_equal(a, rc.want_21(c, ori, gone=-2)[0]); assert n == rc.want_21(c, ori)[1]
        a, n = bc.expect(oracle, dict(b, ori=ori))
        np.testing.assert_array_equal(a, rc.want_21(c, ori)[0]); assert n == rc.want_21(c, ori)[1]
        m, n = oracle.search_by_bow_keyframes(c["kp1"], c["d1"], ones1, c["kp2"], c["d2"], ones2, pk, pf, ik, jf, 0.8, ori)
        np.testing.assert_array_equal(m, rc.want_12(c, ori)[0]); assert n == rc.want_12(c, ori)[1]
        m, n = oracle.search_for_triangulation(c["kp1"], c["d1"], ur, ones1, c["kp2"], c["d2"], ur, ones2, pk, pf, ik, jf, mc.tri_F12(), ex, ey, sc, sg, False, ori)
        np.testing.assert_array_equal(m, rc.want_12(c, ori)[0]); assert n == rc.want_12(c, ori)[1]
