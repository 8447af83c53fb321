"""The preconditions of tests/test_match_sizes_gpu.py, from the generators (tests/match_cases.py) and the oracle alone: a case
that does not force the branch it is named after would pass on the device without testing anything."""
import numpy as np
import pytest
import match_cases as mc


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,nq_extra", mc.PROJ_SIZES)
def test_cluster_case_exhausts_the_lists(oracle, n, nq_extra, mode):
    """query j of every cluster takes feature j of that cluster (with and without the stereo gate): the j-th query then finds features
    0..j-1 of its static top-8 list taken, and from j = 8 (mode 1: best only) / j = 7 (mode 0: best and second) on the list is spent
    while 12 candidates exist"""
    case = mc.cluster_case(np.random.default_rng(mc.proj_seed(n, 0, mode)), n, 0, nq_extra=nq_extra)
    assert len(case["feats"]) == n and case["cfeat"].shape == (30, mc.CLUSTER) and len(np.unique(case["cfeat"])) == 30 * mc.CLUSTER
    assert not case["occ"][case["cfeat"]].any() and 0.05 < case["occ"].sum() / (n - 30 * mc.CLUSTER) < 0.15
    ratio, th, ori = mc.proj_params(0, mode)
    for ur in (None, case["uright"]):
        a, nm = oracle.search_by_projection(0, mode, case["feats"], case["desc"], case["q"], case["qdesc"], case["occ"], ur, ratio, th, ori)
        assert mc.clusters_taken_in_order(case, a)
        extra = np.setdiff1d(np.arange(len(case["q"])), case["cquery"].ravel())
        assert np.isin(a[a >= 0], extra).sum() > len(extra) // 5          # the ordinary queries match as well
        assert nm >= 30 * mc.CLUSTER + len(extra) // 5
    assert (case["q"]["valid"] == 0).sum() > 0 and (case["q"]["obs_positive"] == 0).sum() > 0
    if mode == 1: assert (a == -2).sum() > 0                              # some ordinary matches fall to the rotation check


def test_cluster_case_lines(oracle):
    n, nq_extra = mc.PROJ_SIZES[1]
    case = mc.cluster_case(np.random.default_rng(mc.proj_seed(n, 1, 0)), n, 1, nq_extra=nq_extra)
    ratio, th, ori = mc.proj_params(1, 0)
    a, nm = oracle.search_by_projection(1, 0, case["feats"], case["desc"], case["q"], case["qdesc"], case["occ"], None, ratio, th, ori)
    assert mc.clusters_taken_in_order(case, a)
    assert nm >= (a >= 0).sum() > 30 * mc.CLUSTER + 50          # (a query without observations does not block its line: it can be taken again)


def test_line_batch_case_shapes():
    l1, l2, n1, n2 = mc.line_batch_case(np.random.default_rng(1), 1100)
    assert l1.shape == l2.shape == (17, 1100, 32) and n1.max() == 1100 and (n1 > 1024).sum() == 2 and (n2 < 2).sum() == 2 and (n1 == 0).sum() == 1
    q, t = mc.line_descriptors(np.random.default_rng(2), 300, 200, 1)
    assert len(np.unique(np.concatenate([q, t]), axis=0)) == 4


def test_bow_case_lists(oracle):
    """disjoint lists (every feature under exactly one node), 8192 + 100 filed features per frame, and matches behind both grid caps"""
    c = mc.bow_case(np.random.default_rng(mc.BOW_SEED), mc.BOW_NODES)
    n1, n2 = len(c["kp1"]), len(c["kp2"])
    assert n1 == n2 == 2 * mc.BOW_NODES == 8192 + 100 and c["ptr1"][-1] == n1 and c["ptr2"][-1] == n2
    assert sorted(c["idx1"].tolist()) == list(range(n1)) and sorted(c["idx2"].tolist()) == list(range(n2))
    cnt1 = np.diff(c["ptr1"]); cnt2 = np.diff(c["ptr2"])
    assert cnt1.min() == 1 and cnt1.max() == 3 and cnt2.min() == 1 and cnt2.max() == 3
    a, nm = oracle.search_by_bow(c["kp1"], c["d1"], np.ones(n1, np.uint8), c["kp2"], c["d2"], c["ptr1"], c["ptr2"], c["idx1"], c["idx2"], 0.9, True)
    assert nm > 1000 and (c["node_of_2"][a >= 0] >= 4096).any()
