"""GPU parity of the matchers at the sizes where csrc/match.hip picks another kernel, LDS layout or grid, and of the ordered
commit's re-scan.  Synthetic inputs (tests/match_cases.py; their preconditions are checked without a GPU in test_match_cases_cpu.py),
every comparison bit-exact against the oracle.

case -> branch
  test_proj_clusters[600]              k_proj_topk + k_proj_commit, features in LDS (re-scan through proj_candidate_lds)
  test_proj_clusters[2100] (+ uright)  k_proj_commit with the features in global memory (re-scan through proj_candidate, live occupancy)
  test_proj_clusters[6200]             the same with more than 48 KB of dynamic LDS (hipFuncSetAttribute)
  test_proj_clusters[8200]             n > 8192: the one-wave k_search_proj
  test_proj_clusters_frame             sslam_search_by_projection_frame at 2100 features
  test_proj_clusters_lines             keylines, features in global memory
  test_fuse_search_grid_cap*           k_fuse_search's stride loop behind min(nq, 8192)
  test_distinctive_grid_cap            k_distinctive behind min(nsets, 4096)
  test_search_by_bow*_grid_cap         k_search_bow behind min(nnodes, 4096), disjoint lists
  test_triangulation_grid_cap          k_tri_search behind min(total1, 8192)
  test_line_match_batch_dev            k_line_match: P2 padding, both medians, LM_MAX, n2 < 2, the 256-wide compaction rounds
  test_line_match_single_limits        sslam_line_match at LM_MAX, SSLAM_ERR_UNSUPPORTED, SSLAM_ERR_CAPACITY
  test_sfi_single_by_size[2300]        more than 150 KB for the speculative kernel: batch branch, k_search_init_lds (> 48 KB)
  test_sfi_single_by_size[2900]        k_search_init (global memory) without an env knob
  test_sfi_batch_by_cap[2100]          k_search_init_lds with ccap = 787 (> 48 KB) and the in-launch fallback of one pair
  test_sfi_batch_by_cap[2800]          k_search_init"""
import ctypes as C
import re
import numpy as np
import pytest
import match_cases as mc

pytestmark = pytest.mark.gpu

NC = 30          # clusters per projection case


def _rescans(capfd):
    err = capfd.readouterr().err
    m = re.findall(r"proj stats: .* re-scans (\d+)", err)
    assert len(m) == 1, err
    return int(m[0])


# ---- A. projection matcher by feature count, lists forced to run dry
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,nq_extra", mc.PROJ_SIZES)
def test_proj_clusters(fe, ctx, oracle, n, nq_extra, mode, monkeypatch, capfd):
    case = mc.cluster_case(np.random.default_rng(mc.proj_seed(n, 0, mode)), n, 0, C=NC, nq_extra=nq_extra)
    ratio, th, ori = mc.proj_params(0, mode)
    two_kernels = n <= 8192
    if two_kernels: monkeypatch.setenv("SSLAM_PROJ_STATS", "1")
    for ur in ((None, case["uright"]) if n == 2100 else (None,)):
        oa, on = oracle.search_by_projection(0, mode, case["feats"], case["desc"], case["q"], case["qdesc"], case["occ"], ur, ratio, th, ori)
        assert mc.clusters_taken_in_order(case, oa)
        capfd.readouterr()
        a, nm = ctx.search_by_projection(0, mode, case["feats"], case["desc"], case["q"], case["qdesc"], case["occ"], ur, ratio, th, ori)
        if two_kernels:
            r = _rescans(capfd)
            print("n %d mode %d uright %s: %d re-scans" % (n, mode, ur is not None, r))
            assert r >= (4 if mode == 1 else 5) * NC
        np.testing.assert_array_equal(a, oa)
        assert nm == on


@pytest.mark.parametrize("mode", [0, 1])
def test_proj_clusters_frame(fe, ctx, oracle, mode, monkeypatch, capfd):
    n, nq_extra = mc.PROJ_SIZES[1]
    case = mc.cluster_case(np.random.default_rng(mc.proj_seed(n, 0, mode)), n, 0, C=NC, nq_extra=nq_extra)
    ratio, th, ori = mc.proj_params(0, mode)
    monkeypatch.setenv("SSLAM_PROJ_STATS", "1")
    oa, on = oracle.search_by_projection(0, mode, case["feats"], case["desc"], case["q"], case["qdesc"], case["occ"], case["uright"], ratio, th, ori)
    assert mc.clusters_taken_in_order(case, oa)
    fr = ctx.frame_upload(0, case["feats"], case["desc"], case["uright"])
    capfd.readouterr()
    a, nm = fr.search_by_projection(mode, case["q"], case["qdesc"], case["occ"], ratio, th, ori)
    assert _rescans(capfd) >= (4 if mode == 1 else 5) * NC
    fr.close()
    np.testing.assert_array_equal(a, oa)
    assert nm == on


def test_proj_clusters_lines(fe, ctx, oracle, monkeypatch, capfd):
    n, nq_extra = mc.PROJ_SIZES[1]
    case = mc.cluster_case(np.random.default_rng(mc.proj_seed(n, 1, 0)), n, 1, C=NC, nq_extra=nq_extra)
    ratio, th, ori = mc.proj_params(1, 0)
    monkeypatch.setenv("SSLAM_PROJ_STATS", "1")
    oa, on = oracle.search_by_projection(1, 0, case["feats"], case["desc"], case["q"], case["qdesc"], case["occ"], None, ratio, th, ori)
    assert mc.clusters_taken_in_order(case, oa)
    capfd.readouterr()
    a, nm = ctx.search_by_projection(1, 0, case["feats"], case["desc"], case["q"], case["qdesc"], case["occ"], None, ratio, th, ori)
    assert _rescans(capfd) >= 5 * NC
    np.testing.assert_array_equal(a, oa)
    assert nm == on


# ---- B. grid caps with a stride loop behind them
@pytest.mark.parametrize("chi2", [0, 1])
def test_fuse_search_grid_cap(fe, ctx, oracle, chi2):
    c = mc.fuse_case(np.random.default_rng(8200 + chi2), 0, 300, 8200 + 37)
    sc = (1.2 ** np.arange(8)).astype(np.float32); inv_sigma2 = (1.0 / (sc * sc)).astype(np.float32)
    oi, od = oracle.fuse_search(0, chi2, c["feats"], c["desc"], c["q"], c["qdesc"], c["uright"], inv_sigma2)
    assert (oi >= 0).sum() >= 1000 and (oi[8192:] >= 0).any()
    kf = ctx.frame_upload(0, c["feats"], c["desc"], c["uright"])
    bi, bd = kf.fuse_search(c["q"], c["qdesc"], chi2, inv_sigma2 if chi2 else None)
    kf.close()
    np.testing.assert_array_equal(bi, oi); np.testing.assert_array_equal(bd, od)


def test_fuse_search_grid_cap_lines(fe, ctx, oracle):
    c = mc.fuse_case(np.random.default_rng(8205), 1, 200, 8200 + 5)
    oi, od = oracle.fuse_search(1, 0, c["feats"], c["desc"], c["q"], c["qdesc"])
    assert (oi >= 0).sum() >= 1000 and (oi[8192:] >= 0).any()
    kf = ctx.frame_upload(1, c["feats"], c["desc"])
    bi, bd = kf.fuse_search(c["q"], c["qdesc"], 0)
    kf.close()
    np.testing.assert_array_equal(bi, oi); np.testing.assert_array_equal(bd, od)


def test_distinctive_grid_cap(ctx, oracle):
    desc, ptr = mc.distinctive_case(np.random.default_rng(4115), 4096 + 19)
    want = oracle.distinctive(desc, ptr)
    assert (np.diff(ptr)[4096:] > 0).all() and (want[4096:] >= 0).all() and (want[4096:] > 0).any()
    got = ctx.distinctive_descriptors(desc, ptr)
    np.testing.assert_array_equal(got, want)


@pytest.fixture(scope="module")
def bow():
    return mc.bow_case(np.random.default_rng(mc.BOW_SEED), mc.BOW_NODES)


def test_search_by_bow_grid_cap(fe, ctx, oracle, bow):
    c = bow
    valid = (np.random.default_rng(1).random(len(c["kp1"])) < 0.9).astype(np.uint8)
    args = (c["kp1"], c["d1"], valid, c["kp2"], c["d2"], c["ptr1"], c["ptr2"], c["idx1"], c["idx2"], 0.9, True)
    oa, on = oracle.search_by_bow(*args)
    assert on > 1000 and (c["node_of_2"][oa >= 0] >= 4096).any()
    a, n = ctx.search_by_bow(*args)
    np.testing.assert_array_equal(a, oa)
    assert n == on


def test_search_by_bow_keyframes_grid_cap(fe, ctx, oracle, bow):
    c = bow
    rng = np.random.default_rng(2)
    v1 = (rng.random(len(c["kp1"])) < 0.9).astype(np.uint8); v2 = (rng.random(len(c["kp2"])) < 0.9).astype(np.uint8)
    args = (c["kp1"], c["d1"], v1, c["kp2"], c["d2"], v2, c["ptr1"], c["ptr2"], c["idx1"], c["idx2"], 0.8, True)
    om, on = oracle.search_by_bow_keyframes(*args)
    assert on > 1000 and (c["node_of_2"][om[om >= 0]] >= 4096).any()
    m, n = ctx.search_by_bow_keyframes(*args)
    np.testing.assert_array_equal(m, om)
    assert n == on


def test_triangulation_grid_cap(fe, ctx, oracle, bow):
    c = bow
    rng = np.random.default_rng(3)
    n1, n2 = len(c["kp1"]), len(c["kp2"])
    assert c["ptr1"][-1] == 8192 + 100                                           # total1: every keyframe-1 feature is filed
    sc = oracle.orb_params()[0].astype(np.float32); sg = (sc * sc).astype(np.float32)
    free1 = (rng.random(n1) < 0.9).astype(np.uint8); free2 = (rng.random(n2) < 0.9).astype(np.uint8)
    ur1 = np.where(rng.random(n1) < 0.3, c["kp1"]["x"] - 5, -1).astype(np.float32); ur2 = np.where(rng.random(n2) < 0.3, c["kp2"]["x"] - 5, -1).astype(np.float32)
    ex, ey = mc.TRI_EPIPOLE
    F12 = mc.tri_F12()
    om, on = oracle.search_for_triangulation(c["kp1"], c["d1"], ur1, free1, c["kp2"], c["d2"], ur2, free2, c["ptr1"], c["ptr2"], c["idx1"], c["idx2"], F12, ex, ey, sc, sg, False, True)
    assert on > 200 and (om[c["idx1"][8192:]] >= 0).any()
    f1 = ctx.frame_upload(0, c["kp1"], c["d1"], ur1); f2 = ctx.frame_upload(0, c["kp2"], c["d2"], ur2)
    m, n = f1.search_for_triangulation(f2, free1, free2, c["ptr1"], c["ptr2"], c["idx1"], c["idx2"], F12, ex, ey, sc, sg, False, True)
    f1.close(); f2.close()
    np.testing.assert_array_equal(m, om)
    assert n == on


# ---- C. line matcher
@pytest.fixture(scope="module")
def line_batch():
    return mc.line_batch_case(np.random.default_rng(1100), 1100)


@pytest.mark.parametrize("gate_scale,ratio_mode", [(0.5, 0), (0.1, 0), (0.5, 1)])
def test_line_match_batch_dev(fe, ctx, oracle, line_batch, gate_scale, ratio_mode):
    import torch
    cap = 1100
    l1, l2, n1, n2 = line_batch
    P = len(n1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dn1, dn2 = t(l1), t(l2), t(n1), t(n2)
    pairs = torch.full((P, cap, 2), -7, dtype=torch.int32, device="cuda"); npairs = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    _p = lambda x: C.c_void_p(x.data_ptr())
    torch.cuda.synchronize()
    rc = fe.lib().sslam_line_match_batch_dev(ctx.h, _p(d1), _p(dn1), _p(d2), _p(dn2), cap, P, C.c_double(gate_scale), ratio_mode, _p(pairs), _p(npairs), None)
    assert rc == 0, fe.lib().sslam_last_error()
    ctx.synchronize()
    pairs = pairs.cpu().numpy(); npairs = npairs.cpu().numpy()
    found = 0
    for p, (a, b) in enumerate(mc.LINE_BATCH_COUNTS):
        if a > 1024 or a == 0 or b < 2:
            assert npairs[p] == 0, (p, a, b, npairs[p])
        else:
            op, _, _ = oracle.line_match(l1[p, :a], l2[p, :b], gate_scale, ratio_mode)
            assert npairs[p] == len(op), (p, a, b, npairs[p], len(op))
            np.testing.assert_array_equal(pairs[p, :npairs[p]], op, err_msg="pair %d (%d x %d)" % (p, a, b))
            found += len(op)
        assert (pairs[p, npairs[p]:] == -7).all(), (p, a, b)                     # nothing written past the pairs
    assert found > 400


@pytest.mark.parametrize("n1", [1023, 1024])
def test_line_match_single_at_limit(ctx, oracle, n1):
    rng = np.random.default_rng(n1)
    q, t = mc.line_descriptors(rng, n1, 700, 0)
    pairs, mad, mad12 = ctx.line_match(q, t, 0.5, False)
    opairs, omad, omad12 = oracle.line_match(q, t, 0.5, False)
    assert len(opairs) > 100
    np.testing.assert_array_equal(pairs, opairs)
    assert mad == omad and mad12 == omad12


def test_line_match_single_limits(fe, ctx, oracle):
    rng = np.random.default_rng(1025)
    q, t = mc.line_descriptors(rng, 1025, 700, 0)
    with pytest.raises(fe.SslamError) as e:
        ctx.line_match(q, t, 0.5, False)
    assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED
    q, t = mc.line_descriptors(rng, 300, 300, 0)
    opairs, _, _ = oracle.line_match(q, t, 0.5, False)
    assert len(opairs) >= 2
    out = np.full((1, 2), -7, np.int32); n = C.c_int(-7)
    rc = fe.lib().sslam_line_match(ctx.h, C.c_void_p(q.ctypes.data), 300, C.c_void_p(t.ctypes.data), 300, C.c_double(0.5), 0, C.c_void_p(out.ctypes.data), 1, C.byref(n), None, None)
    assert rc == fe.SSLAM_ERR_CAPACITY and n.value == len(opairs)
    assert (out == -7).all()                                                     # nothing copied into a buffer that is too small


# ---- D. SearchForInitialization by row capacity
@pytest.mark.parametrize("n,lvl0", [(2300, 0.33), (2900, 0.33)])
def test_sfi_single_by_size(fe, ctx, oracle, n, lvl0):
    kp1, d1, kp2, d2 = mc.sfi_pair(np.random.default_rng(n), n, n, lvl0)
    if n == 2300:          # the LDS body of the batch branch holds 3/8 of the rows in level-0 features: this pair must fit
        assert 64 + n * 17 * 4 > 150 * 1024 and max((kp1["octave"] == 0).sum(), (kp2["octave"] == 0).sum()) <= n * 3 // 8 and 64 + (n * 3 // 8) * 64 > 48 * 1024
    else:
        assert 64 + (n * 3 // 8) * 64 > 64 * 1024
    pm = np.stack([kp1["x"], kp1["y"]], axis=1).astype(np.float32)
    om12, opm, on = oracle.search_for_initialization(kp1, d1, kp2, d2, pm, 100, 0.9, True)
    assert on > 300
    m12, pmo, nm = ctx.search_for_initialization(kp1, d1, kp2, d2, pm, 100, 0.9, True)
    np.testing.assert_array_equal(m12, om12); np.testing.assert_array_equal(pmo, opm)
    assert nm == on


@pytest.mark.parametrize("cap", [2100, 2800])
def test_sfi_batch_by_cap(fe, ctx, oracle, cap):
    import torch
    rng = np.random.default_rng(cap)
    P = 9
    ccap = cap * 3 // 8
    assert (64 + ccap * 64 > 48 * 1024) if cap == 2100 else (64 + ccap * 64 > 64 * 1024)
    kp1 = np.zeros((P, cap), fe.KP_DTYPE); kp2 = np.zeros((P, cap), fe.KP_DTYPE)
    d1 = mc.rand_desc(rng, P * cap).reshape(P, cap, 32); d2 = mc.rand_desc(rng, P * cap).reshape(P, cap, 32)      # junk past the counts
    kp1["x"] = 100; kp1["y"] = 100; kp2["x"] = 100; kp2["y"] = 100
    n1 = np.zeros(P, np.int32); n2 = np.zeros(P, np.int32)
    for p in range(P):
        a, b, lvl0 = int(rng.integers(40, 81)), int(rng.integers(40, 81)), 0.6
        if p == 1: a, b, lvl0 = cap, cap, 0.3                  # rows full, level-0 features fit the LDS capacity
        if p == 4: a = b = 0                                    # an empty pair
        if p == 6: a, b, lvl0 = cap - 300, cap - 450, 0.9      # more level-0 features than ccap: the global-memory body inside the same launch
        kp1[p, :a], d1[p, :a], kp2[p, :b], d2[p, :b] = mc.sfi_pair(rng, a, b, lvl0)
        n1[p], n2[p] = a, b
    assert (kp2[1, :n2[1]]["octave"] == 0).sum() <= ccap and (kp1[1, :n1[1]]["octave"] == 0).sum() <= ccap and (kp2[6, :n2[6]]["octave"] == 0).sum() > ccap
    pm = np.stack([kp1["x"], kp1["y"]], axis=2).astype(np.float32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    g = dict(kp1=t(kp1.view(np.uint8)), d1=t(d1), n1=t(n1), kp2=t(kp2.view(np.uint8)), d2=t(d2), n2=t(n2), pm=t(pm))
    m12 = torch.full((P, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    _p = lambda x: C.c_void_p(x.data_ptr())
    bounds = (C.c_float * 4)(0.0, 640.0, 0.0, 480.0)
    torch.cuda.synchronize()
    rc = fe.lib().sslam_orb_search_for_initialization_batch_dev(ctx.h, _p(g["kp1"]), _p(g["d1"]), _p(g["n1"]), _p(g["kp2"]), _p(g["d2"]), _p(g["n2"]), cap, P, _p(g["pm"]), _p(m12), _p(nm),
                                                                100, C.c_float(0.9), 1, bounds, C.c_void_p(0))
    assert rc == 0, fe.lib().sslam_last_error()
    ctx.synchronize()
    m12 = m12.cpu().numpy(); nm = nm.cpu().numpy(); pmo = g["pm"].cpu().numpy()
    total = 0
    for p in range(P):
        a, b = int(n1[p]), int(n2[p])
        om12, opm, on = oracle.search_for_initialization(kp1[p, :a], d1[p, :a], kp2[p, :b], d2[p, :b], pm[p, :a], 100, 0.9, True)
        assert nm[p] == on, (p, nm[p], on)
        np.testing.assert_array_equal(m12[p, :a], om12, err_msg="pair %d" % p); np.testing.assert_array_equal(pmo[p, :a], opm, err_msg="pair %d" % p)
        assert (m12[p, a:] == -7).all()
        total += on
    assert total > 300
