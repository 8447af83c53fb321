"""The rotation-consistency check of every matcher that has one, on the cases of tests/rot_cases.py (histograms on the 10 % boundary, ties, the two
wraps, a rotation exactly on a bin boundary; tests/test_rot_cases_cpu.py shows without a GPU that the oracle prunes what each case names).  Every
result -- assignment arrays and counts -- bit-exact against the oracle, check on.

entry point -> kernel whose rotation check runs
  test_sfi_single                sslam_orb_search_for_initialization: k_search_init_spec
  test_sfi_batch[2100]           ..._batch_dev, nine pairs: k_search_init_lds
  test_sfi_batch[2800]           ..._batch_dev, nine pairs: k_search_init
  test_proj_single               sslam_search_by_projection mode 1: k_proj_topk + k_proj_commit
  test_proj_single_one_wave      the same with 8200 features: k_search_proj
  test_proj_batch                sslam_search_by_projection_batch_dev: k_proj_commit_batch
  test_bow_single                sslam_orb_search_by_bow, sslam_orb_search_by_bow_keyframes: k_search_bow + k_rot_finish
  test_bow_batch[1638 / 1639]    sslam_orb_search_by_bow_batch_dev, frame side in LDS / in global memory: k_search_bow_batch
  test_triangulation             sslam_orb_search_for_triangulation: k_tri_search + k_rot_finish"""
import ctypes as C
import os, subprocess
import numpy as np
import pytest
import torch
import bow_batch_cases as bc
import match_cases as mc
import rot_cases as rc
import test_bow_batch_gpu as bb          # Call / check: one batch call on packed device buffers
import test_proj_batch_gpu as pb

pytestmark = pytest.mark.gpu

NAMES = list(rc.SPECS)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(line) -> what csrc/match_plan.h itself decides for the sizes of a test (tests/sim/match_plan_dump.cpp, built once): the kernel a case
    reaches is asked of the rule the library uses, not re-derived here"""
    exe = str(tmp_path_factory.mktemp("rot_plan") / "match_plan_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(HERE, "sim", "match_plan_dump.cpp"), "-o", exe])
    return lambda line: subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True, timeout=60).stdout.split()


@pytest.fixture(scope="module")
def cases():
    return rc.all_cases()


@pytest.fixture(scope="module")
def refs(cases, oracle):
    """name -> the oracle's answers, computed once: sfi (m12, prevMatched, n), proj / bow (assigned, n), bowkf / tri (m12, n)"""
    sc = oracle.orb_params()[0].astype(np.float32); sg = (sc * sc).astype(np.float32)
    ex, ey = mc.TRI_EPIPOLE
    out = {}
    for name, c in cases.items():
        n = len(c["kp1"])
        pk, pf, ik, jf = bc.csr_from_nodes(c["node1"], c["node2"])
        ones = np.ones(n, np.uint8); ur = np.full(n, -1, np.float32)
        r = dict(csr=(pk, pf, ik, jf), sc=sc, sg=sg)
        r["sfi"] = oracle.search_for_initialization(c["kp1"], c["d1"], c["kp2"], c["d2"], rc.prev_matched(c), 100, 0.9, True)
        r["proj"] = oracle.search_by_projection(0, 1, c["kp2"], c["d2"], rc.queries(c), c["d1"], None, None, 0.9, 100, True)
        r["bow"] = bc.expect(oracle, rc.bow_pair(c))
        r["bowkf"] = oracle.search_by_bow_keyframes(c["kp1"], c["d1"], ones, c["kp2"], c["d2"], ones, pk, pf, ik, jf, 0.8, True)
        r["tri"] = oracle.search_for_triangulation(c["kp1"], c["d1"], ur, ones, c["kp2"], c["d2"], ur, ones, pk, pf, ik, jf, mc.tri_F12(), ex, ey, sc, sg, False, True)
        kept = int((~c["pruned"]).sum())          # the oracle prunes what the case names (test_rot_cases_cpu.py): no comparison below is vacuous
        assert [r[k][-1] for k in ("sfi", "proj", "bow", "bowkf", "tri")] == [kept] * 5 and kept < len(c["i1"])
        out[name] = r
    return out


# ---- SearchForInitialization
@pytest.mark.parametrize("name", NAMES)
def test_sfi_single(ctx, cases, refs, plan, name):
    c = cases[name]
    assert plan("sfi %d 1" % len(c["kp1"]))[0] == "speculative"
    m12, pm, n = ctx.search_for_initialization(c["kp1"], c["d1"], c["kp2"], c["d2"], rc.prev_matched(c), 100, 0.9, True)
    om12, opm, on = refs[name]["sfi"]
    np.testing.assert_array_equal(m12, om12); np.testing.assert_array_equal(pm, opm); assert n == on


@pytest.mark.parametrize("cap", [2100, 2800])
def test_sfi_batch(fe, ctx, cases, refs, plan, cap):
    """the row capacities of test_match_sizes_gpu.py::test_sfi_batch_by_cap: nine pairs of 2100 rows take the LDS form (ccap = 787), of 2800 the
    global-memory form; the cases sit in six of the pairs, the other three are empty"""
    P = 9
    form, _, ccap = plan("sfi %d %d" % (cap, P))
    assert (form, int(ccap)) == (("lds-batch", 787) if cap == 2100 else ("global", 0))
    assert max(int((c[k]["octave"] == 0).sum()) for c in cases.values() for k in ("kp1", "kp2")) <= 787          # no pair leaves the LDS body for the global-memory one
    rows = dict(zip(NAMES, (0, 2, 3, 5, 6, 8)))
    rng = np.random.default_rng(cap)
    kp1 = np.zeros((P, cap), fe.KP_DTYPE); kp2 = np.zeros((P, cap), fe.KP_DTYPE)
    d1 = mc.rand_desc(rng, P * cap).reshape(P, cap, 32); d2 = mc.rand_desc(rng, P * cap).reshape(P, cap, 32)      # junk past the counts
    pm = np.zeros((P, cap, 2), np.float32); n1 = np.zeros(P, np.int32); n2 = np.zeros(P, np.int32)
    for name, p in rows.items():
        c = cases[name]; n = len(c["kp1"])
        kp1[p, :n] = c["kp1"]; d1[p, :n] = c["d1"]; kp2[p, :n] = c["kp2"]; d2[p, :n] = c["d2"]; pm[p, :n] = rc.prev_matched(c); n1[p] = n2[p] = n
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    g = dict(kp1=t(kp1.view(np.uint8)), d1=t(d1), n1=t(n1), kp2=t(kp2.view(np.uint8)), d2=t(d2), n2=t(n2), pm=t(pm))
    m12 = torch.full((P, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    _p = lambda x: C.c_void_p(x.data_ptr())
    bounds = (C.c_float * 4)(0.0, 640.0, 0.0, 480.0)
    torch.cuda.synchronize()
    rcode = fe.lib().sslam_orb_search_for_initialization_batch_dev(ctx.h, _p(g["kp1"]), _p(g["d1"]), _p(g["n1"]), _p(g["kp2"]), _p(g["d2"]), _p(g["n2"]), cap, P, _p(g["pm"]),
                                                                   _p(m12), _p(nm), 100, C.c_float(0.9), 1, bounds, C.c_void_p(0))
    assert rcode == 0, fe.lib().sslam_last_error()
    ctx.synchronize()
    m12 = m12.cpu().numpy(); nm = nm.cpu().numpy(); pmo = g["pm"].cpu().numpy()
    for name, p in rows.items():
        n = len(cases[name]["kp1"])
        om12, opm, on = refs[name]["sfi"]
        np.testing.assert_array_equal(m12[p, :n], om12, err_msg=name); np.testing.assert_array_equal(pmo[p, :n], opm, err_msg=name)
        assert nm[p] == on, (name, nm[p], on)
        assert (m12[p, n:] == -7).all()
    empty = sorted(set(range(P)) - set(rows.values()))
    assert (nm[empty] == 0).all() and (m12[empty] == -7).all()


# ---- SearchByProjection, mode 1
@pytest.mark.parametrize("name", NAMES)
def test_proj_single(ctx, cases, refs, plan, name):
    c = cases[name]
    assert plan("proj %d %d" % (len(c["kp2"]), len(c["kp1"])))[0] == "two-kernel"
    a, n = ctx.search_by_projection(0, 1, c["kp2"], c["d2"], rc.queries(c), c["d1"], None, None, 0.9, 100, True)
    oa, on = refs[name]["proj"]
    np.testing.assert_array_equal(a, oa); assert n == on and (oa == -2).sum() == cases[name]["pruned"].sum()


@pytest.mark.parametrize("name", NAMES)
def test_proj_single_one_wave(fe, ctx, oracle, cases, plan, name):
    """more than 8192 features: only the rows of the case are real, the rest lie outside the image and every window"""
    n = 8200
    c = cases[name]
    assert plan("proj %d %d" % (n, len(c["kp1"])))[0] == "one-wave"
    rng = np.random.default_rng(8200 + NAMES.index(name))
    rows = np.sort(rng.choice(n, len(c["kp2"]), replace=False))
    feats = np.zeros(n, fe.KP_DTYPE); feats["x"] = -1000; feats["y"] = -1000; feats["size"] = 31
    desc = mc.rand_desc(rng, n)
    feats[rows] = c["kp2"]; desc[rows] = c["d2"]
    q = rc.queries(c)
    oa, on = oracle.search_by_projection(0, 1, feats, desc, q, c["d1"], None, None, 0.9, 100, True)
    want, nwant = rc.want_21(c, True, gone=-2)
    assert on == nwant and np.array_equal(oa[rows], want) and (np.delete(oa, rows) == -1).all()
    a, nm = ctx.search_by_projection(0, 1, feats, desc, q, c["d1"], None, None, 0.9, 100, True)
    np.testing.assert_array_equal(a, oa); assert nm == on


def test_proj_batch(ctx, cases, refs):
    cap = qcap = 64
    frames = [dict(feats=c["kp2"], desc=c["d2"], occ=np.zeros(len(c["kp2"]), np.uint8), uright=None, q=rc.queries(c), qdesc=c["d1"]) for c in cases.values()]
    assert pb.params(0, 1) == (0.9, 100, True)
    call = pb.Call(pb.pack(frames, 0, cap, qcap), 0, 1, cap, qcap, with_occ=False).launch(ctx)
    ctx.synchronize()
    pb.check(call.results(), frames, [refs[name]["proj"] for name in cases], cap)


# ---- SearchByBoW
@pytest.mark.parametrize("name", NAMES)
def test_bow_single(ctx, cases, refs, name):
    c = cases[name]
    ones = np.ones(len(c["kp1"]), np.uint8)
    pk, pf, ik, jf = refs[name]["csr"]
    a, n = ctx.search_by_bow(c["kp1"], c["d1"], ones, c["kp2"], c["d2"], pk, pf, ik, jf, 0.9, True)
    np.testing.assert_array_equal(a, refs[name]["bow"][0]); assert n == refs[name]["bow"][1]
    m, n = ctx.search_by_bow_keyframes(c["kp1"], c["d1"], ones, c["kp2"], c["d2"], ones, pk, pf, ik, jf, 0.8, True)
    np.testing.assert_array_equal(m, refs[name]["bowkf"][0]); assert n == refs[name]["bowkf"][1]


@pytest.mark.parametrize("cap", [bc.LDS_CAP, bc.LDS_CAP + 1])
def test_bow_batch(ctx, cases, refs, cap):
    """both sides of the LDS bound of test_bow_batch_gpu.py::test_size_bound: 1638 rows is the last frame capacity kept in LDS"""
    assert bc.ROW_BYTES * bc.LDS_CAP <= bc.LDS_MAX < bc.ROW_BYTES * (bc.LDS_CAP + 1)
    pairs = [rc.bow_pair(c) for c in cases.values()]
    call = bb.Call([x["kf"] for x in pairs], [x["f"] for x in pairs], cap + 3, cap).launch(ctx)
    ctx.synchronize()
    bb.check(call.results(), [refs[name]["bow"] for name in cases], [len(c["kp2"]) for c in cases.values()])


# ---- SearchForTriangulation
@pytest.mark.parametrize("name", NAMES)
def test_triangulation(ctx, cases, refs, name):
    c = cases[name]; r = refs[name]
    ones = np.ones(len(c["kp1"]), np.uint8)
    pk, pf, ik, jf = r["csr"]
    ex, ey = mc.TRI_EPIPOLE
    f1 = ctx.frame_upload(0, c["kp1"], c["d1"]); f2 = ctx.frame_upload(0, c["kp2"], c["d2"])
    m, n = f1.search_for_triangulation(f2, ones, ones, pk, pf, ik, jf, mc.tri_F12(), ex, ey, r["sc"], r["sg"], False, True)
    f1.close(); f2.close()
    np.testing.assert_array_equal(m, r["tri"][0]); assert n == r["tri"][1]
