"""GPU parity of sslam_two_view_reconstruct / sslam_two_view_reconstruct_batch_dev (the second half of Initializer::Initialize, reference src/Initializer.cc:143-152,
:499-782, :833-1171) with the host model of the same header: tests/reconstruct_sim.py runs csrc/reconstruct_math.h under g++.  Every comparison is bit for bit (a NaN equals
a NaN), and through the testing tap it covers EVERY hypothesis -- R, t, n, the selected cosine, and per match row the stage, the point and the cosine -- not only the winner.
The cases are tests/reconstruct_cases.py's (what each reaches is shown in tests/test_reconstruct_cases_cpu.py).

  test_single_call_and_every_hypothesis   every case through sslam_two_view_reconstruct and through sslam_testing_two_view_reconstruct
  test_batches                            every case as a pair that is not pair 0 of a batch (one launch per parameter triple: sigma, min_parallax and min_triangulated are
                                          the call's), with and without lines in one launch, ragged counts, on a side stream; 0xA5 behind every count and behind the last pair
  test_one_launch_of_70_pairs             70 mixed pairs in one launch on a side stream: F and H, failed and skipped pairs, with and without lines, ragged counts
  test_size_bounds                        a pair at cap 5120 / lcap 1024 runs and equals the model; cap 5121 and lcap 1025 are SSLAM_ERR_UNSUPPORTED with nothing written
  test_argument_errors                    every refused combination is SSLAM_ERR_INVALID and leaves the outputs alone
  test_chain                              synthetic scenes -> sslam_two_view_ransac_batch_dev -> this call with nothing copied to the host in between: a general scene takes the
                                          F path, a planar one the H path"""
import ctypes as C
import numpy as np
import pytest
import torch
import reconstruct_cases as rcases
import reconstruct_sim as sim

pytestmark = pytest.mark.gpu

FILL = 0xA5


def same(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def same_pose(got, want):
    return all(same(np.asarray(got[k]), np.asarray(want[k])) for k in got.dtype.names)


@pytest.fixture(scope="module")
def expected():
    return sim.run(list(rcases.all_cases()))


def keypoints(fe, xy, rng):
    kp = rng.integers(0, 256, (len(xy), fe.KP_DTYPE.itemsize), dtype=np.uint8).view(fe.KP_DTYPE).reshape(-1)
    kp["x"] = xy[:, 0]; kp["y"] = xy[:, 1]
    return kp


def keylines(fe, pts, n, rng):
    kl = rng.integers(0, 256, (n, fe.KL_DTYPE.itemsize), dtype=np.uint8).view(fe.KL_DTYPE).reshape(-1)
    if pts is not None:
        kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"] = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    return kl


def result_of(fe, c):
    r = np.zeros(1, fe.TWO_VIEW_RESULT_DTYPE)
    r["model"] = c["model"]; r["H21"] = c["H21"]; r["F21"] = c["F21"]; r["nmatches"] = int((c["m12"] >= 0).sum())
    return r


def line_args(fe, c, rng):
    return (keylines(fe, c["kl1"], len(c["fn1"]), rng), keylines(fe, None, len(c["fn2"]), rng), c["fn1"], c["fn2"], c["lp"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def check_outputs(name, want, pose, p3d, tri, lines=None):
    assert same_pose(pose, want["pose"]), (name, pose, want["pose"])
    assert same(p3d, want["p3d"]), name
    np.testing.assert_array_equal(tri, want["tri"], err_msg=name)
    if lines is not None:
        assert same(lines[0], want["line_s3d"]) and same(lines[1], want["line_e3d"]), name
        np.testing.assert_array_equal(lines[2], want["line_tri"], err_msg=name)


def test_single_call_and_every_hypothesis(fe, ctx, expected):
    rng = np.random.default_rng(1)
    T = fe.testing_lib()
    p = lambda a: None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)
    for c, want in zip(rcases.all_cases(), expected):
        kp1, kp2 = keypoints(fe, c["kp1"], rng), keypoints(fe, c["kp2"], rng)
        L = line_args(fe, c, rng) if sim.has_lines(c) else None
        out = ctx.two_view_reconstruct(kp1, kp2, c["m12"], result_of(fe, c), c["inliers"], c["K"], c["sigma"], c["min_parallax"], c["min_triangulated"], lines=L)
        check_outputs(c["name"], want, out[0], out[1], out[2], out[3:] if L else None)
        # the tap
        n1, n2 = len(kp1), len(kp2)
        rows = max(n1, n2, 1)
        nm = want["stage"].shape[1]
        pose = np.zeros(1, fe.TWO_VIEW_POSE_DTYPE); p3d = np.full((n1, 3), -9, np.float32); tri = np.full(n1, 9, np.uint8)
        hyp = np.full((8, 15), -9, np.float32); sel = np.full(8, -9, np.float32); stage = np.full((8, rows), -9, np.int32)
        prow = np.full((8, rows, 3), -9, np.float32); cosv = np.full((8, rows), -9, np.float32)
        m12 = np.ascontiguousarray(c["m12"], np.int32); inl = np.ascontiguousarray(c["inliers"], np.uint8); res = result_of(fe, c); Kf = np.ascontiguousarray(c["K"], np.float32)
        if L:
            kl1, kl2, f1, f2, lp = [np.ascontiguousarray(x) for x in L]
            nlp = len(lp)
            ls, le, lt, lerr = np.full((nlp, 3), -9, np.float32), np.full((nlp, 3), -9, np.float32), np.full(nlp, 9, np.uint8), np.full((nlp, 2), -9, np.float64)
            spare = np.zeros(2, np.int32)
            la = [p(kl1), len(kl1), p(kl2), len(kl2), p(f1), p(f2), C.c_void_p(lp.ctypes.data if nlp else spare.ctypes.data), nlp]
            lo = [p(ls), p(le), p(lt)]
        else:
            la, lo, lerr = [None, 0, None, 0, None, None, None, 0], [None, None, None], None
        rc = T.sslam_testing_two_view_reconstruct(ctx.h, p(kp1), n1, p(kp2), n2, p(m12), p(res), p(inl), p(Kf), C.c_float(c["sigma"]), C.c_float(c["min_parallax"]),
                                                  int(c["min_triangulated"]), *la, p(pose), p(p3d), p(tri), *lo, p(hyp), p(sel), p(stage), p(prow), p(cosv),
                                                  None if lerr is None else p(lerr))
        assert rc == 0, (c["name"], T.sslam_last_error())
        check_outputs(c["name"], want, pose[0], p3d, tri, (ls, le, lt) if L else None)
        assert same(hyp, want["hyp"]), (c["name"], hyp, want["hyp"])
        assert same(sel, want["sel"]), (c["name"], sel, want["sel"])
        np.testing.assert_array_equal(stage[:, :nm], want["stage"], err_msg=c["name"])
        assert same(prow[:, :nm], want["rows_p3d"]) and same(cosv[:, :nm], want["rows_cos"]), c["name"]
        assert (stage[:, nm:] == 0).all() and (prow[:, nm:] == 0).all() and (cosv[:, nm:] == 0).all(), c["name"]
        if L and len(L[4]):
            assert same(lerr, want["line_err"]), (c["name"], lerr, want["line_err"])


class Batch:
    """device inputs of one batch call (junk behind every count) and outputs filled with 0xA5, one pair more than the call may touch"""
    def __init__(self, fe, cases, cap, lcap, seed=5):
        rng = np.random.default_rng(seed)
        P = len(cases)
        self.fe, self.P, self.cap, self.lcap, self.cases = fe, P, cap, lcap, cases
        ks, ls = fe.KP_DTYPE.itemsize, fe.KL_DTYPE.itemsize
        kp1 = rng.integers(0, 256, (P, cap, ks), dtype=np.uint8).view(fe.KP_DTYPE).reshape(P, cap)
        kp2 = rng.integers(0, 256, (P, cap, ks), dtype=np.uint8).view(fe.KP_DTYPE).reshape(P, cap)
        m12 = rng.integers(-5, cap + 5, (P, cap)).astype(np.int32); inl = rng.integers(0, 4, (P, cap)).astype(np.uint8)
        res = np.zeros(P, fe.TWO_VIEW_RESULT_DTYPE); K = np.zeros((P, 4), np.float32)
        self.n1 = np.array([len(c["kp1"]) for c in cases], np.int32); self.n2 = np.array([len(c["kp2"]) for c in cases], np.int32)
        for p, c in enumerate(cases):
            kp1[p, :self.n1[p]] = keypoints(fe, c["kp1"], rng); kp2[p, :self.n2[p]] = keypoints(fe, c["kp2"], rng)
            m12[p, :self.n1[p]] = c["m12"]; inl[p, :self.n1[p]] = c["inliers"]; res[p] = result_of(fe, c)[0]; K[p] = c["K"]
        self.d = dict(kp1=dev(kp1), kp2=dev(kp2), n1=dev(self.n1), n2=dev(self.n2), m12=dev(m12), inl=dev(inl), res=dev(res), K=dev(K))
        full = lambda n: torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
        self.pose, self.p3d, self.tri = full((P + 1) * fe.TWO_VIEW_POSE_DTYPE.itemsize), full((P + 1) * cap * 12), full((P + 1) * cap)
        self.lines = None
        if lcap:
            L = lcap
            kl1 = rng.integers(0, 256, (P, L, ls), dtype=np.uint8).view(fe.KL_DTYPE).reshape(P, L)
            kl2 = rng.integers(0, 256, (P, L, ls), dtype=np.uint8).view(fe.KL_DTYPE).reshape(P, L)
            f1 = rng.standard_normal((P, L, 3)); f2 = rng.standard_normal((P, L, 3)); lp = rng.integers(-3, L + 3, (P, L, 2)).astype(np.int32)
            self.nl1, self.nl2, self.nlp = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
            for p, c in enumerate(cases):
                if sim.has_lines(c):
                    a, b, n = len(c["fn1"]), len(c["fn2"]), len(c["lp"])
                    self.nl1[p], self.nl2[p], self.nlp[p] = a, b, n
                    kl1[p, :a] = keylines(fe, c["kl1"], a, rng); f1[p, :a] = c["fn1"]; f2[p, :b] = c["fn2"]; lp[p, :n] = c["lp"]
            self.ls, self.le, self.lt = full((P + 1) * L * 12), full((P + 1) * L * 12), full((P + 1) * L)
            self.lines = [dev(kl1), dev(self.nl1), dev(kl2), dev(self.nl2), dev(f1), dev(f2), dev(lp), dev(self.nlp), self.ls, self.le, self.lt]
        torch.cuda.synchronize()

    def launch(self, ctx, sigma, min_parallax, min_triangulated, stream=None, cap=None, npairs=None, lcap=None, lines="own", **kw):
        d = dict(self.d); d.update(pose=self.pose, p3d=self.p3d, tri=self.tri); d.update(kw)
        ctx.two_view_reconstruct_batch_dev(d["kp1"], d["n1"], d["kp2"], d["n2"], self.cap if cap is None else cap, self.P if npairs is None else npairs, d["m12"], d["res"],
                                           d["inl"], d["K"], d["pose"], d["p3d"], d["tri"], sigma=sigma, min_parallax=min_parallax, min_triangulated=min_triangulated,
                                           lines=self.lines if lines == "own" else lines, lcap=self.lcap if lcap is None else lcap, stream=stream)
        return self

    def untouched(self):
        bufs = [self.pose, self.p3d, self.tri] + ([self.ls, self.le, self.lt] if self.lines else [])
        return all(bool((b == FILL).all().item()) for b in bufs)

    def check(self, expected):
        fe, P, cap = self.fe, self.P, self.cap
        pose = self.pose.cpu().numpy().view(fe.TWO_VIEW_POSE_DTYPE)
        p3d = self.p3d.cpu().numpy().view(np.float32).reshape(P + 1, cap, 3); tri = self.tri.cpu().numpy().reshape(P + 1, cap)
        assert (pose[P:].view(np.uint8) == FILL).all() and (p3d[P].view(np.uint8) == FILL).all() and (tri[P] == FILL).all()
        if self.lines:
            L = self.lcap
            ls = self.ls.cpu().numpy().view(np.float32).reshape(P + 1, L, 3); le = self.le.cpu().numpy().view(np.float32).reshape(P + 1, L, 3)
            lt = self.lt.cpu().numpy().reshape(P + 1, L)
            assert (ls[P].view(np.uint8) == FILL).all() and (le[P].view(np.uint8) == FILL).all() and (lt[P] == FILL).all()
        for p, (c, want) in enumerate(zip(self.cases, expected)):
            n1 = self.n1[p]
            check_outputs(c["name"], want, pose[p], p3d[p, :n1], tri[p, :n1])
            assert (p3d[p, n1:].view(np.uint8) == FILL).all() and (tri[p, n1:] == FILL).all(), c["name"]
            if self.lines:
                n = self.nlp[p]
                if sim.has_lines(c):
                    assert same(ls[p, :n], want["line_s3d"]) and same(le[p, :n], want["line_e3d"]), c["name"]
                    np.testing.assert_array_equal(lt[p, :n], want["line_tri"], err_msg=c["name"])
                assert (ls[p, n:].view(np.uint8) == FILL).all() and (le[p, n:].view(np.uint8) == FILL).all() and (lt[p, n:] == FILL).all(), c["name"]


def test_batches(fe, ctx, expected):
    """about 70 pairs over the launches: F and H, failed and skipped pairs, with and without lines, ragged counts; cap on both sides of the 48 KB opt-in of the dynamic LDS"""
    cases = rcases.all_cases()
    groups = {}
    for c, w in zip(cases, expected):
        groups.setdefault((float(c["sigma"]), float(c["min_parallax"]), int(c["min_triangulated"])), []).append((c, w))
    side = torch.cuda.Stream()
    total = 0
    for k, (key, items) in enumerate(sorted(groups.items(), key=lambda kv: -len(kv[1]))):
        items = [items[-1]] + items                    # pair 0 is a pair of its own: every case runs as a later pair
        cs, ws = [c for c, _ in items], [w for _, w in items]
        cap = max(max(len(c["kp1"]), len(c["kp2"])) for c in cs) + (0 if k % 2 else 3)
        lcap = max([max(len(c["fn1"]), len(c["fn2"]), len(c["lp"])) for c in cs if sim.has_lines(c)] + [0])
        if k == 0:
            cap = 1100                                  # 26 624 + 21 * 1100 bytes: beyond the opt-in; the small groups stay below it
        B = Batch(fe, cs, cap, lcap + (2 if lcap else 0), seed=10 + k)
        B.launch(ctx, *key, stream=side.cuda_stream if k % 2 == 0 else None)
        side.synchronize(); ctx.synchronize()
        B.check(ws)
        total += len(cs)
    assert total >= len(cases) + len(groups)


def test_one_launch_of_70_pairs(fe, ctx, expected):
    """ONE launch of 70 pairs under the default parameters (sigma 1, min_parallax 1, min_triangulated 50): the cases that take them, and scenes of ragged sizes beside them
    -- general and planar, with points beside the plane and without (no clear winner), too few matches (fails), model 0 (skipped), with 0 .. 12 line pairs and without lines"""
    cases = rcases.all_cases()
    cs = [c for c in cases if (float(c["sigma"]), float(c["min_parallax"]), int(c["min_triangulated"])) == (1.0, 1.0, 50)]
    u = 0
    while len(cs) < 70:
        n = 20 + 13 * (u % 11)
        c = rcases._h_scene(900 + u, n, n // 2 if u % 6 else 0, unmatched=u % 9) if u % 3 == 0 else rcases.scene(900 + u, n, unmatched=u % 9, extra2=u % 4)
        if u % 4 == 1: c = rcases.add_lines(c, 950 + u, u % 13, swap=min(u % 3, u % 13))
        if u % 11 == 5: c = rcases.named(c, "x", model=0)
        cs.append(rcases.named(c, "extra_%d" % u)); u += 1
    want = sim.run(cs)
    ok = [int(w["pose"]["ok"]) for w in want]; models = [c["model"] for c in cs]; reasons = {int(w["pose"]["reason"]) for w in want}
    assert len(cs) == 70 and 0 < sum(ok) < 70 and {0, 1, 2} <= set(models) and {0, 1, 3} <= reasons and any(sim.has_lines(c) for c in cs) and not all(sim.has_lines(c) for c in cs)
    cap = max(max(len(c["kp1"]), len(c["kp2"])) for c in cs) + 5
    lcap = max(max(len(c["fn1"]), len(c["fn2"]), len(c["lp"])) for c in cs if sim.has_lines(c)) + 1
    side = torch.cuda.Stream()
    B = Batch(fe, cs, cap, lcap, seed=77)
    B.launch(ctx, 1.0, 1.0, 50, stream=side.cuda_stream)
    side.synchronize()
    B.check(want)


def test_size_bounds(fe, ctx, expected):
    cases = rcases.all_cases()
    i = [c["name"] for c in cases].index("lines_65")
    c, want = cases[i], expected[i]
    B = Batch(fe, [cases[0], c], 5120, 1024)
    B.launch(ctx, c["sigma"], c["min_parallax"], c["min_triangulated"]); ctx.synchronize()
    B.check([expected[0], want])
    U = Batch(fe, [cases[0], c], 5121, 1025)
    for cap, lcap in ((5121, 1024), (5120, 1025)):
        with pytest.raises(fe.SslamError) as e:
            U.launch(ctx, 1.0, 1.0, 50, cap=cap, lcap=lcap)
        assert e.value.code == fe.SSLAM_ERR_UNSUPPORTED
    ctx.synchronize()
    assert U.untouched()


def test_argument_errors(fe, ctx):
    cases = rcases.all_cases()
    c = [c for c in cases if c["name"] == "lines_2"][0]
    B = Batch(fe, [c, c], 128, 8)
    bad = [dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(min_triangulated=-1), dict(cap=0), dict(npairs=0), dict(lcap=0), dict(cap=1 << 30, npairs=2)]
    for kw in bad:
        a = dict(sigma=1.0, min_parallax=1.0, min_triangulated=50); a.update(kw)
        with pytest.raises(fe.SslamError) as e:
            B.launch(ctx, a.pop("sigma"), a.pop("min_parallax"), a.pop("min_triangulated"), **a)
        assert e.value.code == fe.SSLAM_ERR_INVALID, kw
    for name in ("kp1", "kp2", "n1", "n2", "m12", "res", "inl", "K", "pose", "p3d", "tri"):
        own = dict(B.d, pose=B.pose, p3d=B.p3d, tri=B.tri)[name]
        for ptr in (None, own.data_ptr() + 1):
            if ptr is not None and name in ("inl", "tri"):
                continue                                # bytes: any address is aligned
            with pytest.raises(fe.SslamError) as e:
                B.launch(ctx, 1.0, 1.0, 50, **{name: ptr})
            assert e.value.code == fe.SSLAM_ERR_INVALID, (name, ptr)
    for k in range(11):                                 # lines given in part, or misaligned
        part = list(B.lines); part[k] = None
        with pytest.raises(fe.SslamError) as e:
            B.launch(ctx, 1.0, 1.0, 50, lines=part)
        assert e.value.code == fe.SSLAM_ERR_INVALID, k
        if k != 10:
            mis = list(B.lines); mis[k] = B.lines[k].data_ptr() + (4 if k in (4, 5) else 1)
            with pytest.raises(fe.SslamError) as e:
                B.launch(ctx, 1.0, 1.0, 50, lines=mis)
            assert e.value.code == fe.SSLAM_ERR_INVALID, k
    ctx.synchronize()
    assert B.untouched()
    B.launch(ctx, 1.0, 1.0, 50, lines=None); ctx.synchronize()      # none of the line arguments: a call without lines
    assert not B.untouched()


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def _dir_angle(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.degrees(np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1))))


def test_chain(fe, ctx):
    """Synthetic scenes with known K, R, t, projected to kp1 / kp2 with a quarter of a pixel of noise, in sslam_orb_search_for_initialization_batch_dev's layout ->
    sslam_two_view_ransac_batch_dev -> sslam_two_view_reconstruct_batch_dev; d_matches12, d_result and d_inliers never leave the device in between.  The pose equals the host
    model's on the same RANSAC result bit for bit, so the tolerance against the truth is the host model's own deviation on this input: the device's R21 and the direction of
    its t21 may be off by no more than the model's (both figures are printed per pair).  Measured: the host model is off by 0.2751 degrees of rotation and 1.2162 degrees of
    direction on the general scene (F path) and by 0.1187 / 0.2786 degrees on the planar one (H path), and the device gives the same figures; the bounds asked of the model
    are four times the larger measured figure, 1.1 degrees of rotation and 4.9 degrees of direction."""
    g = rcases.scene(501, 300, noise=0.25, unmatched=40, extra2=10)
    h = rcases.scene(502, 260, planar=True, plane=((-0.4, -0.1, 1.0), 3.5), R=rcases.rot((0.3, 1.0, 0.2), 10.0), t=(0.95, -0.4, -0.27), noise=0.25, unmatched=30)
    cs = [g, h]
    cap = max(max(len(c["kp1"]), len(c["kp2"])) for c in cs)
    B = Batch(fe, cs, cap, 0)
    res = torch.full((2 * fe.TWO_VIEW_RESULT_DTYPE.itemsize,), FILL, dtype=torch.uint8, device="cuda"); inl = torch.full((2 * cap,), FILL, dtype=torch.uint8, device="cuda")
    ctx.two_view_ransac_batch_dev(B.d["kp1"], B.d["n1"], B.d["kp2"], B.d["n2"], cap, 2, B.d["m12"], res, inl, iterations=200, sigma=1.0, seed=3)
    B.launch(ctx, 1.0, 1.0, 50, res=res, inl=inl); ctx.synchronize()
    pose = B.pose.cpu().numpy().view(fe.TWO_VIEW_POSE_DTYPE)[:2]
    r = res.cpu().numpy().view(fe.TWO_VIEW_RESULT_DTYPE); il = inl.cpu().numpy().reshape(2, cap)
    assert [int(x) for x in r["model"]] == [2, 1], r["model"]
    model_in = []
    for p, c in enumerate(cs):
        m = dict(c); m["model"] = int(r["model"][p]); m["H21"] = r["H21"][p]; m["F21"] = r["F21"][p]; m["inliers"] = il[p, :len(c["kp1"])]
        model_in.append(m)
    want = sim.run(model_in)
    for p, c in enumerate(cs):
        assert same_pose(pose[p], want[p]["pose"]), (p, pose[p], want[p]["pose"])
        assert pose[p]["ok"] == 1, pose[p]
        R, t = c["truth"]
        dev_r, dev_t = _angle(pose[p]["R21"].reshape(3, 3).astype(np.float64), R), _dir_angle(pose[p]["t21"], t)
        mod_r, mod_t = _angle(want[p]["pose"]["R21"].reshape(3, 3).astype(np.float64), R), _dir_angle(want[p]["pose"]["t21"], t)
        print("chain pair %d: model %d, R off by %.4f deg (host model %.4f), t direction off by %.4f deg (host model %.4f)" % (p, r["model"][p], dev_r, mod_r, dev_t, mod_t))
        assert dev_r <= mod_r and dev_t <= mod_t
        assert mod_r < 1.1 and mod_t < 4.9
