"""The cases of the map-creation unit (csrc/newmap_math.h, csrc/newmap.hip): pairs of keyframes with known poses, matched key points or key lines, and what each case is
there to reach; tests/test_newmap_cases_cpu.py asserts on the host model's output that it does.  A case is one pair in the layout tests/newmap_sim.py documents, plus a
name.  Cases that sit on a gate are found with the host model (tests/newmap_sim.py, the plain build) or with the gate's own float expression in numpy, never by looking at
the kernel: `edge` of such a case names the rows on the two sides.  pool_scene() is the many-keyframe pool of the GPU tests.  all_cases() builds the list once per process."""
import functools
import numpy as np

f32 = np.float32
NLEVELS = 8
SCALE_FACTOR = 1.2
SF = np.ones(NLEVELS, np.float32)
for _i in range(1, NLEVELS):
    SF[_i] = SF[_i - 1] * f32(SCALE_FACTOR)          # ORBextractor's mvScaleFactor
SIGMA2 = (SF * SF).astype(np.float32)                # mvLevelSigma2
KA = (520.0, 510.0, 320.0, 240.0)
KB = (500.0, 505.0, 310.0, 250.0)                    # another camera: the cx1-for-line-2 quirk of :1032-1035 shows
KP2 = (512.0, 512.0, 320.0, 240.0)                   # powers of two: the exact zeros of the w == 0 cases
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513)      # matches per pair
LINE_COUNTS = (0, 1, 63, 64, 65, 125)                # line rows per pair (keyframe 2 has three lines more: lcap <= 128)


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * S + (1 - np.cos(t)) * S @ S


def pose(R, O, K, t=None):
    """float32 [21], the words of sslam_kf_pose: Rcw, tcw = -Rcw O (or t as given, Ow = -Rcw^T t), Ow, fx fy cx cy, invfx invfy"""
    R = np.asarray(R, np.float64)
    if t is None:
        O = np.asarray(O, np.float64); t = -R @ O
    else:
        t = np.asarray(t, np.float64); O = -R.T @ t
    K = np.asarray(K, np.float32)
    return np.concatenate([R.ravel(), t, O, K, [f32(1) / K[0], f32(1) / K[1]]]).astype(np.float32)


def project(P, X):
    """pixels of world points through the centre of camera P (points behind it included)"""
    P = np.asarray(P, np.float64); R, t = P[:9].reshape(3, 3), P[9:12]
    Xc = np.asarray(X, np.float64).reshape(-1, 3) @ R.T + t
    return np.stack([P[15] * Xc[:, 0] / Xc[:, 2] + P[17], P[16] * Xc[:, 1] / Xc[:, 2] + P[18]], 1)


def line_fn(p, q):
    """the normalised line through two image points (src/ExtractLineSegment.cpp:56-68 leaves such coefficients)"""
    l = np.cross(np.append(p, 1.0), np.append(q, 1.0))
    return l / np.hypot(l[0], l[1])


def nxt(x, up=True):
    return np.nextafter(f32(x), f32(np.inf if up else -np.inf))


def _sim():
    import newmap_sim
    return newmap_sim


def point_case(name, p1, p2, kp1, oct1, kp2, oct2, m12, sf=SF, sigma2=SIGMA2, scale_factor=SCALE_FACTOR, **kw):
    return dict(name=name, pose1=np.asarray(p1, np.float32), pose2=np.asarray(p2, np.float32), kp1=np.asarray(kp1, np.float32).reshape(-1, 2), oct1=np.asarray(oct1, np.int32),
                kp2=np.asarray(kp2, np.float32).reshape(-1, 2), oct2=np.asarray(oct2, np.int32), m12=np.asarray(m12, np.int32), sf=np.asarray(sf, np.float32),
                sigma2=np.asarray(sigma2, np.float32), scale_factor=float(scale_factor), **kw)


def line_case(name, p1, p2, kl1, loct1, fn1, kl2, loct2, fn2, lp, median, sf=SF, free1=None, free2=None, **kw):
    return dict(name=name, pose1=np.asarray(p1, np.float32), pose2=np.asarray(p2, np.float32), kl1=np.asarray(kl1, np.float32).reshape(-1, 4), loct1=np.asarray(loct1, np.int32),
                fn1=np.asarray(fn1, np.float64).reshape(-1, 3), kl2=np.asarray(kl2, np.float32).reshape(-1, 4), loct2=np.asarray(loct2, np.int32),
                fn2=np.asarray(fn2, np.float64).reshape(-1, 3), lp=np.asarray(lp, np.int32).reshape(-1, 2), median=float(median), sf=np.asarray(sf, np.float32),
                free1=None if free1 is None else np.asarray(free1, np.uint8), free2=None if free2 is None else np.asarray(free2, np.uint8), **kw)


# ---- the two cameras of the ordinary scenes
CAM1 = pose(np.eye(3), (0, 0, 0), KA)
CAM2 = pose(rot((0.1, 1.0, 0.05), 4.0), (0.35, 0.02, 0.05), KB)


def point_scene(name, seed, nmatch, nun=3, extra2=2):
    """nmatch matched rows with a mix of fates, nun rows of keyframe 1 without a match (-1, below -1, at and past n2) interleaved, extra2 rows of keyframe 2 that nothing
    matches; keyframe 2's rows are permuted"""
    g = np.random.RandomState(seed)
    kind = g.choice(9, nmatch, p=[0.4, 0.08, 0.08, 0.08, 0.08, 0.08, 0.08, 0.06, 0.06])
    z = g.uniform(2.0, 6.0, nmatch)
    z[kind == 1] = 400.0                                             # no parallax (:497)
    X = np.concatenate([g.uniform(-0.4, 0.4, (nmatch, 2)) * z[:, None], z[:, None]], 1)
    a = project(CAM1, X) + 0.3 * g.standard_normal((nmatch, 2)); b = project(CAM2, X) + 0.3 * g.standard_normal((nmatch, 2))
    o1 = g.randint(0, NLEVELS, nmatch); o2 = np.clip(o1 + g.randint(-2, 3, nmatch), 0, NLEVELS - 1)
    k = kind == 2; a[k, 1] += 9.0; o1[k] = 0; o2[k] = 0                  # reprojection 1 and 2 fail at level 0
    k = kind == 3; a[k, 1] += 9.0; o1[k] = 7; o2[k] = 6                  # reprojection 1 passes at level 7, 2 fails
    k = kind == 4; a[k], b[k] = b[k].copy(), a[k].copy()                 # the disparity reversed: the rays meet behind the cameras
    k = kind == 5; o1[k] = 7; o2[k] = 0                                  # scale consistency, first side of :615
    k = kind == 6; o1[k] = 0; o2[k] = 7                                  # second side
    k = kind == 7; o1[k] = g.choice([-1, -5, NLEVELS, 100], k.sum()); o2[k] = g.choice([-2, NLEVELS + 1, 3], k.sum())      # octaves outside [0, nlevels)
    k = np.nonzero(kind == 8)[0]                                          # NaN / inf key points, rays more than 90 degrees apart
    for j, i in enumerate(k):
        if j % 4 == 0: a[i, 0] = np.nan
        elif j % 4 == 1: b[i, 1] = np.inf
        elif j % 4 == 2: a[i, 0] = -9000.0; b[i, 0] = 9000.0
        else: a[i] = (-np.inf, np.nan)
    n1, n2 = nmatch + nun, nmatch + extra2
    rows1 = np.sort(g.permutation(n1)[:nmatch]); perm2 = g.permutation(n2)[:nmatch]
    kp1 = g.uniform(20, 600, (n1, 2)); kp2 = g.uniform(20, 600, (n2, 2)); oc1 = g.randint(0, NLEVELS, n1); oc2 = g.randint(0, NLEVELS, n2)
    kp1[rows1] = a; kp2[perm2] = b; oc1[rows1] = o1; oc2[perm2] = o2
    m12 = np.zeros(n1, np.int32); m12[rows1] = perm2
    rest = np.setdiff1d(np.arange(n1), rows1); m12[rest] = [(-1, -9, n2, n2 + 7)[k % 4] for k in range(len(rest))]
    return point_case(name, CAM1, CAM2, kp1, oc1, kp2, oc2, m12, nmatch=nmatch)


def segment_obs(P, S, E):
    """key line (start x y, end x y) and its function for the world segment S - E in camera P"""
    p = project(P, np.stack([S, E]))
    return np.concatenate([p[0], p[1]]), line_fn(p[0], p[1])


def line_rows(p1, p2, segs, g=None, noise=0.0):
    kl1, fn1, kl2, fn2 = [], [], [], []
    for S, E in segs:
        a, fa = segment_obs(p1, S, E); b, fb = segment_obs(p2, S, E)
        if g is not None and noise:
            a = a + noise * g.standard_normal(4); b = b + noise * g.standard_normal(4)
            fa = line_fn(a[:2], a[2:]); fb = line_fn(b[:2], b[2:])
        kl1.append(a); fn1.append(fa); kl2.append(b); fn2.append(fb)
    return np.array(kl1).reshape(-1, 4), np.array(fn1).reshape(-1, 3), np.array(kl2).reshape(-1, 4), np.array(fn2).reshape(-1, 3)


LCAM2 = pose(rot((0.0, 1.0, 0.0), -10.0), (0.7, 0.03, 0.1), KB)


def line_scene(name, seed, nrows, with_free=False, extra=3):
    """nrows line rows with a mix of fates between CAM1 and LCAM2 (other intrinsics), median depth 3; rows with an index outside [0, nl) interleaved; with_free: some lines
    already have a map line.  Every fourth line of keyframe 1 and every fifth of keyframe 2 has its endpoints in the other order"""
    g = np.random.RandomState(seed)
    nl = max(nrows, 1)
    kind = g.choice(4, nl, p=[0.55, 0.15, 0.15, 0.15])
    segs = []
    for k in kind:
        z = g.uniform(2.0, 4.0); c = np.array([g.uniform(-0.3, 0.3) * z, g.uniform(-0.25, 0.25) * z, z])
        d = np.array([g.uniform(-0.3, 0.3), g.choice([-1.0, 1.0]), g.uniform(-0.3, 0.3)]); d /= np.linalg.norm(d)
        half = g.uniform(0.2, 0.6)
        if k == 1: c = c * 40.0                                          # no parallax (:1053)
        if k == 2: half = g.uniform(1.2, 2.0)                            # too long (ratio3)
        if k == 3: c = c * (0.7 / z); half = 0.1                          # too near (ratio1 / ratio2)
        segs.append((c - half * d, c + half * d))
    kl1, fn1, kl2, fn2 = line_rows(CAM1, LCAM2, segs, g, 0.2)
    for i in range(0, nl, 4):
        kl1[i] = kl1[i][[2, 3, 0, 1]]; fn1[i] = line_fn(kl1[i][:2], kl1[i][2:])
    perm = g.permutation(nl + extra)[:nl]
    k2 = g.uniform(20, 600, (nl + extra, 4)); f2 = np.array([line_fn(r[:2], r[2:]) for r in k2])
    k2[perm] = kl2; f2[perm] = fn2
    for i in range(0, nl + extra, 5):
        k2[i] = k2[i][[2, 3, 0, 1]]; f2[i] = line_fn(k2[i][:2], k2[i][2:])
    o1 = g.randint(0, NLEVELS, nl); o2 = g.randint(0, NLEVELS, nl + extra)
    o1[::7] = (-1, NLEVELS, 77)[seed % 3]
    lp = np.stack([np.arange(nl), perm], 1)[:nrows].astype(np.int32)
    order = g.permutation(nrows)                                          # the matcher's rows are in query order; the call takes any order
    lp = lp[order] if nrows > 3 else lp
    if nrows > 8:
        lp[2] = (-1, lp[2, 1]); lp[5] = (lp[5, 0], nl + extra); lp[7] = (nl, 0)      # indices outside [0, nl)
    free1 = free2 = None
    if with_free:
        free1 = (g.random_sample(nl) < 0.8).astype(np.uint8); free2 = (g.random_sample(nl + extra) < 0.8).astype(np.uint8)
    return line_case(name, CAM1, LCAM2, kl1, o1, fn1, k2, o2, f2, lp, 3.0, free1=free1, free2=free2)


# ---- cases built for one exit each
def _p_wzero():
    """x3D(3) == 0 exactly (:511): both cameras look along z, at (-a, 0, 0) and (a, 0, 0) with a a power of two, and the two key points have the SAME x.  Column 3 of A is
    then orthogonal to the other three in exact arithmetic (every product is exact and the sums cancel), cyclic Jacobi never mixes it in, and with different y (so that the
    rays are not parallel: cos < 0.9998) the smallest eigenvector lies in the x y z block"""
    a = 0.125
    p1 = pose(np.eye(3), None, KP2, t=(a, 0, 0)); p2 = pose(np.eye(3), None, KP2, t=(-a, 0, 0))
    kp1 = [(384, 240), (384, 200), (400, 240)]; kp2 = [(384, 256), (384, 230), (380, 256)]      # the third row has a disparity: an ordinary point
    return point_case("p_w_zero", p1, p2, kp1, [0, 1, 0], kp2, [0, 1, 0], [0, 1, 2], want={0: 3, 1: 3})


def _p_behind2():
    """z1 > 0, z2 <= 0 (:538): keyframe 2 stands beyond the point and looks the same way, so the point projects into its image through the centre"""
    p2 = pose(np.eye(3), (0.5, 0.0, 5.0), KA)
    X = np.array([[0.1, 0.1, 2.0], [-0.3, 0.2, 2.5], [0.0, 0.0, 3.0]])
    return point_case("p_behind2", CAM1, p2, project(CAM1, X), [0, 1, 2], project(p2, X), [0, 1, 2], [0, 1, 2], want={0: 5, 1: 5, 2: 5})


def _p_dist_zero(which):
    """dist1 == 0 resp. dist2 == 0 (:607): the camera centre of the pose IS the triangulated point (GetCameraCenter is an input of its own; at the true centre z would be 0
    and :534 would end the row first).  The point comes from the host model's own run with the ordinary centres"""
    X = np.array([[0.2, -0.1, 3.0]])
    c = point_case("p_dist%d_zero" % which, CAM1, CAM2, project(CAM1, X), [2], project(CAM2, X), [2], [0], want={0: 8})
    x3d = _sim().run_plain([c])[0]["x3d"][0]
    assert np.isfinite(x3d).all() and abs(x3d[2] - 3.0) < 0.05
    c["pose%d" % which] = c["pose%d" % which].copy(); c["pose%d" % which][12:15] = x3d
    return c


def _p_cos_edge():
    """cosParallaxRays < 0.9998 (:497) on neighbouring floats: key point 2's x moves by one float between the two rows"""
    X = np.array([[0.3, 0.2, 17.0]])
    a, b = project(CAM1, X)[0], project(CAM2, X)[0]
    def created(x2):
        c = point_case("probe", CAM1, CAM2, [a], [3], [(x2, b[1])], [3], [0])
        return _sim().run_plain([c])[0]["stage"][0] != 2
    lo, hi = f32(b[0] - 3.0), f32(b[0] + 3.0)
    plo = created(lo)
    assert created(hi) != plo
    while nxt(lo) != hi:
        mid = f32((np.float64(lo) + np.float64(hi)) / 2)
        if created(mid) == plo: lo = mid
        else: hi = mid
    return point_case("p_cos_edge", CAM1, CAM2, [a, a], [3, 3], [(lo, b[1]), (hi, b[1])], [3, 3], [0, 1], edge=(0, 1))


def _p_err_edge():
    """5.991 * sigmaSquare (:557, :584) on neighbouring floats: the level tables are the call's, so rows of one geometry sit at levels whose sigma2 are neighbours"""
    X = np.array([[0.3, 0.2, 4.0]])
    a, b = project(CAM1, X)[0] + (0.0, 2.6), project(CAM2, X)[0]
    big = np.full(NLEVELS, 1000.0, np.float32); ones = np.ones(NLEVELS, np.float32)
    c = point_case("p_err_edge", CAM1, CAM2, [a] * 4, [1, 2, 7, 7], [b] * 4, [7, 7, 3, 4], [0, 1, 2, 3], sf=ones, sigma2=big, edge=((0, 1), (2, 3)))
    e = _sim().run_plain([c])[0]["err"][0]
    def last_tripping(err):      # the largest float32 s with err > 5.991 * s
        s = f32(np.float64(err) / 5.991)
        while not np.float64(err) > 5.991 * np.float64(s): s = nxt(s, False)
        while np.float64(err) > 5.991 * np.float64(nxt(s)): s = nxt(s)
        return s
    s1, s2 = last_tripping(e[0]), last_tripping(e[1])
    sg = big.copy(); sg[1] = s1; sg[2] = nxt(s1); sg[3] = s2; sg[4] = nxt(s2)
    c["sigma2"] = sg
    return c


def _p_scale_edge():
    """both sides of :615 on neighbouring floats of the scale factors: ratioDist * ratioFactor < sf[l1] / sf[l2] and ratioDist > sf[l1] / sf[l2] * ratioFactor"""
    X = np.array([[0.3, 0.2, 4.0]])
    a, b = project(CAM1, X)[0], project(CAM2, X)[0]
    big = np.full(NLEVELS, 1000.0, np.float32); sf = np.ones(NLEVELS, np.float32)
    c = point_case("p_scale_edge", CAM1, CAM2, [a] * 4, [1, 2, 0, 0], [b] * 4, [0, 0, 3, 4], [0, 1, 2, 3], sf=sf, sigma2=big, edge=((0, 1), (2, 3)))
    rd = _sim().run_plain([c])[0]["ratio"][0, 0]
    rf = f32(1.5) * f32(SCALE_FACTOR)
    s = f32(rd * rf)                                  # ratioOctave = s / 1: not below it
    sf[1] = s; sf[2] = nxt(s)
    second = lambda v: bool(rd > f32(f32(f32(1) / f32(v)) * rf))
    lo, hi = f32(1.0), f32(4.0)
    assert not second(lo) and second(hi)
    while nxt(lo) != hi:
        mid = f32((np.float64(lo) + np.float64(hi)) / 2)
        if second(mid): hi = mid
        else: lo = mid
    sf[3] = lo; sf[4] = hi
    c["sf"] = sf
    return c


def _l_wzero():
    """s3D(3) == 0 and e3D(3) == 0 exactly (:1066, :1084): the cameras of _p_wzero, line 1 horizontal (its function has no x term), line 2 vertical with x term 1 / fx, and
    the endpoint of line 1 at line 2's x: column 3 of A is orthogonal to the others in exact arithmetic.  Row 0 ends at s3D; row 1 is the same line with its endpoints in
    the other order and ends at e3D"""
    a = 0.125
    p1 = pose(np.eye(3), None, KP2, t=(a, 0, 0)); p2 = pose(np.eye(3), None, KP2, t=(-a, 0, 0))
    kl1 = [(384, 240, 448, 240), (448, 240, 384, 240)]; fn1 = [(0, 1, -240), (0, 1, -240)]
    kl2 = [(384, 400, 384, 480)]; fn2 = [(1.0 / 512, 0, -0.75)]
    return line_case("l_w_zero", p1, p2, kl1, [0, 0], fn1, kl2, [0], fn2, [(0, 0), (1, 0)], 1.0, want={0: 4, 1: 5})


def _l_near():
    """ratio1, ratio2, ratio4, ratio5 (:1102-1131) one by one: two cameras 0.3 apart looking along z, median depth 1, short segments near one camera or the other"""
    p2 = pose(np.eye(3), (0.3, 0, 0), KA)
    segs = [((0.0, 0.0, 0.2), (0.0, 0.1, 0.25)),          # start near camera 1
            ((0.25, 0.0, 0.2), (0.25, 0.3, 0.45)),         # start 0.32 from camera 1, 0.21 from camera 2
            ((0.0, 0.0, 0.5), (0.0, 0.05, 0.25)),          # end near camera 1
            ((0.3, 0.0, 0.5), (0.3, 0.05, 0.25)),          # end near camera 2
            ((0.1, -0.1, 0.6), (0.2, 0.2, 0.7))]           # created
    kl1, fn1, kl2, fn2 = line_rows(CAM1, p2, [(np.array(s), np.array(e)) for s, e in segs])
    return line_case("l_near", CAM1, p2, kl1, [0, 1, 2, 3, 4], fn1, kl2, [0, 1, 2, 3, 4], fn2, [(i, i) for i in range(5)], 1.0, want={0: 6, 1: 7, 2: 9, 3: 10, 4: 0})


def _l_behind():
    """SZC1, SZC2, EZC1, EZC2 (:1135-1148), one pair each: a segment projects into a camera it lies behind through the centre"""
    out = []
    seg = lambda s, e: [(np.array(s, np.float64), np.array(e, np.float64))]
    # both ends behind both cameras
    p2 = pose(np.eye(3), (0.8, 0, 0), KA)
    out.append(("l_szc1", CAM1, p2, seg((0.3, 0.2, -2.0), (0.35, -0.2, -2.1)), 3.0, 11))
    # camera 2 stands beyond the segment
    p2 = pose(np.eye(3), (0.6, 0, 2.0), KA)
    out.append(("l_szc2", CAM1, p2, seg((0.0, 0.2, 1.0), (0.05, -0.2, 1.05)), 2.0, 12))
    # the segment crosses camera 1's plane; camera 2 looks at it from the side
    p2 = pose(rot((0, 1, 0), 45.0), (2.0, 0, -1.0), KA)
    out.append(("l_ezc1", CAM1, p2, seg((0.3, 0.2, 0.5), (0.3, 0.25, -0.4)), 1.6, 13))
    out.append(("l_ezc2", p2, CAM1, seg((0.3, 0.2, 0.5), (0.3, 0.25, -0.4)), 1.6, 14))
    cases = []
    for name, a, b, s, med, stage in out:
        kl1, fn1, kl2, fn2 = line_rows(a, b, s)
        cases.append(line_case(name, a, b, kl1, [1], fn1, kl2, [1], fn2, [(0, 0)], med, want={0: stage}))
    return cases


def _l_cos_edge():
    """cosParallaxRays < 0.98 (:1053) on neighbouring floats: the end x of key line 2 moves by one float between the two rows"""
    S, E = np.array([0.2, -0.3, 3.0]), np.array([0.25, 0.3, 3.1])
    kl1, fn1, kl2, fn2 = line_rows(CAM1, LCAM2, [(S, E)])
    def passes(x):
        k2 = kl2.copy(); k2[0, 2] = x
        c = line_case("probe", CAM1, LCAM2, kl1, [0], fn1, k2, [0], fn2, [(0, 0)], 3.0)
        return _sim().run_plain([c])[0]["stage"][0] != 3
    lo, hi = f32(kl2[0, 2]), f32(kl2[0, 2] + 100.0)
    assert passes(lo) and not passes(hi)
    while nxt(lo) != hi:
        mid = f32((np.float64(lo) + np.float64(hi)) / 2)
        if passes(mid): lo = mid
        else: hi = mid
    k2 = np.repeat(kl2, 2, axis=0); k2[0, 2] = lo; k2[1, 2] = hi
    return line_case("l_cos_edge", CAM1, LCAM2, kl1, [0], fn1, k2, [0, 0], np.repeat(fn2, 2, axis=0), [(0, 0), (0, 1)], 3.0, edge=(0, 1))


def _l_ratio_edges():
    """ratio < 0.3 and ratio > 0.61 on neighbouring floats of the neighbour's median depth (an input of the pair): two pairs per gate.  With median depth 1 the model's trace
    gives the distances themselves"""
    S, E = np.array([0.2, -0.3, 3.0]), np.array([0.25, 0.22, 3.1])
    kl1, fn1, kl2, fn2 = line_rows(CAM1, LCAM2, [(S, E)])
    mk = lambda name, med, **kw: line_case(name, CAM1, LCAM2, kl1, [0], fn1, kl2, [0], fn2, [(0, 0)], med, **kw)
    d = _sim().run_plain([mk("probe", 1.0)])[0]["ratio"][0]
    assert (d > 0).all()
    def adjacent(pred, lo, hi):      # float32 medians next to each other with pred false at the first and true at the second
        lo, hi = f32(lo), f32(hi)
        assert not pred(lo) and pred(hi)
        while nxt(lo, hi > lo) != hi:
            mid = f32((np.float64(lo) + np.float64(hi)) / 2)
            if pred(mid): hi = mid
            else: lo = mid
        return lo, hi
    dmin = f32(min(d[0], d[1], d[3], d[4]))
    a, b = adjacent(lambda m: np.float64(f32(dmin / f32(m))) < 0.3, dmin / f32(0.4), dmin / f32(0.2))          # a larger median makes the ratio smaller
    c, e = adjacent(lambda m: np.float64(f32(d[2] / f32(m))) > 0.61, d[2] / f32(0.5), d[2] / f32(0.7))          # a smaller median makes ratio3 larger
    return [mk("l_ratio_lo_pass", a, edge="0.3"), mk("l_ratio_lo_trip", b, edge="0.3"), mk("l_ratio3_pass", c, edge="0.61"), mk("l_ratio3_trip", e, edge="0.61")]


def _l_swapped():
    """a key line 1 and the same line with its endpoints in the other order (and the same function), both matched with one key line 2: s3D and e3D change places"""
    S, E = np.array([0.2, -0.3, 3.0]), np.array([0.25, 0.22, 3.1])
    kl1, fn1, kl2, fn2 = line_rows(CAM1, LCAM2, [(S, E)])
    kl1 = np.concatenate([kl1, kl1[:, [2, 3, 0, 1]]]); fn1 = np.repeat(fn1, 2, axis=0)
    return line_case("l_swapped", CAM1, LCAM2, kl1, [1, 1], fn1, kl2, [2], fn2, [(0, 0), (1, 0)], 3.0, want={0: 0, 1: 0})


def _l_many_rows(nrows=300):
    """more rows than the 256 lanes of k_newmap_lines: the lanes' second turn, in both passes.  The rows name the lines of a scene of 60 several times over (two rows may
    name one line: the flags are read before any is cleared), with flags; for the single call (a batch slot of 300 lines is above the tests' lcap)"""
    c = line_scene("l_rows_%d" % nrows, 260, 60, with_free=True)
    g = np.random.RandomState(261)
    c["lp"] = np.ascontiguousarray(c["lp"][g.randint(0, len(c["lp"]), nrows)])
    c["single_only"] = True
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [point_scene("p_count_%d" % n, 100 + n, n) for n in COUNTS]
    cases += [_p_wzero(), _p_behind2(), _p_dist_zero(1), _p_dist_zero(2), _p_cos_edge(), _p_err_edge(), _p_scale_edge()]
    cases += [line_scene("l_count_%d" % n, 200 + n, n, with_free=(n in (64, 125))) for n in LINE_COUNTS]
    cases += [_l_wzero(), _l_near()] + _l_behind() + [_l_cos_edge()] + _l_ratio_edges() + [_l_swapped(), _l_many_rows()]
    assert len(set(c["name"] for c in cases)) == len(cases)
    return cases


def point_cases():
    return [c for c in all_cases() if "lp" not in c]


def line_cases():
    return [c for c in all_cases() if "lp" in c]


# ---- pools of many keyframes (the GPU tests): one cloud of points or segments seen from keyframes on an arc, rows in each keyframe's own order
def _arc_pose(k, nkf, K):
    O = np.array([0.3 * (k - nkf / 2.0), 0.03 * (k % 5), 0.06 * (k % 3)])
    return pose(rot((0, 1, 0), np.rad2deg(np.arctan2(O[0], 5.0)) * -0.8) @ rot((1, 0, 0), 0.7 * (k % 4)), O, K)


def pool_counts(nkf, cap):
    ragged = [cap, 0, 1, 63, 64, 65, cap - 1]
    return [min(cap, ragged[k % len(ragged)]) if k % 3 == 2 else cap - (k % 4) for k in range(nkf)]


def point_pool(seed, nkf=24, cap=96, npts=None, counts=None):
    """-> dict(poses float32 [nkf, 21], kp [nkf] of float32 [n, 2], oct [nkf] of int32 [n], ids [nkf] of int32 [n]): keyframe k sees n_k of the cloud's points (ragged
    counts, 0 and 1 among them); ids name the point of a row.  Even keyframes use camera KA, odd ones KB"""
    g = np.random.RandomState(seed)
    npts = npts or cap + 20
    X = np.stack([g.uniform(-2.0, 2.0, npts), g.uniform(-1.2, 1.2, npts), g.uniform(3.5, 7.0, npts)], 1)
    poses = np.stack([_arc_pose(k, nkf, KA if k % 2 == 0 else KB) for k in range(nkf)])
    kp, octs, ids = [], [], []
    for k, n in enumerate(counts or pool_counts(nkf, cap)):
        sel = g.permutation(npts)[:n].astype(np.int32)
        kp.append((project(poses[k], X[sel]) + 0.3 * g.standard_normal((n, 2))).astype(np.float32)); octs.append(g.randint(0, 4, n).astype(np.int32)); ids.append(sel)
    return dict(poses=poses, kp=kp, oct=octs, ids=ids, X=X)


def matches_by_id(ids1, ids2):
    where = {int(p): j for j, p in enumerate(ids2)}
    return np.array([where.get(int(p), -1) for p in ids1], np.int32)


def pool_point_case(P, a, b, m12=None, name=None):
    """the pair (keyframe a, keyframe b) of a point pool as a case of the host model"""
    m12 = matches_by_id(P["ids"][a], P["ids"][b]) if m12 is None else m12
    return point_case(name or "pool_%d_%d" % (a, b), P["poses"][a], P["poses"][b], P["kp"][a], P["oct"][a], P["kp"][b], P["oct"][b], m12)


def line_pool(seed, nkf=24, lcap=48, nseg=None, median=5.0, counts=None):
    """the same for segments -> dict(poses, kl [nkf] of float32 [n, 4], oct, fn [nkf] of float64 [n, 3], ids, median)"""
    g = np.random.RandomState(seed)
    nseg = nseg or lcap + 10
    poses = np.stack([_arc_pose(k, nkf, KA if k % 2 == 0 else KB) for k in range(nkf)])
    segs = []
    for _ in range(nseg):
        c = np.array([g.uniform(-2.0, 2.0), g.uniform(-1.0, 1.0), g.uniform(3.5, 6.5)])
        d = np.array([g.uniform(-0.3, 0.3), g.choice([-1.0, 1.0]), g.uniform(-0.3, 0.3)]); d /= np.linalg.norm(d)
        half = g.uniform(0.3, 1.3)
        segs.append((c - half * d, c + half * d))
    kl, octs, fn, ids = [], [], [], []
    for k, n in enumerate(counts or pool_counts(nkf, lcap)):
        sel = g.permutation(nseg)[:n].astype(np.int32)
        rows = [segment_obs(poses[k], *segs[i]) for i in sel]
        kl.append(np.array([r[0] for r in rows], np.float32).reshape(-1, 4)); fn.append(np.array([r[1] for r in rows], np.float64).reshape(-1, 3))
        octs.append(g.randint(0, 3, n).astype(np.int32)); ids.append(sel)
    return dict(poses=poses, kl=kl, oct=octs, fn=fn, ids=ids, median=median)


def pool_line_case(P, a, b, lp, free1=None, free2=None, name=None):
    return line_case(name or "lpool_%d_%d" % (a, b), P["poses"][a], P["poses"][b], P["kl"][a], P["oct"][a], P["fn"][a], P["kl"][b], P["oct"][b], P["fn"][b], lp, P["median"],
                     free1=free1, free2=free2)


def f12_of(p1, p2):
    """LocalMapping::ComputeF12 (src/LocalMapping.cc:1176-1194) for two poses, scaled to a largest entry of 1, and the epipole of camera 1 in image 2 (src/ORBmatcher.cc:667-673)
    -> (F12 float32 [3, 3], ex, ey)"""
    a, b = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    R1, t1, R2, t2 = a[:9].reshape(3, 3), a[9:12], b[:9].reshape(3, 3), b[9:12]
    R12 = R1 @ R2.T; t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Km = lambda p: np.array([[p[15], 0, p[17]], [0, p[16], p[18]], [0, 0, 1.0]])
    F = np.linalg.inv(Km(a)).T @ tx @ R12 @ np.linalg.inv(Km(b))
    C2 = R2 @ a[12:15] + t2
    return (F / np.abs(F).max()).astype(np.float32), float(f32(b[15] * C2[0] / C2[2] + b[17])), float(f32(b[16] * C2[1] / C2[2] + b[18]))
