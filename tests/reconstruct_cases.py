"""The cases of the reconstruct unit (csrc/reconstruct_math.h, csrc/reconstruct.hip): synthetic two-view scenes with known K, R, t, their exact H21 / F21 and inlier bytes
in the layout sslam_two_view_ransac leaves them, and lines with their functions.  Each case names what it is there to reach; tests/test_reconstruct_cases_cpu.py asserts on
the host model's trace that it does.  Cases that sit on a gate are found by searching with the host model (tests/reconstruct_sim.py, the plain build), never by looking at the
kernel.  all_cases() builds the list once per process."""
import functools
import numpy as np

K0 = (520.0, 510.0, 320.0, 240.0)      # fx != fy: the fx of :1129 shows
K1 = (1.0, 1.0, 0.0, 0.0)              # normalised coordinates: A = invK * H21 * K is H21 itself


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * S + (1 - np.cos(t)) * S @ S


def kmat(K):
    return np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def project(K, R, t, X):
    Xc = X @ R.T + t
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)


def line_fn(p, q):
    """the normalised line through two image points (src/ExtractLineSegment.cpp:56-68 leaves such coefficients)"""
    l = np.cross(np.append(p, 1.0), np.append(q, 1.0))
    return l / np.hypot(l[0], l[1])


def scene(seed, n, K=K0, R=None, t=None, planar=False, noise=0.0, unmatched=0, extra2=0, depth=(4.0, 9.0), plane=((0.25, -0.15, 1.0), 6.0)):
    """n matched points seen from [I | 0] and [R | t], `unmatched` rows of frame 1 without a match interleaved, extra2 rows of frame 2 that nothing matches; frame 2's rows are
    permuted.  planar: the points lie on a tilted plane, and H21 is its homography; F21 is exact either way."""
    g = np.random.RandomState(seed)
    R = rot((0.2, 1.0, 0.1), 6.0) if R is None else R
    t = np.array([0.6, 0.05, 0.1]) if t is None else np.asarray(t, np.float64)
    xy = g.uniform(-0.45, 0.45, (n, 2))
    nrm, d = np.asarray(plane[0], np.float64), float(plane[1])
    nrm = nrm / np.linalg.norm(nrm)
    if planar:
        ray = np.concatenate([xy, np.ones((n, 1))], 1)
        X = ray * (d / (ray @ nrm))[:, None]
    else:
        z = g.uniform(depth[0], depth[1], n)
        X = np.concatenate([xy * z[:, None], z[:, None]], 1)
    p1 = project(K, np.eye(3), np.zeros(3), X) + noise * g.standard_normal((n, 2))
    p2 = project(K, R, t, X) + noise * g.standard_normal((n, 2))
    n1, n2 = n + unmatched, n + extra2
    rows1 = np.sort(g.permutation(n1)[:n])
    perm2 = g.permutation(n2)[:n]
    kp1 = g.uniform(20, 600, (n1, 2)); kp2 = g.uniform(20, 600, (n2, 2))
    kp1[rows1] = p1; kp2[perm2] = p2
    m12 = np.full(n1, -1, np.int32); m12[rows1] = perm2
    inl = np.zeros(n1, np.uint8); inl[rows1] = 3
    Km = kmat(K); Ki = np.linalg.inv(Km)
    F = Ki.T @ skew(t) @ R @ Ki
    H = Km @ (R + np.outer(t, nrm) / d) @ Ki
    return {"kp1": kp1.astype(np.float32), "kp2": kp2.astype(np.float32), "m12": m12, "inliers": inl, "model": 1 if planar else 2,
            "H21": (H / H[2, 2]).astype(np.float32).ravel(), "F21": (F / np.abs(F).max()).astype(np.float32).ravel(), "K": np.asarray(K, np.float32), "sigma": 1.0,
            "min_parallax": 1.0, "min_triangulated": 50, "lp": None, "truth": (R, t), "rows1": rows1, "X": X}


def add_lines(c, seed, nlp, bad_index=False, nonfinite=None, swap=0):
    """nlp pairs of 3-D segments seen in both frames; the lines of frame 2 are permuted.  bad_index: the second pair names a line past nl1 and the last one a negative one;
    nonfinite: that row's start point is +inf.  swap: so many pairs get the function of a wrong line of frame 2 (large errors)"""
    g = np.random.RandomState(seed)
    K, (R, t) = c["K"].astype(np.float64), c["truth"]
    nl = max(nlp, 1) + 2
    a = np.concatenate([g.uniform(-0.4, 0.4, (nl, 2)), np.ones((nl, 1))], 1) * g.uniform(4, 9, (nl, 1))
    b = a + g.uniform(-0.8, 0.8, (nl, 3))
    s1, e1 = project(K, np.eye(3), np.zeros(3), a), project(K, np.eye(3), np.zeros(3), b)
    s2, e2 = project(K, R, t, a), project(K, R, t, b)
    perm = g.permutation(nl)
    kl1 = np.concatenate([s1, e1], 1).astype(np.float32)
    fn1 = np.array([line_fn(s1[i], e1[i]) for i in range(nl)])
    fn2 = np.zeros((nl, 3)); fn2[perm] = np.array([line_fn(s2[i], e2[i]) for i in range(nl)])
    lp = np.stack([np.arange(nlp), perm[:nlp]], 1).astype(np.int32)
    for j in range(swap):
        lp[nlp - 1 - j, 1] = perm[(nlp - j) % nl]
    if bad_index and nlp >= 3:
        lp[1, 0] = nl; lp[nlp - 1, 1] = -1
    if nonfinite is not None:
        kl1[lp[nonfinite, 0], 0] = np.inf
    c = dict(c)
    c.update(kl1=kl1, fn1=fn1, fn2=fn2, lp=lp)
    return c


def named(c, name, **kw):
    c = dict(c); c["name"] = name; c.update(kw)
    return c


def _sim():
    import reconstruct_sim
    return reconstruct_sim


def _next(x, up=True):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


def _f_winners():
    """general scenes whose true motion comes out as each of the four hypotheses of :527-530"""
    sim = _sim()
    found, seed = {}, 0
    while len(found) < 4 and seed < 64:
        g = np.random.RandomState(1000 + seed)
        c = scene(100 + seed, 80, R=rot(g.standard_normal(3), g.uniform(2, 12)), t=g.uniform(-1, 1, 3) * (0.8, 0.4, 0.3), unmatched=7, extra2=5)
        r = sim.run_plain([c])[0]["pose"]
        if r["ok"] and int(r["hypothesis"]) not in found:
            found[int(r["hypothesis"])] = named(c, "f_winner_%d" % int(r["hypothesis"]))
        seed += 1
    assert len(found) == 4, sorted(found)
    return [found[h] for h in range(4)]


def _join(c, o):
    """the rows of scene o behind those of scene c (c's matrices stay)"""
    c = dict(c)
    n1, n2 = len(c["kp1"]), len(c["kp2"])
    c["kp1"] = np.concatenate([c["kp1"], o["kp1"]]); c["kp2"] = np.concatenate([c["kp2"], o["kp2"]])
    c["m12"] = np.concatenate([c["m12"], np.where(o["m12"] >= 0, o["m12"] + n2, -1)]).astype(np.int32); c["inliers"] = np.concatenate([c["inliers"], o["inliers"]])
    c["rows1"] = np.concatenate([c["rows1"], o["rows1"] + n1])
    return c


def _h_scene(seed, nplane, noff, **kw):
    """a planar scene whose inliers are its plane points and `noff` points off the plane that move with the true motion: the twin of Faugeras' solution takes the plane points
    alone, so bestGood = nplane + noff and secondBestGood = nplane"""
    R, t = rot((0.1, 1.0, 0.0), 8.0), np.array([0.9, 0.1, 0.15])
    c = scene(seed, nplane, planar=True, R=R, t=t, **kw)
    if noff:
        c = _join(c, scene(seed + 1, noff, R=R, t=t, depth=(3.0, 5.0)))
    return c


def _gate_cases():
    """cases on the gates of ReconstructF / ReconstructH / CheckRT, found with the host model"""
    sim = _sim()
    out = []
    base = scene(7, 120, unmatched=9, extra2=4)
    r = sim.run_plain([base])[0]
    pose = r["pose"]
    assert pose["ok"] == 1
    w = int(pose["hypothesis"]); g = int(pose["n_good"][w]); par = pose["parallax"][w]
    # maxGood one below / at nMinGood (:537, :550): 0.9 * N stays below
    out += [named(base, "f_maxgood_below_min", min_triangulated=g + 1), named(base, "f_maxgood_at_min", min_triangulated=g)]
    # parallax on the neighbouring floats of min_parallax: F asks >, H asks >=
    out += [named(base, "f_parallax_at_min", min_parallax=float(par)), named(base, "f_parallax_above_min", min_parallax=float(_next(par, False)))]
    # the tie of nGood: nothing is good anywhere, minTriangulated 0 lets :550 pass, the FIRST hypothesis is taken and fails on its parallax of 0
    one = scene(8, 1)
    one["kp2"] = one["kp2"] + np.float32(40.0)
    out.append(named(one, "f_tie_first_taken", min_triangulated=0))
    out.append(named(one, "f_tie_first_taken_wins", min_triangulated=0, min_parallax=-1.0))
    # nsimilar > 1 (:540-550): fifty points that move with (R, t) and forty-five that move with (R, -t) satisfy the same F21; two hypotheses take one group each
    R, t = rot((0.2, 1.0, 0.1), 6.0), np.array([0.6, 0.05, 0.1])
    out.append(named(_join(scene(300, 50, R=R, t=t), scene(301, 45, R=R, t=-t)), "f_nsimilar", min_triangulated=0))
    # 0.9 * N on both sides of an integer (:763): N = 60, 54 good is not above 54.0, 55 is.  The bad inliers are moved by 10 pixels in frame 2
    for good in (54, 55):
        c = _h_scene(21, 40, 20)
        for i in c["rows1"][:60 - good]:
            c["kp2"][c["m12"][i]] += np.float32(10.0)
        out.append(named(c, "h_09n_%d_of_60" % good))
    # secondBestGood at 0.75 of bestGood (:763): 60 plane points and 20 / 21 beside them
    # plane points with a growing number of points beside them: 4 * second == 3 * best is not below, the nearest count under it is
    found = {}
    for seed in range(22, 120):
        cand = [_h_scene(seed * 100, 60, k) for k in range(8, 32)]
        for c, r in zip(cand, sim.run_plain(cand)):
            ng = np.sort(r["pose"]["n_good"])[::-1]
            d = 4 * int(ng[1]) - 3 * int(ng[0])
            if ng[0] == int(r["pose"]["n_inliers"]) and d == 0: found.setdefault("h_second_at_075", c)
            if ng[0] == int(r["pose"]["n_inliers"]) and -3 <= d < 0: found.setdefault("h_second_below_075", c)
        if len(found) == 2: break
    assert len(found) == 2, sorted(found)
    out += [named(c, n) for n, c in sorted(found.items())]
    hb = _h_scene(23, 70, 30, unmatched=6)
    rh = sim.run_plain([hb])[0]["pose"]
    assert rh["ok"] == 1
    ph = rh["parallax"][int(rh["hypothesis"])]
    out += [named(hb, "h_parallax_at_min", min_parallax=float(ph)), named(hb, "h_parallax_below_min", min_parallax=float(_next(ph)))]
    # d1 / d2 and d2 / d3 on the neighbouring floats of 1.00001 (:639): a diagonal H21 in normalised coordinates keeps its entries as singular values
    lo = np.float32(1.00001)
    lo = lo if float(lo) < 1.00001 else _next(lo, False)
    hi = _next(lo)
    assert float(lo) < 1.00001 <= float(hi)
    for nm_, d in (("h_d1d2_below", (lo, 1, 0.5)), ("h_d1d2_above", (hi, 1, 0.5)), ("h_d2d3_below", (2, lo, 1)), ("h_d2d3_above", (2, hi, 1))):
        c = scene(24, 12, K=K1, planar=True)
        c["H21"] = np.diag(np.asarray(d, np.float32)).ravel()
        out.append(named(c, nm_))
    # either reprojection error on the float at th2 and on the one above (:923, :934).  An error is a squared difference of coordinates, so it moves in steps of its own ulp
    # only where the coordinates are no larger than the difference: normalised coordinates, sigma 0.5 (th2 = 1) and one row of frame 1 / frame 2 pushed along y until its
    # error reaches 1; the floats around that push, at several pushes along x, are scanned for the two values
    th2 = np.float32(1.0)
    for which, col in ((1, 0), (2, 1)):
        c0 = scene(31, 20, K=K1, t=None if which == 1 else (0.6, 0.05, -0.8))      # the DLT leaves the larger error in the frame the point is nearer to
        c0["sigma"] = 0.5; c0["min_triangulated"] = 0
        i = int(c0["rows1"][5]); slot = 5
        key = "kp1" if which == 1 else "kp2"
        j = i if which == 1 else int(c0["m12"][i])

        def variant(y, dx):
            c = dict(c0); kp = c0[key].copy()
            kp[j, 1] = np.float32(y); kp[j, 0] += np.float32(dx)
            c[key] = kp
            return c
        wv = int(sim.run_plain([c0])[0]["pose"]["hypothesis"])
        found = {}
        for dx in np.linspace(-0.2, 0.2, 60):
            lo_, hi_ = float(c0[key][j, 1]), float(c0[key][j, 1]) + 4.0
            for _ in range(40):
                mid = 0.5 * (lo_ + hi_)
                e = sim.run_plain([variant(mid, dx)])[0]["rows_err"][wv, slot, col]
                lo_, hi_ = (mid, hi_) if e < th2 else (lo_, mid)
            y = np.float32(lo_)
            for _ in range(30): y = _next(y, False)
            cand = []
            for _ in range(60):
                cand.append(variant(y, dx)); y = _next(y)
            for c, r in zip(cand, sim.run_plain(cand)):
                e = r["rows_err"][wv, slot, col]
                if e == th2: found.setdefault("at", c)
                if e == _next(th2): found.setdefault("above", c)
            if len(found) == 2: break
        assert len(found) == 2, (which, sorted(found))
        out += [named(found["at"], "err%d_at_th2" % which, gate_row=(wv, slot)), named(found["above"], "err%d_above_th2" % which, gate_row=(wv, slot))]
    return out


LINE_SEED = [46]      # of the lines of the gate scene: the first seed with a row above the threshold of errorC1 whose errorC2 passes its own


def _line_gate_cases():
    """a line error exactly at 2 * 1.4826 * MAD and on the double above (:1166), on a row whose errorC1 lies above the threshold and whose errorC2 passes.  The error reads
    the line's function as doubles, so its c moves errorC1 double by double -- in steps below the error's own ulp only while |c| is small.  So c is first walked to where
    errorC1 meets the threshold, then the image origin is moved along the line's normal by that c: in the moved scene the meeting lies at c = 0, and the doubles around it
    are scanned for the two values"""
    sim = _sim()

    def build(K):
        c = add_lines(scene(41, 12, K=K), LINE_SEED[0], 9)
        c["min_triangulated"] = 0
        return c

    def narrow(err, thr, above, below):
        """above / below: values of c whose error lies above / not above thr -> the adjacent doubles of that kind, 32 probes a run"""
        while True:
            xs = [float(v) for v in np.linspace(above, below, 34)[1:-1]]
            xs = [v for k, v in enumerate(xs) if v not in (above, below) and v not in xs[:k]]
            if not xs: return above, below
            e = err(xs)
            k = int(np.argmax(~(e > thr))) if (~(e > thr)).any() else len(xs)
            above, below = (xs[k - 1] if k > 0 else above), (xs[k] if k < len(xs) else below)
    base = build(K0)
    rb = sim.run_plain([base])[0]
    assert rb["pose"]["ok"] == 1
    for row in np.argsort(-rb["line_err"][:, 0]):
        row = int(row); a = int(base["lp"][row, 0])
        if not rb["line_err"][row, 0] > rb["mad"][0]: break

        def errs(c0, thr):
            def f(cvals):
                vs = []
                for v in cvals:
                    c = dict(c0); fn = c0["fn1"].copy(); fn[a, 2] = v; c["fn1"] = fn; vs.append(c)
                rs = sim.run_plain(vs)
                return np.array([r["line_err"][row, 0] if r["mad"][0] == thr else np.nan for r in rs])      # where the row moves the median or the MAD: no answer
            return f
        thr = rb["mad"][0]
        cb = base["fn1"][a, 2]
        grid = [float(v) for v in cb + np.linspace(0.0, -2.0 * cb, 400)]
        eg = errs(base, thr)(grid)
        k = int(np.argmax(~(eg > thr)))
        if k == 0 or np.isnan(eg[:k + 1]).any(): continue
        ca, _ = narrow(errs(base, thr), thr, grid[k - 1], grid[k])
        l = base["fn1"][a]
        o = -ca * l[:2] / (l[0] * l[0] + l[1] * l[1])                    # l . o = -ca: the meeting moves to c = 0
        c0 = build((K0[0], K0[1], K0[2] - o[0], K0[3] - o[1]))
        r0 = sim.run_plain([c0])[0]
        thr = r0["mad"][0]
        f = errs(c0, thr)
        e = f([-1.0, 1.0])
        if r0["pose"]["ok"] != 1 or np.isnan(e).any() or (e[0] > thr) == (e[1] > thr): continue
        ca, cb = narrow(f, thr, -1.0 if e[0] > thr else 1.0, 1.0 if e[0] > thr else -1.0)
        # The walk ends on a step of the error (LineTriangulate reads the function as floats, and now and then its endpoints jump with c).  On the upper side of the
        # step the error moves with c alone, double by double: that side is followed until the error is down at the threshold, and the doubles there are scanned
        away = 1.0 if ca > cb else -1.0
        gap = f([ca])[0] - thr
        ds = [ca + away * gap * m for m in (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 5.0, 9.0)]
        ed = f(ds)
        below = [k for k in range(len(ds)) if not ed[k] > thr]
        if not below or np.isnan(ed[:below[0] + 1]).any(): continue
        k = below[0]
        ua, ub = narrow(f, thr, ds[k - 1] if k else ca, ds[k])
        # one double of c is far less than one of the error here: steps of c that move the error by about an eighth of its ulp, over a few ulps on either side
        step = 0.125 * np.spacing(thr)
        vals = [float(min(ua, ub) + step * j) for j in range(-64, 65)]
        found = {}
        for v, ev in zip(vals, f(vals)):
            c = dict(c0); fn = c0["fn1"].copy(); fn[a, 2] = v; c["fn1"] = fn
            if ev == thr: found.setdefault("at", c)
            if ev == np.nextafter(thr, np.inf): found.setdefault("above", c)
        if len(found) == 2:
            ra, rv = sim.run_plain([found["at"], found["above"]])
            if ra["line_tri"][row] == 1 and rv["line_tri"][row] == 0:      # errorC2 of the row passes: the flag follows errorC1 alone
                return [named(found["at"], "line_err_at_mad", line_row=row), named(found["above"], "line_err_above_mad", line_row=row)]
    raise AssertionError("no line gate case found")


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    out += _f_winners()
    out.append(named(scene(2, 150, planar=True, unmatched=11, extra2=3), "h_planar_twins"))          # both twins take every point: no clear winner
    out.append(named(_h_scene(3, 90, 45, unmatched=8, extra2=2), "h_winner"))
    out += _gate_cases()
    for n in (1, 50, 51, 52):                                                                          # accepted counts at the min(50, size - 1) edge
        out.append(named(scene(50 + n, n), "f_accepted_%d" % n, min_triangulated=0))
    for n in (8, 63, 64, 65, 257):                                                                     # match counts around the wave and the workgroup
        out.append(named(scene(60 + n, n, unmatched=n // 3 + 1, extra2=2), "f_matches_%d" % n, min_triangulated=min(50, n // 2)))
    c = scene(70, 100, unmatched=30)
    c["inliers"][c["rows1"][::3]] = 1                                                                  # inliers of H alone: not of this model
    out.append(named(c, "f_partial_inliers"))
    c = scene(71, 70)
    c["kp1"][c["rows1"][4], 0] = np.inf                                                                # Triangulate's point is not finite (:885)
    out.append(named(c, "f_not_finite"))
    out.append(named(scene(72, 40), "model_0", model=0))
    out.append(named(scene(73, 0, unmatched=5), "no_matches", min_triangulated=0))
    base = scene(80, 100, unmatched=10)
    for nlp in (0, 1, 2, 65):
        out.append(named(add_lines(base, 81 + nlp, nlp), "lines_%d" % nlp))
    out.append(named(add_lines(base, 90, 10, bad_index=True, swap=2), "lines_even_bad_index"))
    out.append(named(add_lines(base, 91, 9, nonfinite=3, swap=1), "lines_odd_nonfinite"))
    out.append(named(add_lines(_h_scene(3, 90, 45), 92, 12, swap=2), "h_lines"))
    out.append(named(add_lines(scene(7, 120), 93, 6), "lines_not_ok", min_triangulated=500))
    out += _line_gate_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)
