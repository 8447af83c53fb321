"""An independent restatement of the two loop bodies of the map-creation unit in numpy float64, with the 4 x 4 null vector from LAPACK (np.linalg.svd) instead of the
Jacobi solver of csrc/reconstruct_math.h: what tests/test_newmap_ref_cpu.py compares the host model with on stage, counts and coordinates.  It shares no code with
csrc/newmap_math.h and does not try to reproduce its bits: every gate also returns how far, relatively, the compared value was from its threshold, and a row whose
smallest such margin is below the caller's bound is not well conditioned -- its stage may differ between float32 and float64 -- and is left out of the comparison.
Inputs are the cases of tests/newmap_cases.py; the quirks of the reference (key line 2 normalised with camera 1's intrinsics, the neighbour's median depth in all five
ratios) are restated here too, because they are what the reference computes."""
import numpy as np


def _pose(p):
    p = np.asarray(p, np.float64)
    return dict(R=p[:9].reshape(3, 3), t=p[9:12], O=p[12:15], fx=p[15], fy=p[16], cx=p[17], cy=p[18], ifx=p[19], ify=p[20])


def _clamp(o, n):
    return min(max(int(o), 0), n - 1)


class _Gates:
    """collects the margin of every comparison a row makes"""
    def __init__(self):
        self.margin = np.inf

    def lt(self, a, b):      # a < b
        self.margin = min(self.margin, abs(a - b) / max(abs(a), abs(b), 1e-300)) if np.isfinite(a) and np.isfinite(b) else self.margin
        return a < b


def _null(A, g):
    _, s, vt = np.linalg.svd(A)
    g.margin = min(g.margin, (s[2] - s[3]) / max(s[0], 1e-300))      # a smallest singular value that is not separated leaves the null vector open
    return vt[3]


def _cos(P1, xn1, P2, xn2):
    with np.errstate(all="ignore"):
        r1, r2 = P1["R"].T @ xn1, P2["R"].T @ xn2
        return (r1 @ r2) / (np.linalg.norm(r1) * np.linalg.norm(r2))


def _tcw(P):
    return np.concatenate([P["R"], P["t"][:, None]], 1)


def point_rows(c):
    """-> stage [n1], x3d [n1, 3], normal [n1, 3], dist [n1, 2], margin [n1] (float64)"""
    P1, P2 = _pose(c["pose1"]), _pose(c["pose2"])
    sf, s2 = np.asarray(c["sf"], np.float64), np.asarray(c["sigma2"], np.float64)
    nl, n1, n2 = len(sf), len(c["oct1"]), len(c["oct2"])
    rf = 1.5 * float(np.float32(c["scale_factor"]))
    stage = np.zeros(n1, np.int32); x3d = np.zeros((n1, 3)); normal = np.zeros((n1, 3)); dist = np.zeros((n1, 2)); margin = np.full(n1, np.inf)
    T1, T2 = _tcw(P1), _tcw(P2)
    for i in range(n1):
        m = int(c["m12"][i])
        if m < 0 or m >= n2:
            stage[i] = 1; continue
        g = _Gates()
        k1, k2 = np.asarray(c["kp1"][i], np.float64), np.asarray(c["kp2"][m], np.float64)
        l1, l2 = _clamp(c["oct1"][i], nl), _clamp(c["oct2"][m], nl)
        with np.errstate(all="ignore"):
            xn1 = np.array([(k1[0] - P1["cx"]) * P1["ifx"], (k1[1] - P1["cy"]) * P1["ify"], 1.0]); xn2 = np.array([(k2[0] - P2["cx"]) * P2["ifx"], (k2[1] - P2["cy"]) * P2["ify"], 1.0])
        cs = _cos(P1, xn1, P2, xn2)
        if not np.isfinite(cs) or not (g.lt(0.0, cs) and g.lt(cs, 0.9998)):
            stage[i] = 2; margin[i] = g.margin; continue
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
        h = _null(A, g)
        g.margin = min(g.margin, abs(h[3]))
        with np.errstate(all="ignore"):
            x = h[:3] / h[3]
        def finish(s):
            stage[i] = s; margin[i] = g.margin
        c1, c2 = P1["R"] @ x + P1["t"], P2["R"] @ x + P2["t"]
        if not g.lt(0.0, c1[2]): finish(4); continue
        if not g.lt(0.0, c2[2]): finish(5); continue
        e1 = (P1["fx"] * c1[0] / c1[2] + P1["cx"] - k1[0]) ** 2 + (P1["fy"] * c1[1] / c1[2] + P1["cy"] - k1[1]) ** 2
        if g.lt(5.991 * s2[l1], e1): finish(6); continue
        e2 = (P2["fx"] * c2[0] / c2[2] + P2["cx"] - k2[0]) ** 2 + (P2["fy"] * c2[1] / c2[2] + P2["cy"] - k2[1]) ** 2
        if g.lt(5.991 * s2[l2], e2): finish(7); continue
        d1, d2 = np.linalg.norm(x - P1["O"]), np.linalg.norm(x - P2["O"])
        g.margin = min(g.margin, d1, d2)
        if d1 == 0 or d2 == 0: finish(8); continue
        rd, ro = d2 / d1, sf[l1] / sf[l2]
        if g.lt(rd * rf, ro) or g.lt(ro * rf, rd): finish(9); continue
        finish(0)
        x3d[i] = x
        normal[i] = ((x - P1["O"]) / d1 + (x - P2["O"]) / d2) / 2
        dist[i, 0] = d1 * sf[l1]; dist[i, 1] = dist[i, 0] / sf[nl - 1]
    return stage, x3d, normal, dist, margin


def line_rows(c):
    """-> stage [nrows], s3d, e3d, normal [nrows, 3], dist [nrows, 2], margin [nrows] (float64)"""
    P1, P2 = _pose(c["pose1"]), _pose(c["pose2"])
    sf = np.asarray(c["sf"], np.float64)
    nl, nl1, nl2, nr = len(sf), len(c["loct1"]), len(c["loct2"]), len(c["lp"])
    med = float(np.float32(c["median"]))
    stage = np.zeros(nr, np.int32); s3d = np.zeros((nr, 3)); e3d = np.zeros((nr, 3)); normal = np.zeros((nr, 3)); dist = np.zeros((nr, 2)); margin = np.full(nr, np.inf)
    T1, T2 = _tcw(P1), _tcw(P2)
    Km = lambda P: np.array([[P["fx"], 0, P["cx"]], [0, P["fy"], P["cy"]], [0, 0, 1.0]])
    M1, M2 = Km(P1) @ T1, Km(P2) @ T2
    nrm1 = lambda x, y: np.array([(x - P1["cx"]) * P1["ifx"], (y - P1["cy"]) * P1["ify"], 1.0])      # camera 1's intrinsics for BOTH key lines (:1025-1035)
    for r in range(nr):
        a, b = int(c["lp"][r, 0]), int(c["lp"][r, 1])
        if a < 0 or a >= nl1 or b < 0 or b >= nl2:
            stage[r] = 1; continue
        if c.get("free1") is not None and (not c["free1"][a] or not c["free2"][b]):
            stage[r] = 2; continue
        g = _Gates()
        def finish(s):
            stage[r] = s; margin[r] = g.margin
        k1, k2 = np.asarray(c["kl1"][a], np.float64), np.asarray(c["kl2"][b], np.float64)
        f1 = np.asarray(c["fn1"][a], np.float32).astype(np.float64); f2 = np.asarray(c["fn2"][b], np.float32).astype(np.float64)      # klF is a float matrix
        S1, E1, S2, E2 = nrm1(k1[0], k1[1]), nrm1(k1[2], k1[3]), nrm1(k2[0], k2[1]), nrm1(k2[2], k2[3])
        cs = _cos(P1, (S1 + E1) / 2, P2, (S2 + E2) / 2)
        if not np.isfinite(cs) or not (g.lt(0.0, cs) and g.lt(cs, 0.98)): finish(3); continue
        pts = []
        for X in (S1, E1):
            A = np.stack([f1 @ M1, f2 @ M2, X[0] * T1[2] - T1[0], X[1] * T1[2] - T1[1]])
            h = _null(A, g)
            g.margin = min(g.margin, abs(h[3]))
            with np.errstate(all="ignore"):
                pts.append(h[:3] / h[3])
        s, e = pts
        d = [np.linalg.norm(s - P1["O"]), np.linalg.norm(s - P2["O"]), np.linalg.norm(e - s), np.linalg.norm(e - P1["O"]), np.linalg.norm(e - P2["O"])]
        if g.lt(d[0] / med, 0.3): finish(6); continue
        if g.lt(d[1] / med, 0.3): finish(7); continue
        if g.lt(0.61, d[2] / med): finish(8); continue
        if g.lt(d[3] / med, 0.3): finish(9); continue
        if g.lt(d[4] / med, 0.3): finish(10); continue
        z = [(P1["R"] @ s + P1["t"])[2], (P2["R"] @ s + P2["t"])[2], (P1["R"] @ e + P1["t"])[2], (P2["R"] @ e + P2["t"])[2]]
        done = False
        for k in range(4):
            if not g.lt(0.0, z[k]):
                finish(11 + k); done = True; break
        if done: continue
        finish(0)
        mid = 0.5 * (s + e)
        n1, n2 = mid - P1["O"], mid - P2["O"]
        s3d[r], e3d[r] = s, e
        normal[r] = (n1 / np.linalg.norm(n1) + n2 / np.linalg.norm(n2)) / 2
        dist[r, 0] = np.linalg.norm(mid - P1["O"]) * sf[_clamp(c["loct1"][a], nl)]; dist[r, 1] = dist[r, 0] / sf[nl - 1]
    return stage, s3d, e3d, normal, dist, margin
