"""A numpy restatement of ReconstructF / ReconstructH / CheckRT / Triangulate (reference src/Initializer.cc:499-782, :833-1000) in float64 with LAPACK's SVD and numpy's
arccos: what csrc/reconstruct_math.h computes with decision D18's leaves, computed with none of them.  reconstruct(case) -> ok, R21, t21, p3d (by keypoint 1), tri.  The
order of the hypotheses follows the signs LAPACK gives its singular vectors, so the winner is compared as a pose, not as an index.  robust(name): the cases whose outcome
does not hang on a gate.  MEASURED: the largest deviation of the host model from this restatement over those cases; the test asserts four times that."""
import numpy as np

MEASURED = {"R21": 5.8e-8, "t21": 3.6e-7, "p3d": 1.8e-6}      # as printed by tests/test_reconstruct_ref_cpu.py::test_numpy_restatement

ON_A_GATE = ("parallax_at", "parallax_above", "parallax_below", "maxgood", "err1_", "err2_", "h_09n", "h_second", "h_d1d2", "h_d2d3", "f_tie", "f_not_finite", "line_err")


def robust(name):
    return not any(s in name for s in ON_A_GATE)


def _kmat(K):
    return np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]], np.float64)


def check_rt(R, t, K, rows, th2):
    """:833-961 over rows (u1, v1, u2, v2) of the inlier matches -> nGood, parallax, good mask, points"""
    Km = _kmat(K)
    P1 = np.hstack([Km, np.zeros((3, 1))]); P2 = Km @ np.hstack([R, t.reshape(3, 1)])
    O2 = -R.T @ t
    good = np.zeros(len(rows), bool); pts = np.zeros((len(rows), 3)); cosv = []
    for i, (u1, v1, u2, v2) in enumerate(rows):
        A = np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]])
        x = np.linalg.svd(A)[2][3]
        p = x[:3] / x[3]
        if not np.isfinite(p).all():
            continue
        n2 = p - O2
        c = p @ n2 / (np.linalg.norm(p) * np.linalg.norm(n2))
        if p[2] <= 0:
            continue
        q = R @ p + t
        if q[2] <= 0:
            continue
        e1 = (K[0] * p[0] / p[2] + K[2] - u1) ** 2 + (K[1] * p[1] / p[2] + K[3] - v1) ** 2
        e2 = (K[0] * q[0] / q[2] + K[2] - u2) ** 2 + (K[1] * q[1] / q[2] + K[3] - v2) ** 2
        if e1 > th2 or e2 > th2:
            continue
        good[i] = True; pts[i] = p; cosv.append(c)
    par = 0.0
    if cosv:
        cosv = np.sort(cosv)
        par = np.degrees(np.arccos(min(cosv[min(50, len(cosv) - 1)], 1.0)))
    return int(good.sum()), par, good, pts


def hypotheses_f(F, K):
    Km = _kmat(K)
    U, _, Vt = np.linalg.svd(Km.T @ F.reshape(3, 3).astype(np.float64) @ Km)
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    R1 = U @ W @ Vt; R2 = U @ W.T @ Vt
    R1 = -R1 if np.linalg.det(R1) < 0 else R1; R2 = -R2 if np.linalg.det(R2) < 0 else R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def hypotheses_h(H, K):
    Km = _kmat(K)
    U, w, Vt = np.linalg.svd(np.linalg.inv(Km) @ H.reshape(3, 3).astype(np.float64) @ Km)
    V = Vt.T
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = w
    if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return None
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)); aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]; x3 = [aux3, -aux3, aux3, -aux3]
    ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2); ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [ast, -ast, -ast, ast]
    asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2); cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [asp, -asp, -asp, asp]
    out = []
    for i in range(4):
        Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]])
        t = U @ (np.array([x1[i], 0, -x3[i]]) * (d1 - d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    for i in range(4):
        Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]])
        t = U @ (np.array([x1[i], 0, x3[i]]) * (d1 + d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out


def reconstruct(c):
    K = np.asarray(c["K"], np.float64)
    n1 = len(c["kp1"])
    bit = 1 if c["model"] == 1 else 2
    idx = [i for i in range(n1) if c["m12"][i] >= 0 and c["model"] != 0 and c["inliers"][i] & bit]
    rows = [(c["kp1"][i, 0], c["kp1"][i, 1], c["kp2"][c["m12"][i], 0], c["kp2"][c["m12"][i], 1]) for i in idx]
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    N = len(idx)
    fail = {"ok": 0}
    if c["model"] == 0:
        return fail
    hyps = hypotheses_h(c["H21"], K) if c["model"] == 1 else hypotheses_f(c["F21"], K)
    if hyps is None:
        return fail
    th2 = 4.0 * float(c["sigma"]) ** 2
    res = [check_rt(R, t, K, rows, th2) for R, t in hyps]
    ng = [r[0] for r in res]
    mp, mt = float(c["min_parallax"]), int(c["min_triangulated"])
    if c["model"] == 2:
        mx = max(ng)
        if mx < max(int(0.9 * N), mt) or sum(g > 0.7 * mx for g in ng) > 1:
            return fail
        w = ng.index(mx)
        if not res[w][1] > mp:
            return fail
    else:
        w = int(np.argmax(ng)); second = sorted(ng)[-2]
        if not (second < 0.75 * ng[w] and res[w][1] >= mp and ng[w] > mt and ng[w] > 0.9 * N):
            return fail
    p3d = np.zeros((n1, 3)); tri = np.zeros(n1, np.uint8)
    good = res[w][2]
    p3d[np.asarray(idx)[good]] = res[w][3][good]; tri[np.asarray(idx)[good]] = 1
    return {"ok": 1, "R21": hyps[w][0], "t21": hyps[w][1], "p3d": p3d, "tri": tri}
