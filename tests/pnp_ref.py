"""PnPsolver (reference src/PnPsolver.cc) restated in numpy, independently of csrc/pnp_math.h: LAPACK (eigh, svd, lstsq, pinv) for the leaves the reference hands to
OpenCV, plain Python for the control flow, Refine literally on every qualifying iteration.  Its poses differ from the host model's by conditioning, not by design
(decision D17); its integers and booleans must not differ on the cases of tests/pnp_cases.py."""
import math
import numpy as np
from ransac_ref import hash32, draw

F32 = np.float32


def ransac_params(probability, min_inliers, max_iterations, epsilon, N):
    """SetRansacParameters (:129-152) with the minimal set of four -> (mRansacMinInliers, mRansacMaxIts); N below its own min_inliers: (that value, 0)"""
    eps = F32(epsilon)
    n_min = int(F32(N) * eps)
    n_min = max(n_min, min_inliers, 4)
    if N < n_min:
        return n_min, 0
    ratio = F32(n_min) / F32(N)
    if eps < ratio:
        eps = ratio
    if n_min == N:
        return n_min, 1
    d = math.ceil(math.log(1 - probability) / math.log(1 - float(eps) ** 3))
    return n_min, max(1, min(int(d), max_iterations))


def correspondences(c):
    """the constructor (:67-110) -> (idx: frame rows, X float32 [N, 3], uv float32 [N, 2], max_err float32 [N])"""
    nkf, nlev = len(c["xw"]), len(c["sigma2"])
    idx = [j for j in range(len(c["oct"])) if 0 <= c["assigned"][j] < nkf and c["valid"][c["assigned"][j]] and 0 <= c["oct"][j] < nlev]
    idx = np.array(idx, np.int64)
    a = np.asarray(c["assigned"], np.int64)[idx]
    X = np.asarray(c["xw"], F32).reshape(-1, 3)[a]
    uv = np.asarray(c["pt"], F32).reshape(-1, 2)[idx]
    me = np.asarray(c["sigma2"], F32)[np.asarray(c["oct"], np.int64)[idx]] * F32(c["th2"])
    return idx, X, uv, me.astype(F32)


def check_inliers(R, t, K, X, uv, max_err):
    """CheckInliers (:308-339) -> bool [N]"""
    with np.errstate(all="ignore"):
        return errors2(R, t, K, X, uv) < max_err


def errors2(R, t, K, X, uv):
    """error2 of CheckInliers (:317-327) with its float / double types -> float32 [N]"""
    fu, fv, uc, vc = [float(k) for k in np.asarray(K, F32)]
    Xd = X.astype(np.float64)
    with np.errstate(all="ignore"):
        Xc = (R[0, 0] * Xd[:, 0] + R[0, 1] * Xd[:, 1] + R[0, 2] * Xd[:, 2] + t[0]).astype(F32)
        Yc = (R[1, 0] * Xd[:, 0] + R[1, 1] * Xd[:, 1] + R[1, 2] * Xd[:, 2] + t[1]).astype(F32)
        iz = (1 / (R[2, 0] * Xd[:, 0] + R[2, 1] * Xd[:, 1] + R[2, 2] * Xd[:, 2] + t[2])).astype(F32)
        ue = uc + fu * Xc.astype(np.float64) * iz.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * iz.astype(np.float64)
        dx = (uv[:, 0].astype(np.float64) - ue).astype(F32)
        dy = (uv[:, 1].astype(np.float64) - ve).astype(F32)
        return dx * dx + dy * dy


def _lstsq(A, b):
    """the least-squares solution; NaNs where LAPACK refuses the input (a NaN or an infinity in it)"""
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return np.full(A.shape[1], np.nan)
    try:
        return np.linalg.lstsq(A, b, rcond=None)[0]
    except np.linalg.LinAlgError:
        return np.full(A.shape[1], np.nan)


def _gauss_newton(L, rho, betas):
    b = np.array(betas, np.float64)
    for _ in range(5):
        A = np.empty((6, 4)); r = np.empty(6)
        for i in range(6):
            l = L[i]
            A[i] = [2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3], l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3],
                    l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3], l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3]]
            r[i] = rho[i] - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1] + l[3] * b[0] * b[2] + l[4] * b[1] * b[2] + l[5] * b[2] * b[2] +
                             l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3] + l[9] * b[3] * b[3])
        b = b + _lstsq(A, r)      # qr_solve: the least-squares solution of a full-rank 6 x 4
    return b


def compute_pose(X, uv, K):
    """compute_pose (:477-525) on n points -> (R [3, 3], t [3], dict of the intermediates)"""
    fu, fv, uc, vc = [float(k) for k in np.asarray(K, F32)]
    pws = X.astype(np.float64); us = uv.astype(np.float64); n = len(pws)
    with np.errstate(all="ignore"):
        c0 = pws.sum(0) / n
        P = pws - c0
        dc, uct = np.linalg.eigh(P.T @ P)
        order = np.argsort(-np.abs(dc), kind="stable")
        cws = [c0] + [c0 + math.sqrt(abs(dc[o]) / n) * uct[:, o] for o in order]
        CC = np.array([[cws[j][i] - cws[0][i] for j in (1, 2, 3)] for i in range(3)])
        ci = np.linalg.pinv(CC)
        al = np.empty((n, 4))
        al[:, 1:] = (pws - c0) @ ci.T
        al[:, 0] = 1.0 - al[:, 1] - al[:, 2] - al[:, 3]
        M = np.zeros((2 * n, 12))
        for i in range(4):
            M[0::2, 3 * i] = al[:, i] * fu; M[0::2, 3 * i + 2] = al[:, i] * (uc - us[:, 0])
            M[1::2, 3 * i + 1] = al[:, i] * fv; M[1::2, 3 * i + 2] = al[:, i] * (vc - us[:, 1])
        d, u = np.linalg.eigh(M.T @ M)
        order = np.argsort(-np.abs(d), kind="stable")
        ut = u[:, order].T
        v = [ut[11], ut[10], ut[9], ut[8]]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dv = [[vi[3 * a:3 * a + 3] - vi[3 * b:3 * b + 3] for (a, b) in pairs] for vi in v]
        L = np.empty((6, 10))
        for i in range(6):
            D = lambda p, q: float(np.dot(dv[p][i], dv[q][i]))
            L[i] = [D(0, 0), 2 * D(0, 1), D(1, 1), 2 * D(0, 2), 2 * D(1, 2), D(2, 2), 2 * D(0, 3), 2 * D(1, 3), 2 * D(2, 3), D(3, 3)]
        rho = np.array([np.sum((cws[a] - cws[b]) ** 2) for (a, b) in pairs])
        betas = []
        b4 = _lstsq(L[:, [0, 1, 3, 6]], rho)
        s = -1.0 if b4[0] < 0 else 1.0
        b0 = math.sqrt(s * b4[0]) if s * b4[0] >= 0 else float("nan")
        betas.append([b0, s * b4[1] / b0, s * b4[2] / b0, s * b4[3] / b0])
        for cols in ([0, 1, 2], [0, 1, 2, 3, 4]):
            b = _lstsq(L[:, cols], rho)
            if b[0] < 0:
                b0, b1 = math.sqrt(-b[0]), (math.sqrt(-b[2]) if b[2] < 0 else 0.0)
            else:
                b0, b1 = math.sqrt(b[0]), (math.sqrt(b[2]) if b[2] > 0 else 0.0)
            if b[1] < 0:
                b0 = -b0
            betas.append([b0, b1, b[3] / b0 if len(cols) == 5 else 0.0, 0.0])
        sols = []
        for b in betas:
            b = _gauss_newton(L, rho, b)
            ccs = sum(b[i] * v[i] for i in range(4)).reshape(4, 3)
            pcs = al @ ccs
            if pcs[0, 2] < 0:
                ccs, pcs = -ccs, -pcs
            pc0, pw0 = pcs.mean(0), pws.mean(0)
            ABt = (pcs - pc0).T @ (pws - pw0)
            if np.isfinite(ABt).all():
                U, _, Vt = np.linalg.svd(ABt)
                R = U @ Vt
            else:
                R = np.full((3, 3), np.nan)
            if np.linalg.det(R) < 0:
                R[2] = -R[2]
            t = pc0 - R @ pw0
            pc = pws @ R.T + t
            ue = uc + fu * pc[:, 0] / pc[:, 2]; ve = vc + fv * pc[:, 1] / pc[:, 2]
            rep = float(np.mean(np.sqrt((us[:, 0] - ue) ** 2 + (us[:, 1] - ve) ** 2)))
            sols.append((rep, R, t, b))
    N = 1
    if sols[1][0] < sols[0][0]:
        N = 2
    if sols[2][0] < sols[N - 1][0]:
        N = 3
    return sols[N - 1][1], sols[N - 1][2], dict(N=N, rep=[s[0] for s in sols], betas=[s[3] for s in sols])


def sets_of(c, N, its):
    """the four indices of iterations its (absolute) -> list of (set, valid)"""
    out = []
    for it in its:
        if c.get("sets") is not None:
            s = np.asarray(c["sets"], np.int64).reshape(-1, 4)
            if it < len(s):
                out.append((list(s[it]), all(0 <= int(x) < N for x in s[it])))
            else:
                out.append(([-1] * 4, False))
        elif N >= 4:
            out.append((draw(N, [hash32(c.get("seed", 0), c.get("pair", 0), it, j) % (N - j) for j in range(4)]), True))
        else:
            out.append(([-1] * 4, False))
    return out


def run(c):
    """every call of the case on one solver -> dict(n, min_inliers, max_its, idx, calls: [dict(its, counts [k, 4], poses [k, 12], N, state fields, Tcw, inliers)])"""
    idx, X, uv, me = correspondences(c)
    N = len(idx)
    n_min, max_its = ransac_params(c["probability"], c["min_inliers"], c["max_iterations"], c["epsilon"], N)
    out = dict(n=N, min_inliers=n_min, max_its=max_its, idx=idx, max_err=me, calls=[])
    its_done, best_inliers, best_it, refine_ok = 0, 0, -1, 0
    best_marks, best_R, best_t = None, np.zeros((3, 3)), np.zeros(3)
    nf = len(c["oct"])
    for new_its in c["calls"]:
        r = dict(its=[], counts=[], poses=[], sets=[], found=0, found_it=-1, n_inliers=0, no_more=0, Tcw=np.zeros(12, F32), inliers=np.zeros(nf, np.uint8))
        if N < n_min:
            r["no_more"] = 1
        else:
            current = 0
            while its_done < max_its or current < new_its:
                current += 1
                it = its_done; its_done += 1
                (s, ok), = sets_of(c, N, [it])
                if ok:
                    R, t, info = compute_pose(X[s], uv[s], c["K"])
                    marks = check_inliers(R, t, c["K"], X, uv, me)
                    count = int(marks.sum())
                else:
                    R, t, info, marks, count = np.zeros((3, 3)), np.zeros(3), dict(N=0), np.zeros(N, bool), -1
                ran, rcount = 0, 0
                if count >= n_min:
                    if count > best_inliers:
                        best_inliers, best_it, best_marks, best_R, best_t = count, it, marks.copy(), R.copy(), t.copy()
                    Rr, tr, _ = compute_pose(X[best_marks], uv[best_marks], c["K"])
                    rmarks = check_inliers(Rr, tr, c["K"], X, uv, me)
                    ran, rcount = 1, int(rmarks.sum())
                    refine_ok = int(rcount > n_min)
                    if refine_ok:
                        r.update(found=1, found_it=it, n_inliers=rcount, Tcw=np.hstack([Rr, tr[:, None]]).astype(F32).ravel())
                        r["inliers"][idx[rmarks]] = 1
                r["its"].append(it); r["sets"].append(s); r["counts"].append([count, info["N"], ran, rcount]); r["poses"].append(np.hstack([R.ravel(), t]))
                if r["found"]:
                    break
            if not r["found"] and its_done >= max_its:
                r["no_more"] = 1
                if best_inliers >= n_min:
                    r.update(found=2, found_it=best_it, n_inliers=best_inliers, Tcw=np.hstack([best_R, best_t[:, None]]).astype(F32).ravel())
                    r["inliers"][idx[best_marks]] = 1
        r.update(its_done=its_done, best_inliers=best_inliers, best_it=best_it if its_done else 0, refine_ok=refine_ok, best_R=best_R.ravel().copy(), best_t=best_t.copy())
        k = len(r["its"])
        r["counts"] = np.array(r["counts"], np.int64).reshape(k, 4); r["poses"] = np.array(r["poses"], np.float64).reshape(k, 12)
        out["calls"].append(r)
    return out
