"""Sim3Solver (reference src/Sim3Solver.cc) restated in numpy, one numpy operation per source operation (scalars, or arrays over the correspondences where the source loops
over them), float32 where the source has float and float64 where it has double.  Written from the reference's text and decision D16's wording, independently of
csrc/sim3_math.h: the constructor's filters and values (:62-109), SetRansacParameters (:114-138), the draw of :166-177 given the random integers, iterate's control flow
(:158-207) given the counts, ComputeSim3 (:226-337) around the eigenvector, CheckInliers (:340-364) and Project (:382-403).  The Jacobi eigenvector is the sim's (it is
checked against LAPACK in tests/test_sim3_cases_cpu.py); everything downstream of it is recomputed here."""
import math
import numpy as np
from ransac_ref import mix32, hash32, draw      # the draw of :163-177 given the random integers, and the library's stand-in for rand()

f32, f64 = np.float32, np.float64


def max_its(probability, min_inliers, max_iterations, N):
    """:125-135 with libm (math.log and math.pow are the C library's)"""
    epsilon = f32(f32(min_inliers) / f32(N))
    if min_inliers == N:
        n = 1
    else:
        n = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(epsilon), 3)))
    return max(1, min(n, max_iterations))


def max_error(sigma2):
    """:87-88: a size_t"""
    return f32(int(f64(9.210) * f64(f32(sigma2))))


def camera_to_image(X, K):
    """:417-421 over rows of X (float32 [n, 3]); K = fx fy cx cy"""
    X = np.asarray(X, f32).reshape(-1, 3); fx, fy, cx, cy = [f32(k) for k in K]
    with np.errstate(all="ignore"):
        invz = f32(1) / X[:, 2]
        x = X[:, 0] * invz; y = X[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], 1).astype(f32)


def correspondences(c):
    """:62-109: (idx1, idx2, X1, X2, P1im1, P2im2, maxErr1, maxErr2) in mvnIndices1's order"""
    k1, k2 = c["kf1"], c["kf2"]
    n1, n2, nl = len(k1["oct"]), len(k2["oct"]), len(c["sigma2"])
    i1 = [i for i in range(n1) if 0 <= c["m12"][i] < n2 and k1["valid"][i] and k2["valid"][c["m12"][i]] and 0 <= k1["oct"][i] < nl and 0 <= k2["oct"][c["m12"][i]] < nl]
    i1 = np.array(i1, np.int64); i2 = np.asarray(c["m12"], np.int64)[i1]
    X1 = np.asarray(k1["x3dc"], f32).reshape(-1, 3)[i1]; X2 = np.asarray(k2["x3dc"], f32).reshape(-1, 3)[i2]
    e1 = np.array([max_error(c["sigma2"][o]) for o in np.asarray(k1["oct"])[i1]], f32); e2 = np.array([max_error(c["sigma2"][o]) for o in np.asarray(k2["oct"])[i2]], f32)
    return i1, i2, X1, X2, camera_to_image(X1, k1["K"]), camera_to_image(X2, k2["K"]), e1, e2


def _mul(A, B):
    """the stand-in's A * B in float32: ((a0 b0 + a1 b1) + a2 b2), row by row"""
    A = np.asarray(A, f32); B = np.asarray(B, f32)
    out = np.zeros((A.shape[0], B.shape[1]), f32)
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            acc = f32(A[i, 0] * B[0, j])
            for k in range(1, A.shape[1]):
                acc = f32(acc + f32(A[i, k] * B[k, j]))
            out[i, j] = acc
    return out


def _centroid(P):
    """:217-223: cv::reduce SUM in column order, C / 3 as (float)(c * (1.0 / 3))"""
    C = np.zeros(3, f32); Pr = np.zeros((3, 3), f32)
    for i in range(3):
        s = f32(f32(P[i, 0] + P[i, 1]) + P[i, 2])
        C[i] = f32(f64(s) * (f64(1.0) / f64(3.0)))
        for j in range(3):
            Pr[i, j] = f32(P[i, j] - C[i])
    return Pr, C


def n_entries(P1, P2):
    """:238-260: Pr1, Pr2, O1, O2 and N11 N12 N13 N14 N22 N23 N24 N33 N34 N44 (float sums, left to right)"""
    with np.errstate(all="ignore"):
        Pr1, O1 = _centroid(P1); Pr2, O2 = _centroid(P2)
        M = _mul(Pr2, Pr1.T)
        n = [f32(f32(M[0, 0] + M[1, 1]) + M[2, 2]), f32(M[1, 2] - M[2, 1]), f32(M[2, 0] - M[0, 2]), f32(M[0, 1] - M[1, 0]), f32(f32(M[0, 0] - M[1, 1]) - M[2, 2]),
             f32(M[0, 1] + M[1, 0]), f32(M[2, 0] + M[0, 2]), f32(f32(f32(-M[0, 0]) + M[1, 1]) - M[2, 2]), f32(M[1, 2] + M[2, 1]), f32(f32(f32(-M[0, 0]) - M[1, 1]) + M[2, 2])]
    return Pr1, Pr2, O1, O2, np.array(n, f32)


def n_matrix(n):
    a, b, c, d, e, f, g, h, i, j = [f64(x) for x in n]
    return np.array([[a, b, c, d], [b, e, f, g], [c, f, h, i], [d, g, i, j]], f64)


def rotation_closed_form(q):
    """D16: R = I + (2 / (w^2 + v.v)) (w [v]x + [v]x^2) in float64, element by element, rounded once"""
    w, x, y, z = [f64(t) for t in q]
    if x == 0 and y == 0 and z == 0:
        return np.full((3, 3), np.nan, f32)
    with np.errstate(all="ignore"):
        k = f64(2.0) / (((w * w + x * x) + y * y) + z * z)
        R = [[1.0 - k * (y * y + z * z), k * (x * y - w * z), k * (x * z + w * y)],
             [k * (x * y + w * z), 1.0 - k * (x * x + z * z), k * (y * z - w * x)],
             [k * (x * z - w * y), k * (y * z + w * x), 1.0 - k * (x * x + y * y)]]
    return np.array(R, f64).astype(f32)


def rotation_literal(q):
    """:274-284 in float64: ang = atan2(|v|, w), vec = 2 ang v / |v|, Rodrigues' formula R = cos I + (1 - cos) r r^T + sin [r]x.  Returns float64 [3, 3]"""
    w = f64(q[0]); v = np.asarray(q[1:], f64)
    nv = np.sqrt(v @ v)
    ang = np.arctan2(nv, w)
    vec = 2 * ang * v / nv
    theta = np.sqrt(vec @ vec)
    r = vec / theta
    rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], f64)
    return np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(r, r) + np.sin(theta) * rx


def finish_sim3(Pr1, Pr2, O1, O2, R, fix_scale):
    """:288-316 from mR12i (float32 [3, 3]): ms12i, mt12i"""
    with np.errstate(all="ignore"):
        P3 = _mul(R, Pr2)
        if not fix_scale:
            nom = f64(0); den = f64(0)
            for i in range(3):
                for j in range(3):
                    nom = nom + f64(Pr1[i, j]) * f64(P3[i, j])
            aux = (P3 * P3).astype(f32)
            for i in range(3):
                for j in range(3):
                    den = den + f64(aux[i, j])
            s = f32(nom / den)
        else:
            s = f32(1.0)
        sR = (R.astype(f64) * f64(s)).astype(f32)
        t = (O1 - _mul(sR, O2.reshape(3, 1)).reshape(3)).astype(f32)
    return s, t


def transforms(s, R, t):
    """:323-336: (sR, t12, sRinv, t21)"""
    with np.errstate(all="ignore"):
        R = np.asarray(R, f32).reshape(3, 3); t = np.asarray(t, f32).reshape(3)
        sR = (R.astype(f64) * f64(f32(s))).astype(f32)
        sRinv = (R.T.astype(f64) * (f64(1.0) / f64(f32(s)))).astype(f32)
        tinv = _mul(-sRinv, t.reshape(3, 1)).reshape(3)
    return sR, t, sRinv, tinv


def project(A, t, X, K):
    """:396-401 over rows of X"""
    with np.errstate(all="ignore"):
        c = np.stack([((A[i, 0] * X[:, 0] + A[i, 1] * X[:, 1]) + A[i, 2] * X[:, 2]) + t[i] for i in range(3)], 1).astype(f32)
    return camera_to_image(c, K)


def errors(s, R, t, X1, X2, p1, p2, K1, K2):
    """:343-354: err1, err2 (float32 [N])"""
    sR, t12, sRinv, t21 = transforms(s, R, t)
    with np.errstate(all="ignore"):
        d1 = (p1 - project(sR, t12, X2, K1)).astype(f32); d2 = (project(sRinv, t21, X1, K2) - p2).astype(f32)
        e1 = (d1[:, 0].astype(f64) * d1[:, 0].astype(f64) + d1[:, 1].astype(f64) * d1[:, 1].astype(f64)).astype(f32)
        e2 = (d2[:, 0].astype(f64) * d2[:, 0].astype(f64) + d2[:, 1].astype(f64) * d2[:, 1].astype(f64)).astype(f32)
    return e1, e2


def check_inliers(s, R, t, X1, X2, p1, p2, e1max, e2max, K1, K2):
    e1, e2 = errors(s, R, t, X1, X2, p1, p2, K1, K2)
    with np.errstate(all="ignore"):
        return (e1 < e1max) & (e2 < e2max)


def iterate(counts, first_it, state, min_inliers, maxits, new_iterations):
    """:158-207 on the counts of the iterations from first_it on (-1: a set that cannot become the best).  state = (its_done, best_inliers, best_it); returns
    (its_done, best_inliers, best_it, found_it, n_inliers, no_more)"""
    its_done, best, best_it = state
    cur = 0
    while its_done < maxits and cur < new_iterations:
        cur += 1
        it = its_done; its_done += 1
        c = counts[it - first_it]
        if c >= 0 and c >= best:
            best, best_it = c, it
            if c > min_inliers:
                return its_done, best, best_it, it, c, 0
    return its_done, best, best_it, -1, 0, int(its_done >= maxits)
