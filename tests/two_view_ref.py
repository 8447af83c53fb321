"""The reference-owned parts of Initializer::Initialize (reference src/Initializer.cc) restated in numpy, one numpy operation per source operation (scalars, or arrays over the matches where the source loops over them), float32 where
the source has float and float64 where it has double.  Written from the reference's text, independently of csrc/two_view_math.h: Normalize (:784-830), CheckHomography and
CheckFundamental (:334-497), the draw of :93-108 given the random integers, and the selection (:118, :143, :196, :246).  The 8-point solves and the matrix compositions are
OpenCV's (decision D15) and are not here: the Check functions take the matrices the sim made."""
import numpy as np
from ransac_ref import mix32, hash32, draw      # the draw of :93-108 given the random integers, and the library's stand-in for rand()

f32, f64 = np.float32, np.float64


def normalize(xy):
    """:784-830 on the keypoints' pt (float32 [n, 2]).  Returns (vNormalizedPoints float32 [n, 2], T float32 [3, 3])"""
    xy = np.asarray(xy, f32)
    N = len(xy)
    with np.errstate(all="ignore"):
        meanX = f32(0); meanY = f32(0)
        for i in range(N):
            meanX = f32(meanX + xy[i, 0])
            meanY = f32(meanY + xy[i, 1])
        meanX = f32(meanX / f32(N))
        meanY = f32(meanY / f32(N))
        meanDevX = f32(0); meanDevY = f32(0)
        pts = np.zeros((N, 2), f32)
        for i in range(N):
            pts[i, 0] = f32(xy[i, 0] - meanX)
            pts[i, 1] = f32(xy[i, 1] - meanY)
            meanDevX = f32(meanDevX + np.abs(pts[i, 0]))
            meanDevY = f32(meanDevY + np.abs(pts[i, 1]))
        meanDevX = f32(meanDevX / f32(N))
        meanDevY = f32(meanDevY / f32(N))
        sX = f32(f64(1.0) / f64(meanDevX))
        sY = f32(f64(1.0) / f64(meanDevY))
        for i in range(N):
            pts[i, 0] = f32(pts[i, 0] * sX)
            pts[i, 1] = f32(pts[i, 1] * sY)
        T = np.eye(3, dtype=f32)
        T[0, 0] = sX
        T[1, 1] = sY
        T[0, 2] = f32(f32(-meanX) * sX)
        T[1, 2] = f32(f32(-meanY) * sY)
    return pts, T


def match_rows(kp1, kp2, m12):
    """mvMatches12 (:67-76) as rows (u1, v1, u2, v2) in ascending keypoint-1 index, and the keypoint-1 index of every row"""
    kp1 = np.asarray(kp1, f32).reshape(-1, 2); kp2 = np.asarray(kp2, f32).reshape(-1, 2)
    idx = [i for i in range(len(kp1)) if 0 <= m12[i] < len(kp2)]
    rows = np.array([[kp1[i, 0], kp1[i, 1], kp2[m12[i], 0], kp2[m12[i], 1]] for i in idx], f32).reshape(-1, 4)
    return rows, np.array(idx, np.int64)


def _inv_sigma_square(sigma):
    sigma = f32(sigma)
    return f32(f64(1.0) / f64(f32(sigma * sigma)))


def _cols(rows):
    rows = np.asarray(rows, f32).reshape(-1, 4)
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


def _recip(x):
    """1.0 / x of the source: the float operand widened, the division in double, the quotient stored to a float"""
    return (f64(1.0) / x.astype(f64)).astype(f32)


def homography_terms(H21, H12, rows, sigma):
    """the per-match quantities of :366-414 for all matches at once (every array operation below is the source's scalar operation on each match, in float32):
    (chiSquare1, chiSquare2) float32 [N, 2]"""
    h11, h12, h13, h21, h22, h23, h31, h32, h33 = [f32(x) for x in np.asarray(H21, f32).ravel()]
    h11inv, h12inv, h13inv, h21inv, h22inv, h23inv, h31inv, h32inv, h33inv = [f32(x) for x in np.asarray(H12, f32).ravel()]
    invSigmaSquare = _inv_sigma_square(sigma)
    u1, v1, u2, v2 = _cols(rows)
    with np.errstate(all="ignore"):
        w2in1inv = _recip(h31inv * u2 + h32inv * v2 + h33inv)
        u2in1 = (h11inv * u2 + h12inv * v2 + h13inv) * w2in1inv
        v2in1 = (h21inv * u2 + h22inv * v2 + h23inv) * w2in1inv
        squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)
        chiSquare1 = squareDist1 * invSigmaSquare
        w1in2inv = _recip(h31 * u1 + h32 * v1 + h33)
        u1in2 = (h11 * u1 + h12 * v1 + h13) * w1in2inv
        v1in2 = (h21 * u1 + h22 * v1 + h23) * w1in2inv
        squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)
        chiSquare2 = squareDist2 * invSigmaSquare
    out = np.stack([chiSquare1, chiSquare2], 1)
    assert out.dtype == f32
    return out


def fundamental_terms(F21, rows, sigma):
    """the per-match quantities of :442-494, as homography_terms: (chiSquare1, chiSquare2) float32 [N, 2]"""
    f11, f12, f13, f21, f22, f23, f31, f32_, f33 = [f32(x) for x in np.asarray(F21, f32).ravel()]
    invSigmaSquare = _inv_sigma_square(sigma)
    u1, v1, u2, v2 = _cols(rows)
    with np.errstate(all="ignore"):
        a2 = f11 * u1 + f12 * v1 + f13
        b2 = f21 * u1 + f22 * v1 + f23
        c2 = f31 * u1 + f32_ * v1 + f33
        num2 = a2 * u2 + b2 * v2 + c2
        squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2)
        chiSquare1 = squareDist1 * invSigmaSquare
        a1 = f11 * u2 + f21 * v2 + f31
        b1 = f12 * u2 + f22 * v2 + f32_
        c1 = f13 * u2 + f23 * v2 + f33
        num1 = a1 * u1 + b1 * v1 + c1
        squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1)
        chiSquare2 = squareDist2 * invSigmaSquare
    out = np.stack([chiSquare1, chiSquare2], 1)
    assert out.dtype == f32
    return out


def score_terms(chi, th, th_score):
    """the terms the loops of :366-414 / :442-494 add, in the order they add them (None where a term is not added), and bIn per match"""
    terms, inl = [], np.zeros(len(chi), bool)
    with np.errstate(all="ignore"):
        for i in range(len(chi)):
            bIn = True
            for k in (0, 1):
                if chi[i, k] > th:
                    bIn = False
                else:
                    terms.append(f32(th_score - chi[i, k]))
            inl[i] = bIn
    return terms, inl


def sum_in_order(terms):
    s = f32(0)
    with np.errstate(all="ignore"):
        for t in terms:
            s = f32(s + t)
    return s


TH_H, TH_F, TH_SCORE = f32(5.991), f32(3.841), f32(5.991)


def check_homography(H21, H12, rows, sigma):
    """:334-417: (score float32, vbMatchesInliers bool [N])"""
    terms, inl = score_terms(homography_terms(H21, H12, rows, sigma), TH_H, TH_H)
    return sum_in_order(terms), inl


def check_fundamental(F21, rows, sigma):
    """:419-497"""
    terms, inl = score_terms(fundamental_terms(F21, rows, sigma), TH_F, TH_SCORE)
    return sum_in_order(terms), inl


def select(scores):
    """:168-201 / :218-251 over the scores of the iterations in order: (best score, winning iteration or -1)"""
    best, it = f32(0), -1
    for i, s in enumerate(scores):
        if f32(s) > best:
            best, it = f32(s), i
    return best, it


def model(SH, SF):
    """:118, :143: (RH float32, 1 = H / 2 = F)"""
    with np.errstate(all="ignore"):
        RH = f32(f32(SH) / f32(f32(SH) + f32(SF)))
    return RH, 1 if f64(RH) > 0.40 else 2
