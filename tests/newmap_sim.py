"""csrc/newmap_math.h on the host as the test modules ask for it: tests/sim/newmap_sim.cpp through tests/host_sim.py (plain and under -fsanitize=address,undefined, as
stand-alone programs; nothing is loaded into Python).
A point case is a dict with pose1 / pose2 (float32 [21]: Rcw[9] tcw[3] Ow[3] fx fy cx cy invfx invfy, the words of frontend.KF_POSE_DTYPE), kp1 / kp2 (float32 [n, 2]: the
undistorted pt.x, pt.y), oct1 / oct2 (int32 [n]), m12 (int32 [n1]), sf / sigma2 (float32 [nlevels]) and scale_factor.  The answer: stage (uint8 [n1]), x3d / normal
(float32 [n1, 3]), dist (float32 [n1, 2]: max, min), cos (float32 [n1]), hom (float32 [n1, 4]), nnew and the model's own trace: err (float32 [n1, 2]: the squared reprojection errors) and ratio (float32 [n1, 2]: ratioDist, ratioOctave).
A line case is a dict with pose1 / pose2, kl1 / kl2 (float32 [nl, 4]: start x y, end x y), loct1 / loct2 (int32 [nl]), fn1 / fn2 (float64 [nl, 3]), lp (int32 [nrows, 2]),
median (pKF2->ComputeSceneMedianDepth(2)), sf and free1 / free2 (uint8 [nl] or None = every line is free).  The answer: stage, s3d / e3d (float32 [nrows, 3]), normal
(float64 [nrows, 3]), dist, cos, hom (float32 [nrows, 8]: s3D, e3D), nnew and the model's own trace ratio (float32 [nrows, 5]: ratio1 .. ratio5)."""
import os
import numpy as np
import host_sim
from host_sim import bits as _bits, ints as _ints

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "newmap_sim.cpp")


def _bits64(a):
    return " ".join(map(str, np.ascontiguousarray(a, np.float64).view(np.uint64).ravel().tolist()))


def is_lines(c):
    return "lp" in c


def _rows(xy, octave):
    if not len(octave):
        return ""
    xy = np.ascontiguousarray(xy, np.float32).reshape(len(octave), -1)
    cols = [xy[:, k].view(np.uint32).astype(np.int64) for k in range(xy.shape[1])] + [np.asarray(octave, np.int64)]
    return _ints(np.stack(cols, axis=1))


def encode(c):
    sf = np.asarray(c["sf"], np.float32)
    if not is_lines(c):
        head = "0 %d %d %d %s" % (len(c["oct1"]), len(c["oct2"]), len(sf), _bits(np.float32(c["scale_factor"])))
        parts = [head, _bits(c["pose1"]), _bits(c["pose2"]), _bits(sf), _bits(c["sigma2"]), _rows(c["kp1"], c["oct1"]), _rows(c["kp2"], c["oct2"]), _ints(c["m12"])]
    else:
        free = c.get("free1") is not None
        head = "1 %d %d %d %d %s %d" % (len(c["loct1"]), len(c["loct2"]), len(c["lp"]), len(sf), _bits(np.float32(c["median"])), 1 if free else 0)
        parts = [head, _bits(c["pose1"]), _bits(c["pose2"]), _bits(sf), _rows(c["kl1"], c["loct1"]), _bits64(c["fn1"]), _rows(c["kl2"], c["loct2"]), _bits64(c["fn2"]), _ints(c["lp"])]
        if free:
            parts += [_ints(c["free1"]), _ints(c["free2"])]
    return "\n".join(parts) + "\n"


def decode(text, cases):
    lines = text.splitlines()
    assert len(lines) == len(cases), (len(lines), len(cases))
    out = []
    for c, ln in zip(cases, lines):
        t = ln.split()
        n, nnew = int(t[1]), int(t[2])
        if not is_lines(c):
            assert t[0] == "points" and n == len(c["oct1"])
            a = np.array([int(x) for x in t[3:]], np.uint64).reshape(n, 18)
            f = np.ascontiguousarray(a[:, 1:].astype(np.uint32)).view(np.float32)
            out.append({"stage": a[:, 0].astype(np.uint8), "x3d": f[:, 0:3].copy(), "normal": f[:, 3:6].copy(), "dist": f[:, 6:8].copy(), "cos": f[:, 8].copy(),
                        "hom": f[:, 9:13].copy(), "err": f[:, 13:15].copy(), "ratio": f[:, 15:17].copy(), "nnew": nnew})
        else:
            assert t[0] == "lines" and n == len(c["lp"])
            a = np.array([int(x) for x in t[3:]], np.uint64).reshape(n, 26)
            f = lambda lo, hi: np.ascontiguousarray(a[:, lo:hi].astype(np.uint32)).view(np.float32)
            out.append({"stage": a[:, 0].astype(np.uint8), "s3d": f(1, 4), "e3d": f(4, 7), "normal": np.ascontiguousarray(a[:, 7:10]).view(np.float64), "dist": f(10, 12),
                        "cos": f(12, 13)[:, 0].copy(), "hom": f(13, 21), "ratio": f(21, 26), "nnew": nnew})
    return out


def run_plain(cases):
    """the plain build alone: for searches, whose finds go through run() afterwards"""
    return decode(host_sim.run_plain(SRC, "".join(encode(c) for c in cases)), cases)


def run(cases):
    return decode(host_sim.run(SRC, "".join(encode(c) for c in cases)), cases)
