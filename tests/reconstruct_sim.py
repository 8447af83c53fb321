"""csrc/reconstruct_math.h on the host as the test modules ask for it: tests/sim/reconstruct_sim.cpp through tests/host_sim.py (plain and under
-fsanitize=address,undefined, as stand-alone programs; nothing is loaded into Python).  A case is a dict with kp1 / kp2 (float32 [n, 2]: the undistorted pt.x, pt.y), m12
(int32 [n1]), inliers (uint8 [n1], bit 0 H, bit 1 F, by keypoint 1), model (0, 1 = H, 2 = F), H21 / F21 (float32 [9]), K (fx fy cx cy), sigma, min_parallax,
min_triangulated and, for lines, kl1 (float32 [nl1, 4]: start x y, end x y), fn1 / fn2 (float64 [nl, 3]) and lp (int32 [nlp, 2]); lp None = the call without lines.
The answer per case: pose (a frontend.TWO_VIEW_POSE_DTYPE record), hyp (float32 [8, 15]: R, t, n), sel (float32 [8]: the selected cosine), stage (int32 [8, nm]),
rows_p3d (float32 [8, nm, 3]), rows_cos (float32 [8, nm]), rows_err (float32 [8, nm, 2]: squareError1 / 2, the model's own trace), p3d (float32 [n1, 3]), tri (uint8 [n1]), line_s3d / line_e3d (float32 [nlp, 3]), line_tri (uint8 [nlp]),
line_err (float64 [nlp, 2]) and mad (float64 [2]: the inlier thresholds)."""
import os
import numpy as np
import host_sim
import pkg
from host_sim import bits as _bits, ints as _ints, floats as _floats

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "reconstruct_sim.cpp")


def _bits64(a):
    return " ".join(map(str, np.ascontiguousarray(a, np.float64).view(np.uint64).ravel().tolist()))


def _doubles(tokens):
    return np.array([int(t) for t in tokens], np.uint64).view(np.float64)


def has_lines(c):
    return c.get("lp") is not None


def encode(c):
    kp1 = np.asarray(c["kp1"], np.float32).reshape(-1, 2); kp2 = np.asarray(c["kp2"], np.float32).reshape(-1, 2)
    L = has_lines(c)
    nl1, nl2, nlp = (len(c["fn1"]), len(c["fn2"]), len(c["lp"])) if L else (0, 0, 0)
    head = "%d %d %d %s %s %d %s %d %d %d %d" % (len(kp1), len(kp2), c["model"], _bits(np.float32(c["sigma"])), _bits(np.float32(c["min_parallax"])), c["min_triangulated"],
                                                _bits(np.asarray(c["K"], np.float32)), nl1, nl2, nlp, 1 if L else 0)
    parts = [head, _bits(kp1), _bits(kp2), _ints(c["m12"]), _ints(c["inliers"]), _bits(c["H21"]), _bits(c["F21"])]
    if L:
        parts += [_bits(c["kl1"]), _bits64(c["fn1"]), _bits64(c["fn2"]), _ints(c["lp"])]
    return "\n".join(parts) + "\n"


def decode(text, cases):
    fe = pkg.frontend()
    lines = text.splitlines()
    out, at = [], 0
    for c in cases:
        r = {}
        t = lines[at].split(); at += 1
        assert t[0] == "pose"
        p = np.zeros(1, fe.TWO_VIEW_POSE_DTYPE)[0]
        p["ok"], p["reason"], p["model"], p["hypothesis"], p["n_inliers"] = [int(x) for x in t[1:6]]
        p["n_good"] = [int(x) for x in t[6:14]]
        p["parallax"] = _floats(t[14:22]); p["R21"] = _floats(t[22:31]); p["t21"] = _floats(t[31:34])
        p["n_triangulated"], p["n_lines"], p["n_lines_triangulated"] = [int(x) for x in t[34:37]]
        r["pose"] = p
        hyp, sel = np.zeros((8, 15), np.float32), np.zeros(8, np.float32)
        for h in range(8):
            t = lines[at].split(); at += 1
            assert t[0] == "hyp" and int(t[1]) == h
            hyp[h] = _floats(t[2:17]); sel[h] = _floats(t[17:18])[0]
        r["hyp"], r["sel"] = hyp, sel
        st, rp, rc, re = [], [], [], []
        for h in range(8):
            t = lines[at].split(); at += 1
            assert t[0] == "rows" and int(t[1]) == h
            nm = int(t[2])
            a = np.array([int(x) for x in t[3:]], np.uint64).reshape(nm, 7)
            st.append(a[:, 0].astype(np.int32)); rp.append(a[:, 1:4].astype(np.uint32).view(np.float32)); rc.append(a[:, 4].astype(np.uint32).view(np.float32)); re.append(a[:, 5:7].astype(np.uint32).view(np.float32))
        r["stage"], r["rows_p3d"], r["rows_cos"] = np.array(st, np.int32).reshape(8, -1), np.array(rp, np.float32).reshape(8, -1, 3), np.array(rc, np.float32).reshape(8, -1)
        r["rows_err"] = np.array(re, np.float32).reshape(8, -1, 2)
        t = lines[at].split(); at += 1
        assert t[0] == "p3d"
        r["p3d"] = _floats(t[1:]).reshape(-1, 3)
        t = lines[at].split(); at += 1
        assert t[0] == "tri" and len(t) == 1 + len(c["m12"])
        r["tri"] = np.array([int(x) for x in t[1:]], np.uint8)
        t = lines[at].split(); at += 1
        assert t[0] == "lines"
        nlp = int(t[1])
        a = np.array([int(x) for x in t[2:]], np.uint64).reshape(nlp, 9)
        r["line_s3d"], r["line_e3d"] = a[:, 0:3].astype(np.uint32).view(np.float32).reshape(nlp, 3), a[:, 3:6].astype(np.uint32).view(np.float32).reshape(nlp, 3)
        r["line_tri"] = a[:, 6].astype(np.uint8)
        r["line_err"] = np.ascontiguousarray(a[:, 7:9]).view(np.float64).reshape(nlp, 2)
        t = lines[at].split(); at += 1
        assert t[0] == "mad"
        r["mad"] = _doubles(t[1:3])
        out.append(r)
    assert at == len(lines)
    return out


def run_plain(cases):
    """the plain build alone: for the searches of tests/reconstruct_cases.py, whose finds go through run() afterwards"""
    return decode(host_sim.run_plain(SRC, "".join(encode(c) for c in cases)), cases)


def run(cases):
    return decode(host_sim.run(SRC, "".join(encode(c) for c in cases)), cases)


def acos(values):
    """acos_f of csrc/reconstruct_math.h itself on float32 values, through both builds of the sim"""
    v = np.ascontiguousarray(values, np.float32).ravel()
    t = host_sim.run(SRC, "-1 %d 0\n%s\n" % (len(v), _bits(v))).split()
    assert t[0] == "acos" and len(t) == 1 + len(v)
    return _floats(t[1:])
