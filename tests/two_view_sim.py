"""csrc/two_view_math.h on the host as the test modules ask for it.  The header holds no HIP: tests/sim/two_view_sim.cpp compiles it with plain g++, once with
-O2 -ffp-contract=off and once more under -fsanitize=address,undefined, as a stand-alone program -- both once per process, whichever module asks first; nothing is
loaded into Python.  run(cases) sends every case through both builds: both must exit 0 with an empty stderr and answer alike.  A case is a dict with kp1 / kp2
(float32 [n, 2]: the undistorted pt.x, pt.y), m12 (int32 [n1]), sets (None or int32 [iterations, 8]), iterations, sigma, seed and pair; the answer per case is a dict
with norm (float32 [8]), sets (int32 [iterations, 8]), mats (float32 [iterations, 6, 9]: Hn, H21i, H12i, Fn, F21i and Fpre, which the testing tap does not return), scores (float32 [iterations, 2]), result (a
frontend.TWO_VIEW_RESULT_DTYPE record) and inliers (uint8 [n1]); a pair below 8 matches has zeros in sets, mats and scores, as the testing tap has."""
import os
import numpy as np
import host_sim
import pkg
from host_sim import bits as _bits, ints as _ints, floats as _floats

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "two_view_sim.cpp")


def programs():
    """(plain, sanitised): the two builds of the sim (host_sim.py)"""
    return host_sim.programs(SRC)


def encode(c):
    kp1 = np.asarray(c["kp1"], np.float32).reshape(-1, 2); kp2 = np.asarray(c["kp2"], np.float32).reshape(-1, 2)
    head = "%d %d %d %s %d %d %d" % (len(kp1), len(kp2), c["iterations"], _bits(np.float32(c["sigma"])), c.get("seed", 0), c.get("pair", 0), 0 if c.get("sets") is None else 1)
    parts = [head, _bits(kp1), _bits(kp2), _ints(c["m12"])]
    if c.get("sets") is not None:
        assert np.asarray(c["sets"]).shape == (c["iterations"], 8)
        parts.append(_ints(c["sets"]))
    return "\n".join(parts) + "\n"


def decode(text, cases):
    fe = pkg.frontend()
    lines = text.splitlines()
    out, at = [], 0
    for c in cases:
        it = c["iterations"]
        r = {"sets": np.zeros((it, 8), np.int32), "mats": np.zeros((it, 6, 9), np.float32), "scores": np.zeros((it, 2), np.float32)}
        t = lines[at].split(); at += 1
        assert t[0] == "norm"
        r["norm"] = _floats(t[1:])
        while lines[at].startswith("hyp"):
            t = lines[at].split(); at += 1
            i = int(t[1])
            r["sets"][i] = [int(x) for x in t[2:10]]
            r["mats"][i] = _floats(t[10:64]).reshape(6, 9)
            r["scores"][i] = _floats(t[64:66])
        t = lines[at].split(); at += 1
        assert t[0] == "res"
        res = np.zeros(1, fe.TWO_VIEW_RESULT_DTYPE)[0]
        res["nmatches"], res["model"], res["best_it_h"], res["best_it_f"] = [int(x) for x in t[1:5]]
        res["score_h"], res["score_f"], res["rh"] = _floats(t[5:8])
        res["H21"] = _floats(t[8:17]); res["F21"] = _floats(t[17:26])
        r["result"] = res
        t = lines[at].split(); at += 1
        assert t[0] == "inl" and len(t) == 1 + len(c["m12"])
        r["inliers"] = np.array([int(x) for x in t[1:]], np.uint8)
        out.append(r)
    assert at == len(lines)
    return out


def run_plain(cases):
    """the plain build alone: for the searches of tests/two_view_cases.py, whose finds go through run() afterwards"""
    return decode(host_sim.run_plain(SRC, "".join(encode(c) for c in cases)), cases)


def run(cases):
    return decode(host_sim.run(SRC, "".join(encode(c) for c in cases)), cases)
