"""csrc/sim3_math.h on the host as the test modules ask for it.  The header holds no HIP: tests/sim/sim3_sim.cpp compiles it with plain g++, once with
-O2 -ffp-contract=off and once more under -fsanitize=address,undefined, as a stand-alone program -- both once per process, whichever module asks first; nothing is
loaded into Python.  run(cases) sends every case through both builds: both must exit 0 with an empty stderr and answer alike.

A case is a dict: kf1 / kf2 = dict(oct int32 [n], valid uint8 [n], x3dc float32 [n, 3], K float32 [4] = fx fy cx cy), sigma2 float32 [nlevels], m12 int32 [n1],
fix_scale, probability, min_inliers, max_iterations, calls (the new_iterations of successive calls on one state that starts zero-filled), sets (None or int32
[max_iterations, 3]), seed, pair.  The answer per case: n, idx1 (int [N]: mvnIndices1), img (float32 [N, 6]: P1im1, P2im2, maxErr1, maxErr2) and calls, one dict per
call: its (the iterations it ran), sets (int32 [k, 3]), mats (float32 [k, 13]: s, R, t), counts (int32 [k]), nent (float32 [k, 10]), q (float64 [k, 4]), marks
(uint8 [k, N]: mvbInliersi), state (a frontend.SIM3_STATE_DTYPE record) and inliers (uint8 [n1])."""
import os
import numpy as np
import host_sim
import pkg
from host_sim import bits as _bits, ints as _ints, floats as _floats

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "sim3_sim.cpp")


def programs():
    """(plain, sanitised): the two builds of the sim (host_sim.py)"""
    return host_sim.programs(SRC)


def encode(c):
    k1, k2 = c["kf1"], c["kf2"]
    n1, n2 = len(k1["oct"]), len(k2["oct"])
    assert len(c["m12"]) == n1
    head = "%d %d %d %d %d %d %d %d %d %d %d" % (n1, n2, len(c["sigma2"]), int(c["fix_scale"]), c["min_inliers"], c["max_iterations"], c.get("seed", 0), c.get("pair", 0),
                                                 0 if c.get("sets") is None else 1, len(c["calls"]), int(np.float64(c["probability"]).view(np.uint64)))
    parts = [head, _bits(k1["K"]), _bits(k2["K"]), _bits(c["sigma2"]), _ints(k1["oct"]), _ints(k1["valid"]), _bits(k1["x3dc"]), _ints(k2["oct"]), _ints(k2["valid"]),
             _bits(k2["x3dc"]), _ints(c["m12"])]
    if c.get("sets") is not None:
        assert np.asarray(c["sets"]).shape == (c["max_iterations"], 3)
        parts.append(_ints(c["sets"]))
    parts.append(_ints(c["calls"]))
    return "\n".join(parts) + "\n"


def decode(text, cases):
    fe = pkg.frontend()
    lines = text.splitlines()
    out, at = [], 0
    for c in cases:
        t = lines[at].split(); at += 1
        assert t[0] == "n"
        N = int(t[1])
        body = np.array([int(x) for x in t[2:]], np.uint64).reshape(N, 7)
        r = {"n": N, "idx1": body[:, 0].astype(np.int64), "img": body[:, 1:].astype(np.uint32).view(np.float32).reshape(N, 6), "calls": []}
        for _ in c["calls"]:
            its, sets, mats, counts, nent, q, marks = [], [], [], [], [], [], []
            while lines[at].startswith("hyp"):
                t = lines[at].split(); at += 1
                its.append(int(t[1])); sets.append([int(x) for x in t[2:5]]); mats.append(_floats(t[5:18])); counts.append(int(t[18]))
                nent.append(_floats(t[19:29])); q.append(np.array([int(x) for x in t[29:33]], np.uint64).view(np.float64))
                marks.append(np.zeros(0, np.uint8) if t[33] == "-" else np.frombuffer(t[33].encode(), np.uint8) - 48)
            t = lines[at].split(); at += 1
            assert t[0] == "state"
            st = np.zeros(1, fe.SIM3_STATE_DTYPE)[0]
            for k, v in zip(("its_done", "best_inliers", "best_it", "n", "max_its", "found_it", "n_inliers", "no_more"), t[1:9]):
                st[k] = int(v)
            f = _floats(t[9:22])
            st["s12"] = f[0]; st["R12"] = f[1:10]; st["t12"] = f[10:13]
            t = lines[at].split(); at += 1
            assert t[0] == "inl" and len(t) == 1 + len(c["m12"])
            k = len(its)
            r["calls"].append(dict(its=np.array(its, np.int64), sets=np.array(sets, np.int32).reshape(k, 3), mats=np.array(mats, np.float32).reshape(k, 13),
                                   counts=np.array(counts, np.int32), nent=np.array(nent, np.float32).reshape(k, 10), q=np.array(q, np.float64).reshape(k, 4),
                                   marks=np.array(marks, np.uint8).reshape(k, N), state=st, inliers=np.array([int(x) for x in t[1:]], np.uint8)))
        out.append(r)
    assert at == len(lines)
    return out


def run_plain(cases):
    """the plain build alone: for the searches of tests/sim3_cases.py, whose finds go through run() afterwards"""
    return decode(host_sim.run_plain(SRC, "".join(encode(c) for c in cases)), cases)


def run(cases):
    return decode(host_sim.run(SRC, "".join(encode(c) for c in cases)), cases)
