"""csrc/pnp_math.h on the host as the test modules ask for it.  The header holds no HIP: tests/sim/pnp_sim.cpp compiles it with plain g++, once with
-O2 -ffp-contract=off and once more under -fsanitize=address,undefined, as a stand-alone program (host_sim.py); nothing is loaded into Python.  run(cases) sends
every case through both builds: both must exit 0 with an empty stderr and answer alike.

A case is a dict: oct int32 [nf], pt float32 [nf, 2] (mvKeysUn), K float32 [4] = fx fy cx cy, xw float32 [nkf, 3], valid uint8 [nkf], assigned int32 [nf], sigma2
float32 [nlevels], probability, min_inliers, max_iterations, epsilon, th2, calls (the new_iterations of successive calls on one state that starts zero-filled), sets
(None or int32 [nsets, 4]), seed, pair.  The answer per case: n, min_inliers, max_its, idx (int [N]: mvKeyPointIndices), max_err (float32 [N]) and calls, one dict per
call: its (the iterations it ran), sets (int32 [k, 4]), poses (float64 [k, 12]: R, t), counts (int32 [k, 4]: count, N, Refine ran, refined count), trace (float64
[k, 15]: rep_errors, betas), marks (uint8 [k, N]: mvbInliersi), state (a frontend.PNP_STATE_DTYPE record) and inliers (uint8 [nf])."""
import os
import numpy as np
import host_sim
import pkg
from host_sim import bits as _bits, ints as _ints, floats as _floats

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "pnp_sim.cpp")
_INT_FIELDS = ("its_done", "best_inliers", "best_it", "refine_ok", "n", "min_inliers", "max_its", "found", "found_it", "n_inliers", "no_more")


def _d64(x):
    return str(int(np.float64(x).view(np.uint64)))


def _doubles(tokens):
    return np.array([int(t) for t in tokens], np.uint64).view(np.float64)


def encode(c):
    nf, nkf = len(c["oct"]), len(c["xw"])
    assert len(c["assigned"]) == nf and len(c["pt"]) == nf and len(c["valid"]) == nkf
    sets = c.get("sets")
    head = "case %d %d %d %d %d %d %d %d %d %s" % (nf, nkf, len(c["sigma2"]), c["min_inliers"], c["max_iterations"], c.get("seed", 0), c.get("pair", 0),
                                                 -1 if sets is None else len(sets), len(c["calls"]), _d64(c["probability"]))
    parts = [head, _bits([c["epsilon"], c["th2"]]), _bits(c["K"]), _bits(c["sigma2"]), _ints(c["oct"]), _bits(c["pt"]), _ints(c["valid"]), _bits(c["xw"]), _ints(c["assigned"])]
    if sets is not None:
        assert np.asarray(sets).reshape(-1, 4).shape[0] == len(sets)
        parts.append(_ints(sets))
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
        body = np.array([int(x) for x in t[4:]], np.uint64).reshape(N, 2)
        r = {"n": N, "min_inliers": int(t[2]), "max_its": int(t[3]), "idx": body[:, 0].astype(np.int64), "max_err": body[:, 1].astype(np.uint32).view(np.float32), "calls": []}
        for _ in c["calls"]:
            its, sets, poses, counts, trace, marks = [], [], [], [], [], []
            while lines[at].startswith("hyp"):
                t = lines[at].split(); at += 1
                its.append(int(t[1])); sets.append([int(x) for x in t[2:6]]); poses.append(_doubles(t[6:18]))
                counts.append([int(t[18]), int(t[19]), int(t[35]), int(t[36])]); trace.append(_doubles(t[20:35]))
                marks.append(np.zeros(0, np.uint8) if t[37] == "-" else np.frombuffer(t[37].encode(), np.uint8) - 48)
            t = lines[at].split(); at += 1
            assert t[0] == "state"
            st = np.zeros(1, fe.PNP_STATE_DTYPE)[0]
            for k, v in zip(_INT_FIELDS, t[1:12]):
                st[k] = int(v)
            d = _doubles(t[12:24])
            st["best_R"] = d[:9]; st["best_t"] = d[9:]; st["Tcw"] = _floats(t[24:36])
            t = lines[at].split(); at += 1
            assert t[0] == "inl" and len(t) == 1 + len(c["assigned"])
            k = len(its)
            r["calls"].append(dict(its=np.array(its, np.int64), sets=np.array(sets, np.int32).reshape(k, 4), poses=np.array(poses, np.float64).reshape(k, 12),
                                   counts=np.array(counts, np.int32).reshape(k, 4), trace=np.array(trace, np.float64).reshape(k, 15),
                                   marks=np.array(marks, np.uint8).reshape(k, N), state=st, inliers=np.array([int(x) for x in t[1:]], np.uint8)))
        out.append(r)
    assert at == len(lines)
    return out


def run_plain(cases):
    """the plain build alone: for the searches of tests/pnp_cases.py, whose finds go through run() afterwards"""
    return decode(host_sim.run_plain(SRC, "".join(encode(c) for c in cases)), cases)


def run(cases):
    return decode(host_sim.run(SRC, "".join(encode(c) for c in cases)), cases)


def plan(cap):
    """pnp_plan(cap) of csrc/match_plan.h -> dict"""
    t = host_sim.run(SRC, "plan %d\n" % cap).split()
    assert t[0] == "plan"
    return dict(zip(("rowBytes", "ldsBytes", "ldsOptIn", "threads", "maxCap"), map(int, t[1:])))


def table(probability, min_inliers, max_iterations, epsilon, cap):
    """(mRansacMinInliers, mRansacMaxIts) for N = 0 .. cap -> int [cap + 1, 2]"""
    t = host_sim.run(SRC, "table %s %d %d %s %d\n" % (_d64(probability), min_inliers, max_iterations, _bits([epsilon]), cap)).split()
    assert t[0] == "table"
    return np.array([int(x) for x in t[1:]], np.int64).reshape(cap + 1, 2)


def params_ok(has_sigma=1, nlevels=8, probability=0.99, min_inliers=10, max_iterations=300, new_iterations=5, epsilon=0.5, th2=5.991, npairs=1, cap=100, nframes=1, nkeyframes=1,
              kfcap=100, has_sets=0, nsets=0):
    """(pnp_params_ok, pnp_sizes_ok) of csrc/match_check.h"""
    t = host_sim.run(SRC, "params %d %d %s %d %d %d %s %d %d %d %d %d %d %d\n" % (has_sigma, nlevels, _d64(probability), min_inliers, max_iterations, new_iterations,
                                                                                _bits([epsilon, th2]), npairs, cap, nframes, nkeyframes, kfcap, has_sets, nsets)).split()
    assert t[0] == "params"
    return bool(int(t[1])), bool(int(t[2]))
