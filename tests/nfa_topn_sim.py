"""csrc/nfa_topn.h on the host as the test modules and tools/nfa_topn_count.py ask for it.  The header holds no HIP.  model(): tests/sim/nfa_topn_sim.cpp, the sliced
validation over (u, final, accepted) triples, through host_sim's two g++ builds (plain and under the sanitizers).  oracle_frame(): tests/sim/nfa_topn_oracle.cpp, the CPU
oracle's LSD main loop with the header's r0 / margin beside what rect_improve did to every candidate, a shared object built once per process in a temporary directory;
oracle_rects(): the same with every candidate's full first record; oracle_verdicts(): the oracle's rect_nfa / rect_improve on records the caller supplies
(tests/nfa_stage_cases.py).  model(mutant=k): the model built wrong in one way (MUTANTS), for tests/test_nfa_stage_cases_cpu.py."""
import atexit, ctypes as C, functools, os, shutil, subprocess, tempfile
import numpy as np
import host_sim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "nfa_topn_sim.cpp")
ORACLE_SRC = os.path.join(HERE, "sim", "nfa_topn_oracle.cpp")
RANK_CAP = 960           # csrc/lsd_nfa.h NFA_RANK_CAP
FIELDS = ("r0", "margin", "at_once", "accepted", "final", "area", "x1", "y1", "x2", "y2", "shift", "pad")


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


MUTANTS = {1: "tau = the (N-1)-th largest accepted response", 2: "tau = the (N+1)-th largest", 3: "excluded with <=", 4: "the edge margin replaced by the inner one",
           5: "exclusion allowed with exactly N accepted", 6: "ties in the ranking broken by descending index"}      # tests/sim/nfa_topn_sim.cpp -DTOPN_MUTANT=k


def model(cases, plain_only=False, mutant=0):
    """cases: (N, w, h, u[n] float32, final[n] float32, accepted[n][, uin[n] float32]) -> per case (flags[n], ranked, slices, validated).  uin: u with the inner margin
    (frame_case gives it; u itself where a case has none).  mutant k > 0: the model built with -DTOPN_MUTANT=k, the plain build alone."""
    text = []
    for c in cases:
        N, w, h, u, fin, acc = c[:6]
        uin = c[6] if len(c) > 6 else u
        n = len(u)
        text.append("%d %d %d %d %d" % (n, N, RANK_CAP, w, h))
        if n:
            rows = np.stack([f32bits(u).astype(np.int64), f32bits(fin).astype(np.int64), np.asarray(acc, np.int64), f32bits(uin).astype(np.int64)], 1)
            text.append(" ".join(map(str, rows.ravel().tolist())))
    text = "\n".join(text) + "\n"
    if mutant: out = host_sim.run_plain(SRC, text, ("TOPN_MUTANT=%d" % mutant,)).split("\n")
    else: out = (host_sim.run_plain if plain_only else host_sim.run)(SRC, text).split("\n")
    res = []
    for k, c in enumerate(cases):
        fl = out[2 * k].split(); st = out[2 * k + 1].split()
        assert fl[0] == "flags" and st[0] == "stat" and len(fl) == 1 + len(c[3])
        res.append((np.array(fl[1:], np.int64), int(st[1]), int(st[2]), int(st[3])))
    return res


@functools.lru_cache(maxsize=None)
def _oracle_lib():
    d = tempfile.mkdtemp(prefix="nfa_topn_oracle_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libnfa_topn_oracle.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, ORACLE_SRC])
    L = C.CDLL(so)
    L.nfa_topn_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.nfa_topn_frame_rects.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.nfa_topn_verdicts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return L


def oracle_frame(gray):
    """every candidate rectangle of the frame in emission order -> dict of float64 arrays named FIELDS"""
    gray = np.ascontiguousarray(gray, np.uint8); h, w = gray.shape
    cap = 8192
    out = np.zeros((cap, len(FIELDS)), np.float64)
    n = _oracle_lib().nfa_topn_frame(gray.ctypes.data, w, h, out.ctypes.data, cap)
    assert 0 <= n <= cap
    return {k: out[:n, i].copy() for i, k in enumerate(FIELDS)}


def oracle_rects(gray):
    """oracle_frame(gray) and every candidate's full first record [n, 12] float64 (the RectD fields as region2rect / refine left them), in emission order"""
    gray = np.ascontiguousarray(gray, np.uint8); h, w = gray.shape
    cap = 8192
    out = np.zeros((cap, len(FIELDS)), np.float64); rects = np.zeros((cap, 12), np.float64)
    n = _oracle_lib().nfa_topn_frame_rects(gray.ctypes.data, w, h, out.ctypes.data, rects.ctypes.data, cap)
    assert 0 <= n <= cap
    return {k: out[:n, i].copy() for i, k in enumerate(FIELDS)}, rects[:n].copy()


def oracle_verdicts(gray, rects):
    """the oracle's prologue of the frame, then rect_nfa / rect_improve on each of the records [n, 12] on its own -> dict of float64 arrays named FIELDS"""
    gray = np.ascontiguousarray(gray, np.uint8); h, w = gray.shape
    rects = np.ascontiguousarray(rects, np.float64).reshape(-1, 12)
    out = np.zeros((len(rects), len(FIELDS)), np.float64)
    assert _oracle_lib().nfa_topn_verdicts(gray.ctypes.data, w, h, rects.ctypes.data, len(rects), out.ctypes.data) == len(rects)
    return {k: out[:, i].copy() for i, k in enumerate(FIELDS)}


def frame_case(fr, N, w, h, inner=False):
    """the model's input for an oracle_frame() / oracle_verdicts() result; inner: with uin, the upper bound under the inner margin alone, behind it"""
    r0 = fr["r0"].astype(np.float32)
    u = (r0 + fr["margin"].astype(np.float32)).astype(np.float32)      # one float addition: nfa_topn.h upper()
    uin = (r0 + np.float32(0.125) / np.float32(max(w, h))).astype(np.float32)      # MARGIN_IN_PX for every candidate: what mutant 4 ranks by
    return (N, w, h, u, fr["final"].astype(np.float32), fr["accepted"].astype(np.int64)) + ((uin,) if inner else ())


def top_n(resp, ok, N):
    """emission indices of the N accepted candidates of the largest response, ties by emission order: what k_keylines outputs"""
    idx = np.flatnonzero(ok)
    order = np.lexsort((idx, -resp[idx].astype(np.float64)))
    return idx[order][:N]
