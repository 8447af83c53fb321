"""Rectangle lists for the NFA stage (csrc/lsd_nfa.h: the 18 launches, k_nfa_all, k_nfa_topn) -- what tests/test_nfa_stage_gpu.py injects through sslam_testing_lines_nfa
(include/sslam_testing.h).  A case is a frame, a list of RectD records and N (max_lines).  The records are the CPU oracle's own candidates (nfa_topn_sim.oracle_rects: each
candidate's first record as region2rect / refine left it) of a 320 x 240 frame of lsd_cases / synth -- the same frame, or ANOTHER one of the same size ("foreign" records: the
stage reads nothing of a record's history, only the angle plane under it) -- selected, repeated or reordered by numpy with fixed seeds; one family lives at 333 x 251, off the
fused-gradient geometry, where margin()'s W - 2 tests see other numbers.  Every record is therefore inside the value range the core emits.  The reference verdicts come from the
oracle's own rect_nfa / rect_improve on each record by itself (nfa_topn_sim.oracle_verdicts), the 0 / 1 / 2 flags from the host model of csrc/nfa_topn.h
(nfa_topn_sim.model).  tests/test_nfa_stage_cases_cpu.py asserts from those two alone what each case reaches and that the set tells every mutant of the model
(nfa_topn_sim.MUTANTS) from the rule.  Nothing is searched at import time; what was searched once is written down:

  * ties at tau.  `excluded` is u < tau: a candidate whose u EQUALS tau is validated.  tau is the final response of an accepted candidate and u = r0 + margin > r0, so a tie
    needs two different records A, B with response(A) == upper(B) bit for bit.  Searched: all 13 709 candidates of waves, spiral8, the checkerboards of 6 .. 16, 18, 20 and 24
    pixels and the seven dense scenes, every accepted final response against every u.  ONE pair: dense scene 3, record 32 (accepted at its first evaluation: its response is
    r0) and waves, record 616.  `ties_at_tau` puts eight copies of waves[616] among dense scene 3's records with N = the rank of record 32's response.
  * the border margin.  A candidate with MARGIN_EDGE_PX whose u is at or above the final tau while r0 + MARGIN_IN_PX is below it: the seven dense scenes at 320 x 240 and at
    333 x 251 with N = 5, 10, 20, 40, 80 -- 47 of the 70 combinations hold one that is validated; the first scene's are kept (N = 40 / N = 20).
  * a GROWING candidate, i.e. an accepted one whose final response exceeds r0 + MARGIN_IN_PX (checkLineExtremes clamps an end point of the first record, and rect_improve
    moves it back inside): none among the 503 accepted edge candidates of the dense scenes at both sizes, waves and the checkerboards of 8, 10 and 12 pixels; spiral8 has
    exactly one, record 83 (r0 0.02914, final 0.02963), whose margin is the edge one as nfa_topn.h demands; it is the 80th largest response of the frame.  `spiral_grows`
    keeps that frame whole with N = 80, so that the record is validated and leaves among the top N.
"""
import collections, functools
import numpy as np
import lsd_cases as lc
import nfa_topn_sim as sim
from synth import synth_frame

W, H = lc.CORE_W, lc.CORE_H
ODD_W, ODD_H = 333, 251
RANK_CAP, RANK_BASE, CHUNK = sim.RANK_CAP, 1024, 768          # csrc/lsd_nfa.h: NFA_RANK_CAP, NFA_RANK_BASE, k_nfa_topn<768>'s chunk
TIE_A, TIE_B = 32, 616                                        # dense scene 3's record / waves' record of the tie (see above)
SPIRAL_GROWS = 83                                             # spiral8's growing record

Case = collections.namedtuple("Case", "name frame rects N")


def slice_size(need):
    return need + (need >> 3) + 8          # csrc/nfa_topn.h


@functools.lru_cache(maxsize=None)
def source(name):
    """(frame, the oracle's candidate records [n, 12]) of a source frame: a name of lsd_cases.CORE, `dense<i>` (the scenes of tests/test_nfa_topn_gpu.py) or `odd<i>` (the same
    at 333 x 251)"""
    if name.startswith("dense") or name.startswith("odd"):
        i = int(name[-1]); w, h = (W, H) if name.startswith("dense") else (ODD_W, ODD_H)
        img = synth_frame(7100 + i, w=w, h=h, nshapes=30 + 4 * i, nstrokes=20 + 3 * i, noise=2.0)
    else: img = lc.frame("core", name)
    img = np.ascontiguousarray(img); img.setflags(write=False)
    rects = sim.oracle_rects(img)[1]; rects.setflags(write=False)
    return img, rects


def _tile(rects, n):
    return rects[np.arange(n) % len(rects)]


def _exactly(name, nacc):
    """every rejected record of the source and the `nacc` accepted ones of the largest response, in emission order: the rejected ones of a smaller u are what a rule
    that excludes too early would leave out"""
    img, r = source(name)
    v = sim.oracle_verdicts(img, r)
    keep = np.sort(np.concatenate([np.flatnonzero(v["accepted"] == 0), sim.top_n(v["final"], v["accepted"] == 1, nacc)]))
    return r[keep]


def _repeat_one(name, N, copies):
    """the accepted records of the source with ONE of them repeated in place: the one whose u ranks eight positions before the end of the first slice, so that the
    copies -- one u, ties broken by emission index -- straddle that end"""
    img, r = source(name)
    v = sim.oracle_verdicts(img, r)
    r = r[v["accepted"] == 1]
    u = sim.frame_case(sim.oracle_verdicts(img, r), N, img.shape[1], img.shape[0])[3]
    k = np.lexsort((np.arange(len(u)), -u.astype(np.float64)))[slice_size(N + 1) - 8]
    return np.concatenate([r[:k], np.repeat(r[k:k + 1], copies, 0), r[k + 1:]])


def _ties_at_tau():
    """dense scene 3's records, eight copies of waves[TIE_B] spread over the emission order and, in front, the four records of waves with the largest u among those the
    oracle rejects over THIS frame: they only take places in the ranking, which puts all eight copies behind the end of the first slice -- it is tau that lets them in"""
    img, r = source("dense3")
    wr = source("waves")[1]
    wv = sim.oracle_verdicts(img, wr)
    wu = np.where(wv["accepted"] == 0, sim.frame_case(wv, 1, W, H)[3].astype(np.float64), -1.0)
    out = list(r)
    for at in (5, 40, 41, 90, 150, 151, 200, 243 + 7): out.insert(min(at, len(out)), wr[TIE_B])
    return np.array(list(wr[np.argsort(-wu, kind="stable")[:4]]) + out)


def _tie_rank():
    """N of ties_at_tau: the rank of the response of dense scene 3's record TIE_A among the accepted ones of the list"""
    img, r = source("dense3")
    v = sim.oracle_verdicts(img, _ties_at_tau())
    fin = v["final"].astype(np.float32)
    a = np.float32(sim.oracle_verdicts(img, r[TIE_A:TIE_A + 1])["final"][0])
    return int(((v["accepted"] == 1) & (fin >= a)).sum())


# name -> (frame source, records, N).  N may be a callable (evaluated with the records).
_BUILD = {
    # slices
    "one_slice": ("dense0", lambda: source("dense0")[1], 10),
    "waves200": ("waves", lambda: source("waves")[1], 200),
    "never_more_than_n": ("checker10", lambda: source("checker10")[1][:900], 200),
    "foreign_short_first_slice": ("dense1", lambda: source("waves")[1][:500], 60),
    # accept-count boundaries
    "exactly_n_accepted": ("dense0", lambda: _exactly("dense0", 30), 30),
    "n_plus_1_accepted": ("dense0", lambda: _exactly("dense0", 31), 30),
    # count boundaries
    "n_eq_N": ("dense1", lambda: source("dense1")[1][:40], 40),
    "n_eq_N_plus_1": ("dense1", lambda: source("dense1")[1][:41], 40),
    "n960": ("dense2", lambda: _tile(source("dense2")[1], RANK_CAP), 40),
    "n961": ("dense2", lambda: _tile(source("dense2")[1], RANK_CAP + 1), 40),
    "N1": ("dense3", lambda: source("dense3")[1], 1),
    "N_ge_n": ("dense3", lambda: source("dense3")[1], 300),
    "n960_N700": ("waves", lambda: _tile(source("waves")[1], RANK_CAP), 700),
    # ties
    "ties_at_tau": ("dense3", _ties_at_tau, _tie_rank),
    "checker10_ties": ("checker10", lambda: source("checker10")[1][np.random.Generator(np.random.PCG64(3)).permutation(1480)[:RANK_CAP]], 60),
    "repeat_one": ("dense4", lambda: _repeat_one("dense4", 40, 12), 40),
    # the border margin, moved and growing rectangles
    "edge_margin": ("dense0", lambda: source("dense0")[1], 40),
    "odd_edge_margin": ("odd0", lambda: source("odd0")[1], 20),
    "odd_one_slice": ("odd3", lambda: source("odd3")[1], 10),
    "spiral_grows": ("spiral8", lambda: source("spiral8")[1], 80),
}
NAMES = tuple(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    src, build, N = _BUILD[name]
    rects = np.ascontiguousarray(build(), np.float64); rects.setflags(write=False)
    return Case(name, source(src)[0], rects, N() if callable(N) else N)


@functools.lru_cache(maxsize=None)
def verdicts(name):
    """the oracle's verdict on every record of the case (nfa_topn_sim.FIELDS), computed once and shared"""
    c = case(name)
    v = sim.oracle_verdicts(c.frame, c.rects) if len(c.rects) else {k: np.zeros(0) for k in sim.FIELDS}
    for a in v.values(): a.setflags(write=False)
    return v


def model_case(name):
    c = case(name); h, w = c.frame.shape
    return sim.frame_case(verdicts(name), c.N, w, h, inner=True)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(flags [n] 0 / 1 / 2 of the model, ranked, slices, validated) of the case under the rule"""
    flags, ranked, slices, validated = sim.model([model_case(name)])[0]
    flags.setflags(write=False)
    return flags, ranked, slices, validated


# The mixed call: nine frames of one size in ONE call with one N.  (source of the frame, records)
MIXED_N = 40
_MIXED = (
    ("dense0", lambda: source("dense0")[1][:0]),                                   # no candidate
    ("dense1", lambda: source("dense1")[1][7:8]),                                  # a single one
    ("dense2", lambda: source("dense2")[1]),                                       # ranked
    ("checker10", lambda: source("checker10")[1][:1000]),                          # over 960: validated in place, below the ranked copy's base
    ("checker8", lambda: source("checker8")[1]),                                   # over 1024: its records lie where a ranked frame's copy would
    ("waves", lambda: source("waves")[1]),                                         # ranked, 716
    ("dense3", lambda: source("dense3")[1][:41]),                                  # ranked, the smallest: N + 1
    ("dense5", lambda: _tile(source("dense5")[1], RANK_CAP)),                      # ranked, the largest: 960
    ("dense6", lambda: source("waves")[1][::3]),                                   # ranked, foreign records
)


@functools.lru_cache(maxsize=None)
def mixed():
    """-> (frames [9, H, W], list of records per frame, per frame the verdicts, per frame the model's (flags, ranked, slices, validated))"""
    frames = np.stack([source(s)[0] for s, _ in _MIXED])
    rects = [np.ascontiguousarray(b(), np.float64) for _, b in _MIXED]
    ver = [sim.oracle_verdicts(f, r) if len(r) else {k: np.zeros(0) for k in sim.FIELDS} for f, r in zip(frames, rects)]
    exp = sim.model([sim.frame_case(v, MIXED_N, W, H, inner=True) for v in ver])
    return frames, rects, ver, exp


def pack(rect_lists):
    """records of several frames -> (rects [nf, nmax, 12] zero-padded, ncand [nf])"""
    nmax = max(1, max(len(r) for r in rect_lists))
    out = np.zeros((len(rect_lists), nmax, 12), np.float64)
    for i, r in enumerate(rect_lists): out[i, :len(r)] = r
    return out, np.array([len(r) for r in rect_lists], np.int32)


def tau_of(name):
    """the model's final tau of a ranked case: the N-th largest final response among the validated and accepted candidates (None while no more than N are accepted)"""
    c = case(name); v = verdicts(name); flags = expected(name)[0]
    fin = v["final"].astype(np.float32)[(flags == 1)]
    return np.sort(fin)[::-1][c.N - 1] if len(fin) > c.N else None
