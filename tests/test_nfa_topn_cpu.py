"""The rule of the NFA stage's top-N form (csrc/nfa_topn.h) on the host.  (1) The model of the sliced validation (tests/sim/nfa_topn_sim.cpp, plain and sanitised build)
on random candidate sets: the top N of the validated subset are the top N of all candidates, in order, and no excluded candidate is among them.  (2) The bound itself
against the REFERENCE side: over the CPU oracle's own rectangles (tests/sim/nfa_topn_oracle.cpp walks oracle/lsd_oracle.cpp), |final response - r0| <= margin for every
accepted segment, r0 is the final response bit for bit when the first evaluation accepts, and the model on those frames keeps the oracle's top N."""
import numpy as np
import pytest
import nfa_topn_sim as sim
from synth import synth_frame, noise_frame

W, H = 640, 480
M_IN, M_EDGE = np.float32(0.125) / np.float32(640), np.float32(6.125) / np.float32(640)


def _case(rng, n, N, kind):
    """candidates as the stage meets them: r0, a margin of either size, accept / reject, and a final response within the margin of r0 (equal when `at once`)"""
    if kind == "ties": r0 = rng.choice(np.float32([0.05, 0.1, 0.1, 0.2]), n)
    else: r0 = (rng.random(n) ** 2 * 0.9).astype(np.float32)
    m = np.where(rng.random(n) < 0.1, M_EDGE, M_IN).astype(np.float32)
    u = (r0 + m).astype(np.float32)
    acc = rng.random(n) < (0.0 if kind == "none" else 0.85)
    if kind == "exactly_n" and n > N:
        acc[:] = False; acc[rng.choice(n, N, replace=False)] = True
    at_once = rng.random(n) < 0.8
    shift = rng.random(n) * 2 - 1
    if kind == "on_the_bound": shift = rng.choice([-1.0, 1.0], n)
    fin = np.where(at_once, r0, np.clip(r0.astype(np.float64) + shift * m.astype(np.float64), 0, None).astype(np.float32)).astype(np.float32)
    fin = np.minimum(fin, u)          # (the float addition of upper() may round below r0 + m: the final response is bounded by u, which is what the rule uses)
    return (N, W, H, u, fin, acc.astype(np.int64))


def _check(case, res):
    N, w, h, u, fin, acc = case
    flags, ranked, slices, validated = res
    n = len(u)
    v = flags != 2
    assert np.array_equal(flags[v], acc[v])                     # a validated candidate carries its verdict
    assert validated == v.sum() and (ranked or v.all())
    if not (n > N and n <= sim.RANK_CAP): assert not ranked and v.all()
    all_top = sim.top_n(fin, acc == 1, N)
    sub_top = sim.top_n(fin, (acc == 1) & v, N)
    assert np.array_equal(all_top, sub_top)
    assert v[all_top].all()
    if not v.all():      # something was left out: more than N were accepted among the validated, so the reference's sort / no-sort decision is the same
        assert ((acc == 1) & v).sum() > N
    return ranked, slices, int(v.sum())


def test_model_on_random_candidate_sets():
    rng = np.random.default_rng(20260)
    cases = []
    for kind in ("plain", "ties", "none", "exactly_n", "on_the_bound"):
        for N in (1, 10, 40, 200):
            for n in sorted(set([0, 1, N - 1, N, N + 1, N + 2, 2 * N + 3, 700] + [int(x) for x in rng.integers(0, 701, 6)])):
                if n >= 0: cases.append(_case(rng, n, N, kind))
    cases.append(_case(rng, sim.RANK_CAP, 40, "plain")); cases.append(_case(rng, sim.RANK_CAP + 1, 40, "plain"))      # the ranking's capacity and one beyond (validated in full)
    res = sim.model(cases)
    left_out = 0
    for c, r in zip(cases, res):
        ranked, slices, nv = _check(c, r)
        left_out += len(c[3]) - nv
    assert left_out > 1000       # the rule does leave candidates out on these sets


@pytest.fixture(scope="module")
def oracle_frames():
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # bench.py lies at the repository's root
    import bench
    cur, _ = bench.synth_frames(W, H, 64, 0)
    frames = [(f, W, H) for f in cur]
    rng = np.random.default_rng(7)
    for it in range(24):          # frames as tools/fuzz_parity.py draws them: random sizes (every third a 5-to-4 geometry), densities and noise
        w = int(rng.integers(96, 500)); h = int(rng.integers(80, 400))
        if it % 3 == 0: w, h = (w // 20) * 20, (h // 5) * 5
        seed = int(rng.integers(0, 1 << 30))
        img = noise_frame(seed, w, h) if rng.random() < 0.1 else synth_frame(seed, w, h, nshapes=int(rng.integers(2, 120)), nstrokes=int(rng.integers(0, 80)), noise=float(rng.choice([0.0, 1.0, 2.0, 4.0, 8.0])))
        frames.append((img, w, h))
    return [(sim.oracle_frame(img), w, h) for img, w, h in frames]


def test_bound_holds_on_the_oracles_rectangles(oracle_frames):
    nacc = nmoved = 0
    for fr, w, h in oracle_frames:
        acc = fr["accepted"] == 1
        d = np.abs(fr["final"] - fr["r0"])
        assert (d[acc] <= fr["margin"][acc]).all(), (w, h, float((d[acc] / fr["margin"][acc]).max()))
        once = fr["at_once"] == 1
        assert (fr["accepted"][once] == 1).all() and np.array_equal(fr["final"][once], fr["r0"][once])      # accepted at once: r0 IS the response, bit for bit
        assert (fr["shift"] <= 1.5625 + 1e-9).all()                                                            # rect_improve moves an end point by at most SHIFT_PX
        nacc += int(acc.sum()); nmoved += int((fr["shift"][acc] > 0).sum())
    assert nacc > 20000 and nmoved > 100, (nacc, nmoved)       # the bound was exercised by rectangles that did move


@pytest.mark.parametrize("N", [40, 200])
def test_model_keeps_the_oracles_top_n(oracle_frames, N):
    cases = [sim.frame_case(fr, N, w, h) for fr, w, h in oracle_frames]
    skipped = total = 0
    for c, r in zip(cases, sim.model(cases, plain_only=True)):
        ranked, slices, nv = _check(c, r)
        skipped += len(c[3]) - nv; total += len(c[3])
    assert skipped > total // 5
