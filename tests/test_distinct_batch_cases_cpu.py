"""The inputs of tests/test_distinct_batch_gpu.py reach what they are meant to reach, shown on the CPU with helper + oracle (tests/distinct_batch_cases.py):
every tie case has two entries at the least median and the stated winner, the two k cases choose another entry under the wrong k, every skipped entry
would change its set's winner if it were read, the count cases sit in two classes.  Where the reference's own ComputeDistinctiveDescriptors was built
(oracle/_ref/libref_slices.so), a family of sets with bad keyframes is held against it, as map points and as map lines."""
import ctypes as C
import os
import numpy as np
import pytest
import distinct_batch_cases as dc

SLICES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_slices.so")


@pytest.fixture(scope="module")
def pool():
    return dc.make_pool(np.random.default_rng(9100))


def one(oracle, pool, s, **kw):
    o, ptr = dc.pack([s])
    b, m, _ = dc.expect(oracle, pool, o, ptr, **kw)
    return int(b[0]), int(m[0])


def test_pool_is_poisoned(pool):
    c = dc.counts(pool)
    assert c[dc.OVER] == dc.CAP and c[dc.UNDER] == 0 and c[dc.EMPTY] == 0 and c[dc.FULL] == dc.CAP and pool["n"][dc.OVER] == dc.CAP + 5 and pool["n"][dc.UNDER] == -3
    raw, base = pool["raw"], pool["base"]
    assert (raw[0] == base).all() and (raw[-1] == base).all()
    for k in range(dc.NK):
        assert (raw[k + 1, c[k]:] == base).all()
        real = raw[k + 1, :c[k]]
        if pool["bad"][k]: assert (real == base).all()
        elif k == dc.TIE: assert dc.hamming(real[0], base) == 8 and (real[0] == real[1]).all()
        else: assert (dc.hamming(real, base) >= 20).all() and (dc.hamming(real, base) <= 60).all()
    # the poison wins a set of five or more real rows it is put into (with fewer, the median is the distance to the nearest row, and a real row may tie)
    rng = np.random.default_rng(1)
    for m in (5, 8, 20, 70):
        rows = np.concatenate([dc.raw_rows(pool, dc.random_entries(rng, pool, m)), base[None]])
        assert dc.winner(rows) == m


def test_expect_is_the_oracle_on_the_admissible_rows(oracle, pool):
    rng = np.random.default_rng(9110)
    sets = dc.size_sets(rng, pool)
    o, ptr = dc.pack(sets)
    best, med, chosen = dc.expect(oracle, pool, o, ptr)
    assert [len(s) for s in sets[:-1]] == list(dc.SIZES) and best[0] == -1 and best[-1] == -1 and med[0] == med[-1] == dc.INT_MAX
    for s, b, m, ch in zip(sets[1:-1], best[1:-1], med[1:-1], chosen[1:-1]):
        rows = dc.raw_rows(pool, s)
        if len(s) <= 129:
            assert b == dc.winner(rows) and m == dc.medians(rows)[b]
        assert b == oracle.distinctive(rows, np.array([0, len(rows)], np.int32))[0] and (ch == rows[b]).all()
    assert len(set(best[2:].tolist())) > 8          # the winner is not always the first


def test_tie_cases_have_the_stated_winner(oracle, pool):
    T = dc.tie_sets(np.random.default_rng(9120), pool)
    assert len(T) == 11
    for name, (s, want) in T.items():
        adm = dc.admissible(pool, s)
        med = dc.medians(dc.raw_rows(pool, s[adm]))
        pos = np.flatnonzero(adm)
        tied = pos[med == med.min()]
        assert len(tied) >= 2 and tied[0] == want, (name, tied)
        assert one(oracle, pool, s) == (want, med.min()), name
    assert dc.winner(dc.raw_rows(pool, T["large_67_131"][0])) == 67
    assert [dc.SMALL_MAX < len(T[n][0]) for n in ("small", "medium", "large_3_67")] == [False, True, True] and len(T["medium"][0]) <= dc.MEDIUM_MAX < len(T["large_3_67"][0])
    for n in ("first_behind_skipped_small", "first_behind_skipped_medium", "first_behind_skipped_large"):
        assert not dc.admissible(pool, T[n][0])[:2].any() and dc.admissible(pool, T[n][0])[2:].all()


def test_k_cases_choose_another_entry_under_the_wrong_k(oracle, pool):
    K = dc.k_sets(np.random.default_rng(9130), pool)
    s = K["k_from_admissible"]
    adm = dc.admissible(pool, s)
    assert len(s) == 9 and adm.sum() == 8 and not adm[6]
    rows = dc.raw_rows(pool, s[adm]); pos = np.flatnonzero(adm)
    assert int(0.5 * (8 - 1)) == 3 and int(0.5 * (9 - 1)) == 4
    assert one(oracle, pool, s)[0] == pos[dc.winner(rows, 3)] != pos[dc.winner(rows, 4)]
    s = K["lower_middle"]
    rows = dc.raw_rows(pool, s)
    assert len(s) == 4 and dc.admissible(pool, s).all() and int(0.5 * (4 - 1)) == 1
    assert one(oracle, pool, s)[0] == dc.winner(rows, 1) != dc.winner(rows, 2)


def test_a_skipped_entry_would_win_if_it_were_read(oracle, pool):
    S = dc.skip_sets(np.random.default_rng(9140), pool)
    assert len(S) == 9
    for name, (s, p) in S.items():
        adm = dc.admissible(pool, s)
        if p is None:
            assert adm.all() and s["row"][0] == dc.CAP - 1 and pool["n"][s["kf"][0]] > dc.CAP, name
            continue
        assert not adm[p] and adm.sum() == len(s) - 1, name
        assert (dc.raw_rows(pool, s[p:p + 1])[0] == pool["base"]).all(), name
        b, _ = one(oracle, pool, s)
        assert b != p and one(oracle, pool, s, read_everything=True)[0] == p, name


def test_count_cases_sit_in_two_classes(oracle, pool):
    Cn = dc.count_sets(np.random.default_rng(9150), pool)
    for name, m, cls in (("70_entries_8_admissible", 70, dc.MEDIUM_MAX), ("9_entries_8_admissible", 9, dc.SMALL_MAX)):
        s = Cn[name]
        assert len(s) == m > cls and dc.admissible(pool, s).sum() == 8 <= dc.SMALL_MAX
        b, med = one(oracle, pool, s)
        assert dc.admissible(pool, s)[b] and b != one(oracle, pool, s, read_everything=True)[0]


def test_refused_ranges(oracle, pool):
    rng = np.random.default_rng(9160)
    sets = [dc.random_entries(rng, pool, m) for m in (5, 4, 6, dc.LARGE_MAX + 1, 3)]
    o, ptr = dc.pack(sets)
    best, med, _ = dc.expect(oracle, pool, o, ptr)
    assert best[3] == -2 and med[3] == dc.INT_MAX and (best[[0, 1, 2, 4]] >= 0).all()
    bad = ptr.copy(); bad[2] = bad[1] - 2                          # set 1 decreases, set 2 starts before set 1's start and is still a valid range
    b2, _, _ = dc.expect(oracle, pool, o, bad)
    assert b2[1] == -2 and b2[0] == best[0] and b2[2] >= 0 and b2[4] == best[4]
    b3, _, _ = dc.expect(oracle, pool, o, ptr, nobs=len(o) - 1)   # the last set ends beyond nobs
    assert b3[4] == -2 and (b3[:3] == best[:3]).all()


def test_packing_and_workload(oracle, pool):
    sets = dc.packing_sets(np.random.default_rng(9170), pool)
    assert len(sets) == 64 and [len(s) for s in sets[:8]] == list(dc.PACK_SIZES)
    for g in range(8):
        assert sorted(len(sets[8 * r + g]) for r in range(8)) == sorted(dc.PACK_SIZES)          # every group position sees every size
    o, ptr = dc.pack(sets)
    best, _, _ = dc.expect(oracle, pool, o, ptr)
    assert ((best >= 0) == (np.diff(ptr) > 0)).all()
    o, ptr = dc.many_small_sets(np.random.default_rng(9180), pool, 500)
    best, _, _ = dc.expect(oracle, pool, o, ptr)
    assert np.diff(ptr).max() == dc.SMALL_MAX and (best[-19:] >= 0).all() and (~dc.admissible(pool, o)).sum() > 50
    desc, o, ptr = dc.workload(np.random.default_rng(9190), nsets=200)
    assert np.diff(ptr).min() == 3 and np.diff(ptr).max() == 14 and len(np.unique(o.view(np.int64))) == len(o)


@pytest.mark.skipif(not os.path.exists(SLICES), reason="oracle/_ref/libref_slices.so was not built (the reference tree is absent)")
def test_reference_agrees_with_expect(oracle, pool):
    R = C.CDLL(SLICES)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rng = np.random.default_rng(9200)
    sets = []
    for m in (1, 2, 3, 4, 5, 8, 9, 13, 20, 40, 64, 65, 100):
        for _ in range(4):
            s = dc.random_entries(rng, pool, m)
            s["kf"][rng.random(m) < 0.3] = dc.BAD_SLOTS[int(rng.integers(0, 3))]
            sets.append(s)
    sets.append(dc.obs([(dc.BAD_SLOTS[0], 1), (dc.BAD_SLOTS[1], 2)]))
    o, ptr = dc.pack(sets)
    best, _, chosen = dc.expect(oracle, pool, o, ptr)
    seen_bad = 0
    for s, b, ch in zip(sets, best, chosen):
        rows = np.ascontiguousarray(dc.raw_rows(pool, s)); bad = np.ascontiguousarray(pool["bad"][s["kf"]])
        seen_bad += int(bad.any())
        good = rows[bad == 0]
        for lines in (0, 1):
            got = R.ref_distinctive(lines, p(rows), len(rows), p(bad))
            # the reference keeps a CLONE of the chosen row: any admissible row with those bytes is the same answer
            assert (got == -1 and b == -1) or (got >= 0 and b >= 0 and (good[got] == ch).all()), (len(s), lines, got, b)
    assert seen_bad > 20 and best[-1] == -1
