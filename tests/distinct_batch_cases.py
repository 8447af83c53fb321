"""Inputs and expectations of sslam_distinctive_descriptors_batch_dev (numpy only; the oracle is handed in).

A POOL is 40 keyframe slots of capacity 37 between two guard slots.  Every real row is BASE with 20 .. 60 flipped bits; every row at or past a slot's
count, every row of a bad slot and both guard slots hold BASE itself -- the POISON: its distance to a real row is that row's flip count, about half of
what two real rows are apart, so a set of five or more rows that read a poisoned row would choose it.  Slots with a purpose:
    3, 11, 20   bad keyframes (d_kf_bad), rows all poison          5   d_n = cap + 5, every row real        6   d_n = -3, every row poison
    7           d_n = 0                                            8   d_n = cap                            9   count 20 (behind it: the full slot 8)
    30          rows 0 and 1 are the SAME low-noise descriptor X (8 flips): two entries that tie at the least median
    31          every row is the same descriptor Y
A SET is an array of OBS_DTYPE entries (keyframe slot, row); pack() lays sets out as d_obs / d_ptr.  expect() is the contract restated: admissible entries
in entry order -> oracle.distinctive -> the entry position, -1 without an admissible entry, -2 for a refused range."""
import numpy as np

CAP, NK = 37, 40
INT_MAX = 0x7fffffff
SMALL_MAX, MEDIUM_MAX, LARGE_MAX = 8, 64, 1024          # the class bounds of csrc/match_plan.h (tests/test_distinct_batch_plan_cpu.py holds them against the header)
SETS_PER_WAVE, WAVES, GRID_MAX = 8, 4, 2048
OBS_DTYPE = np.dtype([("kf", "<i4"), ("row", "<i4")])
BAD_SLOTS = (3, 11, 20)
OVER, UNDER, EMPTY, FULL, SHORT, TIE, SAME = 5, 6, 7, 8, 9, 30, 31
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024)
POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)


def hamming(a, b):
    """Hamming distance of byte rows, broadcasting"""
    return POP8[np.bitwise_xor(a, b)].sum(-1)


def flipped(rng, base, lo, hi):
    bits = np.zeros(256, np.uint8)
    bits[rng.permutation(256)[:int(rng.integers(lo, hi + 1))]] = 1
    return base ^ np.packbits(bits)


def make_pool(rng):
    """-> dict(raw [NK + 2, CAP, 32] with the guards, n [NK] as the device gets it, bad [NK], base)"""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    n = rng.integers(20, CAP, NK).astype(np.int32)          # below CAP: the last row of an ordinary slot is poison
    n[OVER] = CAP + 5; n[UNDER] = -3; n[EMPTY] = 0; n[FULL] = CAP; n[SHORT] = 20; n[TIE] = 30; n[SAME] = 30
    bad = np.zeros(NK, np.uint8); bad[list(BAD_SLOTS)] = 1
    raw = np.tile(base, (NK + 2, CAP, 1))
    for k in range(NK):
        if bad[k]: continue
        for r in range(min(max(int(n[k]), 0), CAP)):
            raw[k + 1, r] = flipped(rng, base, 20, 60)
    raw[TIE + 1, 0] = raw[TIE + 1, 1] = flipped(rng, base, 8, 8)
    raw[SAME + 1, :30] = flipped(rng, base, 30, 30)
    return dict(raw=raw, n=n, bad=bad, base=base)


def plain_pool(desc, n=None):
    """any [nk, cap, 32] descriptors as a pool: guards of zeros, no bad slot, every row counted unless n says otherwise"""
    nk, cap = desc.shape[:2]
    raw = np.zeros((nk + 2, cap, 32), np.uint8); raw[1:-1] = desc
    return dict(raw=raw, n=np.full(nk, cap, np.int32) if n is None else np.asarray(n, np.int32), bad=np.zeros(nk, np.uint8), base=np.zeros(32, np.uint8))


def counts(pool):
    return np.clip(pool["n"], 0, pool["raw"].shape[1])


def obs(pairs):
    a = np.zeros(len(pairs), OBS_DTYPE)
    if len(pairs): a["kf"], a["row"] = np.asarray(pairs, np.int64).T
    return a


def admissible(pool, o):
    kf, row = o["kf"].astype(np.int64), o["row"].astype(np.int64)
    ok = (kf >= 0) & (kf < len(pool["n"]))
    k = np.where(ok, kf, 0)
    return ok & (pool["bad"][k] == 0) & (row >= 0) & (row < counts(pool)[k])


def raw_rows(pool, o):
    """the 32 bytes a kernel WITHOUT the rules would read for each entry: (kf * cap + row) * 32 behind d_desc, inside the guards"""
    flat = pool["raw"].reshape(-1, 32)
    return flat[np.clip((o["kf"].astype(np.int64) + 1) * pool["raw"].shape[1] + o["row"], 0, len(flat) - 1)]


def medians(rows, k=None):
    """per row the median the reference takes, sorted[int(0.5 * (N - 1))] (or sorted[k])"""
    D = np.sort(hamming(rows[:, None, :], rows[None, :, :]), axis=1)
    return D[:, int(0.5 * (len(rows) - 1)) if k is None else k]


def winner(rows, k=None):
    return int(np.argmin(medians(rows, k)))          # argmin: the first of equals


def random_entries(rng, pool, m):
    """m admissible entries, repeats allowed"""
    c = counts(pool)
    slots = np.array([k for k in range(NK) if c[k] > 0 and not pool["bad"][k] and k not in (TIE, SAME)])
    kf = rng.choice(slots, m)
    o = np.zeros(m, OBS_DTYPE); o["kf"] = kf; o["row"] = (rng.random(m) * c[kf]).astype(np.int32)
    return o


def pack(sets):
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    o = np.concatenate([np.zeros(0, OBS_DTYPE)] + [np.asarray(s, OBS_DTYPE) for s in sets])
    return o, ptr


def gather(pool, o, ptr, nobs=None, read_everything=False):
    """what a caller of the single call does on the host -> (rows of the admissible entries in entry order, their CSR ptr, their entry positions, valid ranges)"""
    nobs = len(o) if nobs is None else nobs
    ptr = np.asarray(ptr, np.int64); ns = len(ptr) - 1
    beg, end = ptr[:-1], ptr[1:]
    ok = (beg >= 0) & (beg <= end) & (end <= nobs) & (end - beg <= LARGE_MAX)
    cnt = np.where(ok, end - beg, 0)
    sid = np.repeat(np.arange(ns), cnt)
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    e = o[np.repeat(np.where(ok, beg, 0), cnt) + off]
    adm = np.ones(len(e), bool) if read_everything else admissible(pool, e)
    rows, sid_a, off_a = np.ascontiguousarray(raw_rows(pool, e)[adm]), sid[adm], off[adm]
    N = np.bincount(sid_a, minlength=ns)
    ptr2 = np.concatenate([[0], np.cumsum(N)]).astype(np.int32)
    return rows, ptr2, off_a, ok


def expect(oracle, pool, o, ptr, nobs=None, read_everything=False):
    """-> (best, median, chosen descriptors [nsets, 32], zero where there is none).  read_everything: what a kernel that skipped nothing would answer"""
    rows, ptr2, off_a, ok = gather(pool, o, ptr, nobs, read_everything)
    ns = len(ptr2) - 1; N = np.diff(ptr2); sid_a = np.repeat(np.arange(ns), N)
    b = oracle.distinctive(rows if len(rows) else np.zeros((1, 32), np.uint8), ptr2)
    best = np.full(ns, -1, np.int32); median = np.full(ns, INT_MAX, np.int32); chosen = np.zeros((ns, 32), np.uint8)
    has = N > 0
    assert ((b >= 0) == has).all()
    if has.any():
        at = (ptr2[:-1] + b)[has]
        best[has] = off_a[at]; chosen[has] = rows[at]
        d = hamming(rows, rows[(ptr2[:-1] + np.maximum(b, 0))[sid_a]])
        order = np.lexsort((d, sid_a))
        median[has] = d[order][(ptr2[:-1] + (N - 1) // 2)[has]]
    best[~ok] = -2
    return best, median, chosen


# ---------------------------------------------------------------- the named sets
def size_sets(rng, pool):
    """one set per admissible N of SIZES, every entry admissible; and N = 0 once more as three entries that are all skipped"""
    return [random_entries(rng, pool, m) for m in SIZES] + [obs([(BAD_SLOTS[0], 0), (-1, 0), (4, CAP)])]


def tie_sets(rng, pool):
    """name -> (set, stated winner): two entries with the descriptor X of slot TIE tie at the least median"""
    X0, X1 = (TIE, 0), (TIE, 1)
    def with_x(m, i, j, a=X0, b=X1):
        for _ in range(100):          # until X holds the least median and no real row in front of it does (in a handful of rows X's nearest neighbour reaches it too)
            s = random_entries(rng, pool, m); s[i] = a; s[j] = b
            med = medians(raw_rows(pool, s))
            t = np.flatnonzero(med == med.min())
            if t[0] == i and j in t: return s
        raise AssertionError("no tie case found")
    T = {"small": (with_x(5, 1, 3), 1), "medium": (with_x(20, 4, 11), 4), "large_3_67": (with_x(140, 3, 67), 3), "large_67_131": (with_x(140, 67, 131), 67),
         "same_entry_twice": (with_x(6, 2, 5, X0, X0), 2)}
    T["all_identical_small"] = (obs([(SAME, r) for r in range(6)]), 0)
    T["all_identical_medium"] = (obs([(SAME, r % 30) for r in range(40)]), 0)
    T["all_identical_large"] = (obs([(SAME, r % 30) for r in range(100)]), 0)
    for name, m in (("first_behind_skipped_small", 7), ("first_behind_skipped_medium", 30), ("first_behind_skipped_large", 90)):
        T[name] = (obs([(BAD_SLOTS[1], 2), (SAME, 35)] + [(SAME, r % 30) for r in range(m - 2)]), 2)
    return T


def skip_sets(rng, pool):
    """name -> (set, position of the skipped entry): one entry each that a rule skips and that holds the poison where a kernel would read it"""
    c = counts(pool)
    assert c[SHORT - 1] == CAP and c[SHORT] == 20 and c[OVER] == CAP and c[UNDER] == 0 and c[4] < CAP and c[NK - 1] < CAP
    skipped = {"bad_keyframe": (BAD_SLOTS[2], 4), "kf_-1": (-1, 5), "kf_nkeyframes": (NK, 0), "row_-1": (5, -1), "row_n": (SHORT, 20), "row_n_to_cap": (SHORT, 29),
               "n_above_cap_row_cap": (OVER, CAP), "n_below_0": (UNDER, 0)}
    out = {}
    for i, (name, e) in enumerate(skipped.items()):
        s = random_entries(rng, pool, 6); p = i % 6
        s[p] = e
        out[name] = (s, p)
    s = random_entries(rng, pool, 6); s[0] = (OVER, CAP - 1)          # the last row of the slot whose count is above the capacity IS read
    out["n_above_cap_last_row"] = (s, None)
    return out


def k_sets(rng, pool):
    """'k_from_admissible': nine entries, one in a bad keyframe -- k = 3 (N = 8) and k = 4 (from 9) choose different entries; 'lower_middle': N = 4, k = 1 and
    k = N / 2 = 2 choose different entries.  Found by search with the generator's stream"""
    out = {}
    for _ in range(10000):
        s = random_entries(rng, pool, 9); s[6] = (BAD_SLOTS[0], 1)
        r = raw_rows(pool, s[admissible(pool, s)])
        if winner(r, 3) != winner(r, 4): out["k_from_admissible"] = s; break
    for _ in range(10000):
        s = random_entries(rng, pool, 4)
        r = raw_rows(pool, s)
        if winner(r, 1) != winner(r, 2): out["lower_middle"] = s; break
    assert len(out) == 2
    return out


def count_sets(rng, pool):
    """entry count and admissible count in different classes: 70 entries with 8 admissible, 9 entries with 8 admissible"""
    def mixed(m, keep):
        s = obs([(BAD_SLOTS[i % 3], i % 20) for i in range(m)])
        s[keep] = random_entries(rng, pool, len(keep))
        return s
    return {"70_entries_8_admissible": mixed(70, [0, 9, 17, 33, 47, 63, 64, 69]), "9_entries_8_admissible": mixed(9, [0, 1, 2, 3, 5, 6, 7, 8])}


PACK_SIZES = (0, 8, 1, 9, 7, 64, 2, 65)


def packing_sets(rng, pool):
    """eight runs of eight consecutive sets: PACK_SIZES and its rotations, so every group of eight lanes sits beside every class; one entry in five is skipped"""
    sets = []
    for r in range(8):
        for m in PACK_SIZES[r:] + PACK_SIZES[:r]:
            s = random_entries(rng, pool, m)
            s["kf"][rng.random(m) < 0.2] = BAD_SLOTS[0]
            sets.append(s)
    return sets


def many_small_sets(rng, pool, nsets):
    """nsets sets of 0 .. 8 entries (the last 19 not empty), one entry in ten skipped: what reaches the stride loop behind the grid cap"""
    sizes = rng.integers(0, SMALL_MAX + 1, nsets); sizes[-19:] = rng.integers(2, SMALL_MAX + 1, 19)
    o = random_entries(rng, pool, int(sizes.sum()))
    o["row"][rng.random(len(o)) < 0.1] = CAP
    return o, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def workload(rng, nsets=2000, nk=21, n=1000):
    """the mix of tools/bench_matchers.py on a pool: nsets map points with 3 .. 14 observations in nk keyframes of n features, each observation a noisy copy of
    the point's descriptor -> (desc [nk, n, 32], obs, ptr); a keyframe sees a point once"""
    sizes = rng.integers(3, 15, nsets)
    desc = rng.integers(0, 256, (nk, n, 32), dtype=np.uint8)
    o = np.zeros(int(sizes.sum()), OBS_DTYPE); at = 0
    fill = np.zeros(nk, np.int64)
    for m in sizes:
        kfs = rng.permutation(nk)[:m]
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for kf in kfs:
            r = fill[kf] % n; fill[kf] += 1
            desc[kf, r] = base ^ np.packbits(rng.random(256) < 0.08)
            o[at] = (kf, r); at += 1
    return desc, o, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
