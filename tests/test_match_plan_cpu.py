"""The host-side plans of the matcher entry points (csrc/match_plan.h): which kernel a call launches for its sizes, the LDS bytes / capacity /
grid that follow, and the scratch arena of a staged call.  The header holds no HIP, so tests/sim/match_plan_dump.cpp compiles it with plain g++ --
once as it is and once with -fsanitize=address,undefined -- and prints the plan for the inputs it reads; nothing is loaded into Python.  Every
expected value below is worked out here from the documented rule, never read back from the header:

  knn-2 batch               tiles of 32 train rows, <= 128 tiles (4096 rows): matrix cores, else xor + popcount
  SearchForInitialization   npairs <= 8 and 64 + cap * 17 * 4 <= 150 KB: speculative; else ccap = min(cap, max(256, cap * 3 / 8)) and
                            64 + ccap * 64 <= 64 KB: LDS batch; else global memory
  projection                n <= 8192: two kernels, the features in the commit's LDS up to 2048 of them; else one wave
  arena                     every block starts on the next multiple of 256 bytes behind the block before it"""
import pytest
import plan_dump

KP, PQ = 28, 44          # sizeof(sslam_keypoint), sizeof(sslam_proj_query): include/sslam_frontend.h


@pytest.fixture(scope="module")
def ask():
    """ask(lines) -> one list of tokens per line; the plain and the sanitised build must answer alike, and the sanitised one must end clean (plan_dump.py)"""
    return plan_dump.asker()


def al(v):
    return (v + 255) // 256 * 256


def test_struct_sizes(ask):
    assert ask(["sizes"]) == [[str(KP), str(PQ)]]


def test_knn2_batch_plan(ask):
    r = ask(["knn2 4096 5", "knn2 4097 5", "knn2 1000 12", "knn2 96 5", "knn2 33 12", "knn2 4200 5", "knn2 1 1"])
    # 4096 rows = 128 tiles: the last capacity of the matrix-core form; 64 queries per workgroup, frames rounded up to groups of eight
    assert r[0] == ["matrix-core", "128", "64", str(8 * 1 * 64), str(5 * 128 * 8192)]
    assert r[1] == ["popcount", "129", "0", str((4097 + 15) // 16), "0"]
    assert r[2] == ["matrix-core", "32", "16", str(8 * 2 * 16), str(12 * 32 * 8192)]
    assert r[3] == ["matrix-core", "3", "2", "16", str(5 * 3 * 8192)]
    assert r[4] == ["matrix-core", "2", "1", "16", str(12 * 2 * 8192)]
    assert r[5] == ["popcount", "132", "0", "263", "0"]
    assert r[6] == ["matrix-core", "1", "1", "8", "8192"]


def _sfi_expect(cap, npairs):
    if npairs <= 8 and 64 + cap * 17 * 4 <= 150 * 1024:
        return ["speculative", str(64 + cap * 68), "0"]
    ccap = min(cap, max(256, cap * 3 // 8))
    if 64 + ccap * 64 <= 64 * 1024:
        return ["lds-batch", str(64 + ccap * 64), str(ccap)]
    return ["global", "0", "0"]


def test_sfi_plan(ask):
    last_spec = (150 * 1024 - 64) // 68                     # 2257: the last row capacity whose candidates fit 150 KB
    assert 64 + last_spec * 68 <= 150 * 1024 < 64 + (last_spec + 1) * 68
    last_lds = 2730                                         # the last capacity with 64 + (cap * 3 // 8) * 64 <= 64 KB
    assert 64 + (last_lds * 3 // 8) * 64 <= 64 * 1024 < 64 + ((last_lds + 1) * 3 // 8) * 64
    cases = [(last_spec, 1), (last_spec + 1, 1), (1000, 8), (1000, 9), (last_lds, 9), (last_lds + 1, 9), (last_lds, 1), (last_lds + 1, 1),
             (600, 9), (682, 9), (683, 9), (684, 20), (100, 9), (256, 9), (257, 9), (1, 1), (1, 9), (1040, 1), (2600, 9), (2800, 9), ((1 << 19) - 1, 1)]
    r = ask(["sfi %d %d" % c for c in cases])
    for c, got in zip(cases, r):
        assert got == _sfi_expect(*c), (c, got)
    forms = {c: g[0] for c, g in zip(cases, r)}
    assert forms[(last_spec, 1)] == "speculative" and forms[(last_spec + 1, 1)] == "lds-batch"
    assert forms[(1000, 8)] == "speculative" and forms[(1000, 9)] == "lds-batch"
    assert forms[(last_lds, 9)] == "lds-batch" and forms[(last_lds + 1, 9)] == "global"
    assert forms[(last_lds, 1)] == "lds-batch" and forms[(last_lds + 1, 1)] == "global"      # a single pair too long for the speculative kernel
    ccap = {c: int(g[2]) for c, g in zip(cases, r)}
    assert ccap[(600, 9)] == 256 and ccap[(682, 9)] == 256 and ccap[(683, 9)] == 256 and ccap[(684, 20)] == 256      # the floor: 3/8 of the rows is less
    assert ccap[(100, 9)] == 100 and ccap[(256, 9)] == 256 and ccap[(257, 9)] == 256 and ccap[(1, 9)] == 1          # clamped to the rows
    assert ccap[(1000, 9)] == 375 and ccap[(last_lds, 9)] == 1023


def test_proj_plan(ask):
    r = ask(["proj 2048 1000", "proj 2049 1000", "proj 8192 1", "proj 8193 1", "proj 1 5", "proj 500000 7"])
    assert r[0] == ["two-kernel", "1", str(64 * 2048 + 64), "250"]
    assert r[1] == ["two-kernel", "0", str(8 * 2049 + 64), "250"]
    assert r[2] == ["two-kernel", "0", str(8 * 8192 + 64), "1"]
    assert r[3] == ["one-wave", "0", "0", "0"]
    assert r[4] == ["two-kernel", "1", "128", "2"]
    assert r[5] == ["one-wave", "0", "0", "0"]


def test_cases_of_test_match_sizes_gpu(ask):
    """the case -> branch table in the docstring of tests/test_match_sizes_gpu.py"""
    r = ask(["proj 600 400", "proj 2100 400", "proj 6200 400", "proj 8200 400", "sfi 2300 1", "sfi 2900 1", "sfi 2100 9", "sfi 2800 9"])
    assert r[0][:2] == ["two-kernel", "1"] and int(r[0][2]) <= 48 * 1024                # features in LDS
    assert r[1][:2] == ["two-kernel", "0"] and int(r[1][2]) <= 48 * 1024                # features in global memory
    assert r[2][:2] == ["two-kernel", "0"] and int(r[2][2]) > 48 * 1024                 # more than 48 KB of dynamic LDS
    assert r[3][0] == "one-wave"
    assert r[4][0] == "lds-batch" and int(r[4][1]) > 48 * 1024 and int(r[4][2]) == 2300 * 3 // 8      # more than 150 KB for the speculative kernel
    assert r[5][0] == "global"
    assert r[6] == ["lds-batch", str(64 + 787 * 64), "787"] and 64 + 787 * 64 > 48 * 1024
    assert r[7][0] == "global"


@pytest.mark.parametrize("sizes", [[1], [0], [0, 0, 5], [256, 257, 255, 0, 1], [1000, 0, 0, 44000, 3, 256, 512, 0], [4 << 30, 1, (1 << 33) + 1, 0]])
def test_arena_layout(ask, sizes):
    """every block is 256-aligned and starts where the one before it ends, rounded up: blocks of non-zero size get strictly increasing offsets
    and never overlap; a block of size zero takes no room (it shares its offset with its successor, which is what the entry points rely on
    for absent inputs)"""
    got = [int(x) for x in ask(["arena " + " ".join(str(s) for s in sizes)])[0]]
    offs, total = got[:-1], got[-1]
    assert len(offs) == len(sizes) and offs[0] == 0
    for i, (o, b) in enumerate(zip(offs, sizes)):
        nxt = offs[i + 1] if i + 1 < len(offs) else total
        assert o % 256 == 0 and nxt == o + al(b)
        assert nxt >= o + b and (nxt > o) == (b > 0)
    assert total == sum(al(b) for b in sizes)


@pytest.mark.parametrize("n,nq", [(1000, 1000), (1, 1), (2100, 437), (8200, 37)])
def test_proj_arena(ask, n, nq):
    """search_proj_core: occ[n] | q[nq] | qdesc[32 nq] | assigned[4 n] | count (256) | scratch[4 (2 n + 2 nq)] | top[8 K nq] | cnt[4 nq]; the head up to the
    count has a pinned mirror"""
    K = 8
    blocks = [n, PQ * nq, 32 * nq, 4 * n, 256, 4 * (2 * n + 2 * nq), 8 * K * nq, 4 * nq]
    offs = [sum(al(b) for b in blocks[:i]) for i in range(len(blocks) + 1)]
    got = [int(x) for x in ask(["proj_arena %d %d %d" % (n, nq, K)])[0]]
    assert got[:9] == offs
    assert got[9] == offs[4] + 256 and got[10] == offs[4] + 64
    if (n, nq) == (1000, 1000):      # the formulas of the entry point before the helper existed (oO .. oC, total), by hand
        oQ = 1024; oQD = oQ + 44032; oA = oQD + 32000; oN = oA + 4096; oS = oN + 256; oT = oS + 16128; oC = oT + 64000; total = oC + 4096
        assert got[:9] == [0, oQ, oQD, oA, oN, oS, oT, oC, total] and total == 165632


@pytest.mark.parametrize("nkf,nf,nnodes,nk,nfi", [(1000, 900, 300, 950, 870), (1, 1, 1, 0, 0), (8292, 8300, 4115, 8292, 8300)])
def test_bow_arena(ask, nkf, nf, nnodes, nk, nfi):
    """search_by_bow_core: kpKF | dKF | validKF | kpF | dF | ptrKF | ptrF | idxKF | idxF (index lists of at least one entry) | assigned | count (256) | qbin | validF"""
    blocks = [KP * nkf, 32 * nkf, nkf, KP * nf, 32 * nf, 4 * (nnodes + 1), 4 * (nnodes + 1), 4 * max(nk, 1), 4 * max(nfi, 1), 4 * nf, 256, 4 * nf, nf]
    offs = [sum(al(b) for b in blocks[:i]) for i in range(len(blocks) + 1)]
    got = [int(x) for x in ask(["bow_arena %d %d %d %d %d" % (nkf, nf, nnodes, nk, nfi)])[0]]
    assert got == offs
    if nkf == 1000:                  # o[0] .. o[12] and the total of the entry point before the helper existed, by hand
        assert got == [0, 28160, 60160, 61184, 86528, 115456, 116736, 118016, 121856, 125440, 129280, 129536, 133376, 134400]
