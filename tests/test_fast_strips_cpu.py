"""k_fast_cells' strips on the CPU (csrc/fast_strips.h through tests/sim/fast_strips_dump.cpp): the magic divisions are exact over every range a plan can ask for,
every cell is in exactly one strip, and the frames tests/test_fast_strips_gpu.py runs reach what they are named after -- from the oracle's candidates and a numpy
replay of the pre-test."""
import numpy as np
import pytest
import fast_strip_cases as fc
import orb_tail_cases as otc
from synth import synth_frame, warp_prev

SIZES = [(640, 480), (1280, 960), (97, 83), (fc.CAP_W, fc.CAP_H), (320, 240)] + [(w, 97) for w in fc.ROW_WIDTHS.values()]
BUSIEST_BENCH_STRIP = 2009          # survivors of the pre-test in the busiest strip of the 16 bench frames below (a strip has 3 774 pixels at most; the cap is 2 496)
BENCH_KINDS = [(60, 40, 2.0), (35, 25, 2.0), (90, 60, 2.0), (60, 40, 3.5), (45, 70, 1.0), (75, 30, 2.5), (60, 40, 2.0), (50, 50, 2.0)]      # bench.py synth_frames


def _groups(x0, w):
    t0 = ((x0 - 3) & 3) + 3
    return ((t0 + w - 1) >> 2) - (t0 >> 2) + 1


def _stage_dwords(x0, w):
    return (((x0 - 3) & 3) + w + 9) >> 2


def test_magic_divisions_are_exact_for_every_strip_a_plan_can_produce():
    """(i * magic) >> shift == i // w for every i the kernel divides: pixel index by strip width, pass A's item by the dword groups per row, the staging's lane number
    and step (i <= 64) by the dwords per row -- with both operands of the multiply within 24 bits and the product within 32, as v_mul_u32_u24 computes it"""
    seen = set()
    for w, h in SIZES:
        consts, strips, _ = fc.plan(w, h)
        sh = consts["shift"]
        for s in strips:
            sw, ch = s["x1"] - s["x0"], s["y1"] - s["y0"]
            assert sw * ch <= 1 << consts["idx_bits"]
            ng, nd = _groups(s["x0"], sw), _stage_dwords(s["x0"], sw)
            for d, m, n in ((sw, s["magic"], sw * ch), (ng, s["gmagic"], ng * ch), (nd, s["smagic"], 65)):
                if (d, m, n) in seen: continue
                seen.add((d, m, n))
                assert m == (1 << sh) // d + 1 < 1 << 24 and n <= 1 << 24
                i = np.arange(n, dtype=np.uint64)
                p = i * np.uint64(m)
                assert int(p.max()) < 1 << 32
                assert np.array_equal(p >> np.uint64(sh), i // np.uint64(d)), (w, h, d, n)
    print("distinct (divisor, constant, range) triples:", len(seen))
    assert len(seen) > 10


def test_divisions_over_the_whole_admitted_range():
    """whatever strip fast_strip_fits admits (not only those of the sizes above): every width up to the 13-bit index range, with the largest item count of that width"""
    sh, top = fc.consts()["shift"], 1 << fc.consts()["idx_bits"]
    for d in range(1, 257):
        m = (1 << sh) // d + 1
        e = m * d - (1 << sh)
        n = min(top, ((1 << sh) - 1) // e + 1)          # fast_div_exact admits i * e < 2^shift
        i = np.arange(n, dtype=np.uint64)
        assert np.array_equal((i * np.uint64(m)) >> np.uint64(sh), i // np.uint64(d)), d
        if d <= 128: assert n == top, d                 # e <= d: up to 128 columns a strip has the whole index range (2^20 / 128 = 2^13); wider ones as far as e allows


@pytest.mark.parametrize("w,h", SIZES)
def test_every_cell_is_in_exactly_one_strip(w, h):
    consts, strips, cells = fc.plan(w, h)
    K = consts["K"]
    owner = np.zeros(len(cells), int)
    for s in strips:
        mine = cells[s["cellBeg"]:s["cellBeg"] + s["nc"]]
        assert 1 <= s["nc"] <= K and len(mine) == s["nc"]
        owner[s["cellBeg"]:s["cellBeg"] + s["nc"]] += 1
        assert {c[0] for c in mine} == {s["level"]} and {(c[2], c[4]) for c in mine} == {(s["y0"], s["y1"])}      # one level, one cell row
        assert mine[0][1] == s["x0"] and mine[-1][3] == s["x1"]
        for k, c in enumerate(mine):
            assert c[1] == s["x0"] + k * s["wc"] and c[3] == (s["x1"] if k == s["nc"] - 1 else c[1] + s["wc"])     # abutting, equal widths but for the last
    assert (owner == 1).all()
    # per cell row: full strips, then one of nCols mod K cells
    for l, L in enumerate(otc.levels(w, h, fc.NLEVELS)):
        for y0 in sorted({c[1] for c in L["cells"]}):
            ncols = sum(1 for c in L["cells"] if c[1] == y0)
            got = [s["nc"] for s in strips if s["level"] == l and s["y0"] == y0]
            assert got == [K] * (ncols // K) + ([ncols % K] if ncols % K else []), (l, y0, ncols, got)


def test_a_cell_beyond_the_index_range_is_refused_and_a_wide_row_is_cut_short():
    consts, strips = fc.dump([(0, 19, 19, 19 + 100, 19 + 100)])
    assert strips is None
    consts, strips = fc.dump([(0, 19 + 59 * k, 19, 19 + 59 * (k + 1), 19 + 59) for k in range(3)])      # 3 x 59 x 59 = 10 443 pixels: two cells, then one
    assert [s["nc"] for s in strips] == [2, 1]


def test_level0_rows_have_the_cell_counts_they_are_named_after():
    K = fc.consts()["K"]
    want = {"row1": 1, "rowK": K, "rowK1": K + 1, "row2K1": 2 * K + 1}
    for name, w in fc.ROW_WIDTHS.items():
        img = fc.frame(name)
        assert img.shape == (97, w)
        L0 = otc.levels(w, 97, fc.NLEVELS)[0]
        assert len({c[0] for c in L0["cells"]}) == want[name], name
    assert [len(L["cells"]) for L in otc.levels(97, 83, fc.NLEVELS)] == [2, 1, 0, 0, 0, 0, 0, 0] and fc.frame("small").shape == (83, 97)


@pytest.mark.parametrize("name,path", [("bands", "list"), ("noise320", "restart")])
def test_corners_on_either_side_of_a_border(oracle, name, path):
    """two corners of different scores in adjacent columns: the weaker one lives only because the stronger one belongs to the next cell -- inside a strip (the rim mask
    of keep_code) and across a strip border (the score tile's zero rim)"""
    img = fc.frame(name)
    cap = fc.consts()["cap"]
    busiest = int(fc.survivors(oracle, img)[0].max())
    pairs = fc.border_pairs(oracle, img)
    inner, outer = [p for p in pairs if p[1]], [p for p in pairs if not p[1]]
    print(name, "busiest strip:", busiest, "pairs inside a strip:", len(inner), "across strips:", len(outer))
    assert (busiest <= cap) if path == "list" else (busiest > cap)
    assert len(inner) >= 10 and len(outer) >= 10
    assert all(p[2] < p[3] and p[2] >= fc.MIN_TH for p in pairs)


def test_ini_and_min_threshold_cells_share_a_strip(oracle):
    img = fc.frame("ini_min")
    _, strips, cells = fc.plan(img.shape[1], img.shape[0])
    mixed = 0
    for s in strips:
        if s["level"] or s["nc"] < 2: continue
        best = []
        for c in cells[s["cellBeg"]:s["cellBeg"] + s["nc"]]:
            cc = fc.cell_candidates(oracle, img, 0, c)
            assert len(cc) > 0
            best.append(int(cc[:, 2].max()))
        assert min(best) < fc.INI_TH <= max(best), best          # a cell whose candidates are all below iniTh came through the minTh fallback
        mixed += 1
    assert mixed >= 2


def test_an_empty_cell_between_two_cells_with_candidates(oracle):
    img = fc.frame("empty_between")
    _, strips, cells = fc.plan(img.shape[1], img.shape[0])
    found = 0
    for s in strips:
        if s["level"] or s["nc"] < 3: continue
        n = [len(fc.cell_candidates(oracle, img, 0, c)) for c in cells[s["cellBeg"]:s["cellBeg"] + s["nc"]]]
        assert n[1] == 0 and n[0] > 0 and n[2] > 0, n
        found += 1
    assert found >= 2


def test_strips_at_the_cap_and_one_beyond(oracle):
    cap = fc.consts()["cap"]
    for name, want in (("at_cap", cap), ("cap_plus_1", cap + 1)):
        img = fc.frame(name)
        st, ce = fc.survivors(oracle, img)
        _, strips, cells = fc.plan(img.shape[1], img.shape[0])
        k = int(st.argmax())
        s = strips[k]
        print(name, "busiest strip:", int(st[k]), "its cells:", ce[s["cellBeg"]:s["cellBeg"] + s["nc"]])
        assert int(st[k]) == want and s["level"] == 0 and s["nc"] == 3
        assert (np.delete(st, k) < cap).all()
        third = cells[s["cellBeg"] + 2]
        assert 0 < ce[s["cellBeg"] + 2] <= 50 and len(fc.cell_candidates(oracle, img, 0, third)) > 0      # the sparse neighbour, with corners of its own


def test_no_strip_of_the_bench_scenes_exceeds_the_cap(oracle):
    """the condition FAST_LIST_CAP carries over from cells to strips: one scene of each of bench.py's eight kinds and its warped predecessor, all eight levels (the
    frames tests/test_guest_budget_gpu.py replays per cell: busiest cell 825)"""
    cap = fc.consts()["cap"]
    worst, over = 0, 0
    for i in (0, 1, 2, 3, 4, 5, 30, 7):
        ns, nst, noise = BENCH_KINDS[i % 8]
        f = synth_frame(2000 + i, 640, 480, nshapes=ns, nstrokes=nst, noise=noise)
        for img in (f, warp_prev(f)):
            st = fc.survivors(oracle, img)[0]
            worst = max(worst, int(st.max())); over += int((st > cap).sum())
    print("busiest strip of 16 bench frames:", worst)
    assert over == 0 and worst == BUSIEST_BENCH_STRIP <= cap

