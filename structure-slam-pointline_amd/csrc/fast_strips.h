// k_fast_cells' strip table (csrc/orb.hip): which FAST cells one wave handles together, and the constants of its exact divisions.  No HIP in here: build_plan
// includes it, and tests/sim/fast_strips_dump.cpp compiles it with plain g++ so that the CPU tests see the strips and constants the kernel gets.
#pragma once
#include <cstdint>
#include <vector>

namespace sslam_fast {

// A strip is up to FAST_STRIP_K horizontally adjacent cells of one cell row of one level.  Their detection rectangles abut (cell j + 1 starts where cell j ends), so
// the strip is one rectangle; every cell but the strip's last has the same width.  Three cells: tile + score tile + list stay at eleven LDS granules of 1 280 B for
// 640 x 480 (four cells with a list for four would take fifteen; beside the LSD core's guest form a compute unit has room for four waves of twelve).
constexpr int FAST_STRIP_K = 3;
// Survivors of the pre-test a strip keeps as a list: what three cells of the single-cell kernel's 832 kept.  The busiest cell of the bench's scenes has 825, so no
// strip of theirs can exceed it (tests/test_fast_strips_cpu.py replays the strips themselves: the busiest has 2 009).
constexpr int FAST_LIST_CAP = 832 * FAST_STRIP_K;
// A list entry is the pixel's index in the strip (row-major over the strip's rectangle) in 13 bits, its keep-code in bits 13-14.
constexpr int FAST_IDX_BITS = 13;
constexpr int FAST_MAX_PIXELS = 1 << FAST_IDX_BITS;
// floor(i / w) == (i * (2^20 / w + 1)) >> 20 as one 24-bit multiply (v_mul_u32_u24) and a shift: see fast_div_exact
constexpr int FAST_DIV_SHIFT = 20;

struct StripInfo {
    short level, x0, y0, x1, y1;  // the strip's detection rectangle [x0,x1) x [y0,y1) in level coordinates
    short nc;                     // cells in the strip (1 .. FAST_STRIP_K)
    short wc;                     // width of a cell of the strip (its last cell may be narrower)
    short pad;
    int cellBeg;                  // the strip's first cell in the frame's cell table
    unsigned magic, gmagic;       // 2^20 / strip width + 1 and 2^20 / (dword groups per row) + 1
    unsigned smagic;              // 2^20 / (dwords staged per tile row) + 1
};

inline unsigned fast_div_magic(int w) { return (1u << FAST_DIV_SHIFT) / (unsigned)w + 1; }

// Whether (i * fast_div_magic(w)) >> 20 == i / w for EVERY i < n with the kernel's arithmetic: both operands within 24 bits, the product within 32, and the
// constant's excess e = m * w - 2^20 (0 < e <= w) too small to carry into the quotient: i * m / 2^20 = i / w + i * e / (w * 2^20), and the second term stays
// below 1 / w -- the distance of i / w to the next integer is at least that -- as long as i * e < 2^20.
inline bool fast_div_exact(int w, int n) {
    if (w < 1 || n < 1) return false;
    const uint64_t m = fast_div_magic(w), e = m * (uint64_t)w - (1u << FAST_DIV_SHIFT);
    return m < (1u << 24) && (uint64_t)n <= (1u << 24) && (uint64_t)(n - 1) * m < (1ull << 32) && (uint64_t)(n - 1) * e < (1u << FAST_DIV_SHIFT);
}

// dword groups of a tile row that hold pixels of a rectangle starting at level column x0, w wide (the tile's first byte is the aligned column below x0 - 3)
inline int fast_groups(int x0, int w) {
    const int T0 = ((x0 - 3) & 3) + 3;
    return ((T0 + w - 1) >> 2) - (T0 >> 2) + 1;
}

// dwords staged per tile row: from the aligned column at or below x0 - 3 up to the dword that holds column x0 + w + 2
inline int fast_stage_dwords(int x0, int w) { return (((x0 - 3) & 3) + w + 6 + 3) >> 2; }

// whether one wave can take the rectangle [x0, x0 + w) x h: its pixels indexable in 13 bits, both divisions exact over their whole range
inline bool fast_strip_fits(int x0, int w, int h) {
    const int ng = fast_groups(x0, w);
    // (staging divides the lane number and the step of 64 by the dwords per row)
    return w * h <= FAST_MAX_PIXELS && fast_div_exact(w, w * h) && fast_div_exact(ng, ng * h) && fast_div_exact(fast_stage_dwords(x0, w), 65);
}

// The strips of a frame's cell table (cells in plan order: level by level, row by row, left to right).  A strip ends at the end of a cell row, after FAST_STRIP_K
// cells, after a cell narrower than the strip's first, before a cell that does not abut, and before a cell with which it would leave the range fast_strip_fits proves.
// false: a single cell is outside that range.
template <class Cell>
inline bool fast_build_strips(const Cell* cells, int n, std::vector<StripInfo>& out) {
    out.clear();
    for (int k = 0; k < n; ++k) {
        const Cell& c = cells[k];
        const int h = c.y1 - c.y0;
        bool extend = false;
        if (!out.empty()) {
            const StripInfo& s = out.back();
            extend = s.level == c.level && s.y0 == c.y0 && s.y1 == c.y1 && s.x1 == c.x0 && s.nc < FAST_STRIP_K && s.cellBeg + s.nc == k &&
                     s.x1 - s.x0 == s.nc * s.wc && c.x1 - c.x0 <= s.wc && fast_strip_fits(s.x0, c.x1 - s.x0, h);
        }
        if (extend) { out.back().x1 = c.x1; out.back().nc++; }
        else {
            if (!fast_strip_fits(c.x0, c.x1 - c.x0, h)) return false;
            StripInfo s{};
            s.level = c.level; s.x0 = c.x0; s.y0 = c.y0; s.x1 = c.x1; s.y1 = c.y1; s.nc = 1; s.wc = (short)(c.x1 - c.x0); s.cellBeg = k;
            out.push_back(s);
        }
    }
    for (StripInfo& s : out) { s.magic = fast_div_magic(s.x1 - s.x0); s.gmagic = fast_div_magic(fast_groups(s.x0, s.x1 - s.x0)); s.smagic = fast_div_magic(fast_stage_dwords(s.x0, s.x1 - s.x0)); }
    return true;
}

}  // namespace sslam_fast
