// The strip table of k_fast_cells as build_plan makes it (csrc/fast_strips.h holds no HIP), for tests/fast_strip_cases.py: plain g++, a stand-alone program.
// stdin: one cell per line "level x0 y0 x1 y1", in plan order.  stdout: a first line "K cap idx_bits shift", then one line per strip
// "level x0 y0 x1 y1 nc wc cellBeg magic gmagic smagic"; "refused" instead when a cell is outside the proven range.
#include <cstdio>
#include <vector>
#include "../../structure-slam-pointline_amd/csrc/fast_strips.h"

struct Cell { int level, x0, y0, x1, y1; };

int main() {
    using namespace sslam_fast;
    std::vector<Cell> cells;
    Cell c;
    while (std::scanf("%d %d %d %d %d", &c.level, &c.x0, &c.y0, &c.x1, &c.y1) == 5) cells.push_back(c);
    std::vector<StripInfo> strips;
    std::printf("%d %d %d %d\n", FAST_STRIP_K, FAST_LIST_CAP, FAST_IDX_BITS, FAST_DIV_SHIFT);
    if (!fast_build_strips(cells.data(), (int)cells.size(), strips)) { std::printf("refused\n"); return 0; }
    for (const StripInfo& s : strips)
        std::printf("%d %d %d %d %d %d %d %d %u %u %u\n", s.level, s.x0, s.y0, s.x1, s.y1, s.nc, s.wc, s.cellBeg, s.magic, s.gmagic, s.smagic);
    return 0;
}
