// Prints what csrc/match_plan.h decides for a batch of SearchForTriangulation pairs (sslam_orb_search_for_triangulation_batch_dev), one answer per
// line of stdin (tests/test_tri_batch_plan_cpu.py).  Host code only:
//   consts           -> TRI_BATCH_WAVES TRI_BATCH_ROW_BYTES TRI_BATCH_LDS_MAX DYNAMIC_LDS_DEFAULT_MAX
//   plan CAP NPAIRS  -> form ldsBytes ldsOptIn threads grid
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../../structure-slam-pointline_amd/csrc/match_plan.h"

using namespace sslam;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        long long v[2] = {0, 0};
        int nv = 0;
        while (nv < 2 && in >> v[nv]) ++nv;
        if (cmd == "consts" && nv == 0) {
            printf("%d %d %zu %zu\n", TRI_BATCH_WAVES, TRI_BATCH_ROW_BYTES, TRI_BATCH_LDS_MAX, DYNAMIC_LDS_DEFAULT_MAX);
        } else if (cmd == "plan" && nv == 2) {
            const TriBatchPlan P = tri_batch_plan((int)v[0], (int)v[1]);
            printf("%s %zu %d %u %u\n", P.form == TriBatchForm::Lds ? "lds" : "global", P.ldsBytes, P.ldsOptIn, P.threads, P.grid);
        } else {
            fprintf(stderr, "tri_batch_plan_dump: cannot read '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
