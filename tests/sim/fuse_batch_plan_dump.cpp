// Prints what csrc/match_plan.h decides for a batch of Fuse / SearchBySim3 candidate searches (sslam_fuse_search_batch_dev), one answer per line of
// stdin (tests/test_fuse_batch_plan_cpu.py).  Host code only:
//   consts                -> FUSE_BATCH_WAVES FUSE_BATCH_ROW_BYTES FUSE_BATCH_CHUNK FUSE_BATCH_LDS_MAX DYNAMIC_LDS_DEFAULT_MAX
//   plan CAP QCAP NJOBS   -> form ldsBytes ldsOptIn threads chunks grid
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
        long long v[3] = {0, 0, 0};
        int nv = 0;
        while (nv < 3 && in >> v[nv]) ++nv;
        if (cmd == "consts" && nv == 0) {
            printf("%d %d %d %zu %zu\n", FUSE_BATCH_WAVES, FUSE_BATCH_ROW_BYTES, FUSE_BATCH_CHUNK, FUSE_BATCH_LDS_MAX, DYNAMIC_LDS_DEFAULT_MAX);
        } else if (cmd == "plan" && nv == 3) {
            const FuseBatchPlan P = fuse_batch_plan((int)v[0], (int)v[1], (int)v[2]);
            printf("%s %zu %d %u %u %llu\n", P.form == FuseBatchForm::Lds ? "lds" : "global", P.ldsBytes, P.ldsOptIn, P.threads, P.chunks, P.grid);
        } else {
            fprintf(stderr, "fuse_batch_plan_dump: cannot read '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
