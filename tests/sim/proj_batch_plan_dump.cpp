// Prints what csrc/match_plan.h decides for a batch of the projection-window matcher (sslam_search_by_projection_batch_dev), one answer per line
// of stdin (tests/test_proj_batch_plan_cpu.py).  Host code only:
//   consts                                     -> PROJ_MAXN PROJ_TWO_KERNEL_MAXN PROJ_K PROJ_BATCH_SCRATCH_MAX PROJ_BATCH_MAX_SLICE DYNAMIC_LDS_DEFAULT_MAX
//   plan CAP QCAP NFRAMES [MAXSLICE FEATSINLDS] -> form featsInLds ldsBytes ldsOptIn topkGrid frameBytes slice
//   arena CAP QCAP SLICE PROJ_K                -> scratch top cnt total
//   slices CAP QCAP NFRAMES [MAXSLICE]         -> first:count of every slice in launch order
//   single N NQ                                -> form of proj_plan(N, NQ)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../../structure-slam-pointline_amd/csrc/match_plan.h"

using namespace sslam;

static const char* form_name(ProjForm f) { return f == ProjForm::TwoKernel ? "two-kernel" : "one-wave"; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        long long v[5] = {0, 0, 0, 0, 0};
        int nv = 0;
        while (nv < 5 && in >> v[nv]) ++nv;
        ProjBatchTuning tune;
        if (cmd == "consts" && nv == 0) {
            printf("%d %d %d %zu %d %zu\n", PROJ_MAXN, PROJ_TWO_KERNEL_MAXN, PROJ_K, PROJ_BATCH_SCRATCH_MAX, PROJ_BATCH_MAX_SLICE, DYNAMIC_LDS_DEFAULT_MAX);
        } else if (cmd == "plan" && (nv == 3 || nv == 5)) {
            tune.maxSlice = (int)v[3]; tune.featsInLds = (int)v[4];
            const ProjBatchPlan P = proj_batch_plan((int)v[0], (int)v[1], (int)v[2], tune);
            printf("%s %d %zu %d %u %zu %d\n", form_name(P.form), P.featsInLds, P.ldsBytes, P.ldsOptIn, P.topkGrid, P.frameBytes, P.slice);
        } else if (cmd == "arena" && nv == 4) {
            const ProjBatchArena a = proj_batch_arena((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
            printf("%zu %zu %zu %zu\n", a.scratch, a.top, a.cnt, a.total);
        } else if (cmd == "slices" && (nv == 3 || nv == 4)) {
            tune.maxSlice = (int)v[3];
            const int nframes = (int)v[2];
            const ProjBatchPlan P = proj_batch_plan((int)v[0], (int)v[1], nframes, tune);
            const int ns = proj_batch_slices(P, nframes);
            for (int s = 0; s < ns; ++s) {
                const ProjBatchSlice sl = proj_batch_slice(P, nframes, s);
                printf("%d:%d%s", sl.first, sl.count, s + 1 < ns ? " " : "");
            }
            printf("\n");
        } else if (cmd == "single" && nv == 2) {
            printf("%s\n", form_name(proj_plan((int)v[0], (int)v[1]).form));
        } else {
            fprintf(stderr, "proj_batch_plan_dump: cannot read '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
