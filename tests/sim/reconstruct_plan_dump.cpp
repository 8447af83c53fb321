// reconstruct_plan (csrc/match_plan.h) and the argument rules of the reconstruct entry points (csrc/match_check.h) on the host: a stand-alone program that
// tests/test_reconstruct_plan_cpu.py builds with plain g++, once as it is and once under the sanitizers.
//   in : "plan" cap lcap | "params" sigma-bits min_triangulated | "sizes" npairs cap lcap | "lines" 11 x 0/1 lcap          (one request per line, until end of input)
//   out: plan: rowBytes lineRowBytes wsOff lineOff rowOff keyOff flagOff ldsBytes ldsOptIn threads maxCap maxLcap | one 0/1 or -1/0/1 for the rules
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include "../../structure-slam-pointline_amd/csrc/match_check.h"

namespace sslam { void set_error(const char*, ...) {} }
using namespace sslam;

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "plan")) {
            int cap, lcap;
            if (scanf("%d %d", &cap, &lcap) != 2) return 2;
            const ReconstructPlan P = reconstruct_plan(cap, lcap);
            printf("%d %d %zu %zu %zu %zu %zu %zu %d %u %d %d\n", P.rowBytes, P.lineRowBytes, P.wsOff, P.lineOff, P.rowOff, P.keyOff, P.flagOff, P.ldsBytes, P.ldsOptIn, P.threads,
                   P.maxCap, P.maxLcap);
        } else if (!strcmp(what, "params")) {
            unsigned u; int mt; float sigma;
            if (scanf("%u %d", &u, &mt) != 2) return 2;
            memcpy(&sigma, &u, 4);
            printf("%d\n", reconstruct_params_ok(sigma, mt) ? 1 : 0);
        } else if (!strcmp(what, "sizes")) {
            int np, cap, lcap;
            if (scanf("%d %d %d", &np, &cap, &lcap) != 3) return 2;
            printf("%d\n", reconstruct_sizes_ok(np, cap, lcap) ? 1 : 0);
        } else if (!strcmp(what, "lines")) {
            int g[11], lcap;
            for (int& x : g) if (scanf("%d", &x) != 1) return 2;
            if (scanf("%d", &lcap) != 1) return 2;
            static const char one = 0;
            const void* p[11];
            for (int i = 0; i < 11; ++i) p[i] = g[i] ? &one : nullptr;
            printf("%d\n", reconstruct_lines_given(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], lcap));
        } else return 2;
    }
    return 0;
}
