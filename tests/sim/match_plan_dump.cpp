// Prints what csrc/match_plan.h decides for the inputs on stdin, one answer per line (tests/test_match_plan_cpu.py).  Host code only:
//   knn2 CAP NFRAMES                 -> form tilesCap qblocks grid expandBytes
//   sfi CAP NPAIRS                   -> form ldsBytes ccap
//   proj N NQ                        -> form featsInLds ldsBytes topkGrid
//   proj_arena N NQ PROJ_K           -> occ q qdesc assigned count scratch top cnt total pinnedBytes stats
//   bow_arena NKF NF NNODES NK NFI   -> in[0..8] assigned count qbin validF total
//   arena BYTES...                   -> the offset of every take(), then size()
//   sizes                            -> sizeof(sslam_keypoint) sizeof(sslam_proj_query)
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
        long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int nv = 0;
        if (cmd != "arena") while (nv < 8 && in >> v[nv]) ++nv;
        if (cmd == "knn2" && nv == 2) {
            const Knn2Plan P = knn2_batch_plan((int)v[0], (int)v[1]);
            printf("%s %d %d %u %zu\n", P.form == Knn2Form::MatrixCore ? "matrix-core" : "popcount", P.tilesCap, P.qblocks, P.grid, P.expandBytes);
        } else if (cmd == "sfi" && nv == 2) {
            const SfiPlan P = sfi_plan((int)v[0], (int)v[1]);
            printf("%s %zu %d\n", P.form == SfiForm::Speculative ? "speculative" : P.form == SfiForm::LdsBatch ? "lds-batch" : "global", P.ldsBytes, P.ccap);
        } else if (cmd == "proj" && nv == 2) {
            const ProjPlan P = proj_plan((int)v[0], (int)v[1]);
            printf("%s %d %zu %u\n", P.form == ProjForm::TwoKernel ? "two-kernel" : "one-wave", P.featsInLds, P.ldsBytes, P.topkGrid);
        } else if (cmd == "proj_arena" && nv == 3) {
            const ProjArena a = proj_arena((int)v[0], (int)v[1], (int)v[2]);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", a.occ, a.q, a.qdesc, a.assigned, a.count, a.scratch, a.top, a.cnt, a.total, a.pinnedBytes(), a.stats());
        } else if (cmd == "bow_arena" && nv == 5) {
            const BowArena a = bow_arena((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]);
            for (int i = 0; i < 9; ++i) printf("%zu ", a.in[i]);
            printf("%zu %zu %zu %zu %zu\n", a.assigned, a.count, a.qbin, a.validF, a.total);
        } else if (cmd == "arena") {
            ArenaLayout L;
            unsigned long long b;
            while (in >> b) printf("%zu ", L.take((size_t)b));
            printf("%zu\n", L.size());
        } else if (cmd == "sizes") {
            printf("%zu %zu\n", sizeof(sslam_keypoint), sizeof(sslam_proj_query));
        } else {
            fprintf(stderr, "match_plan_dump: cannot read '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
