// Prints what csrc/match_plan.h decides for the inputs on stdin, one answer per line (tests/plan_dump.py and the tests/test_*plan_cpu.py).  Host code only.
// Without a family in front, the plans of the single calls and the arenas (tests/test_match_plan_cpu.py):
//   knn2 CAP NFRAMES                 -> form tilesCap qblocks grid expandBytes
//   sfi CAP NPAIRS                   -> form ldsBytes ccap
//   proj N NQ                        -> form featsInLds ldsBytes topkGrid
//   proj_arena N NQ PROJ_K           -> occ q qdesc assigned count scratch top cnt total pinnedBytes stats
//   bow_arena NKF NF NNODES NK NFI   -> in[0..8] assigned count qbin validF total
//   arena BYTES...                   -> the offset of every take(), then size()
//   sizes                            -> sizeof(sslam_keypoint) sizeof(sslam_proj_query)
//   twoview CAP, sim3 CAP            -> rowBytes ldsBytes ldsOptIn threads maxCap (two_view_plan, sim3_plan: the RANSAC units)
// The first token of a line may name the family of a device-resident batch instead:
//   proj_batch (sslam_search_by_projection_batch_dev)
//     consts                                      -> PROJ_MAXN PROJ_TWO_KERNEL_MAXN PROJ_K PROJ_BATCH_SCRATCH_MAX PROJ_BATCH_MAX_SLICE DYNAMIC_LDS_DEFAULT_MAX
//     plan CAP QCAP NFRAMES [MAXSLICE FEATSINLDS] -> form featsInLds ldsBytes ldsOptIn topkGrid frameBytes slice
//     arena CAP QCAP SLICE PROJ_K                 -> scratch top cnt total
//     slices CAP QCAP NFRAMES [MAXSLICE]          -> first:count of every slice in launch order
//     single N NQ                                 -> form of proj_plan(N, NQ)
//   bow_batch (sslam_orb_search_by_bow_batch_dev), tri_batch (sslam_orb_search_for_triangulation_batch_dev)
//     consts                -> BATCH_WAVES {BOW,TRI}_BATCH_ROW_BYTES BATCH_LDS_MAX DYNAMIC_LDS_DEFAULT_MAX
//     plan CAP NPAIRS       -> form ldsBytes ldsOptIn threads grid
//   fuse_batch (sslam_fuse_search_batch_dev)
//     consts                -> BATCH_WAVES FUSE_BATCH_ROW_BYTES FUSE_BATCH_CHUNK BATCH_LDS_MAX DYNAMIC_LDS_DEFAULT_MAX
//     plan CAP QCAP NJOBS   -> form ldsBytes ldsOptIn threads chunks grid
//   distinct_batch (sslam_distinctive_descriptors_batch_dev)
//     consts          -> DISTINCT_SMALL_MAX DISTINCT_MEDIUM_MAX DISTINCT_LARGE_MAX DISTINCT_SETS_PER_WAVE DISTINCT_BATCH_WAVES DISTINCT_BATCH_GRID_MAX
//                        DISTINCT_MEDIUM_ROW_BYTES DISTINCT_MEDIUM_DIST_BYTES DISTINCT_LARGE_CHUNK DISTINCT_LARGE_GRID_MAX DISTINCT_LARGE_LDS_BYTES
//     class ENTRIES   -> small | medium | large | refused
//     plan NSETS      -> launches threads grid ldsBytes largeThreads largeGrid largeLdsBytes
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../../structure-slam-pointline_amd/csrc/match_plan.h"

using namespace sslam;

static const char* form_name(ProjForm f) { return f == ProjForm::TwoKernel ? "two-kernel" : "one-wave"; }

// every function answers one line whose command is `cmd` and whose numbers are v[0 .. nv), and says whether it could
static bool single_calls(const std::string& cmd, const long long* v, int nv) {
    if (cmd == "knn2" && nv == 2) {
        const Knn2Plan P = knn2_batch_plan((int)v[0], (int)v[1]);
        printf("%s %d %d %u %zu\n", P.form == Knn2Form::MatrixCore ? "matrix-core" : "popcount", P.tilesCap, P.qblocks, P.grid, P.expandBytes);
    } else if (cmd == "sfi" && nv == 2) {
        const SfiPlan P = sfi_plan((int)v[0], (int)v[1]);
        printf("%s %zu %d\n", P.form == SfiForm::Speculative ? "speculative" : P.form == SfiForm::LdsBatch ? "lds-batch" : "global", P.ldsBytes, P.ccap);
    } else if (cmd == "proj" && nv == 2) {
        const ProjPlan P = proj_plan((int)v[0], (int)v[1]);
        printf("%s %d %zu %u\n", form_name(P.form), P.featsInLds, P.ldsBytes, P.topkGrid);
    } else if (cmd == "proj_arena" && nv == 3) {
        const ProjArena a = proj_arena((int)v[0], (int)v[1], (int)v[2]);
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", a.occ, a.q, a.qdesc, a.assigned, a.count, a.scratch, a.top, a.cnt, a.total, a.pinnedBytes(), a.stats());
    } else if (cmd == "bow_arena" && nv == 5) {
        const BowArena a = bow_arena((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]);
        for (int i = 0; i < 9; ++i) printf("%zu ", a.in[i]);
        printf("%zu %zu %zu %zu %zu\n", a.assigned, a.count, a.qbin, a.validF, a.total);
    } else if ((cmd == "twoview" || cmd == "sim3") && nv == 1) {
        const RansacPlan P = cmd == "sim3" ? sim3_plan((int)v[0]) : two_view_plan((int)v[0]);
        printf("%d %zu %d %u %d\n", P.rowBytes, P.ldsBytes, P.ldsOptIn, P.threads, P.maxCap);
    } else if (cmd == "sizes") {
        printf("%zu %zu\n", sizeof(sslam_keypoint), sizeof(sslam_proj_query));
    } else return false;
    return true;
}

static bool proj_batch(const std::string& cmd, const long long* v, int nv) {
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
    } else return false;
    return true;
}

static void print_batch_plan(const BatchPlan& P) { printf("%s %zu %d %u", P.form == BatchForm::Lds ? "lds" : "global", P.ldsBytes, P.ldsOptIn, P.threads); }

// SearchByBoW and SearchForTriangulation: the shared plan at the matcher's bytes per row, one workgroup per pair
static bool pair_batch(int rowBytes, const std::string& cmd, const long long* v, int nv) {
    if (cmd == "consts" && nv == 0) {
        printf("%d %d %zu %zu\n", BATCH_WAVES, rowBytes, BATCH_LDS_MAX, DYNAMIC_LDS_DEFAULT_MAX);
    } else if (cmd == "plan" && nv == 2) {
        print_batch_plan(batch_plan(rowBytes, (int)v[0]));
        printf(" %u\n", (unsigned)(int)v[1]);
    } else return false;
    return true;
}

static bool fuse_batch(const std::string& cmd, const long long* v, int nv) {
    if (cmd == "consts" && nv == 0) {
        printf("%d %d %d %zu %zu\n", BATCH_WAVES, FUSE_BATCH_ROW_BYTES, FUSE_BATCH_CHUNK, BATCH_LDS_MAX, DYNAMIC_LDS_DEFAULT_MAX);
    } else if (cmd == "plan" && nv == 3) {
        print_batch_plan(batch_plan(FUSE_BATCH_ROW_BYTES, (int)v[0]));
        printf(" %u %llu\n", fuse_batch_chunks((int)v[1]), fuse_batch_grid((int)v[2], (int)v[1]));
    } else return false;
    return true;
}

static bool distinct_batch(const std::string& cmd, const long long* v, int nv) {
    if (cmd == "consts" && nv == 0) {
        printf("%d %d %d %d %d %u %zu %zu %d %u %zu\n", DISTINCT_SMALL_MAX, DISTINCT_MEDIUM_MAX, DISTINCT_LARGE_MAX, DISTINCT_SETS_PER_WAVE, DISTINCT_BATCH_WAVES,
               DISTINCT_BATCH_GRID_MAX, DISTINCT_MEDIUM_ROW_BYTES, DISTINCT_MEDIUM_DIST_BYTES, DISTINCT_LARGE_CHUNK, DISTINCT_LARGE_GRID_MAX, DISTINCT_LARGE_LDS_BYTES);
    } else if (cmd == "class" && nv == 1) {
        static const char* const names[] = {"small", "medium", "large", "refused"};
        printf("%s\n", names[(int)distinct_class(v[0])]);
    } else if (cmd == "plan" && nv == 1) {
        const DistinctBatchPlan P = distinct_batch_plan((int)v[0]);
        printf("%d %u %u %zu %u %u %zu\n", P.launches, P.threads, P.grid, P.ldsBytes, P.largeThreads, P.largeGrid, P.largeLdsBytes);
    } else return false;
    return true;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string family, cmd;
        if (!(in >> family)) continue;
        if (family == "arena") {      // the one command with any number of operands
            ArenaLayout L;
            unsigned long long b;
            while (in >> b) printf("%zu ", L.take((size_t)b));
            printf("%zu\n", L.size());
            continue;
        }
        const bool batch = family == "proj_batch" || family == "bow_batch" || family == "tri_batch" || family == "fuse_batch" || family == "distinct_batch";
        if (batch) in >> cmd; else cmd = family;
        long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int nv = 0;
        while (nv < 8 && in >> v[nv]) ++nv;
        const bool ok = !batch ? single_calls(cmd, v, nv) : family == "proj_batch" ? proj_batch(cmd, v, nv) : family == "bow_batch" ? pair_batch(BOW_BATCH_ROW_BYTES, cmd, v, nv) :
                        family == "tri_batch" ? pair_batch(TRI_BATCH_ROW_BYTES, cmd, v, nv) : family == "fuse_batch" ? fuse_batch(cmd, v, nv) : distinct_batch(cmd, v, nv);
        if (!ok) {
            fprintf(stderr, "match_plan_dump: cannot read '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
