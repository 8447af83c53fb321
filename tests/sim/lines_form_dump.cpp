// Prints what csrc/lines_form.h decides for the inputs on stdin, one answer per line (tests/plan_dump.py, tests/test_lines_form_cpu.py, tests/test_lines_form_gpu.py).
// Host code only.  Behind the numbers a line may set environment knobs as NAME=VALUE tokens: they are what lines_knobs_from's lookup finds, and nothing else is.
//   consts                                               -> LINES_CLUSTER_MAX_FRAMES LINES_CLUSTER_MAX_SW LINES_CLUSTER_MAX_SH LINES_CLUSTER_LDS_SW LINES_CLUSTER_LDS_SH LINES_CL_MAXWG
//                                                           LINES_CL_SUB LINES_SORT_RUNS_MAX_SIDE LINES_LBD_RPI_MAX_SIDE LINES_NFA_BEHIND_WAVES
//   knobs [NAME=VALUE ...]                               -> lone cluster persist clWgs clWindow clSmap nfaStreamWaves nfaSpinTicks nfaFused
//   forms W H SW SH NFRAMES NUMCUS COREEVENT TOPNMAXLINES [NAME=VALUE ...]
//                                                        -> core guestGrid guestFits sortRuns clWgs clWindow clSmap bigFrame nfa evalWaves countWaves topnMaxLines streamWaves
//                                                           spinTicks forkBlurSobel lbdRpi
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../../structure-slam-pointline_amd/csrc/lines_form.h"

using namespace sslam;

static std::map<std::string, std::string> g_env;      // the knobs of the line being answered
static const char* lookup(const char* name) {
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

int main() {
    static const char* const core[] = {"cluster_stream", "cluster", "lone", "guest", "per_frame", "six_wave"};
    static const char* const nfa[] = {"stream", "launches", "all", "topn"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int nv = 0;
        bool ok = true;
        g_env.clear();
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq != std::string::npos) g_env[tok.substr(0, eq)] = tok.substr(eq + 1);
            else if (nv < 8 && g_env.empty()) {
                try { size_t used = 0; v[nv] = std::stoll(tok, &used); ok = ok && used == tok.size(); ++nv; } catch (...) { ok = false; }
            } else ok = false;
        }
        if (ok && cmd == "consts" && nv == 0 && g_env.empty()) {
            printf("%d %d %d %d %d %d %d %d %d %d\n", LINES_CLUSTER_MAX_FRAMES, LINES_CLUSTER_MAX_SW, LINES_CLUSTER_MAX_SH, LINES_CLUSTER_LDS_SW, LINES_CLUSTER_LDS_SH, LINES_CL_MAXWG,
                   LINES_CL_SUB, LINES_SORT_RUNS_MAX_SIDE, LINES_LBD_RPI_MAX_SIDE, LINES_NFA_BEHIND_WAVES);
        } else if (ok && cmd == "knobs" && nv == 0) {
            const LinesKnobs K = lines_knobs_from(lookup);
            printf("%d %d %d %d %d %d %d %lld %d\n", K.lone, (int)K.cluster, K.persist, K.clWgs, K.clWindow, K.clSmap, K.nfaStreamWaves, K.nfaSpinTicks, K.nfaFused);
        } else if (ok && cmd == "forms" && nv == 8) {
            const LinesForms F = lines_forms((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] != 0, (int)v[7], lines_knobs_from(lookup));
            printf("%s %d %d %d %d %d %d %d %s %d %d %d %d %lld %d %d\n", core[(int)F.core], F.guestGrid, (int)F.guestFits, (int)F.sortRuns, F.clWgs, F.clWindow, F.clSmap, (int)F.bigFrame,
                   nfa[(int)F.nfa], F.evalWaves, F.countWaves, F.topnMaxLines, F.streamWaves, F.spinTicks, (int)F.forkBlurSobel, (int)F.lbdRpi);
        } else {
            fprintf(stderr, "lines_form_dump: cannot read '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
