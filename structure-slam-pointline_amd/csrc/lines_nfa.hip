// The NFA stage of the line front-end (rect_nfa / rect_improve of LSD_REFINE_ADV: lsd_nfa.h) as a translation unit of its own.
// Why: build.py compiles THIS unit with -mllvm -disable-machine-licm.  The stage is fp64 polynomial code (log-gamma terms, log10, the binomial
// tail) inside loops; with machine LICM the compiler hoists the polynomials' constants out of the loops into registers the fused kernel does
// not have at four waves per SIMD, spills them, and reloads them from scratch one at a time with a wait each -- 208 bytes of scratch and 213
// scratch loads in k_nfa_all.  Without it the constants are rematerialised where they are used: 16 bytes of scratch, 28.4 -> 26.8 ms per
// 12 288 frames.  The sequential core in lines.hip is the other way round (78.9 -> 79.4 ms without the hoisting), hence two units
// (docs/history/DESIGN_rounds_1-4.md 5g).  The kernels are launched from here, in the form lines_forms (lines_form.h) chose; lines.hip calls sslam::launch_nfa_stage.
#include "common.h"
#include "nfa_topn.h"
#include "lines_form.h"
#include <cmath>
#include <cstring>
#include <cfloat>
#include <algorithm>

using namespace sslam;

namespace {

#define SSLAM_NFA_STAGE_ONLY 1
#include "lsd_plan.h"
#include "lsd_nfa.h"

}  // namespace

namespace sslam {

// The stage behind the core in the form lines_forms chose (lines_form.h): the 18 launches with countWaves / evalWaves waves per frame, k_nfa_all, or k_nfa_topn with the
// topnMaxLines lines that leave a frame (sslam_lines_set_topn_only).  Nothing is decided here and no environment is read.
int launch_nfa_stage(sslam_ctx* ctx, hipStream_t st, uint8_t* ws, const void* plan, size_t planBytes, const double* lgam, int nframes, NfaForm form, int evalWaves, int countWaves, int topnMaxLines) {
    if (planBytes != sizeof(LsdPlan)) { set_error("launch_nfa_stage: plan layout mismatch between translation units"); return SSLAM_ERR_INVALID; }
    if (form == NfaForm::Stream || evalWaves < 1 || countWaves < 1) { set_error("launch_nfa_stage: not a form of the stage behind the core"); return SSLAM_ERR_INVALID; }
    LsdPlan P; memcpy(&P, plan, sizeof(P));
    if (form == NfaForm::TopN) {
        sslam::ProfScope _ps(ctx, "k_nfa_all", st);
        hipLaunchKernelGGL(k_nfa_topn<768>, dim3(nframes), dim3(64), 0, st, ws, P, lgam, topnMaxLines);
    } else if (form == NfaForm::All) {
        sslam::ProfScope _ps(ctx, "k_nfa_all", st);
        hipLaunchKernelGGL(k_nfa_all<768>, dim3(nframes), dim3(64), 0, st, ws, P, lgam);
    } else {
        for (int stage = 0; stage <= 4; ++stage) {
            { sslam::ProfScope _ps(ctx, "k_nfa_count", st); hipLaunchKernelGGL(k_nfa_count, dim3(countWaves, nframes), dim3(64), 0, st, ws, P, stage); }
            if (stage == 0) {
                { sslam::ProfScope _ps(ctx, "k_nfa_eval", st); hipLaunchKernelGGL(k_nfa_eval, dim3(evalWaves, nframes), dim3(64), 0, st, ws, P, -1, lgam); }
                { sslam::ProfScope _ps(ctx, "k_nfa_accept", st); hipLaunchKernelGGL(k_nfa_accept, dim3(4, nframes), dim3(256), 0, st, ws, P, -1); }
            }
            { sslam::ProfScope _ps(ctx, "k_nfa_eval", st); hipLaunchKernelGGL(k_nfa_eval, dim3(evalWaves, nframes), dim3(64), 0, st, ws, P, stage, lgam); }
            { sslam::ProfScope _ps(ctx, "k_nfa_accept", st); hipLaunchKernelGGL(k_nfa_accept, dim3(4, nframes), dim3(256), 0, st, ws, P, stage); }
        }
        { sslam::ProfScope _ps(ctx, "k_nfa_finish", st); hipLaunchKernelGGL(k_nfa_finish, dim3(4, nframes), dim3(256), 0, st, ws, P); }
    }
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

// The streaming form (lsd_nfa.h, k_nfa_stream): `waves` single-wave workgroups per frame.  Called twice per extraction: on the second stream next to the core
// (besideCore; spinTicks > 0: the waves wait for the main wave's rectangles), and on the main stream behind both (spinTicks = 0: takes what is unclaimed and returns).
constexpr size_t kNfaStreamLdsPad = 40 * 1024;      // dynamic LDS the kernel does not use, beside the core only: it keeps the consumers off the compute units of the main wave
                                                    // and of the helpers (their workgroups hold > 120 KB of the 160; a consumer that asks for 40 KB does not fit beside them: a
                                                    // wave sharing the main wave's SIMD would slow the one chain the frame waits for)
constexpr int kNfaStreamTake = NFA_STREAM_BLOCK;    // rectangles per claim at most (lsd_nfa.h)
constexpr int kNfaStreamSleep = 1;                  // s_sleep(127) between two polls of a waiting consumer (lsd_nfa.h)
int launch_nfa_stream(sslam_ctx* ctx, hipStream_t st, uint8_t* ws, const void* plan, size_t planBytes, const double* lgam, uint8_t* clArea, size_t clFrameBytes,
                      size_t stageOff, int nframes, int waves, long long spinTicks, bool besideCore) {
    if (planBytes != sizeof(LsdPlan)) { set_error("launch_nfa_stream: plan layout mismatch between translation units"); return SSLAM_ERR_INVALID; }
    if (waves < 1 || nframes < 1 || (stageOff & 7)) { set_error("launch_nfa_stream: invalid arguments"); return SSLAM_ERR_INVALID; }
    LsdPlan P; memcpy(&P, plan, sizeof(P));
    if (besideCore) hipLaunchKernelGGL(k_nfa_stream, dim3(waves, nframes), dim3(64), kNfaStreamLdsPad, st, ws, P, lgam, clArea, clFrameBytes, stageOff, spinTicks, kNfaStreamTake, kNfaStreamSleep);
    else { sslam::ProfScope _ps(ctx, "k_nfa_stream", st); hipLaunchKernelGGL(k_nfa_stream, dim3(waves, nframes), dim3(64), 0, st, ws, P, lgam, clArea, clFrameBytes, stageOff, spinTicks, kNfaStreamTake, kNfaStreamSleep); }
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

}  // namespace sslam
