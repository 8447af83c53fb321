// Host-side form plan of the line extractor (lines.hip, lines_nfa.hip): the environment knobs of the line path and everything a call of sslam_lines_extract_batch_dev
// decides from integers -- the launch form of the sequential core, the seed sort, the cluster form's parameters, the NFA stage's form and waves, the side-stream fork of the
// tail, k_lbd's template argument.  Pure functions of integers and no HIP in here, as in match_plan.h: tests/sim/lines_form_dump.cpp compiles this header with a plain host
// compiler and tests/test_lines_form_cpu.py checks both sides of every boundary, every knob's parse and clamp, and the rows of DESIGN.md section 5's table "Which call takes
// which form".  A size rule of the line path lives here and nowhere else; lines_knobs_from is the only place in the line path that names an environment variable.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace sslam {

// -------------------------------------------------------------- size limits (lines.hip pins each to the device code's own constant with a static_assert)
// Up to 64 frames (one to eight per XCD, four workgroups each) of up to 2 048 x 1 024 scaled pixels take the cluster form -- helper waves on several
// compute units, results through global memory, monotonic pixel map (lsd_cluster.h).  Per call, cluster form against the multi-wave form of rounds 2-4 (tools/small_batch_probe.py,
// round 3): 1 frame 5.9 / 7.9 ms, 8: 8.5 / 11.2, 16: 9.0 / 11.9, 24: 9.4 / 12.6, 32: 10.3 / 13.1, 64: 13.5 / 15.7, 96: 21.6 / 15.9
constexpr int LINES_CLUSTER_MAX_FRAMES = 64;
constexpr int LINES_CLUSTER_MAX_SW = 2048, LINES_CLUSTER_MAX_SH = 1024;      // TorusGlobal: the cluster form's pixel map
constexpr int LINES_CLUSTER_LDS_SW = 1024, LINES_CLUSTER_LDS_SH = 512;       // TorusFrame: the main wave's bitmap in LDS; a larger scaled image keeps it in global memory (bigFrame)
constexpr int LINES_CL_MAXWG = 16;                  // lsd_cluster.h CL_MAXWG: workgroups per frame at most
constexpr int LINES_CL_SUB = 4;                     // lsd_cluster.h CL_SUB: seed positions per sub-chunk
constexpr int LINES_SORT_RUNS_MAX_SIDE = 2048;      // lsd_front.h 1 << SORT_XY_BITS: a sorted entry's packing (k_lsd_hist_sort, k_lsd_scatter_runs)
constexpr int LINES_LBD_RPI_MAX_SIDE = 16384;       // lbd.h: the walk's one-conversion rounding (k_lbd<true>) covers source images up to this many pixels a side
constexpr int LINES_NFA_BEHIND_WAVES = 16;          // waves per frame of the k_nfa_stream launch BEHIND the streaming core (what the consumers beside it left)

// -------------------------------------------------------------- the environment knobs
// Read on every call (tests and bench.py set them between calls).
struct LinesKnobs {
    int lone = -1;                      // SSLAM_LSD_FLAVOUR: 1 = "cl" / "lat" (lone waves where the cluster form does not apply), 0 = "thr"; -1 (unset): lone waves below 1 024 frames
    bool cluster = true;                // the cluster form where it applies; false under SSLAM_LSD_CLUSTER=0 or a SSLAM_LSD_FLAVOUR other than "cl"
    int persist = 0;                    // SSLAM_LSD_PERSIST=g: the guest form's grid (0: lines_forms' own)
    int clWgs = 10, clWindow = 640 / LINES_CL_SUB, clSmap = 0;      // the cluster form (lsd_cluster.h): SSLAM_CL_WGS = workgroups per frame (4 waves each); SSLAM_CL_WINDOW = how many
                                        // sub-chunks of seed positions the helpers may run ahead (-1: no helpers at all, the main wave alone), + 1 << 20 under SSLAM_CL_NO_FEEDER (the main
                                        // wave fetches everything itself); SSLAM_CL_SMAP = cell size (log2) of the shared map that steers the helpers' seed choice (-1: none)
    int nfaStreamWaves = 16;            // SSLAM_NFA_STREAM: consumer waves per frame of the NFA stage next to the cluster form (0: the stage behind the core, the round-4 default)
    long long nfaSpinTicks = 5000000;   // SSLAM_NFA_STREAM_TICKS: how long a consumer wave waits without progress before it leaves its blocks to the launch behind the core.  50 ms of the
                                        // 100 MHz clock (ten single-frame cores); 0.2 s in round 5: on a GPU shared with another process the consumers can be resident before the producer,
                                        // and the wait was the spike
    int nfaFused = 1;                   // SSLAM_NFA_FUSED=0 forces the 18 launches, =2 the one-wave form, 1 (unset): by batch size
};
using LinesKnobLookup = const char* (*)(const char*);      // getenv in the library, a table in the dump program
inline LinesKnobs lines_knobs_from(LinesKnobLookup lookup) {
    LinesKnobs K;
    if (const char* e = lookup("SSLAM_LSD_FLAVOUR")) { K.lone = e[0] == 'l' || e[0] == 'c'; K.cluster = e[0] == 'c'; }
    if (const char* e = lookup("SSLAM_LSD_CLUSTER")) K.cluster = K.cluster && atoi(e) != 0;
    if (const char* e = lookup("SSLAM_LSD_PERSIST")) { const int g = atoi(e) & ~7; if (g >= 8) K.persist = g; }
    if (const char* e = lookup("SSLAM_CL_WGS")) K.clWgs = std::max(1, std::min(LINES_CL_MAXWG, atoi(e)));
    if (const char* e = lookup("SSLAM_CL_WINDOW")) K.clWindow = std::max(-1, atoi(e));
    if (lookup("SSLAM_CL_NO_FEEDER") && K.clWindow >= 0) K.clWindow |= 1 << 20;
    if (const char* e = lookup("SSLAM_CL_SMAP")) K.clSmap = atoi(e);
    if (const char* e = lookup("SSLAM_NFA_STREAM")) { const int n = atoi(e); K.nfaStreamWaves = std::max(0, std::min(64, n == 1 ? 16 : n)); }
    if (const char* e = lookup("SSLAM_NFA_STREAM_TICKS")) K.nfaSpinTicks = std::max(0ll, atoll(e));
    if (const char* e = lookup("SSLAM_NFA_FUSED")) K.nfaFused = atoi(e) == 2 ? 2 : atoi(e) == 0 ? 0 : 1;
    return K;
}

// -------------------------------------------------------------- what a call decides
// The launch forms of the sequential core (lsd_regions.h, lsd_cluster.h).  The order is word 0 of sslam_testing_lines_last_forms (include/sslam_testing.h).
enum class CoreForm {
    ClusterStream,      // k_lsd_regions_cl<1>, the NFA stage next to it on the side stream (k_nfa_stream)
    Cluster,            // k_lsd_regions_cl<0>, the NFA stage behind it (SSLAM_NFA_STREAM=0)
    Lone,               // k_lsd_regions<true, 4>, one wave per frame: the shortest chain
    Guest,              // k_lsd_regions<false, 4> on a persistent grid
    PerFrame,           // k_lsd_regions<false, 4>, one workgroup per frame
    SixWave,            // k_lsd_regions<false, 6>, one workgroup per frame
};
// The forms of the NFA stage (lsd_nfa.h): k_nfa_stream beside the streaming core; behind the core the 18 launches, k_nfa_all, or k_nfa_topn
enum class NfaForm { Stream, Launches, All, TopN };

struct LinesForms {
    CoreForm core;
    int guestGrid;              // the guest form's persistent grid -- reported whatever the form (sslam_lines_core_guest_form)
    bool guestFits;             // a co-running branch was announced and the batch is at least two rounds of that grid: Guest unless the knobs choose lone waves
    bool sortRuns;              // the seeds through k_lsd_hist_sort + k_lsd_scatter_runs (k_lsd_hist + k_lsd_scatter otherwise)
    int clWgs, clWindow, clSmap;      // the cluster form: workgroups per frame after the clamp for calls of more than 8 frames, the helpers' window, the shared map's shift
    bool bigFrame;              // the cluster form: the main wave's bitmap in global memory instead of LDS
    NfaForm nfa;
    int evalWaves, countWaves;  // waves per frame walking the NFA evaluations / the rectangle counts of the 18 launches; 1 / 1 for k_nfa_all and k_nfa_topn; Stream: the consumer waves and 0
    int topnMaxLines;           // TopN: the lines that leave a frame (k_nfa_topn's argument)
    int streamWaves;            // Stream: consumer waves per frame beside the core
    long long spinTicks;        // Stream: how long they wait without progress
    bool forkBlurSobel;         // the tail runs k_blur_sobel on the side stream beside the NFA stage (unless the streaming core forked that stream already: it runs there then)
    bool lbdRpi;                // k_lbd's template argument
};

// w x h: the source image, sw x sh: LSD's scaled image (LsdPlan), numCus: the device's compute units, coreEvent: the caller announced a branch running beside the core
// (sslam_lines_set_core_event), topnMaxLines > 0: only that many lines leave a frame (sslam_lines_set_topn_only).
inline LinesForms lines_forms(int w, int h, int sw, int sh, int nframes, int numCus, bool coreEvent, int topnMaxLines, const LinesKnobs& K) {
    LinesForms F{};
    // The guest form (lsd_regions.h): a persistent grid of 20 (16 for smaller batches) workgroups per compute unit.
    // What a compute unit holds beside the core is decided by registers AND by LDS, which gfx950 hands out in granules of 1 280 B (tools/lds_granule_probe.hip).  A core
    // workgroup takes 94 VGPRs and four granules (5 120 B, lsd_regions.h), a k_fast_cells wave -- one per strip of three cells -- 32 VGPRs and eleven granules at 640 x 480 (orb.hip):
    //   20 per compute unit: five core waves on every SIMD (480 of 512 VGPRs), one FAST wave beside them; 100 KB of the 160 KB of LDS for the core, room for four FAST waves;
    //   18 per compute unit: two SIMDs hold five core waves, two hold four and keep 128 registers: ten FAST waves by registers, five by LDS.
    // Before the LDS budgets (core 5 648 B = five granules, FAST 7 290 B = six) 18 left six FAST waves and was the optimum (17 / 19 / 20: 150.8 / 149.4 / 150.0 ms per step against
    // 149.3).  With them it is not: ten FAST waves beside 18 core workgroups slow the core more (92 -> 96 ms) than they speed up FAST (76.4 -> 74.3), 151.4 ms per step; 20 with the
    // FAST waves the registers then leave gives 148.5.  Also measured, no better: k_lsd_regions<false, 6> (80 VGPRs) on the grid at 20 / 22 / 24 per compute unit -- the core
    // drops to 90 / 85 / 79 ms, FAST beside it stays at 76 - 77 ms whatever its slot count, and the step at 148 - 149 ms (profiles/guest_grid_lds_budgets.txt).
    // (Those figures are from k_fast_cells per cell at four granules.  Per strip FAST takes 73.0 ms beside the grid of 20 and the step 146.2 ms; 18 / 19 / 20 per compute unit
    // were run again with it, profiles/fast_strips.txt section 6.)
    F.guestGrid = 20 * numCus;
    if (2 * F.guestGrid > nframes) F.guestGrid = 16 * numCus;
    if (K.persist) F.guestGrid = K.persist;
    // at least two full rounds of the persistent grid: a batch of 1.5 grids (sslam_frontend_batch's chunks of 6 144 frames) would run half of the slots twice and the
    // other half once -- measured on the bench's frame sequence, 24 576 frames through host memory: 61.1 k frames/s in this form against 66.0 k in the other (profiles/r06g_*)
    F.guestFits = coreEvent && nframes >= 1024 && 2 * F.guestGrid <= nframes;

    // Which form the core takes.  Lone waves below 1 024 frames: at most one wave per SIMD is resident, so the instantiation that spills nothing costs no occupancy.  A caller that
    // announced a branch running beside the core (the bench step's point branch waits for that event) gets the guest form.  Otherwise up to 16 frames per compute unit (four
    // waves per SIMD anyway; BASELINE configs[3]: 3 072 frames) take the spill-free instantiation, larger batches the six-wave one.
    if (K.cluster && nframes <= LINES_CLUSTER_MAX_FRAMES && sw <= LINES_CLUSTER_MAX_SW && sh <= LINES_CLUSTER_MAX_SH) F.core = K.nfaStreamWaves ? CoreForm::ClusterStream : CoreForm::Cluster;
    else if (K.lone >= 0 ? K.lone != 0 : nframes < 1024) F.core = CoreForm::Lone;
    else if (F.guestFits) F.core = CoreForm::Guest;
    else F.core = nframes <= 16 * numCus ? CoreForm::PerFrame : CoreForm::SixWave;

    // the tile-sorted runs where a sorted entry's packing fits
    F.sortRuns = sw <= LINES_SORT_RUNS_MAX_SIDE && sh <= LINES_SORT_RUNS_MAX_SIDE;

    if (F.core == CoreForm::ClusterStream || F.core == CoreForm::Cluster) {
        F.clWgs = K.clWgs; F.clWindow = K.clWindow; F.clSmap = K.clSmap;
        if (nframes > 8) F.clWgs = std::max(2, std::min(F.clWgs, 32 / ((nframes + 7) / 8)));      // the frames of an XCD share its 32 compute units
        F.bigFrame = sw > LINES_CLUSTER_LDS_SW || sh > LINES_CLUSTER_LDS_SH;
    }

    // The NFA stage.  Streaming beside the cluster form: the default since round 5 (whole GPU suite with the knob exported, single frames 6.02 / 7.18 -> 5.76 / 6.89 ms
    // p50 / p90, calls of 2 .. 64 frames -8 .. -24 %: profiles/r05a_*).  Behind the core, the whole stage as ONE launch (lsd_nfa.h): one wave per frame when the frames themselves
    // fill the chip (k_nfa_all, calls of >= 2048 frames; k_nfa_topn where only topnMaxLines lines leave a frame: it validates no more candidates than that takes, nfa_topn.h).
    // Below that the 18 launches stay, and they validate everything: a single frame's stage is bound by the work of each wave, not by launch boundaries (kernel durations add up
    // to the stage's 0.6 ms; a one-workgroup form with sixteen waves was measured at 6.42 / 7.70 ms p50 / p90 per frame against 6.25 / 7.40 and removed in round 5).
    // What helped instead: 128 counting and 32 evaluating waves per frame (round 4: 6.25 -> 6.09 ms per frame; 6.09 / 7.16).
    if (F.core == CoreForm::ClusterStream) {
        F.nfa = NfaForm::Stream; F.streamWaves = K.nfaStreamWaves; F.spinTicks = K.nfaSpinTicks;
        F.evalWaves = K.nfaStreamWaves; F.countWaves = 0;
    } else {
        F.evalWaves = nframes >= 1024 ? 1 : nframes >= 64 ? 4 : nframes >= 16 ? 16 : 32;
        F.countWaves = nframes >= 2048 ? 1 : nframes >= 128 ? 8 : nframes >= 16 ? 64 : 128;
        if (K.nfaFused == 2 || (K.nfaFused != 0 && F.countWaves == 1 && F.evalWaves == 1)) {
            F.nfa = topnMaxLines > 0 ? NfaForm::TopN : NfaForm::All;
            F.topnMaxLines = std::max(0, topnMaxLines);
            F.evalWaves = F.countWaves = 1;
        } else F.nfa = NfaForm::Launches;
    }

    // LBD's gradient image needs the source alone and is bandwidth-bound; the NFA stage behind the core is latency-bound (a third of the vector pipes busy): on the side
    // stream the one runs beside the other instead of behind it -- for a caller WITHOUT a branch of its own beside this one (no core event): 187.5 against 190.1 ms per
    // one-stream step.  With the point branch still running there (two-stream step) the pair costs 3.5 ms instead (164.1 against 160.2: k_blur_sobel and k_nfa_all are 56 KB
    // and 54 KB of code, together more than the 64 KB instruction cache two compute units share, beside a third kernel); profiles/r06f_*.  (LBD's blur + Sobel as one more
    // guest under the core, on the side stream, was measured too: its 126-VGPR waves take the slots FAST needs -- 167.7 ms per step against 160.8 with the kernel in the
    // tail; profiles/r06d_*.)
    F.forkBlurSobel = F.core != CoreForm::ClusterStream && nframes >= 1024 && !coreEvent;

    // the walk's conversion form (lbd.h): images of up to 16 384 pixels a side; the previous form beyond
    F.lbdRpi = w <= LINES_LBD_RPI_MAX_SIDE && h <= LINES_LBD_RPI_MAX_SIDE;
    return F;
}

}  // namespace sslam
