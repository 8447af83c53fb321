// Host-side plans of the matcher entry points (match.hip) and of the RANSAC units (two_view.hip, sim3.hip, pnp.hip): which kernel a call launches for its sizes, the sizes that follow from
// that choice (LDS bytes, capacities, grid), and how a staged call lays out its scratch arena.  Pure functions of integers and no HIP
// in here: tests/sim/match_plan_dump.cpp compiles this header with a plain host compiler and tests/test_match_plan_cpu.py and the
// tests/test_*_batch_plan_cpu.py check both sides of every boundary.  A size rule lives here and nowhere else; the kernels are chosen by arguments alone (no environment).
#pragma once
#include <algorithm>
#include <cstddef>
#include "../../include/sslam_frontend.h"

namespace sslam {

// -------------------------------------------------------------- scratch arena of one call
// take(bytes) hands out the next 256-aligned offset, size() is the total so far: the one layout rule of every staged entry point
struct ArenaLayout {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
    size_t size() const { return off; }
};

// -------------------------------------------------------------- rows of a frame or slot
// A row index takes ROW_INDEX_BITS bits of a packed reduction key, so a frame or a slot holds fewer than MAX_ROWS rows.  The keys that depend on it:
// fuse_key / fuse_key_idx (match_independent.h), the knn-2 and SearchForInitialization keys (match_knn.h, match_ordered.h), and through them every
// frame that sslam_frame_upload admits.
constexpr int ROW_INDEX_BITS = 19;
constexpr int MAX_ROWS = 1 << ROW_INDEX_BITS;

// -------------------------------------------------------------- knn-2 of a batch (sslam_hamming_knn2_batch_dev)
// k_knn2_mfma packs the train tile into 7 bits of its reduction key: 128 tiles of 32 rows, 4096 rows per frame; beyond that xor + popcount
constexpr int KNN_MFMA_MAX_TILES = 128;
enum class Knn2Form { MatrixCore, Popcount };
struct Knn2Plan {
    Knn2Form form;
    int tilesCap;             // train tiles of 32 rows per frame
    int qblocks;              // MatrixCore: blocks of 64 queries per frame (k_knn2_mfma<2>)
    unsigned grid;            // MatrixCore: workgroups of k_knn2_mfma; Popcount: grid.x of k_knn2_batch (grid.y = nframes)
    size_t expandBytes;       // MatrixCore: the train rows as int8 operands, 256 B per row
};
inline Knn2Plan knn2_batch_plan(int cap, int nframes) {
    Knn2Plan P{};
    P.tilesCap = (cap + 31) / 32;
    if (P.tilesCap <= KNN_MFMA_MAX_TILES) {
        P.form = Knn2Form::MatrixCore;
        P.qblocks = (cap + 63) / 64;
        P.grid = 8u * (unsigned)((nframes + 7) / 8) * (unsigned)P.qblocks;
        P.expandBytes = (size_t)nframes * P.tilesCap * 8 * 1024;
    } else {
        P.form = Knn2Form::Popcount;
        P.grid = (unsigned)((cap + 15) / 16);
    }
    return P;
}

// -------------------------------------------------------------- SearchForInitialization (sslam_orb_search_for_initialization_batch_dev)
//   Speculative  a handful of pairs (the single call of Tracking::MonocularInitialization) whose rows fit one compute unit's LDS: sixteen waves
//                per pair, per candidate 15 words (14 + the stamp) and per F1 keypoint 2 -- k_search_init_spec
//   LdsBatch     one wave per pair with the pair's LEVEL-0 features in LDS: capacity 3/8 of the rows and at least 256 (the level-0 quota of an
//                8-level pyramid is 21.7 % of nfeatures), 16 words each; a pair beyond it takes the global-memory body inside the same launch
//                -- k_search_init_lds
//   Global       rows so long that even that capacity passes 64 KB: one wave per pair on global memory -- k_search_init
enum class SfiForm { Speculative, LdsBatch, Global };
struct SfiPlan {
    SfiForm form;
    size_t ldsBytes;          // dynamic LDS of the launch (0: Global)
    int ccap;                 // LdsBatch: LDS capacity in level-0 features (SfiArgs::ccap); 0 otherwise
};
inline SfiPlan sfi_plan(int cap, int npairs) {
    const size_t ldsSpec = 64 + (size_t)cap * 17 * 4;
    if (npairs <= 8 && ldsSpec <= 150 * 1024) return {SfiForm::Speculative, ldsSpec, 0};
    const int ccap = std::min(cap, std::max(256, cap * 3 / 8));
    const size_t ldsBatch = 64 + (size_t)ccap * 16 * 4;
    if (ldsBatch <= 64 * 1024) return {SfiForm::LdsBatch, ldsBatch, ccap};
    return {SfiForm::Global, 0, 0};
}

// -------------------------------------------------------------- projection-window matchers (search_proj_core)
//   TwoKernel  k_proj_topk (one wave per query over the whole chip) + k_proj_commit (one wave, ordered commit); up to PROJ_MAXN features the
//              commit keeps the frame in LDS (64 bytes per feature: its re-scans then never leave the compute unit), beyond that only
//              occupancy and stamps (8 bytes per feature)
//   OneWave    more than 8192 features: k_search_proj
constexpr int PROJ_MAXN = 2048;
constexpr int PROJ_TWO_KERNEL_MAXN = 8192;
enum class ProjForm { TwoKernel, OneWave };
struct ProjPlan {
    ProjForm form;
    int featsInLds;           // TwoKernel: k_proj_commit copies the frame's features into LDS
    size_t ldsBytes;          // TwoKernel: dynamic LDS of k_proj_commit
    unsigned topkGrid;        // TwoKernel: workgroups of k_proj_topk (four queries each)
};
inline ProjPlan proj_plan(int n, int nq) {
    if (n > PROJ_TWO_KERNEL_MAXN) return {ProjForm::OneWave, 0, 0, 0};
    const int featsInLds = n <= PROJ_MAXN ? 1 : 0;
    return {ProjForm::TwoKernel, featsInLds, (size_t)(featsInLds ? 64 : 8) * (size_t)n + 64, (unsigned)((nq + 3) / 4)};
}

// -------------------------------------------------------------- projection-window matcher of a batch (sslam_search_by_projection_batch_dev)
// B independent frames in cap / qcap strided device buffers.  The form follows the row capacity alone (every frame of a launch runs the same kernel):
//   TwoKernel  cap <= PROJ_TWO_KERNEL_MAXN: k_proj_topk_batch (one wave per (frame, query), grid = topkGrid x frames of the slice) +
//              k_proj_commit_batch (one wave per frame, one frame per workgroup).  The commit keeps occupancy and stamps in LDS, 8 bytes per feature:
//              it is a latency-bound sequential walk, and at 8 KB per 1000-keypoint frame a compute unit holds as many frames as it has wave slots
//              (32), where the single call's 64 bytes per feature would hold two.  Its rare re-scans read the features from global memory.
//   OneWave    beyond that: k_search_proj_batch, one workgroup per frame on global memory.
// The batch runs in slices of frames on the caller's stream so that the per-frame scratch (top-PROJ_K lists 8 * PROJ_K * qcap, eligible counts 4 * qcap,
// and 8 * (cap + qcap) of per-frame state) does not grow with nframes: a slice holds as many frames as fit PROJ_BATCH_SCRATCH_MAX and at most
// PROJ_BATCH_MAX_SLICE (grid.y of the candidate kernel), and at least one.
#ifndef SSLAM_PROJ_K
#define SSLAM_PROJ_K 8
#endif
constexpr int PROJ_K = SSLAM_PROJ_K;      // list length of k_proj_topk: with 4, 3 % of the queries of a dense frame ran out of free entries and paid a re-scan (11-13 k cycles each, two thirds of the commit)
constexpr size_t PROJ_BATCH_SCRATCH_MAX = (size_t)256 << 20;
constexpr int PROJ_BATCH_MAX_SLICE = 32768;
constexpr size_t DYNAMIC_LDS_DEFAULT_MAX = 48 * 1024;      // more dynamic LDS than this has to be allowed per kernel (hipFuncSetAttribute)
// what only libsslam_frontend_testing.so can set (sslam_testing_proj_batch_tuning): a smaller slice, so that a test crosses a slice boundary with a handful
// of frames, and the single call's features-in-LDS commit layout, so that tools/proj_batch_probe.py can time it against the one chosen here
struct ProjBatchTuning { int maxSlice = 0; int featsInLds = 0; };
struct ProjBatchPlan {
    ProjForm form;
    int featsInLds;           // TwoKernel: the commit copies the frame's features into LDS (0 unless the testing library asks for it and cap <= PROJ_MAXN)
    size_t ldsBytes;          // TwoKernel: dynamic LDS of k_proj_commit_batch per workgroup (= per frame)
    int ldsOptIn;             // ldsBytes is more than a launch may ask for without hipFuncSetAttribute
    unsigned topkGrid;        // TwoKernel: grid.x of k_proj_topk_batch (four queries per workgroup), at least 1; grid.y = frames of the slice
    size_t frameBytes;        // scratch of one frame of a slice
    int slice;                // frames per slice: 1 <= slice <= max(nframes, 1)
};
inline size_t proj_batch_frame_bytes(int cap, int qcap, int projK) {
    return 8 * ((size_t)cap + (size_t)qcap) + 8 * (size_t)projK * (size_t)qcap + 4 * (size_t)qcap;
}
inline ProjBatchPlan proj_batch_plan(int cap, int qcap, int nframes, ProjBatchTuning tune = ProjBatchTuning()) {
    ProjBatchPlan P{};
    P.form = cap > PROJ_TWO_KERNEL_MAXN ? ProjForm::OneWave : ProjForm::TwoKernel;
    if (P.form == ProjForm::TwoKernel) {
        P.featsInLds = tune.featsInLds && cap <= PROJ_MAXN ? 1 : 0;
        P.ldsBytes = (size_t)(P.featsInLds ? 64 : 8) * (size_t)cap + 64;
        P.ldsOptIn = P.ldsBytes > DYNAMIC_LDS_DEFAULT_MAX ? 1 : 0;
        P.topkGrid = (unsigned)std::max(1, (qcap + 3) / 4);
    }
    P.frameBytes = proj_batch_frame_bytes(cap, qcap, PROJ_K);
    const size_t fit = PROJ_BATCH_SCRATCH_MAX / std::max<size_t>(P.frameBytes, 1);
    int slice = (int)std::min<size_t>(fit, (size_t)PROJ_BATCH_MAX_SLICE);
    if (tune.maxSlice > 0) slice = std::min(slice, tune.maxSlice);
    P.slice = std::max(1, std::min(slice, nframes));
    return P;
}
// the slices of a batch, in launch order: slice s holds frames [first, first + count)
struct ProjBatchSlice { int first, count; };
inline int proj_batch_slices(const ProjBatchPlan& P, int nframes) { return (nframes + P.slice - 1) / P.slice; }
inline ProjBatchSlice proj_batch_slice(const ProjBatchPlan& P, int nframes, int s) {
    const int first = s * P.slice;
    return {first, std::min(P.slice, nframes - first)};
}
// arena of one slice: per frame of the slice scratch[2 cap + 2 qcap] ints (ProjArgs::scratch), top[projK qcap] keys, cnt[qcap] ints.
// total <= max(PROJ_BATCH_SCRATCH_MAX, one frame's bytes) + 3 * 256, whatever nframes is.
struct ProjBatchArena { size_t scratch, top, cnt, total; };
inline ProjBatchArena proj_batch_arena(int cap, int qcap, int slice, int projK) {
    ArenaLayout L; ProjBatchArena a;
    a.scratch = L.take((size_t)slice * 8 * ((size_t)cap + (size_t)qcap));
    a.top = L.take((size_t)slice * 8 * (size_t)projK * (size_t)qcap);
    a.cnt = L.take((size_t)slice * 4 * (size_t)qcap);
    a.total = L.size();
    return a;
}

// -------------------------------------------------------------- rows in LDS or in global memory (the two SearchByBoW batches, the SearchForTriangulation and Fuse batches)
// One workgroup of BATCH_WAVES waves per unit of work, and one rule for where the rows it scans sit.  The form follows the row capacity alone
// (every workgroup of a launch runs the same kernel):
//   Lds     the scanned side sits in the workgroup's LDS, rowBytes per row of the capacity, while rowBytes * cap is at most BATCH_LDS_MAX (64 KB: two
//           workgroups per compute unit at the bound); more than DYNAMIC_LDS_DEFAULT_MAX needs the per-kernel opt-in
//   Global  beyond that: the same kernel template reads the caller's buffers, with no dynamic LDS
// No scratch: a workgroup's state is in its LDS, its registers and its own output rows.  What a row holds, and the grid, are the matcher's own (below).
constexpr int BATCH_WAVES = 8;
constexpr size_t BATCH_LDS_MAX = 64 * 1024;
enum class BatchForm { Lds, Global };
struct BatchPlan {
    BatchForm form;
    size_t ldsBytes;          // dynamic LDS per workgroup (0: Global)
    int ldsOptIn;             // ldsBytes is more than a launch may ask for without hipFuncSetAttribute
    unsigned threads;         // workgroup size
};
inline BatchPlan batch_plan(int rowBytes, int cap) {
    BatchPlan P{};
    const size_t lds = (size_t)rowBytes * (size_t)cap;
    P.form = lds <= BATCH_LDS_MAX ? BatchForm::Lds : BatchForm::Global;
    P.ldsBytes = P.form == BatchForm::Lds ? lds : 0;
    P.ldsOptIn = P.ldsBytes > DYNAMIC_LDS_DEFAULT_MAX ? 1 : 0;
    P.threads = 64u * BATCH_WAVES;
    return P;
}

// SearchByBoW of a batch (sslam_orb_search_by_bow_batch_dev, k_search_bow_batch): one workgroup per (keyframe slot, frame slot) pair, grid = npairs;
// wave w owns the vocabulary nodes with node % BATCH_WAVES == w.  The FRAME side's capacity decides; a row is 32 bytes of descriptor, the node id and
// the live assignment (three pairs per compute unit at 1000 rows).  The Global form keeps the live assignment in d_assigned.
// SearchByBoW between keyframes of a batch (sslam_orb_search_by_bow_keyframes_batch_dev, k_search_bow_kf_batch) stages the same row and reuses the
// constant: one workgroup per pair of keyframe slots, grid = npairs, KEYFRAME 2 staged; a row is 32 bytes of descriptor, the node id and one state
// word (invalid, free, or the owning keyframe-1 row).  The Global form keeps the state words in the pair's d_matches21 rows.
constexpr int BOW_BATCH_ROW_BYTES = 40;

// SearchForTriangulation of a batch (sslam_orb_search_for_triangulation_batch_dev, k_tri_search_batch): one workgroup per pair of keyframe slots,
// grid = npairs; the waves share the keyframe-1 rows in turns of 64 (the queries do not interact).  KEYFRAME 2 is staged; a row is 32 bytes of
// descriptor, the node id, x, y and octave | free | stereo in one word (three pairs per compute unit at 1000 rows).
constexpr int TRI_BATCH_ROW_BYTES = 48;

// Fuse / SearchBySim3 candidate search of a batch (sslam_fuse_search_batch_dev, k_fuse_search_batch): one workgroup per (job, chunk of FUSE_BATCH_CHUNK
// queries); the grid is flattened to one dimension, job-major: workgroup g serves chunk g % chunks of job g / chunks, njobs * chunks in all (64 bits:
// the entry point refuses 2^31 and more).  The keyframe's GEOMETRY is staged, as four arrays of cap words (x, y, uright, octave resp. pt_x, pt_y,
// angle, octave): cap <= 4096 in LDS, the opt-in above 3072; at 1000 rows the 32 wave slots admit four workgroups and the LDS is no limit.
// Descriptors are never staged: a window admits a handful of rows, and only those rows' descriptors are read.
constexpr int FUSE_BATCH_ROW_BYTES = 16;
constexpr int FUSE_BATCH_CHUNK = 256;
// workgroups per job: ceil(qcap / FUSE_BATCH_CHUNK), and 1 where qcap is 0 -- chunk 0 of a job is the one that reports a skipped job, so it exists for every job
inline unsigned fuse_batch_chunks(int qcap) { return (unsigned)std::max(1, (int)(((long long)qcap + FUSE_BATCH_CHUNK - 1) / FUSE_BATCH_CHUNK)); }
inline unsigned long long fuse_batch_grid(int njobs, int qcap) { return (unsigned long long)njobs * fuse_batch_chunks(qcap); }

// -------------------------------------------------------------- ComputeDistinctiveDescriptors of a batch (sslam_distinctive_descriptors_batch_dev)
// A set's kernel follows its ENTRY count, d_ptr[s + 1] - d_ptr[s], which only the device reads: every call enqueues both kernels.
//   Small    0 .. 8 entries: eight consecutive sets share one wave of k_distinct_batch, each in its own group of eight lanes, lane = entry, rows in
//            registers, no LDS
//   Medium   9 .. 64 entries: the wave that owns the set's group of eight runs it alone afterwards, lane = entry: the admissible rows in 2 KB of the
//            wave's LDS, every pair distance once as 16 bits of an 8 KB matrix (two per word, column = lane) that the nine bisection steps count on
//   Large    65 .. 1024 entries: k_distinct_large, one wave per workgroup with the rows (32 KB) and their entry positions (2 KB) in LDS; a wave looks at
//            64 sets at a time (lane = set) and runs the large ones among them, so the reservation never sets the occupancy of the first kernel
//   Refused  a malformed range or more than 1024 entries: -2, written by k_distinct_batch
// k_distinct_batch: DISTINCT_BATCH_WAVES waves per workgroup, wave w of the grid takes the units (runs of eight sets) w, w + waves of the grid, ..;
// the grid is capped at DISTINCT_BATCH_GRID_MAX workgroups (8 per compute unit: the 40 KB of a workgroup admit 4, so two rounds).
// k_distinct_large: chunk c of 64 sets goes to workgroup c % grid, the grid is capped at DISTINCT_LARGE_GRID_MAX.
constexpr int DISTINCT_SMALL_MAX = 8;
constexpr int DISTINCT_MEDIUM_MAX = 64;
constexpr int DISTINCT_LARGE_MAX = 1024;          // = DISTINCT_MAXN of the single call
constexpr int DISTINCT_SETS_PER_WAVE = 8;
constexpr int DISTINCT_BATCH_WAVES = 4;
constexpr unsigned DISTINCT_BATCH_GRID_MAX = 2048;
constexpr size_t DISTINCT_MEDIUM_ROW_BYTES = 32 * (size_t)DISTINCT_MEDIUM_MAX;                                   // 2 KB per wave
constexpr size_t DISTINCT_MEDIUM_DIST_BYTES = 2 * (size_t)DISTINCT_MEDIUM_MAX * (size_t)DISTINCT_MEDIUM_MAX;    // 8 KB per wave
constexpr int DISTINCT_LARGE_CHUNK = 64;
constexpr unsigned DISTINCT_LARGE_GRID_MAX = 1024;
constexpr size_t DISTINCT_LARGE_LDS_BYTES = (32 + 2) * (size_t)DISTINCT_LARGE_MAX;
enum class DistinctClass { Small, Medium, Large, Refused };
constexpr DistinctClass distinct_class(long long entries) {
    return entries < 0 ? DistinctClass::Refused : entries <= DISTINCT_SMALL_MAX ? DistinctClass::Small : entries <= DISTINCT_MEDIUM_MAX ? DistinctClass::Medium :
           entries <= DISTINCT_LARGE_MAX ? DistinctClass::Large : DistinctClass::Refused;
}
struct DistinctBatchPlan {
    int launches;             // 0 without a set, else 2
    unsigned threads;         // k_distinct_batch: workgroup size
    unsigned grid;            // k_distinct_batch: workgroups, at most DISTINCT_BATCH_GRID_MAX (the waves stride over the units)
    size_t ldsBytes;          // k_distinct_batch: static LDS per workgroup
    unsigned largeThreads;    // k_distinct_large: workgroup size (one wave)
    unsigned largeGrid;       // k_distinct_large: workgroups, at most DISTINCT_LARGE_GRID_MAX (they stride over the chunks)
    size_t largeLdsBytes;     // k_distinct_large: static LDS per workgroup
};
inline DistinctBatchPlan distinct_batch_plan(int nsets) {
    DistinctBatchPlan P{};
    P.threads = 64u * DISTINCT_BATCH_WAVES;
    P.ldsBytes = DISTINCT_BATCH_WAVES * (DISTINCT_MEDIUM_ROW_BYTES + DISTINCT_MEDIUM_DIST_BYTES);
    P.largeThreads = 64;
    P.largeLdsBytes = DISTINCT_LARGE_LDS_BYTES;
    if (nsets <= 0) return P;
    const long long perGroup = (long long)DISTINCT_SETS_PER_WAVE * DISTINCT_BATCH_WAVES;
    P.launches = 2;
    P.grid = (unsigned)std::min<long long>(((long long)nsets + perGroup - 1) / perGroup, DISTINCT_BATCH_GRID_MAX);
    P.largeGrid = (unsigned)std::min<long long>(((long long)nsets + DISTINCT_LARGE_CHUNK - 1) / DISTINCT_LARGE_CHUNK, DISTINCT_LARGE_GRID_MAX);
    return P;
}

// -------------------------------------------------------------- RANSAC over the rows of a pair (sslam_two_view_ransac*, two_view.hip; sslam_sim3_ransac*, sim3.hip; sslam_pnp_ransac*, pnp.hip)
// One wave per pair with the pair's compacted rows in dynamic LDS, rowBytes each, and fixedBytes behind them that do not grow with the capacity.  The capacity bound, beyond
// which an entry point refuses before it launches, is whole steps of RANSAC_CAP_STEP rows: what one workgroup can have of the compute unit's LDS beside RANSAC_STATIC_LDS of
// the kernel's static words, and no more than rowsMax bytes of rows.
//   two-view  a row is (u1, v1, u2, v2); behind the rows the Jacobi workspace of the 64 lanes, TWO_VIEW_WS_DOUBLES doubles each (two_view_math.h: the upper triangle of a
//             symmetric 9 x 9 and its eigenvectors); the rows stay within the 64 KB of the batch matchers' rows (BATCH_LDS_MAX): the workspace stays the larger part
//   Sim3      a row is X1, X2, P1im1, P2im2, maxErr1, maxErr2 (sim3_math.h: s3::Row); nothing behind the rows, and they may take the whole LDS
//   PnP       a row is Xw, pt, maxErr (pnp_math.h: pnp::Row); behind the rows the EPnP workspace of the 64 lanes, PNP_WS_DOUBLES doubles each (the upper triangle of the
//             symmetric 12 x 12 and its eigenvectors), and one bit per row of the bound for Refine's set; the rows may take the rest of the LDS
constexpr size_t LDS_PER_CU = 160 * 1024, RANSAC_STATIC_LDS = 256;
constexpr int RANSAC_CAP_STEP = 1024, RANSAC_LANES = 64, TWO_VIEW_ROW_BYTES = 16, TWO_VIEW_WS_DOUBLES = 45 + 81, SIM3_ROW_BYTES = 48;
constexpr size_t TWO_VIEW_WS_BYTES = sizeof(double) * TWO_VIEW_WS_DOUBLES * RANSAC_LANES;
constexpr int ransac_max_cap(size_t rowBytes, size_t fixedBytes, size_t rowsMax) {
    return (int)(std::min(LDS_PER_CU - RANSAC_STATIC_LDS - fixedBytes, rowsMax) / rowBytes / RANSAC_CAP_STEP) * RANSAC_CAP_STEP;
}
constexpr int TWO_VIEW_MAX_CAP = ransac_max_cap(TWO_VIEW_ROW_BYTES, TWO_VIEW_WS_BYTES, BATCH_LDS_MAX), SIM3_MAX_CAP = ransac_max_cap(SIM3_ROW_BYTES, 0, LDS_PER_CU);
static_assert(TWO_VIEW_MAX_CAP == 4096 && SIM3_MAX_CAP == 3072, "the capacities include/sslam_frontend.h promises");
struct RansacPlan {
    int rowBytes; size_t ldsBytes; int ldsOptIn;      // dynamic LDS per workgroup, the rows of the capacity and the fixed part, and whether it needs the per-kernel opt-in
    unsigned threads; int maxCap;                     // one wave; the capacity bound (ldsBytes means nothing beyond it)
};
inline RansacPlan ransac_plan(int rowBytes, size_t fixedBytes, int maxCap, int cap) {
    const size_t lds = (size_t)rowBytes * (size_t)cap + fixedBytes;
    return {rowBytes, lds, lds > DYNAMIC_LDS_DEFAULT_MAX ? 1 : 0, RANSAC_LANES, maxCap};
}
inline RansacPlan two_view_plan(int cap) { return ransac_plan(TWO_VIEW_ROW_BYTES, TWO_VIEW_WS_BYTES, TWO_VIEW_MAX_CAP, cap); }
inline RansacPlan sim3_plan(int cap) { return ransac_plan(SIM3_ROW_BYTES, 0, SIM3_MAX_CAP, cap); }
constexpr int PNP_ROW_BYTES = 24, PNP_WS_DOUBLES = 78 + 144, PNP_MASK_BYTES = 256;
constexpr size_t PNP_WS_BYTES = sizeof(double) * PNP_WS_DOUBLES * RANSAC_LANES, PNP_FIXED_BYTES = PNP_WS_BYTES + PNP_MASK_BYTES;
constexpr int PNP_MAX_CAP = ransac_max_cap(PNP_ROW_BYTES, PNP_FIXED_BYTES, LDS_PER_CU);
static_assert(PNP_MAX_CAP == 2048 && PNP_MAX_CAP <= 8 * PNP_MASK_BYTES, "the capacity include/sslam_frontend.h promises (the c2 configuration extracts 2000 keypoints); one mask bit per row");
inline RansacPlan pnp_plan(int cap) { return ransac_plan(PNP_ROW_BYTES, PNP_FIXED_BYTES, PNP_MAX_CAP, cap); }

// -------------------------------------------------------------- ReconstructH / ReconstructF over the rows of a pair (sslam_two_view_reconstruct*, reconstruct.hip)
// One workgroup of RECON_WAVES waves per pair; all lanes walk the match rows of one hypothesis after the other.  Dynamic LDS: the Jacobi workspace of the 4 x 4 solves,
// RECON_WS_DOUBLES doubles per lane (reconstruct_math.h: WS4_DOUBLES), lane-interleaved; per line row of the capacity the two errors (doubles); per match row of the
// capacity (u1, v1, u2, v2), the key of its cosine and the inlier byte.  The line capacity is bounded by RECON_MAX_LCAP; the row capacity is what the compute unit's LDS
// leaves beside that, the workspace and RECON_STATIC_LDS of static words, in whole steps of RANSAC_CAP_STEP: no less than the RANSAC call's own bound, so every batch it takes
// goes on.  Two waves: a pair at the RANSAC call's bound then takes 110 KB, one at half of it 68 KB, so that two such pairs share a compute unit.
constexpr int RECON_WAVES = 2, RECON_THREADS = 64 * RECON_WAVES, RECON_WS_DOUBLES = 10 + 16, RECON_ROW_BYTES = 16 + 4 + 1, RECON_LINE_ROW_BYTES = 16, RECON_MAX_LCAP = 1024;
constexpr size_t RECON_WS_BYTES = sizeof(double) * RECON_WS_DOUBLES * RECON_THREADS, RECON_STATIC_LDS = 2048;
constexpr int RECON_MAX_CAP = (int)((LDS_PER_CU - RECON_STATIC_LDS - RECON_WS_BYTES - (size_t)RECON_LINE_ROW_BYTES * RECON_MAX_LCAP) / RECON_ROW_BYTES / RANSAC_CAP_STEP) * RANSAC_CAP_STEP;
static_assert(RECON_MAX_CAP == 5120 && RECON_MAX_CAP >= TWO_VIEW_MAX_CAP, "the capacity include/sslam_frontend.h promises; no less than the RANSAC call's");
struct ReconstructPlan {
    int rowBytes, lineRowBytes;
    size_t wsOff, lineOff, rowOff, keyOff, flagOff, ldsBytes;      // offsets into the dynamic LDS and its size
    int ldsOptIn; unsigned threads; int maxCap, maxLcap;            // ldsBytes means nothing beyond the bounds
};
inline ReconstructPlan reconstruct_plan(int cap, int lcap) {
    ReconstructPlan P{};
    P.rowBytes = RECON_ROW_BYTES; P.lineRowBytes = RECON_LINE_ROW_BYTES; P.threads = RECON_THREADS; P.maxCap = RECON_MAX_CAP; P.maxLcap = RECON_MAX_LCAP;
    const size_t c = (size_t)std::max(cap, 0), l = (size_t)std::max(lcap, 0);
    P.wsOff = 0;
    P.lineOff = RECON_WS_BYTES;
    P.rowOff = P.lineOff + RECON_LINE_ROW_BYTES * l;
    P.keyOff = P.rowOff + 16 * c;
    P.flagOff = P.keyOff + 4 * c;
    P.ldsBytes = (P.flagOff + c + 15) & ~(size_t)15;
    P.ldsOptIn = P.ldsBytes > DYNAMIC_LDS_DEFAULT_MAX ? 1 : 0;
    return P;
}
static_assert(RECON_WS_BYTES + (size_t)RECON_LINE_ROW_BYTES * RECON_MAX_LCAP + (size_t)RECON_ROW_BYTES * RECON_MAX_CAP + 16 + RECON_STATIC_LDS <= LDS_PER_CU, "the bounds fit the compute unit");

// arena of search_proj_core.  occ | q | qdesc go up in ONE copy (occ .. assigned), assigned | count come back in one (assigned .. count + 4);
// only that head (.. count + 256) has a pinned mirror.  projK = list length of k_proj_topk (PROJ_K).
struct ProjArena {
    size_t occ, q, qdesc, assigned, count, scratch, top, cnt, total;
    size_t stats() const { return count + 64; }          // SSLAM_PROJ_STATS: counters behind the match count, inside its 256 bytes
    size_t pinnedBytes() const { return count + 256; }
};
inline ProjArena proj_arena(int n, int nq, int projK) {
    ArenaLayout L; ProjArena a;
    a.occ = L.take((size_t)n);
    a.q = L.take(sizeof(sslam_proj_query) * (size_t)nq);
    a.qdesc = L.take(32 * (size_t)nq);
    a.assigned = L.take(4 * (size_t)n);
    a.count = L.take(256);
    a.scratch = L.take(4 * (2 * (size_t)n + 2 * (size_t)nq));      // ProjArgs::scratch: occ[n], key[n], qbin[nq], qidx[nq]
    a.top = L.take(8 * (size_t)projK * (size_t)nq);
    a.cnt = L.take(4 * (size_t)nq);
    a.total = L.size();
    return a;
}

// arena of search_by_bow_core: the nine inputs, then assigned | count | qbin | validF; everything goes up in one copy, assigned .. count + 4 comes back
struct BowArena {
    size_t in[9];             // kpKF, dKF, validKF, kpF, dF, ptrKF, ptrF, idxKF, idxF
    size_t assigned, count, qbin, validF, total;
};
inline BowArena bow_arena(int nkf, int nf, int nnodes, int nk, int nfi) {
    const size_t ks = sizeof(sslam_keypoint);
    ArenaLayout L; BowArena a;
    const size_t len[9] = {ks * nkf, 32 * (size_t)nkf, (size_t)nkf, ks * nf, 32 * (size_t)nf, 4 * (size_t)(nnodes + 1), 4 * (size_t)(nnodes + 1),
                           4 * (size_t)std::max(nk, 1), 4 * (size_t)std::max(nfi, 1)};
    for (int i = 0; i < 9; ++i) a.in[i] = L.take(len[i]);
    a.assigned = L.take(4 * (size_t)nf);
    a.count = L.take(256);
    a.qbin = L.take(4 * (size_t)nf);
    a.validF = L.take((size_t)nf);
    a.total = L.size();
    return a;
}

}  // namespace sslam
