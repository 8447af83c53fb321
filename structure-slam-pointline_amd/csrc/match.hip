// Hamming matchers for MI355X (gfx950): brute-force knn-2 (BFMatcher semantics),
// dense distance matrix, ORBmatcher::SearchForInitialization and the LSDmatcher
// knn2+MAD gates — device side of reference src/ORBmatcher.cc:408-523,1604-1666,
// src/LSDmatcher.cpp:143-183,257-284,364-415, src/Frame.cc:133-148,190-215,368-472.
//
// The path is integer/bitwise: v_bcnt popcounts on 8x u32 XORs, wave-wide min
// reductions with the tie-break order carried in the key; the knn-2 of a batch alone runs on the matrix cores (match_knn.h).
// Which kernel a call launches depends on its sizes alone: the rules are the pure host functions of match_plan.h, and an entry
// point reads as validate, lock, lay out, stage, switch on the plan's form with one launch per case, copy back.  The batches that keep
// their rows in LDS or in global memory share one plan (match_plan.h: batch_plan) and one launch path (launch_batch); the alignment and
// size rules of device-resident batches are the named checks of match_check.h.  The stream choice (pick), the dynamic-LDS opt-in (allow_dynamic_lds) and the
// field-by-field staging of a single call through its arena (Staging) are common.h's, shared with two_view.hip and sim3.hip.
#include "common.h"
#include "match_plan.h"
#include "match_check.h"
#include <algorithm>

using namespace sslam;

namespace {

#include "match_knn.h"
#include "match_rot.h"
#include "match_ordered.h"
#include "match_independent.h"
#include "match_distinct.h"

}  // namespace

// =============================================================== host side
// the one launch of a batch_plan (match_plan.h): the kernel's <true> instantiation with the rows in dynamic LDS, or <false> on global memory
template <class Args>
static int launch_batch(sslam_ctx* ctx, const char* name, void (*lds)(Args), void (*global)(Args), const BatchPlan& P, unsigned grid, hipStream_t st, const Args& A) {
    const bool inLds = P.form == BatchForm::Lds;
    int rc;
    if (inLds && (rc = allow_dynamic_lds((const void*)lds, P.ldsBytes))) return rc;
    sslam::ProfScope _ps(ctx, name, st);
    hipLaunchKernelGGL(inLds ? lds : global, dim3(grid), dim3(P.threads), P.ldsBytes, st, A);
    return SSLAM_OK;
}

extern "C" int sslam_hamming_knn2_dev(sslam_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx, int32_t* d_dist, void* stream) {
    if (!ctx || nq < 0 || nt < 0 || (nq > 0 && (!d_q || !d_idx || !d_dist))) { set_error("sslam_hamming_knn2_dev: invalid arguments"); return SSLAM_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (nq == 0) return SSLAM_OK;
    SSLAM_HIP(hipSetDevice(ctx->device));
    { sslam::ProfScope _ps(ctx, "k_knn2", pick(ctx, stream)); hipLaunchKernelGGL(k_knn2, dim3((nq + 3) / 4), dim3(256), 0, pick(ctx, stream), d_q, nq, d_t, nt, d_idx, d_dist); }
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

extern "C" int sslam_hamming_knn2_batch_dev(sslam_ctx* ctx, const uint8_t* d_q, const int32_t* d_nq, const uint8_t* d_t, const int32_t* d_nt,
                                            int cap, int nframes, int32_t* d_idx, int32_t* d_dist, void* stream) {
    if (!ctx || !d_q || !d_nq || !d_t || !d_nt || !d_idx || !d_dist || cap <= 0 || nframes <= 0) { set_error("sslam_hamming_knn2_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    const Knn2Plan P = knn2_batch_plan(cap, nframes);
    switch (P.form) {
    case Knn2Form::MatrixCore: {       // match_knn.h: train rows expanded to +-64 bytes in operand order, then 64 queries per wave
        int rc;
        // ONE expand buffer per context (256 B per train row: 3 GB at 12 288 frames of 1 000 rows, never shrunk; sslam_frontend_batch counts it in its chunk estimate).
        // k_knn2_expand writes it and k_knn2_mfma reads it on the caller's stream after this call has returned (StreamOrderedBuf, common.h).
        if ((rc = ctx->knnExpand.acquire(st, P.expandBytes))) return rc;
        { sslam::ProfScope _ps(ctx, "k_knn2_expand", st); hipLaunchKernelGGL(k_knn2_expand, dim3(P.tilesCap, nframes), dim3(64), 0, st, d_t, d_nt, cap, P.tilesCap, ctx->knnExpand.as<uint8_t>()); }
        { sslam::ProfScope _ps(ctx, "k_knn2_batch", st);
          hipLaunchKernelGGL(k_knn2_mfma<2>, dim3(P.grid), dim3(64), 0, st, d_q, d_nq, ctx->knnExpand.as<uint8_t>(), d_nt, cap, P.tilesCap, P.qblocks, nframes, d_idx, d_dist); }
        if ((rc = ctx->knnExpand.mark(st))) return rc;
        break;
    }
    case Knn2Form::Popcount: {         // more than 4096 rows per frame: xor + popcount
        sslam::ProfScope _ps(ctx, "k_knn2_batch", st);
        hipLaunchKernelGGL(k_knn2_batch, dim3(P.grid, nframes), dim3(256), 0, st, d_q, d_nq, d_t, d_nt, cap, d_idx, d_dist);
        break;
    }
    }
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

extern "C" int sslam_hamming_knn2(sslam_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, int32_t* dist) {
    if (!ctx || nq < 0 || nt < 0 || (nq > 0 && (!q || !idx || !dist)) || (nt > 0 && !t)) { set_error("sslam_hamming_knn2: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (nq == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->scratch[SCR_KNN_Q].ensure((size_t)nq * 32))) return rc;
    if ((rc = ctx->scratch[SCR_KNN_T].ensure((size_t)std::max(nt, 1) * 32))) return rc;
    if ((rc = ctx->scratch[SCR_KNN_OUT].ensure((size_t)nq * 16))) return rc;
    hipStream_t st = ctx->stream;
    SSLAM_HIP(hipMemcpyAsync(ctx->scratch[SCR_KNN_Q].p, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    if (nt) SSLAM_HIP(hipMemcpyAsync(ctx->scratch[SCR_KNN_T].p, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
    int* di = ctx->scratch[SCR_KNN_OUT].as<int>();
    if ((rc = sslam_hamming_knn2_dev(ctx, ctx->scratch[SCR_KNN_Q].as<uint8_t>(), nq, ctx->scratch[SCR_KNN_T].as<uint8_t>(), nt, di, di + (size_t)nq * 2, st))) return rc;
    SSLAM_HIP(hipMemcpyAsync(idx, di, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipMemcpyAsync(dist, di + (size_t)nq * 2, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipStreamSynchronize(st));
    return SSLAM_OK;
}

extern "C" int sslam_hamming_matrix(sslam_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* D) {
    if (!ctx || nq < 0 || nt < 0 || ((nq > 0 && nt > 0) && (!q || !t || !D))) { set_error("sslam_hamming_matrix: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (nq == 0 || nt == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->scratch[SCR_KNN_Q].ensure((size_t)nq * 32))) return rc;
    if ((rc = ctx->scratch[SCR_KNN_T].ensure((size_t)nt * 32))) return rc;
    if ((rc = ctx->scratch[SCR_KNN_OUT].ensure((size_t)nq * nt * 2))) return rc;
    hipStream_t st = ctx->stream;
    SSLAM_HIP(hipMemcpyAsync(ctx->scratch[SCR_KNN_Q].p, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    SSLAM_HIP(hipMemcpyAsync(ctx->scratch[SCR_KNN_T].p, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
    { sslam::ProfScope _ps(ctx, "k_hamming_matrix", st); hipLaunchKernelGGL(k_hamming_matrix, dim3((nt + 255) / 256, nq), dim3(256), 0, st, ctx->scratch[SCR_KNN_Q].as<uint8_t>(), nq,
                       ctx->scratch[SCR_KNN_T].as<uint8_t>(), nt, ctx->scratch[SCR_KNN_OUT].as<unsigned short>()); }
    SSLAM_HIP(hipGetLastError());
    SSLAM_HIP(hipMemcpyAsync(D, ctx->scratch[SCR_KNN_OUT].p, (size_t)nq * nt * 2, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipStreamSynchronize(st));
    return SSLAM_OK;
}

extern "C" int sslam_orb_search_for_initialization_batch_dev(sslam_ctx* ctx,
        const sslam_keypoint* d_kp1, const uint8_t* d_desc1, const int32_t* d_n1,
        const sslam_keypoint* d_kp2, const uint8_t* d_desc2, const int32_t* d_n2,
        int cap, int npairs, float* d_prev, int32_t* d_m12, int32_t* d_nm,
        int window, float nnratio, int checkOri, const float bounds[4], void* stream) {
    if (!ctx || !d_kp1 || !d_desc1 || !d_kp2 || !d_desc2 || !d_n1 || !d_n2 || !d_prev || !d_m12 || !d_nm || cap <= 0 || !rows_in_range(cap) || npairs <= 0 || !bounds) {
        set_error("sslam_orb_search_for_initialization_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);      // scratch buffers and profile records are shared state
    SSLAM_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->scratch[SCR_SFI_STATE].ensure(sizeof(int) * 5 * (size_t)cap * npairs))) return rc;
    SfiArgs A;
    A.kp1 = d_kp1; A.d1 = d_desc1; A.n1 = d_n1; A.kp2 = d_kp2; A.d2 = d_desc2; A.n2 = d_n2;
    A.cap = cap; A.n1s = 0; A.n2s = 0; A.prevMatched = d_prev; A.m12 = d_m12; A.nmatches = d_nm;
    A.scratch = ctx->scratch[SCR_SFI_STATE].as<int>(); A.window = window; A.nnratio = nnratio; A.checkOri = checkOri;
    A.minX = bounds[0]; A.maxX = bounds[1]; A.minY = bounds[2]; A.maxY = bounds[3];
    const SfiPlan P = sfi_plan(cap, npairs);      // match_plan.h: the kernel by size
    A.ccap = P.ccap;
    hipStream_t st = pick(ctx, stream);
    switch (P.form) {
    case SfiForm::Speculative: {      // a handful of pairs (the single call of Tracking::MonocularInitialization): sixteen waves per pair
        if ((rc = allow_dynamic_lds((const void*)k_search_init_spec, P.ldsBytes))) return rc;
        sslam::ProfScope _ps(ctx, "k_search_init", st);
        hipLaunchKernelGGL(k_search_init_spec, dim3(npairs), dim3(SFI_WAVES * 64), P.ldsBytes, st, A);
        break;
    }
    case SfiForm::LdsBatch: {         // one wave per pair, the pair's level-0 features in LDS
        if ((rc = allow_dynamic_lds((const void*)k_search_init_lds, P.ldsBytes))) return rc;
        sslam::ProfScope _ps(ctx, "k_search_init", st);
        hipLaunchKernelGGL(k_search_init_lds, dim3(npairs), dim3(64), P.ldsBytes, st, A);
        break;
    }
    case SfiForm::Global: {           // one wave per pair on global memory
        sslam::ProfScope _ps(ctx, "k_search_init", st);
        hipLaunchKernelGGL(k_search_init, dim3(npairs), dim3(64), 0, st, A);
        break;
    }
    }
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

extern "C" int sslam_orb_search_for_initialization(sslam_ctx* ctx,
        const sslam_keypoint* kp1, const uint8_t* desc1, int n1, const sslam_keypoint* kp2, const uint8_t* desc2, int n2,
        float* prev_matched, int32_t* matches12, int window, float nnratio, int checkOri, const float bounds[4], int* nmatches_out) {
    if (!ctx || n1 < 0 || n2 < 0 || !nmatches_out || !bounds || (n1 > 0 && (!kp1 || !desc1 || !prev_matched || !matches12)) || (n2 > 0 && (!kp2 || !desc2))) {
        set_error("sslam_orb_search_for_initialization: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    *nmatches_out = 0;
    if (n1 == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    const int cap = std::max(std::max(n1, n2), 1);
    if (cap >= MAX_ROWS) { set_error("too many keypoints"); return SSLAM_ERR_UNSUPPORTED; }
    hipStream_t st = ctx->stream;
    const size_t kb = sizeof(sslam_keypoint) * (size_t)cap, db = 32 * (size_t)cap;
    int rc;
    // device layout: kp1 | kp2 | d1 | d2 | prev | n1,n2,nm (16 B) | m12 -- everything that goes in is one contiguous range, so is everything
    // that comes back (prev .. m12): ONE staged H2D and ONE D2H through pinned memory instead of six + three pageable copies (a pageable
    // hipMemcpyAsync costs 10-20 us of host time each, more than the kernel of a single call)
    const size_t oPrev = 2 * kb + 2 * db, oN = oPrev + 8 * (size_t)cap, oM = oN + 16, total = oM + 4 * (size_t)cap + 64;
    if ((rc = ctx->scratch[SCR_SFI_STAGE].ensure(total))) return rc;
    if ((rc = ctx->pinned[PIN_SFI].ensure(total))) return rc;
    uint8_t* base = ctx->scratch[SCR_SFI_STAGE].as<uint8_t>();
    uint8_t* H = ctx->pinned[PIN_SFI].as<uint8_t>();
    sslam_keypoint* dk1 = (sslam_keypoint*)base; sslam_keypoint* dk2 = (sslam_keypoint*)(base + kb);
    uint8_t* dd1 = base + 2 * kb; uint8_t* dd2 = dd1 + db;
    float* dpm = (float*)(base + oPrev); int* dn = (int*)(base + oN); int* dm12 = (int*)(base + oM);
    memcpy(H, kp1, sizeof(sslam_keypoint) * (size_t)n1);
    if (n2) memcpy(H + kb, kp2, sizeof(sslam_keypoint) * (size_t)n2);
    memcpy(H + 2 * kb, desc1, 32 * (size_t)n1);
    if (n2) memcpy(H + 2 * kb + db, desc2, 32 * (size_t)n2);
    memcpy(H + oPrev, prev_matched, 8 * (size_t)n1);
    int hn[4] = {n1, n2, 0, 0};
    memcpy(H + oN, hn, sizeof(hn));
    SSLAM_HIP(hipMemcpyAsync(base, H, oM, hipMemcpyHostToDevice, st));
    if ((rc = sslam_orb_search_for_initialization_batch_dev(ctx, dk1, dd1, dn, dk2, dd2, dn + 1, cap, 1, dpm, dm12, dn + 2, window, nnratio, checkOri, bounds, st))) return rc;
    SSLAM_HIP(hipMemcpyAsync(H + oPrev, base + oPrev, oM + 4 * (size_t)n1 - oPrev, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipStreamSynchronize(st));
    memcpy(prev_matched, H + oPrev, 8 * (size_t)n1);
    memcpy(matches12, H + oM, 4 * (size_t)n1);
    memcpy(hn, H + oN, sizeof(hn));
    *nmatches_out = hn[2];
    return SSLAM_OK;
}

extern "C" int sslam_line_match_batch_dev(sslam_ctx* ctx, const uint8_t* d_l1, const int32_t* d_n1, const uint8_t* d_l2, const int32_t* d_n2,
                                          int cap, int npf, double gate_scale, int ratio_mode, int32_t* d_pairs, int32_t* d_npairs, void* stream) {
    if (!ctx || !d_l1 || !d_l2 || !d_n1 || !d_n2 || !d_pairs || !d_npairs || cap <= 0 || npf <= 0) { set_error("sslam_line_match_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    { sslam::ProfScope _ps(ctx, "k_line_match", pick(ctx, stream)); hipLaunchKernelGGL(k_line_match, dim3(npf), dim3(256), 0, pick(ctx, stream), d_l1, d_n1, 0, d_l2, d_n2, 0, cap, gate_scale, ratio_mode, d_pairs, d_npairs, (double*)nullptr); }
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

extern "C" int sslam_line_match(sslam_ctx* ctx, const uint8_t* l1, int n1, const uint8_t* l2, int n2, double gate_scale, int ratio_mode,
                                int32_t* pairs_out, int cap, int* npairs_out, double* nn_mad_out, double* nn12_mad_out) {
    if (!ctx || n1 < 0 || n2 < 0 || !npairs_out || (n1 > 0 && (!l1 || !pairs_out)) || (n2 > 0 && !l2)) { set_error("sslam_line_match: invalid arguments"); return SSLAM_ERR_INVALID; }
    *npairs_out = 0;
    if (nn_mad_out) *nn_mad_out = 0;
    if (nn12_mad_out) *nn12_mad_out = 0;
    if (n1 == 0 || n2 < 2) return SSLAM_OK;       // degenerate: defined as no matches
    if (n1 > LM_MAX) { set_error("sslam_line_match: n1=%d exceeds %d", n1, LM_MAX); return SSLAM_ERR_UNSUPPORTED; }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int c = std::max(n1, n2);
    int rc;
    size_t total = 64 * (size_t)c + 8 * (size_t)c + 64;
    if ((rc = ctx->scratch[SCR_LINE_MATCH].ensure(total))) return rc;
    uint8_t* base = ctx->scratch[SCR_LINE_MATCH].as<uint8_t>();
    uint8_t* d1 = base; uint8_t* d2 = base + 32 * (size_t)c;
    int* dp = (int*)(d2 + 32 * (size_t)c); int* dn = dp + 2 * (size_t)c; double* dm = (double*)(dn + 4);
    SSLAM_HIP(hipMemcpyAsync(d1, l1, 32 * (size_t)n1, hipMemcpyHostToDevice, st));
    SSLAM_HIP(hipMemcpyAsync(d2, l2, 32 * (size_t)n2, hipMemcpyHostToDevice, st));
    { sslam::ProfScope _ps(ctx, "k_line_match", st); hipLaunchKernelGGL(k_line_match, dim3(1), dim3(256), 0, st, d1, (const int*)nullptr, n1, d2, (const int*)nullptr, n2, c, gate_scale, ratio_mode, dp, dn, dm); }
    SSLAM_HIP(hipGetLastError());
    int np = 0; double mads[2] = {0, 0};
    std::vector<int> hp(2 * (size_t)c);
    SSLAM_HIP(hipMemcpyAsync(&np, dn, sizeof(int), hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipMemcpyAsync(mads, dm, sizeof(mads), hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipMemcpyAsync(hp.data(), dp, 8 * (size_t)c, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipStreamSynchronize(st));
    *npairs_out = np;
    if (nn_mad_out) *nn_mad_out = mads[0];
    if (nn12_mad_out) *nn12_mad_out = mads[1];
    if (np > cap) { set_error("sslam_line_match: %d pairs exceed capacity %d", np, cap); return SSLAM_ERR_CAPACITY; }
    memcpy(pairs_out, hp.data(), 8 * (size_t)np);
    return SSLAM_OK;
}

// the fields of ProjArgs that a single call and a batch call fill alike
static void proj_shared_args(ProjArgs& A, int kind, int mode, const float bounds[4], float nnratio, int th_dist, int check_orientation) {
    A.kind = kind; A.mode = mode;
    A.minX = bounds[0]; A.maxX = bounds[1]; A.minY = bounds[2]; A.maxY = bounds[3];
    A.nnratio = nnratio; A.thDist = th_dist; A.checkOri = check_orientation;
}

// shared body of the projection matchers: features already on the device (d_feats / d_desc / d_uright), per-call inputs staged here
static int search_proj_core(sslam_ctx* ctx, int kind, int mode, const void* d_feats, const uint8_t* d_desc, int n, const float bounds[4],
                            const float* d_uright, const uint8_t* occupied, const sslam_proj_query* queries, const uint8_t* qdesc, int nq,
                            float nnratio, int th_dist, int check_orientation, int32_t* assigned_out, int* nmatches_out) {
    hipStream_t st = ctx->stream;
    const ProjArena L = proj_arena(n, nq, PROJ_K);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.total))) return rc;
    uint8_t* B = ctx->scratch[SCR_CALL].as<uint8_t>();
    // occupancy, queries and query descriptors sit back to back in B: one staged H2D through pinned memory (each pageable copy costs more
    // host time than it moves data); the results (assigned, count) come back the same way
    if ((rc = ctx->pinned[PIN_PROJ].ensure(L.pinnedBytes()))) return rc;
    uint8_t* H = ctx->pinned[PIN_PROJ].as<uint8_t>();
    if (occupied) memcpy(H + L.occ, occupied, (size_t)n);
    memcpy(H + L.q, queries, sizeof(sslam_proj_query) * (size_t)nq);
    memcpy(H + L.qdesc, qdesc, 32 * (size_t)nq);
    SSLAM_HIP(hipMemcpyAsync(B + L.occ, H + L.occ, L.assigned - L.occ, hipMemcpyHostToDevice, st));
    ProjArgs A;
    proj_shared_args(A, kind, mode, bounds, nnratio, th_dist, check_orientation);
    A.feats = (const uint8_t*)d_feats; A.desc = d_desc; A.n = n;
    A.uright = d_uright; A.occIn = occupied ? B + L.occ : nullptr;
    A.q = (const sslam_proj_query*)(B + L.q); A.qdesc = B + L.qdesc; A.nq = nq;
    A.assigned = (int*)(B + L.assigned); A.nmatches = (int*)(B + L.count); A.scratch = (int*)(B + L.scratch);
    A.stats = getenv("SSLAM_PROJ_STATS") ? (long long*)(B + L.stats()) : nullptr;      // development aid: seven counters behind the match count
    const ProjPlan P = proj_plan(n, nq);
    switch (P.form) {
    case ProjForm::TwoKernel: {      // one wave per query over the whole chip, then an ordered commit with parallel prefixes (match_ordered.h)
        ProjTopArgs T; T.A = A; T.top = (unsigned long long*)(B + L.top); T.cnt = (int*)(B + L.cnt);
        { sslam::ProfScope _ps(ctx, "k_proj_topk", st); hipLaunchKernelGGL(k_proj_topk, dim3(P.topkGrid), dim3(256), 0, st, T); }
        if ((rc = allow_dynamic_lds((const void*)k_proj_commit, P.ldsBytes))) return rc;
        { sslam::ProfScope _ps(ctx, "k_proj_commit", st); hipLaunchKernelGGL(k_proj_commit, dim3(1), dim3(64), P.ldsBytes, st, T, P.featsInLds); }
        break;
    }
    case ProjForm::OneWave: {
        sslam::ProfScope _ps(ctx, "k_search_proj", st);
        hipLaunchKernelGGL(k_search_proj, dim3(1), dim3(64), 0, st, A);
        break;
    }
    }
    SSLAM_HIP(hipGetLastError());
    SSLAM_HIP(hipMemcpyAsync(H + L.assigned, B + L.assigned, L.count + 4 - L.assigned, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipStreamSynchronize(st));
    memcpy(assigned_out, H + L.assigned, 4 * (size_t)n);
    memcpy(nmatches_out, H + L.count, sizeof(int));
    if (A.stats) {
        long long hs[4];
        SSLAM_HIP(hipMemcpy(hs, B + L.stats(), sizeof(hs), hipMemcpyDeviceToHost));
        fprintf(stderr, "proj stats: commit steps %lld, re-scans %lld (%lld cycles), commit kernel %lld cycles\n", hs[0], hs[1], hs[2], hs[3]);
    }
    return SSLAM_OK;
}

extern "C" int sslam_search_by_projection(sslam_ctx* ctx, int kind, int mode, const void* feats, const uint8_t* desc, int n, const float bounds[4],
                                          const float* uright, const uint8_t* occupied, const sslam_proj_query* queries, const uint8_t* qdesc, int nq,
                                          float nnratio, int th_dist, int check_orientation, int32_t* assigned_out, int* nmatches_out) {
    if (!ctx || (kind != 0 && kind != 1) || (mode != 0 && mode != 1) || (kind == 1 && mode == 1 && check_orientation) || n < 0 || nq < 0 || !nmatches_out || !bounds ||
        (n > 0 && (!feats || !desc || !assigned_out)) || (nq > 0 && (!queries || !qdesc)) || n >= MAX_ROWS) {
        set_error("sslam_search_by_projection: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    *nmatches_out = 0;
    for (int i = 0; i < n; ++i) assigned_out[i] = -1;
    if (n == 0 || nq == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t fsz = kind == 0 ? sizeof(sslam_keypoint) : sizeof(sslam_keyline);
    ArenaLayout L;
    const size_t oF = L.take(fsz * n), oD = L.take(32 * (size_t)n), oU = L.take(4 * (size_t)n);
    int rc;
    if ((rc = ctx->scratch[SCR_UPLOAD].ensure(L.size()))) return rc;
    uint8_t* B = ctx->scratch[SCR_UPLOAD].as<uint8_t>();
    const Staging S{B, st};
    if ((rc = S.in(oF, feats, fsz * n)) || (rc = S.in(oD, desc, 32 * (size_t)n)) || (rc = S.in(oU, uright, 4 * (size_t)n))) return rc;
    return search_proj_core(ctx, kind, mode, B + oF, B + oD, n, bounds, uright ? (const float*)(B + oU) : nullptr, occupied, queries, qdesc, nq,
                            nnratio, th_dist, check_orientation, assigned_out, nmatches_out);
}

// ---- the projection-window matcher for B frames that are already on the device (the batch extractors' output buffers), asynchronous
#ifdef SSLAM_TESTING      // libsslam_frontend_testing.so only (include/sslam_testing.h)
static ProjBatchTuning g_projBatchTuning;
extern "C" int sslam_testing_proj_batch_tuning(int max_slice, int feats_in_lds) {
    if (max_slice < 0) { set_error("sslam_testing_proj_batch_tuning: invalid arguments"); return SSLAM_ERR_INVALID; }
    g_projBatchTuning.maxSlice = max_slice; g_projBatchTuning.featsInLds = feats_in_lds != 0;
    return SSLAM_OK;
}
#endif

extern "C" int sslam_search_by_projection_batch_dev(sslam_ctx* ctx, int kind, int mode,
        const void* d_feats, const uint8_t* d_desc, const int32_t* d_n, int cap, int nframes, const float bounds[4],
        const float* d_uright, const uint8_t* d_occupied,
        const sslam_proj_query* d_queries, const uint8_t* d_qdesc, const int32_t* d_nq, int qcap,
        float nnratio, int th_dist, int check_orientation, int32_t* d_assigned, int32_t* d_nmatches, void* stream) {
    if (!ctx || (kind != 0 && kind != 1) || (mode != 0 && mode != 1) || (kind == 1 && mode == 1 && check_orientation) || !rows_in_range(cap) || qcap < 0 ||
        nframes < 0 || !bounds || !d_feats || !d_desc || !d_n || !d_queries || !d_qdesc || !d_nq || !d_assigned || !d_nmatches ||
        !all_aligned<4>(d_feats, d_n, d_uright, d_queries, d_nq, d_assigned, d_nmatches) || !all_aligned<16>(d_desc, d_qdesc)) {      // descriptor rows are read as two 16-byte words
        set_error("sslam_search_by_projection_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (nframes == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
#ifdef SSLAM_TESTING
    const ProjBatchTuning tune = g_projBatchTuning;
#else
    const ProjBatchTuning tune;
#endif
    const ProjBatchPlan P = proj_batch_plan(cap, qcap, nframes, tune);      // match_plan.h: the kernels by row capacity, the slice by scratch
    const ProjBatchArena L = proj_batch_arena(cap, qcap, P.slice, PROJ_K);
    // ONE arena per context, used by the kernels of this call on the caller's stream after the call has returned (StreamOrderedBuf, common.h)
    int rc;
    if ((rc = ctx->projBatch.acquire(st, L.total))) return rc;
    uint8_t* B = ctx->projBatch.as<uint8_t>();
    ProjBatchArgs T;
    ProjArgs& A = T.A;
    proj_shared_args(A, kind, mode, bounds, nnratio, th_dist, check_orientation);
    A.feats = d_feats; A.desc = d_desc; A.n = 0;
    A.uright = d_uright; A.occIn = d_occupied; A.q = d_queries; A.qdesc = d_qdesc; A.nq = 0;
    A.assigned = d_assigned; A.nmatches = d_nmatches; A.scratch = nullptr; A.stats = nullptr;
    T.n = d_n; T.nq = d_nq; T.cap = cap; T.qcap = qcap; T.frame0 = 0;
    T.scratch = (int*)(B + L.scratch); T.top = (unsigned long long*)(B + L.top); T.cnt = (int*)(B + L.cnt);
    if (P.form == ProjForm::TwoKernel && (rc = allow_dynamic_lds((const void*)k_proj_commit_batch, P.ldsBytes))) return rc;
    for (int s = 0; s < proj_batch_slices(P, nframes); ++s) {      // slices of frames, in stream order on the one arena
        const ProjBatchSlice sl = proj_batch_slice(P, nframes, s);
        const int ns = sl.count;
        T.frame0 = sl.first;
        switch (P.form) {
        case ProjForm::TwoKernel: {      // one wave per (frame, query), then one committing wave per frame
            { sslam::ProfScope _ps(ctx, "k_proj_topk_batch", st); hipLaunchKernelGGL(k_proj_topk_batch, dim3(P.topkGrid, ns), dim3(256), 0, st, T); }
            { sslam::ProfScope _ps(ctx, "k_proj_commit_batch", st); hipLaunchKernelGGL(k_proj_commit_batch, dim3(ns), dim3(64), P.ldsBytes, st, T, P.featsInLds); }
            break;
        }
        case ProjForm::OneWave: {
            sslam::ProfScope _ps(ctx, "k_search_proj_batch", st);
            hipLaunchKernelGGL(k_search_proj_batch, dim3(ns), dim3(64), 0, st, T);
            break;
        }
        }
    }
    SSLAM_HIP(hipGetLastError());
    return ctx->projBatch.mark(st);
}

// ---- device-resident frames
extern "C" void sslam_frame_destroy(sslam_frame* f);
extern "C" void sslam_vocab_destroy(sslam_vocab* v);
namespace {
// a handle under construction: destroyed on every early return (the SSLAM_HIP error paths included), handed over with release()
template <class T, void (*Destroy)(T*)> struct HandleGuard {
    T* p; explicit HandleGuard(T* q) : p(q) {}
    ~HandleGuard() { if (p) Destroy(p); }
    T* release() { T* q = p; p = nullptr; return q; }
};
}  // namespace

extern "C" int sslam_frame_upload(sslam_ctx* ctx, int kind, const void* feats, const uint8_t* desc, int n, const float* uright, const float bounds[4],
                                  sslam_frame** out) {
    if (!ctx || !out || (kind != 0 && kind != 1) || !rows_in_range(n) || !bounds || (n > 0 && (!feats || !desc))) {
        set_error("sslam_frame_upload: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    sslam_frame* f = new sslam_frame();
    HandleGuard<sslam_frame, sslam_frame_destroy> guard(f);
    f->ctx = ctx; f->kind = kind; f->n = n; f->hasUright = uright != nullptr;
    for (int i = 0; i < 4; ++i) f->bounds[i] = bounds[i];
    const size_t fsz = kind == 0 ? sizeof(sslam_keypoint) : sizeof(sslam_keyline);
    int rc = SSLAM_OK;
    if ((rc = f->feats.ensure(std::max<size_t>(fsz * n, 256))) || (rc = f->desc.ensure(std::max<size_t>(32 * (size_t)n, 256))) ||
        (uright && (rc = f->uright.ensure(std::max<size_t>(4 * (size_t)n, 256))))) return rc;
    if (n > 0) {
        SSLAM_HIP(hipMemcpyAsync(f->feats.p, feats, fsz * n, hipMemcpyHostToDevice, ctx->stream));
        SSLAM_HIP(hipMemcpyAsync(f->desc.p, desc, 32 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        if (uright) SSLAM_HIP(hipMemcpyAsync(f->uright.p, uright, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        SSLAM_HIP(hipStreamSynchronize(ctx->stream));
    }
    *out = guard.release();
    return SSLAM_OK;
}

// adopt device buffers the extractors already hold (sslam_frame_from_orb / sslam_frame_from_lines): device-to-device snapshot
int sslam_frame_from_device(sslam_ctx* ctx, int kind, const void* d_feats, const uint8_t* d_desc, int n, const float bounds[4], sslam_frame** out) {
    SSLAM_HIP(hipSetDevice(ctx->device));
    sslam_frame* f = new sslam_frame();
    HandleGuard<sslam_frame, sslam_frame_destroy> guard(f);
    f->ctx = ctx; f->kind = kind; f->n = n;
    for (int i = 0; i < 4; ++i) f->bounds[i] = bounds[i];
    const size_t fsz = kind == 0 ? sizeof(sslam_keypoint) : sizeof(sslam_keyline);
    int rc;
    if ((rc = f->feats.ensure(std::max<size_t>(fsz * n, 256))) || (rc = f->desc.ensure(std::max<size_t>(32 * (size_t)n, 256)))) return rc;
    if (n > 0) {
        SSLAM_HIP(hipMemcpyAsync(f->feats.p, d_feats, fsz * n, hipMemcpyDeviceToDevice, ctx->stream));
        SSLAM_HIP(hipMemcpyAsync(f->desc.p, d_desc, 32 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        SSLAM_HIP(hipStreamSynchronize(ctx->stream));
    }
    *out = guard.release();
    return SSLAM_OK;
}

extern "C" void sslam_frame_destroy(sslam_frame* f) {
    if (!f) return;
    if (f->ctx) (void)hipSetDevice(f->ctx->device);
    f->feats.release(); f->desc.release(); f->uright.release();
    delete f;
}

extern "C" int sslam_frame_count(const sslam_frame* f) { return f ? f->n : 0; }

extern "C" int sslam_search_by_projection_frame(sslam_ctx* ctx, const sslam_frame* frame, int mode, const uint8_t* occupied,
                                                const sslam_proj_query* queries, const uint8_t* qdesc, int nq,
                                                float nnratio, int th_dist, int check_orientation, int32_t* assigned_out, int* nmatches_out) {
    if (!ctx || !frame || frame->ctx != ctx || (mode != 0 && mode != 1) || (frame->kind == 1 && mode == 1 && check_orientation) || nq < 0 || !nmatches_out ||
        (frame->n > 0 && !assigned_out) || (nq > 0 && (!queries || !qdesc))) {
        set_error("sslam_search_by_projection_frame: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    *nmatches_out = 0;
    for (int i = 0; i < frame->n; ++i) assigned_out[i] = -1;
    if (frame->n == 0 || nq == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    return search_proj_core(ctx, frame->kind, mode, frame->feats.p, frame->desc.as<uint8_t>(), frame->n, frame->bounds,
                            frame->hasUright ? frame->uright.as<float>() : nullptr, occupied, queries, qdesc, nq, nnratio, th_dist, check_orientation,
                            assigned_out, nmatches_out);
}

extern "C" int sslam_hamming_knn2_frames(sslam_ctx* ctx, const sslam_frame* q, const sslam_frame* t, int32_t* idx, int32_t* dist) {
    if (!ctx || !q || !t || q->ctx != ctx || t->ctx != ctx || (q->n > 0 && (!idx || !dist))) { set_error("sslam_hamming_knn2_frames: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (q->n == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(16 * (size_t)q->n))) return rc;
    int32_t* dI = ctx->scratch[SCR_CALL].as<int32_t>();
    int32_t* dD = dI + 2 * (size_t)q->n;
    if ((rc = sslam_hamming_knn2_dev(ctx, q->desc.as<uint8_t>(), q->n, t->desc.as<uint8_t>(), t->n, dI, dD, (void*)st))) return rc;
    SSLAM_HIP(hipMemcpyAsync(idx, dI, 8 * (size_t)q->n, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipMemcpyAsync(dist, dD, 8 * (size_t)q->n, hipMemcpyDeviceToHost, st));
    SSLAM_HIP(hipStreamSynchronize(st));
    return SSLAM_OK;
}

static int search_by_bow_core(sslam_ctx* ctx, const sslam_keypoint* kf_kp, const uint8_t* kf_desc, const uint8_t* kf_valid, int nkf,
                              const sslam_keypoint* f_kp, const uint8_t* f_desc, const uint8_t* f_valid, int nf, const int32_t* node_kf_ptr, const int32_t* node_f_ptr,
                              int nnodes, const int32_t* kf_idx, const int32_t* f_idx, float nnratio, int check_orientation, int strict_th,
                              int32_t* assigned_out, int* nmatches_out) {
    if (!ctx || nkf < 0 || nf < 0 || nnodes < 0 || !nmatches_out || (nf > 0 && !assigned_out) ||
        (nnodes > 0 && (!node_kf_ptr || !node_f_ptr || !kf_idx || !f_idx || !kf_kp || !kf_desc || !kf_valid || !f_kp || !f_desc))) {
        set_error("sslam_orb_search_by_bow: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    *nmatches_out = 0;
    for (int i = 0; i < nf; ++i) assigned_out[i] = -1;
    if (nnodes == 0 || nf == 0 || nkf == 0) return SSLAM_OK;
    int rc;
    if ((rc = check_csr("sslam_orb_search_by_bow", "keyframe feature", node_kf_ptr, nnodes, kf_idx, nkf)) ||
        (rc = check_csr("sslam_orb_search_by_bow", "frame feature", node_f_ptr, nnodes, f_idx, nf))) return rc;
    const int nk = node_kf_ptr[nnodes], nfi = node_f_ptr[nnodes];
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t ks = sizeof(sslam_keypoint);
    const BowArena L = bow_arena(nkf, nf, nnodes, nk, nfi);
    if ((rc = ctx->scratch[SCR_UPLOAD].ensure(L.total))) return rc;
    uint8_t* B = ctx->scratch[SCR_UPLOAD].as<uint8_t>();
    // every input (and the -1 fill of the two result arrays) goes through ONE pinned staging buffer and one H2D copy: ten small pageable
    // copies cost more host time than the kernels take (0.11 ms of the call's 0.18)
    const void* src[9] = {kf_kp, kf_desc, kf_valid, f_kp, f_desc, node_kf_ptr, node_f_ptr, kf_idx, f_idx};
    const size_t len[9] = {ks * nkf, 32 * (size_t)nkf, (size_t)nkf, ks * nf, 32 * (size_t)nf, 4 * (size_t)(nnodes + 1), 4 * (size_t)(nnodes + 1), 4 * (size_t)nk, 4 * (size_t)nfi};
    if ((rc = ctx->pinned[PIN_BOW].ensure(L.total))) return rc;
    uint8_t* H = ctx->pinned[PIN_BOW].as<uint8_t>();
    for (int i = 0; i < 9; ++i) if (len[i]) memcpy(H + L.in[i], src[i], len[i]);
    memset(H + L.assigned, 0xFF, 4 * (size_t)nf); memset(H + L.count, 0, 256); memset(H + L.qbin, 0xFF, 4 * (size_t)nf);
    if (f_valid) memcpy(H + L.validF, f_valid, (size_t)nf);
    SSLAM_HIP(hipMemcpyAsync(B, H, L.total, hipMemcpyHostToDevice, st));
    BowArgs A;
    A.validF = f_valid ? B + L.validF : nullptr; A.strictTh = strict_th;
    A.kpKF = (const sslam_keypoint*)(B + L.in[0]); A.dKF = B + L.in[1]; A.validKF = B + L.in[2]; A.kpF = (const sslam_keypoint*)(B + L.in[3]); A.dF = B + L.in[4]; A.nF = nf;
    A.ptrKF = (const int*)(B + L.in[5]); A.ptrF = (const int*)(B + L.in[6]); A.nnodes = nnodes; A.idxKF = (const int*)(B + L.in[7]); A.idxF = (const int*)(B + L.in[8]);
    A.nnratio = nnratio; A.checkOri = check_orientation; A.assigned = (int*)(B + L.assigned); A.nmatches = (int*)(B + L.count); A.qbin = (int*)(B + L.qbin);
    bool disjoint = true;                     // DBoW2 puts a feature under exactly one node; if a caller's lists do not, replay in order
    {
        std::vector<uint8_t> seen((size_t)nf, 0);
        for (int i = 0; i < nfi && disjoint; ++i) { if (seen[f_idx[i]]) disjoint = false; seen[f_idx[i]] = 1; }
    }
    { sslam::ProfScope _ps(ctx, "k_search_bow", st); hipLaunchKernelGGL(k_search_bow, dim3(disjoint ? std::min(nnodes, 4096) : 1), dim3(64), 0, st, A); }
    // (a fused form -- the last workgroup to finish runs this pass, saving the launch -- was measured: the two agent-scope fences per
    // workgroup cost more than the launch, 0.111 against 0.103 ms per call; both passes in ONE workgroup of sixteen waves, no fences at
    // all: 0.235 ms -- two nodes per wave in series instead of one workgroup per node)
    { sslam::ProfScope _ps(ctx, "k_bow_finish", st); hipLaunchKernelGGL(k_rot_finish, dim3(1), dim3(256), 0, st, A.assigned, A.qbin, nf, check_orientation, A.nmatches); }
    SSLAM_HIP(hipGetLastError());
    SSLAM_HIP(hipMemcpyAsync(H + L.assigned, B + L.assigned, L.count + 4 - L.assigned, hipMemcpyDeviceToHost, st));      // assigned + the count, back through the same staging
    SSLAM_HIP(hipStreamSynchronize(st));
    memcpy(assigned_out, H + L.assigned, 4 * (size_t)nf);
    memcpy(nmatches_out, H + L.count, sizeof(int));
    return SSLAM_OK;
}

extern "C" int sslam_orb_search_by_bow(sslam_ctx* ctx, const sslam_keypoint* kf_kp, const uint8_t* kf_desc, const uint8_t* kf_valid, int nkf,
                                       const sslam_keypoint* f_kp, const uint8_t* f_desc, int nf, const int32_t* node_kf_ptr, const int32_t* node_f_ptr,
                                       int nnodes, const int32_t* kf_idx, const int32_t* f_idx, float nnratio, int check_orientation,
                                       int32_t* assigned_out, int* nmatches_out) {
    return search_by_bow_core(ctx, kf_kp, kf_desc, kf_valid, nkf, f_kp, f_desc, nullptr, nf, node_kf_ptr, node_f_ptr, nnodes, kf_idx, f_idx, nnratio, check_orientation, 0,
                              assigned_out, nmatches_out);
}

// ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12), src/ORBmatcher.cc:525-658: the same walk with the
// second keyframe in the frame's role, candidates limited to features that own a good map point, `dist < TH_LOW`, and the result indexed by
// the first keyframe's features (every feature sits in one node and a taken candidate is skipped, so the map is one-to-one).
extern "C" int sslam_orb_search_by_bow_keyframes(sslam_ctx* ctx, const sslam_keypoint* kf1_kp, const uint8_t* kf1_desc, const uint8_t* kf1_valid, int n1,
                                                 const sslam_keypoint* kf2_kp, const uint8_t* kf2_desc, const uint8_t* kf2_valid, int n2,
                                                 const int32_t* node_kf1_ptr, const int32_t* node_kf2_ptr, int nnodes, const int32_t* kf1_idx, const int32_t* kf2_idx,
                                                 float nnratio, int check_orientation, int32_t* matches12_out, int* nmatches_out) {
    if (n1 < 0 || (n1 > 0 && !matches12_out) || (n2 > 0 && nnodes > 0 && !kf2_valid)) { set_error("sslam_orb_search_by_bow_keyframes: invalid arguments"); return SSLAM_ERR_INVALID; }
    for (int i = 0; i < n1; ++i) matches12_out[i] = -1;
    std::vector<int32_t> assigned((size_t)std::max(n2, 1), -1);
    const int rc = search_by_bow_core(ctx, kf1_kp, kf1_desc, kf1_valid, n1, kf2_kp, kf2_desc, kf2_valid, n2, node_kf1_ptr, node_kf2_ptr, nnodes, kf1_idx, kf2_idx, nnratio,
                                      check_orientation, 1, assigned.data(), nmatches_out);
    if (rc) return rc;
    for (int j = 0; j < n2; ++j) if (assigned[j] >= 0) matches12_out[assigned[j]] = j;
    return SSLAM_OK;
}


// MapPoint / MapLine ::ComputeDistinctiveDescriptors for `nsets` observation sets at once: set s owns descriptor rows
// ptr[s] .. ptr[s+1] of `desc`; best_out[s] = index (inside the set) of the descriptor with the least median distance to
// the rest, first such row on ties, -1 for an empty set.
extern "C" int sslam_distinctive_descriptors(sslam_ctx* ctx, const uint8_t* desc, const int32_t* ptr, int nsets, int32_t* best_out) {
    if (!ctx || nsets < 0 || (nsets > 0 && (!ptr || !best_out))) { set_error("sslam_distinctive_descriptors: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (nsets == 0) return SSLAM_OK;
    int rc;
    if ((rc = check_csr("sslam_distinctive_descriptors", "set", ptr, nsets, nullptr, 0))) return rc;
    const int total = ptr[nsets];
    if (total > 0 && !desc) { set_error("sslam_distinctive_descriptors: invalid arguments"); return SSLAM_ERR_INVALID; }
    for (int s2 = 0; s2 < nsets; ++s2) {
        const int n = ptr[s2 + 1] - ptr[s2];
        if (n > DISTINCT_MAXN) { set_error("sslam_distinctive_descriptors: a set of %d descriptors exceeds the supported %d", n, DISTINCT_MAXN); return SSLAM_ERR_UNSUPPORTED; }
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ArenaLayout L;
    const size_t oD = L.take(32 * (size_t)std::max(total, 1)), oP = L.take(4 * (size_t)(nsets + 1)), oB = L.take(4 * (size_t)nsets);
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* B = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging S{B, st};
    if ((rc = S.in(oD, desc, 32 * (size_t)total)) || (rc = S.in(oP, ptr, 4 * (size_t)(nsets + 1)))) return rc;
    { sslam::ProfScope _ps(ctx, "k_distinctive", st); hipLaunchKernelGGL(k_distinctive, dim3(std::min(nsets, 4096)), dim3(64), 0, st, B + oD, (const int32_t*)(B + oP), nsets, (int32_t*)(B + oB)); }
    SSLAM_HIP(hipGetLastError());
    if ((rc = S.out(best_out, oB, 4 * (size_t)nsets))) return rc;
    return S.done();
}

// ---- the same choice for observation sets that name rows of a device-resident pool of keyframe slots, asynchronous (match_distinct.h)
extern "C" int sslam_distinctive_descriptors_batch_dev(sslam_ctx* ctx,
        const uint8_t* d_desc, const int32_t* d_n, int cap, int nkeyframes, const uint8_t* d_kf_bad,
        const sslam_observation* d_obs, int nobs, const int32_t* d_ptr, int nsets,
        int32_t* d_best, int32_t* d_median,
        uint8_t* d_out_desc, const int32_t* d_out_row, int nout, void* stream) {
    if (!ctx || !d_desc || !d_n || !d_ptr || !d_best || (nobs > 0 && !d_obs) || (d_out_row && !d_out_desc) ||
        !rows_in_range(cap) || nkeyframes < 0 || nobs < 0 || nsets < 0 || nout < 0 || !fits_31_bits(nkeyframes, cap) ||
        !all_aligned<4>(d_n, d_obs, d_ptr, d_best, d_median, d_out_row) || !all_aligned<16>(d_desc, d_out_desc)) {      // descriptor rows are read and written as two 16-byte words
        set_error("sslam_distinctive_descriptors_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (nsets == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    const DistinctBatchPlan P = distinct_batch_plan(nsets);      // match_plan.h: a set's kernel follows its entry count, which only the device reads
    DistinctArgs A;
    A.desc = d_desc; A.n = d_n; A.cap = cap; A.nkeyframes = nkeyframes; A.bad = d_kf_bad; A.obs = d_obs; A.nobs = nobs; A.ptr = d_ptr; A.nsets = nsets;
    A.best = d_best; A.median = d_median; A.outDesc = d_out_desc; A.outRow = d_out_row; A.nout = nout;
    { sslam::ProfScope _ps(ctx, "k_distinct_batch", st); hipLaunchKernelGGL(k_distinct_batch, dim3(P.grid), dim3(P.threads), 0, st, A); }      // small and medium sets, refusals
    { sslam::ProfScope _ps(ctx, "k_distinct_large", st); hipLaunchKernelGGL(k_distinct_large, dim3(P.largeGrid), dim3(P.largeThreads), 0, st, A); }      // the rare large ones
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

// The candidate search of ORBmatcher::Fuse (both overloads) and LSDmatcher::Fuse on a device-resident keyframe: per query the
// feature with the smallest descriptor distance inside the window (first in GetFeaturesInArea / GetLinesInArea order on ties),
// -1 / INT_MAX when the window holds no admissible feature.  The caller applies `bestDist <= TH_LOW` and the Replace /
// AddObservation bookkeeping in query order, exactly as the reference does after its inner loop.
extern "C" int sslam_fuse_search(sslam_ctx* ctx, const sslam_frame* kf, int chi2_mode, const float* inv_level_sigma2, int nlevels,
                                 const sslam_proj_query* queries, const uint8_t* qdesc, int nq, int32_t* best_idx_out, int32_t* best_dist_out) {
    if (!ctx || !kf || kf->ctx != ctx || (chi2_mode != 0 && chi2_mode != 1) || nq < 0 || (nq > 0 && (!queries || !qdesc || !best_idx_out || !best_dist_out)) ||
        (chi2_mode == 1 && (kf->kind != 0 || !inv_level_sigma2 || nlevels <= 0 || nlevels > 64))) {
        set_error("sslam_fuse_search: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    for (int i = 0; i < nq; ++i) { best_idx_out[i] = -1; best_dist_out[i] = 0x7fffffff; }
    if (nq == 0 || kf->n == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ArenaLayout L;
    const size_t oQ = L.take(sizeof(sslam_proj_query) * (size_t)nq), oQD = L.take(32 * (size_t)nq), oS = L.take(256), oI = L.take(4 * (size_t)nq), oD = L.take(4 * (size_t)nq);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* B = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging S{B, st};
    if ((rc = S.in(oQ, queries, sizeof(sslam_proj_query) * (size_t)nq)) || (rc = S.in(oQD, qdesc, 32 * (size_t)nq)) ||
        (rc = S.in(oS, chi2_mode ? inv_level_sigma2 : nullptr, sizeof(float) * (size_t)nlevels))) return rc;
    FuseArgs A;
    A.kind = kf->kind; A.chi2 = chi2_mode; A.feats = kf->feats.p; A.desc = kf->desc.as<uint8_t>(); A.n = kf->n;
    A.minX = kf->bounds[0]; A.maxX = kf->bounds[1]; A.minY = kf->bounds[2]; A.maxY = kf->bounds[3];
    A.uright = kf->hasUright ? kf->uright.as<float>() : nullptr; A.invSigma2 = (const float*)(B + oS); A.nlevels = nlevels;
    A.q = (const sslam_proj_query*)(B + oQ); A.qdesc = B + oQD; A.nq = nq; A.bestIdx = (int*)(B + oI); A.bestDist = (int*)(B + oD);
    { sslam::ProfScope _ps(ctx, "k_fuse_search", st); hipLaunchKernelGGL(k_fuse_search, dim3(std::min(nq, 8192)), dim3(64), 0, st, A); }
    SSLAM_HIP(hipGetLastError());
    if ((rc = S.out(best_idx_out, oI, 4 * (size_t)nq)) || (rc = S.out(best_dist_out, oD, 4 * (size_t)nq))) return rc;
    return S.done();
}

// ---- the same candidate search for jobs (keyframe slot, block of queries) on a device-resident pool of keyframe slots, asynchronous
extern "C" int sslam_fuse_search_batch_dev(sslam_ctx* ctx, int kind, int chi2_mode,
        const void* d_feats, const uint8_t* d_desc, const float* d_uright, const int32_t* d_n, int cap, int nkeyframes,
        const float bounds[4], const float* inv_level_sigma2, int nlevels,
        const sslam_proj_query* d_queries, int qcap, const uint8_t* d_qdesc, int nqdesc,
        const sslam_fuse_job* d_jobs, int njobs,
        int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_nfound, void* stream) {
    if (!ctx || (kind != 0 && kind != 1) || (chi2_mode != 0 && chi2_mode != 1) || (chi2_mode == 1 && (kind != 0 || !inv_level_sigma2 || nlevels < 1 || nlevels > 64)) ||
        !d_feats || !d_desc || !d_n || !bounds || !d_queries || !d_qdesc || !d_jobs || !d_best_idx || !d_best_dist || !d_nfound ||
        !rows_in_range(cap) || qcap < 0 || nkeyframes < 0 || njobs < 0 || nqdesc < 0 || !fits_31_bits(njobs, qcap) ||
        !all_aligned<4>(d_feats, d_uright, d_n, d_queries, d_jobs, d_best_idx, d_best_dist, d_nfound) || !all_aligned<16>(d_desc, d_qdesc)) {      // descriptor rows are read as two 16-byte words
        set_error("sslam_fuse_search_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    const BatchPlan P = batch_plan(FUSE_BATCH_ROW_BYTES, cap);      // match_plan.h: the keyframe's geometry in LDS or in global memory, by the row capacity alone
    const unsigned chunks = fuse_batch_chunks(qcap);
    const unsigned long long grid = fuse_batch_grid(njobs, qcap);      // one workgroup per (job, chunk of queries), job-major
    if (grid >= (1ull << 31)) { set_error("sslam_fuse_search_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID; }
    if (njobs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    FuseBatchArgs A;
    A.chi2 = chi2_mode; A.feats = d_feats; A.desc = d_desc; A.uright = d_uright; A.n = d_n; A.cap = cap; A.nkeyframes = nkeyframes;
    A.minX = bounds[0]; A.maxX = bounds[1]; A.minY = bounds[2]; A.maxY = bounds[3];
    A.nlevels = chi2_mode ? nlevels : 0;
    A.q = d_queries; A.qcap = qcap; A.qdesc = d_qdesc; A.nqdesc = nqdesc; A.jobs = d_jobs; A.chunks = chunks;
    A.bestIdx = d_best_idx; A.bestDist = d_best_dist; A.nfound = d_nfound;
    for (int i = 0; i < 64; ++i) A.invSigma2[i] = (chi2_mode && i < nlevels) ? inv_level_sigma2[i] : 0.f;
    SSLAM_HIP(hipMemsetAsync(d_nfound, 0, sizeof(int32_t) * (size_t)njobs, st));      // every workgroup ADDS its chunk's count; a skipped job's chunk 0 stores -1
    int rc;
    if ((rc = kind == 0 ? launch_batch(ctx, "k_fuse_search_batch", k_fuse_search_batch<0, true>, k_fuse_search_batch<0, false>, P, (unsigned)grid, st, A)
                        : launch_batch(ctx, "k_fuse_search_batch", k_fuse_search_batch<1, true>, k_fuse_search_batch<1, false>, P, (unsigned)grid, st, A))) return rc;
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

// ORBmatcher::SearchForTriangulation on two device-resident keyframes (their mvuRight travel with the handles).
extern "C" int sslam_orb_search_for_triangulation(sslam_ctx* ctx, const sslam_frame* kf1, const sslam_frame* kf2, const uint8_t* free1, const uint8_t* free2,
                                                  const int32_t* node_kf1_ptr, const int32_t* node_kf2_ptr, int nnodes, const int32_t* kf1_idx, const int32_t* kf2_idx,
                                                  const float F12[9], float ex, float ey, const float* scale_factors2, const float* level_sigma2_2, int nlevels,
                                                  int only_stereo, int check_orientation, int32_t* matches12_out, int* nmatches_out) {
    if (!ctx || !kf1 || !kf2 || kf1->ctx != ctx || kf2->ctx != ctx || kf1->kind != 0 || kf2->kind != 0 || nnodes < 0 || !nmatches_out || !F12 ||
        !scale_factors2 || !level_sigma2_2 || nlevels <= 0 || nlevels > 64 || (kf1->n > 0 && (!free1 || !matches12_out)) || (kf2->n > 0 && !free2) ||
        (nnodes > 0 && (!node_kf1_ptr || !node_kf2_ptr || !kf1_idx || !kf2_idx))) {
        set_error("sslam_orb_search_for_triangulation: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    *nmatches_out = 0;
    const int n1 = kf1->n, n2 = kf2->n;
    for (int i = 0; i < n1; ++i) matches12_out[i] = -1;
    if (n1 == 0 || n2 == 0 || nnodes == 0) return SSLAM_OK;
    int rc;
    if ((rc = check_csr("sslam_orb_search_for_triangulation", "keyframe-1", node_kf1_ptr, nnodes, kf1_idx, n1)) ||
        (rc = check_csr("sslam_orb_search_for_triangulation", "keyframe-2", node_kf2_ptr, nnodes, kf2_idx, n2))) return rc;
    const int total1 = node_kf1_ptr[nnodes], total2 = node_kf2_ptr[nnodes];
    if (total1 == 0 || total2 == 0) return SSLAM_OK;
    std::vector<int32_t> nodeOf((size_t)total1);
    for (int nd = 0; nd < nnodes; ++nd) for (int a = node_kf1_ptr[nd]; a < node_kf1_ptr[nd + 1]; ++a) nodeOf[a] = nd;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ArenaLayout L;
    const size_t oF1 = L.take(n1), oF2 = L.take(n2), oP1 = L.take(4 * (size_t)(nnodes + 1)), oP2 = L.take(4 * (size_t)(nnodes + 1)), oI1 = L.take(4 * (size_t)total1),
                 oI2 = L.take(4 * (size_t)total2), oNO = L.take(4 * (size_t)total1), oSF = L.take(4 * (size_t)nlevels), oSG = L.take(4 * (size_t)nlevels),
                 oM = L.take(4 * (size_t)n1), oQB = L.take(4 * (size_t)n1), oN = L.take(4);
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* B = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging S{B, st};
    const size_t ptrBytes = 4 * (size_t)(nnodes + 1), levelBytes = 4 * (size_t)nlevels;
    if ((rc = S.in(oF1, free1, n1)) || (rc = S.in(oF2, free2, n2)) || (rc = S.in(oP1, node_kf1_ptr, ptrBytes)) || (rc = S.in(oP2, node_kf2_ptr, ptrBytes)) ||
        (rc = S.in(oI1, kf1_idx, 4 * (size_t)total1)) || (rc = S.in(oI2, kf2_idx, 4 * (size_t)total2)) || (rc = S.in(oNO, nodeOf.data(), 4 * (size_t)total1)) ||
        (rc = S.in(oSF, scale_factors2, levelBytes)) || (rc = S.in(oSG, level_sigma2_2, levelBytes))) return rc;
    SSLAM_HIP(hipMemsetAsync(B + oM, 0xFF, 4 * (size_t)n1, st));
    TriArgs A;
    A.kp1 = kf1->feats.as<sslam_keypoint>(); A.d1 = kf1->desc.as<uint8_t>(); A.ur1 = kf1->hasUright ? kf1->uright.as<float>() : nullptr; A.free1 = B + oF1; A.n1 = n1;
    A.kp2 = kf2->feats.as<sslam_keypoint>(); A.d2 = kf2->desc.as<uint8_t>(); A.ur2 = kf2->hasUright ? kf2->uright.as<float>() : nullptr; A.free2 = B + oF2;
    A.ptr1 = (const int*)(B + oP1); A.ptr2 = (const int*)(B + oP2); A.nnodes = nnodes; A.idx1 = (const int*)(B + oI1); A.idx2 = (const int*)(B + oI2);
    A.nodeOf = (const int*)(B + oNO); A.total1 = total1;
    for (int i = 0; i < 9; ++i) A.F[i] = F12[i];
    A.ex = ex; A.ey = ey; A.scale2 = (const float*)(B + oSF); A.sigma2_2 = (const float*)(B + oSG); A.nlevels = nlevels;
    A.onlyStereo = only_stereo; A.checkOri = check_orientation;
    A.m12 = (int*)(B + oM); A.qbin = (int*)(B + oQB); A.nmatches = (int*)(B + oN);
    { sslam::ProfScope _ps(ctx, "k_tri_search", st); hipLaunchKernelGGL(k_tri_search, dim3(std::min(total1, 8192)), dim3(64), 0, st, A); }
    { sslam::ProfScope _ps(ctx, "k_tri_finish", st); hipLaunchKernelGGL(k_rot_finish, dim3(1), dim3(256), 0, st, A.m12, A.qbin, n1, check_orientation, A.nmatches); }
    SSLAM_HIP(hipGetLastError());
    if ((rc = S.out(matches12_out, oM, 4 * (size_t)n1)) || (rc = S.out(nmatches_out, oN, sizeof(int)))) return rc;
    return S.done();
}

// ---- SearchForTriangulation for pairs of keyframe slots that are already on the device, from per-feature node ids (sslam_bow_transform_batch_dev), asynchronous
extern "C" int sslam_orb_search_for_triangulation_batch_dev(sslam_ctx* ctx,
        const sslam_keypoint* d_kp, const uint8_t* d_desc, const int32_t* d_node,
        const uint8_t* d_free, const float* d_uright, const int32_t* d_n, int cap, int nkeyframes,
        const sslam_tri_pair* d_pairs, int npairs,
        const float* scale_factors, const float* level_sigma2, int nlevels,
        int only_stereo, int check_orientation,
        int32_t* d_matches12, int32_t* d_nmatches, void* stream) {
    if (!ctx || !d_kp || !d_desc || !d_node || !d_n || !d_pairs || !d_matches12 || !d_nmatches || !scale_factors || !level_sigma2 ||
        !rows_in_range(cap) || nkeyframes < 0 || npairs < 0 || nlevels < 1 || nlevels > 64 || !fits_31_bits(npairs, cap) ||
        !all_aligned<4>(d_kp, d_node, d_uright, d_n, d_pairs, d_matches12, d_nmatches) || !all_aligned<16>(d_desc)) {      // descriptor rows are read as two 16-byte words
        set_error("sslam_orb_search_for_triangulation_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (npairs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    const BatchPlan P = batch_plan(TRI_BATCH_ROW_BYTES, cap);      // match_plan.h: keyframe 2 in LDS or in global memory, by the row capacity alone
    TriBatchArgs A;
    A.kp = d_kp; A.desc = d_desc; A.node = d_node; A.isFree = d_free; A.uright = d_uright; A.n = d_n; A.cap = cap; A.nkeyframes = nkeyframes;
    A.pairs = d_pairs; A.nlevels = nlevels; A.onlyStereo = only_stereo; A.checkOri = check_orientation; A.m12 = d_matches12; A.nmatches = d_nmatches;
    for (int i = 0; i < 64; ++i) { A.scale2[i] = i < nlevels ? scale_factors[i] : 0.f; A.sigma2_2[i] = i < nlevels ? level_sigma2[i] : 0.f; }
    int rc;
    if ((rc = launch_batch(ctx, "k_tri_search_batch", k_tri_search_batch<true>, k_tri_search_batch<false>, P, (unsigned)npairs, st, A))) return rc;      // one workgroup per pair
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

// ---- DBoW2 vocabulary
extern "C" int sslam_vocab_create(sslam_ctx* ctx, int nnodes, int levels, const int32_t* child_ptr, const int32_t* children, const uint8_t* node_desc,
                                  const int32_t* word_id, const double* weight, sslam_vocab** out) {
    if (!ctx || !out || nnodes < 1 || levels < 1 || !child_ptr || !node_desc || !word_id || !weight) { set_error("sslam_vocab_create: invalid arguments"); return SSLAM_ERR_INVALID; }
    int rc;
    if ((rc = check_csr("sslam_vocab_create", "child", child_ptr, nnodes, nullptr, 0))) return rc;
    const int nch = child_ptr[nnodes];
    if (nch > 0 && !children) { set_error("sslam_vocab_create: invalid arguments"); return SSLAM_ERR_INVALID; }
    for (int i = 0; i < nch; ++i) if (children[i] <= 0 || children[i] >= nnodes) { set_error("sslam_vocab_create: child id out of range"); return SSLAM_ERR_INVALID; }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    sslam_vocab* v = new sslam_vocab();
    HandleGuard<sslam_vocab, sslam_vocab_destroy> guard(v);
    v->ctx = ctx; v->nnodes = nnodes; v->levels = levels;
    for (int i = 1; i < nnodes; ++i) v->nwords += child_ptr[i + 1] == child_ptr[i];
    if ((rc = v->childPtr.ensure(4 * (size_t)(nnodes + 1))) || (rc = v->children.ensure(std::max<size_t>(4 * (size_t)nch, 256))) || (rc = v->desc.ensure(32 * (size_t)nnodes)) ||
        (rc = v->wordId.ensure(4 * (size_t)nnodes)) || (rc = v->weight.ensure(8 * (size_t)nnodes))) return rc;
    hipStream_t st = ctx->stream;
    SSLAM_HIP(hipMemcpyAsync(v->childPtr.p, child_ptr, 4 * (size_t)(nnodes + 1), hipMemcpyHostToDevice, st));
    if (nch > 0) SSLAM_HIP(hipMemcpyAsync(v->children.p, children, 4 * (size_t)nch, hipMemcpyHostToDevice, st));
    SSLAM_HIP(hipMemcpyAsync(v->desc.p, node_desc, 32 * (size_t)nnodes, hipMemcpyHostToDevice, st));
    SSLAM_HIP(hipMemcpyAsync(v->wordId.p, word_id, 4 * (size_t)nnodes, hipMemcpyHostToDevice, st));
    SSLAM_HIP(hipMemcpyAsync(v->weight.p, weight, 8 * (size_t)nnodes, hipMemcpyHostToDevice, st));
    SSLAM_HIP(hipStreamSynchronize(st));
    *out = guard.release();
    return SSLAM_OK;
}

extern "C" void sslam_vocab_destroy(sslam_vocab* v) {
    if (!v) return;
    if (v->ctx) (void)hipSetDevice(v->ctx->device);
    v->childPtr.release(); v->children.release(); v->desc.release(); v->wordId.release(); v->weight.release();
    delete v;
}

static int bow_core(sslam_ctx* ctx, const sslam_vocab* v, const uint8_t* d_desc, int n, int levelsup, int32_t* word_out, double* weight_out, int32_t* node_out) {
    hipStream_t st = ctx->stream;
    ArenaLayout L;
    const size_t oW = L.take(4 * (size_t)n), oV = L.take(8 * (size_t)n), oN = L.take(4 * (size_t)n);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* B = ctx->scratch[SCR_CALL].as<uint8_t>();
    { sslam::ProfScope _ps(ctx, "k_bow_transform", st);
      hipLaunchKernelGGL(k_bow_transform, dim3((n + 255) / 256), dim3(256), 0, st, d_desc, n, (const int*)nullptr, n, v->childPtr.as<int>(), v->children.as<int>(), v->desc.as<uint8_t>(),
                         v->wordId.as<int>(), v->weight.as<double>(), v->levels - levelsup, (int*)(B + oW), (double*)(B + oV), (int*)(B + oN)); }
    SSLAM_HIP(hipGetLastError());
    const Staging S{B, st};
    if ((rc = S.out(word_out, oW, 4 * (size_t)n)) || (rc = S.out(weight_out, oV, 8 * (size_t)n)) || (rc = S.out(node_out, oN, 4 * (size_t)n))) return rc;
    return S.done();
}

extern "C" int sslam_bow_transform_frame(sslam_ctx* ctx, const sslam_vocab* vocab, const sslam_frame* frame, int levelsup,
                                         int32_t* word_out, double* weight_out, int32_t* node_out) {
    if (!ctx || !vocab || !frame || vocab->ctx != ctx || frame->ctx != ctx || levelsup < 0 || (frame->n > 0 && (!word_out || !weight_out || !node_out))) {
        set_error("sslam_bow_transform_frame: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (frame->n == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    return bow_core(ctx, vocab, frame->desc.as<uint8_t>(), frame->n, levelsup, word_out, weight_out, node_out);
}

extern "C" int sslam_bow_transform(sslam_ctx* ctx, const sslam_vocab* vocab, const uint8_t* desc, int n, int levelsup,
                                   int32_t* word_out, double* weight_out, int32_t* node_out) {
    if (!ctx || !vocab || vocab->ctx != ctx || n < 0 || levelsup < 0 || (n > 0 && (!desc || !word_out || !weight_out || !node_out))) {
        set_error("sslam_bow_transform: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (n == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->scratch[SCR_UPLOAD].ensure(32 * (size_t)n))) return rc;
    if ((rc = Staging{ctx->scratch[SCR_UPLOAD].as<uint8_t>(), ctx->stream}.in(0, desc, 32 * (size_t)n))) return rc;
    return bow_core(ctx, vocab, ctx->scratch[SCR_UPLOAD].as<uint8_t>(), n, levelsup, word_out, weight_out, node_out);
}

// ---- the descent for B frames that are already on the device (the batch extractors' descriptor buffer), asynchronous: one launch, no scratch
extern "C" int sslam_bow_transform_batch_dev(sslam_ctx* ctx, const sslam_vocab* vocab, const uint8_t* d_desc, const int32_t* d_n, int cap, int nframes,
                                             int levelsup, int32_t* d_word, double* d_weight, int32_t* d_node, void* stream) {
    if (!ctx || !vocab || vocab->ctx != ctx || !d_desc || !d_n || !d_node || cap < 0 || nframes < 0 || levelsup < 0 || !fits_31_bits(nframes, cap) ||
        !all_aligned<16>(d_desc) || !all_aligned<4>(d_n, d_word, d_node) || !all_aligned<8>(d_weight)) {
        set_error("sslam_bow_transform_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    const int rows = nframes * cap;
    if (rows == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    { sslam::ProfScope _ps(ctx, "k_bow_transform", st);
      hipLaunchKernelGGL(k_bow_transform, dim3(((unsigned)rows + 255u) / 256u), dim3(256), 0, st, d_desc, rows, d_n, cap, vocab->childPtr.as<int>(), vocab->children.as<int>(),
                         vocab->desc.as<uint8_t>(), vocab->wordId.as<int>(), vocab->weight.as<double>(), vocab->levels - levelsup, d_word, d_weight, d_node); }
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

// ---- SearchByBoW for pairs of frames that are already on the device, from per-feature node ids (sslam_bow_transform_batch_dev), asynchronous
extern "C" int sslam_orb_search_by_bow_batch_dev(sslam_ctx* ctx,
        const sslam_keypoint* d_kf_kp, const uint8_t* d_kf_desc, const int32_t* d_kf_node, const uint8_t* d_kf_valid, const int32_t* d_nkf, int kfcap, int nkeyframes,
        const sslam_keypoint* d_f_kp, const uint8_t* d_f_desc, const int32_t* d_f_node, const int32_t* d_nf, int cap, int nframes,
        const int32_t* d_pair_kf, const int32_t* d_pair_f, int npairs,
        float nnratio, int check_orientation, int32_t* d_assigned, int32_t* d_nmatches, void* stream) {
    if (!ctx || !d_kf_kp || !d_kf_desc || !d_kf_node || !d_kf_valid || !d_nkf || !d_f_kp || !d_f_desc || !d_f_node || !d_nf || !d_assigned || !d_nmatches ||
        !rows_in_range(kfcap) || !rows_in_range(cap) || nkeyframes < 0 || nframes < 0 || npairs < 0 ||
        !all_aligned<4>(d_kf_kp, d_kf_node, d_nkf, d_f_kp, d_f_node, d_nf, d_pair_kf, d_pair_f, d_assigned, d_nmatches) ||
        !all_aligned<16>(d_kf_desc, d_f_desc) ||      // descriptor rows are read as two 16-byte words
        (!d_pair_kf && nkeyframes != npairs) || (!d_pair_f && nframes != npairs)) {
        set_error("sslam_orb_search_by_bow_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (npairs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    const BatchPlan P = batch_plan(BOW_BATCH_ROW_BYTES, cap);      // match_plan.h: the frame side in LDS or in global memory, by the row capacity alone
    BowBatchArgs A;
    A.kpKF = d_kf_kp; A.dKF = d_kf_desc; A.nodeKF = d_kf_node; A.validKF = d_kf_valid; A.nKF = d_nkf; A.kfcap = kfcap; A.nkeyframes = nkeyframes;
    A.kpF = d_f_kp; A.dF = d_f_desc; A.nodeF = d_f_node; A.nF = d_nf; A.cap = cap; A.nframes = nframes;
    A.pairKF = d_pair_kf; A.pairF = d_pair_f; A.nnratio = nnratio; A.checkOri = check_orientation; A.assigned = d_assigned; A.nmatches = d_nmatches;
    int rc;
    if ((rc = launch_batch(ctx, "k_search_bow_batch", k_search_bow_batch<true>, k_search_bow_batch<false>, P, (unsigned)npairs, st, A))) return rc;      // one workgroup per pair
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}

// ---- SearchByBoW between pairs of keyframe slots that are already on the device (src/ORBmatcher.cc:525-658, the first matcher of LoopClosing::ComputeSim3),
// from per-feature node ids (sslam_bow_transform_batch_dev), asynchronous.  The reference function writes its own output vector and its local vbMatched2
// alone, so any pair list is exact in one launch.
extern "C" int sslam_orb_search_by_bow_keyframes_batch_dev(sslam_ctx* ctx,
        const sslam_keypoint* d_kp, const uint8_t* d_desc, const int32_t* d_node, const uint8_t* d_valid,
        const int32_t* d_n, int cap, int nkeyframes,
        const int32_t* d_pairs, int npairs,
        float nnratio, int check_orientation,
        int32_t* d_matches12, int32_t* d_matches21, int32_t* d_nmatches, void* stream) {
    if (!ctx || !d_kp || !d_desc || !d_node || !d_n || !d_pairs || !d_matches12 || !d_matches21 || !d_nmatches ||
        !rows_in_range(cap) || nkeyframes < 0 || npairs < 0 || !fits_31_bits(npairs, cap) ||
        !all_aligned<4>(d_kp, d_node, d_n, d_pairs, d_matches12, d_matches21, d_nmatches) || !all_aligned<16>(d_desc)) {      // descriptor rows are read as two 16-byte words
        set_error("sslam_orb_search_by_bow_keyframes_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (npairs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    const BatchPlan P = batch_plan(BOW_BATCH_ROW_BYTES, cap);      // match_plan.h: keyframe 2 in LDS or in global memory, by the row capacity alone
    BowKfBatchArgs A;
    A.kp = d_kp; A.desc = d_desc; A.node = d_node; A.valid = d_valid; A.n = d_n; A.cap = cap; A.nkeyframes = nkeyframes;
    A.pairs = d_pairs; A.nnratio = nnratio; A.checkOri = check_orientation; A.m12 = d_matches12; A.m21 = d_matches21; A.nmatches = d_nmatches;
    int rc;
    if ((rc = launch_batch(ctx, "k_search_bow_kf_batch", k_search_bow_kf_batch<true>, k_search_bow_kf_batch<false>, P, (unsigned)npairs, st, A))) return rc;      // one workgroup per pair
    SSLAM_HIP(hipGetLastError());
    return SSLAM_OK;
}
