// Initializer::Initialize's geometric verification for MI355X (gfx950): the RANSAC over homography and fundamental matrix behind SearchForInitialization -- device side of
// reference src/Initializer.cc:55-118 (sets, FindHomography, FindFundamental, RH), :155-497 and :784-830.  The arithmetic is csrc/two_view_math.h, shared with the host model
// tests/sim/two_view_sim.cpp; this unit is the kernel around it and its entry points.
//
// k_two_view: one wave per frame pair.
//   1. the pair's keypoint coordinates go to LDS; lanes 0 .. 3 run the four sequential Normalize chains (x and y of both frames) on them
//   2. matches12 is compacted into (u1, v1, u2, v2) rows in LDS, ascending keypoint-1 index (ballot + popcount prefix: for_rows, pair_rows.h), over the staged coordinates
//   3. lane l takes iterations l, l + 64, ...: draws or reads the set, solves H then F (the Jacobi matrices of the lane sit in LDS, lane-interleaved: double k of lane l is
//      word k * 64 + l, so run-time indices make no private array and the 32 lanes of a half wave hit 64 distinct banks with their 8-byte accesses), composes, and walks the
//      rows in order (all lanes read the same row: a broadcast), keeping the best (score, iteration, matrix) of its own iterations
//   4. a wave-wide arg-max, ties to the lower iteration, picks each model's winner; its matrix is broadcast and every lane checks rows of its own for the inlier bits
// Every output word has one writer; no atomics.
#include "common.h"
#include "match_check.h"
#include "pair_rows.h"
#include "two_view_math.h"
#include <algorithm>

using namespace sslam;

namespace {

constexpr int TV_LANES = RANSAC_LANES;
constexpr int TV_TAP_MATS = 45;      // Hn, H21i, H12i, Fn, F21i
static_assert(tv::WS_DOUBLES == TWO_VIEW_WS_DOUBLES && sizeof(float4) == TWO_VIEW_ROW_BYTES, "two_view_plan (match_plan.h) sizes this kernel's LDS");

struct TwoViewArgs {
    const sslam_keypoint* kp1; const int32_t* n1;
    const sslam_keypoint* kp2; const int32_t* n2;
    const int32_t* m12; const int32_t* sets;
    int cap, iterations, pair0;
    float sigma; uint32_t seed;
    sslam_two_view_result* res; uint8_t* inl;
    int32_t* tapSets; float* tapMats; float* tapScores;      // sslam_testing_two_view_hypotheses only
};

struct LdsWs {      // tv::WS_DOUBLES doubles of this lane, lane-interleaved
    double* base;
    __device__ __forceinline__ double& at(int k) { return base[k * TV_LANES]; }
};
struct LdsRows {
    const float4* r;
    __device__ __forceinline__ tv::Row operator()(int i) const { const float4 v = r[i]; return tv::Row{v.x, v.y, v.z, v.w}; }
};
// mvMatches12 (:67-76) for keypoint-1 row i: a row is matched when 0 <= matches12 < n2; the keypoint-2 row, or -1
struct Matches12 {
    const int32_t* m12; int n1, n2;
    __device__ __forceinline__ int operator()(int i) const { const int m = i < n1 ? m12[i] : -1; return m >= 0 && m < n2 ? m : -1; }
};

// (score, iteration) order of the selection: a strictly greater score wins, equal scores go to the lower iteration (the first in the reference's loop); it < 0: no candidate
__device__ __forceinline__ bool beats(float s, int it, float bs, int bit) { return it >= 0 && (bit < 0 || s > bs || (s == bs && it < bit)); }

__device__ __forceinline__ void wave_best(float& s, int& it) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(s, o, 64);
        const int oit = __shfl_xor(it, o, 64);
        if (beats(os, oit, s, it)) { s = os; it = oit; }
    }
}

template <bool TAP>
__global__ __launch_bounds__(TV_LANES) void k_two_view(TwoViewArgs A) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ float sNorm[8];
    const int lane = threadIdx.x, p = blockIdx.x, cap = A.cap;
    const size_t base = (size_t)p * cap;
    const int n1 = slot_count(A.n1, p, cap), n2 = slot_count(A.n2, p, cap);
    const sslam_keypoint* kp1 = A.kp1 + base;
    const sslam_keypoint* kp2 = A.kp2 + base;
    float4* rows = (float4*)lds;
    LdsWs ws{(double*)(lds + 16 * (size_t)cap) + lane};

    // 1. Normalize (:784-830) over ALL keypoints of each frame
    float2* stage = (float2*)lds;
    for (int i = lane; i < n1; i += TV_LANES) stage[i] = make_float2(kp1[i].x, kp1[i].y);
    for (int i = lane; i < n2; i += TV_LANES) stage[cap + i] = make_float2(kp2[i].x, kp2[i].y);
    __syncthreads();
    if (lane < 4) {
        const float* src = (const float*)(stage + (lane < 2 ? 0 : cap)) + (lane & 1);
        float mean, s;
        tv::normalize_axis(lane < 2 ? n1 : n2, [&](int i) { return src[2 * i]; }, mean, s);
        sNorm[2 * lane] = mean; sNorm[2 * lane + 1] = s;
    }
    __syncthreads();
    const tv::Norm N1{sNorm[0], sNorm[1], sNorm[2], sNorm[3]}, N2{sNorm[4], sNorm[5], sNorm[6], sNorm[7]};

    // 2. mvMatches12 (:67-76)
    const Matches12 M{A.m12 + base, n1, n2};
    const int nm = for_rows(n1, lane, M, [&](int i, int m, int slot) {
        if (slot >= 0) rows[slot] = make_float4(kp1[i].x, kp1[i].y, kp2[m].x, kp2[m].y);
    });
    __syncthreads();

    float bestSH = 0.f, bestSF = 0.f;
    int bestItH = -1, bestItF = -1;
    float bH[9], bF[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) bH[k] = bF[k] = 0.f;

    // 3. the iterations of this lane
    if (nm >= 8) {
        const LdsRows R{rows};
        for (int it = lane; it < A.iterations; it += TV_LANES) {
            int set[8];
            bool valid = true;
            if (A.sets) {
                const int32_t* s = A.sets + ((size_t)p * A.iterations + it) * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) { set[j] = s[j]; valid = valid && set[j] >= 0 && set[j] < nm; }
            } else {
                draw_set<8>(A.seed, (uint32_t)(A.pair0 + p), (uint32_t)it, nm, set);
            }
            tv::Hypothesis h;
            tv::hypothesis(R, nm, N1, N2, set, valid, A.sigma, ws, h);
            if (h.scoreH > bestSH) {
                bestSH = h.scoreH; bestItH = it;
#pragma unroll
                for (int k = 0; k < 9; ++k) bH[k] = h.H21[k];
            }
            if (h.scoreF > bestSF) {
                bestSF = h.scoreF; bestItF = it;
#pragma unroll
                for (int k = 0; k < 9; ++k) bF[k] = h.F21[k];
            }
            if (TAP) {
#pragma unroll
                for (int j = 0; j < 8; ++j) A.tapSets[(size_t)it * 8 + j] = set[j];
                float* o = A.tapMats + (size_t)it * TV_TAP_MATS;
#pragma unroll
                for (int k = 0; k < 9; ++k) { o[k] = h.Hn[k]; o[9 + k] = h.H21[k]; o[18 + k] = h.H12[k]; o[27 + k] = h.Fn[k]; o[36 + k] = h.F21[k]; }
                A.tapScores[(size_t)it * 2] = h.scoreH; A.tapScores[(size_t)it * 2 + 1] = h.scoreF;
            }
        }
    }

    // 4. the winners (:196, :246): iteration it ran on lane it % 64
    float SH = bestSH, SF = bestSF;
    int itH = bestItH, itF = bestItF;
    wave_best(SH, itH);
    wave_best(SF, itF);
    float H21[9], F21[9], H12[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        H21[k] = __shfl(bH[k], itH < 0 ? 0 : itH & (TV_LANES - 1), 64);
        F21[k] = __shfl(bF[k], itF < 0 ? 0 : itF & (TV_LANES - 1), 64);
        if (itH < 0) H21[k] = 0.f;
        if (itF < 0) F21[k] = 0.f;
    }
    if (itH < 0) SH = 0.f;
    if (itF < 0) SF = 0.f;
    tv::inv3(H21, H12);

    if (lane == 0) {
        sslam_two_view_result r;
        r.nmatches = nm; r.model = 0; r.best_it_h = itH; r.best_it_f = itF;
        r.score_h = SH; r.score_f = SF; r.rh = 0.f;
        if (nm >= 8) tv::select_model(SH, SF, r.rh, r.model);
#pragma unroll
        for (int k = 0; k < 9; ++k) { r.H21[k] = H21[k]; r.F21[k] = F21[k]; }
        A.res[p] = r;
    }

    // vbMatchesInliersH / F of the winners, by keypoint 1; rows [n1, cap) are not written
    const float iss = tv::inv_sigma_square(A.sigma);
    for_rows(n1, lane, M, [&](int i, int, int slot) {
        int b = 0;
        if (slot >= 0 && nm >= 8) {
            const float4 r = rows[slot];
            float s = 0.f;
            if (itH >= 0 && tv::check_homography_match(H21, H12, r.x, r.y, r.z, r.w, iss, s)) b |= 1;
            if (itF >= 0 && tv::check_fundamental_match(F21, r.x, r.y, r.z, r.w, iss, s)) b |= 2;
        }
        if (i < n1) A.inl[base + i] = (uint8_t)b;
    });
}

int two_view_launch(sslam_ctx* ctx, const TwoViewArgs& A, int npairs, bool tap, hipStream_t st) {
    const RansacPlan P = two_view_plan(A.cap);
    return launch_tapped(ctx, "k_two_view", SSLAM_WITH_TAP(k_two_view), tap, (unsigned)npairs, P.threads, P.ldsBytes, st, A);
}

// one host pair on the device and back: shared by the single call and the testing tap
int two_view_host_pair(sslam_ctx* ctx, const char* fn, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12, const int32_t* sets,
                       int iterations, float sigma, uint32_t seed, int pair, sslam_two_view_result* result, uint8_t* inliers,
                       int32_t* sets_out, float* mats_out, float* scores_out) {
    if (!ctx || n1 < 0 || n2 < 0 || iterations < 1 || !(sigma > 0.f) || !result || (n1 > 0 && (!kp1 || !matches12 || !inliers)) || (n2 > 0 && !kp2) || pair < 0) {
        set_error("%s: invalid arguments", fn); return SSLAM_ERR_INVALID;
    }
    const int cap = std::max(std::max(n1, n2), 1);
    if (cap > TWO_VIEW_MAX_CAP) { set_error("%s: %d keypoints exceed the supported %d", fn, cap, TWO_VIEW_MAX_CAP); return SSLAM_ERR_UNSUPPORTED; }
    const bool tap = sets_out != nullptr;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    const size_t its = (size_t)iterations, setsBytes = 32 * its, matsBytes = 4 * TV_TAP_MATS * its, scoresBytes = 8 * its;
    ArenaLayout L;
    const size_t oK1 = L.take(sizeof(sslam_keypoint) * (size_t)cap), oK2 = L.take(sizeof(sslam_keypoint) * (size_t)cap), oN = L.take(256), oM = L.take(4 * (size_t)cap),
                 oS = L.take(sets ? setsBytes : 0), oR = L.take(256), oI = L.take((size_t)cap),
                 oTS = L.take(tap ? setsBytes : 0), oTM = L.take(tap ? matsBytes : 0), oTC = L.take(tap ? scoresBytes : 0);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* d = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging S{d, ctx->stream};
    const int hn[2] = {n1, n2};
    if ((rc = S.in(oK1, kp1, sizeof(sslam_keypoint) * (size_t)n1)) || (rc = S.in(oK2, kp2, sizeof(sslam_keypoint) * (size_t)n2)) || (rc = S.in(oN, hn, sizeof(hn))) ||
        (rc = S.in(oM, matches12, 4 * (size_t)n1)) || (rc = S.in(oS, sets, setsBytes))) return rc;
    if (tap) SSLAM_HIP(hipMemsetAsync(d + oTS, 0, L.size() - oTS, S.st));      // a pair below 8 matches runs no iteration
    TwoViewArgs A;
    A.kp1 = (const sslam_keypoint*)(d + oK1); A.n1 = (const int32_t*)(d + oN); A.kp2 = (const sslam_keypoint*)(d + oK2); A.n2 = (const int32_t*)(d + oN) + 1;
    A.m12 = (const int32_t*)(d + oM); A.sets = sets ? (const int32_t*)(d + oS) : nullptr;
    A.cap = cap; A.iterations = iterations; A.pair0 = pair; A.sigma = sigma; A.seed = seed;
    A.res = (sslam_two_view_result*)(d + oR); A.inl = d + oI;
    A.tapSets = tap ? (int32_t*)(d + oTS) : nullptr; A.tapMats = tap ? (float*)(d + oTM) : nullptr; A.tapScores = tap ? (float*)(d + oTC) : nullptr;
    if ((rc = two_view_launch(ctx, A, 1, tap, S.st)) || (rc = S.out(result, oR, sizeof(sslam_two_view_result))) || (rc = S.out(inliers, oI, (size_t)n1))) return rc;
    if (tap && ((rc = S.out(sets_out, oTS, setsBytes)) || (rc = S.out(mats_out, oTM, matsBytes)) || (rc = S.out(scores_out, oTC, scoresBytes)))) return rc;
    return S.done();
}

}  // namespace

extern "C" int sslam_two_view_ransac_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp1, const int32_t* d_n1, const sslam_keypoint* d_kp2, const int32_t* d_n2,
                                               int cap, int npairs, const int32_t* d_matches12, const int32_t* d_sets, int iterations, float sigma, uint32_t seed,
                                               sslam_two_view_result* d_result, uint8_t* d_inliers, void* stream) {
    if (!ctx || !d_kp1 || !d_n1 || !d_kp2 || !d_n2 || !d_matches12 || !d_result || !d_inliers || cap <= 0 || npairs <= 0 || iterations < 1 || !(sigma > 0.f) ||
        !all_aligned<4>(d_kp1, d_kp2) || !all_aligned<4>(d_n1, d_n2, d_matches12, d_sets) || !all_aligned<4>(d_result) || !fits_31_bits(npairs, cap) ||
        !injected_sets_ok(d_sets, npairs, iterations)) {
        set_error("sslam_two_view_ransac_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (cap > TWO_VIEW_MAX_CAP) { set_error("sslam_two_view_ransac_batch_dev: cap=%d exceeds the supported %d (16 bytes of LDS per row)", cap, TWO_VIEW_MAX_CAP); return SSLAM_ERR_UNSUPPORTED; }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    TwoViewArgs A;
    A.kp1 = d_kp1; A.n1 = d_n1; A.kp2 = d_kp2; A.n2 = d_n2; A.m12 = d_matches12; A.sets = d_sets;
    A.cap = cap; A.iterations = iterations; A.pair0 = 0; A.sigma = sigma; A.seed = seed;
    A.res = d_result; A.inl = d_inliers; A.tapSets = nullptr; A.tapMats = nullptr; A.tapScores = nullptr;
    return two_view_launch(ctx, A, npairs, false, pick(ctx, stream));
}

extern "C" int sslam_two_view_ransac(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12, const int32_t* sets,
                                     int iterations, float sigma, uint32_t seed, sslam_two_view_result* result, uint8_t* inliers) {
    return two_view_host_pair(ctx, "sslam_two_view_ransac", kp1, n1, kp2, n2, matches12, sets, iterations, sigma, seed, 0, result, inliers, nullptr, nullptr, nullptr);
}

#ifdef SSLAM_TESTING
#include "../../include/sslam_testing.h"
extern "C" int sslam_testing_two_view_hypotheses(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12,
                                                 const int32_t* sets, int iterations, float sigma, uint32_t seed, int pair, sslam_two_view_result* result, uint8_t* inliers,
                                                 int32_t* sets_out, float* mats_out, float* scores_out) {
    if (!sets_out || !mats_out || !scores_out) { set_error("sslam_testing_two_view_hypotheses: invalid arguments"); return SSLAM_ERR_INVALID; }
    return two_view_host_pair(ctx, "sslam_testing_two_view_hypotheses", kp1, n1, kp2, n2, matches12, sets, iterations, sigma, seed, pair, result, inliers,
                              sets_out, mats_out, scores_out);
}
#endif
