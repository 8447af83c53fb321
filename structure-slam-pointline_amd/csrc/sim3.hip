// Sim3Solver for MI355X (gfx950): the RANSAC of LoopClosing::ComputeSim3 (reference src/LoopClosing.cc:279-306) between SearchByBoW (:269) and SearchBySim3 (:328) --
// device side of reference src/Sim3Solver.cc.  The arithmetic is csrc/sim3_math.h, shared with the host model tests/sim/sim3_sim.cpp; this unit is the kernel around it and
// its entry points.
//
// k_sim3_ransac: one wave per pair of keyframe slots.
//   1. the pair's correspondences (the constructor's filters, :62-103) are compacted into 48-byte rows in LDS, ascending keyframe-1 row (ballot + popcount prefix: for_rows, pair_rows.h):
//      X1, X2, P1im1, P2im2 (FromCameraToImage), maxErr1, maxErr2
//   2. a round is 64 iterations, its_done + lane: every lane draws or reads its set, solves it (the 4 x 4 Jacobi is unrolled over static (p, q): registers, no scratch) and
//      walks all rows in order (all lanes read the same row: a broadcast), keeping its count and its s, R, t in registers
//   3. iterate's control flow (:183-199) over the round: a wave prefix-maximum of the counts in front of each lane, seeded with best_inliers; the lowest lane with
//      count >= prefix and count > min_inliers is the return, otherwise the highest lane with count >= prefix carries the new best and the next round starts
//   4. the inlier bytes of a return are recomputed from the winner's matrices by all lanes, by keyframe-1 row
// Every output word has one writer; no atomics.
#include "common.h"
#include "match_check.h"
#include "pair_rows.h"
#include "sim3_math.h"
#include <algorithm>

using namespace sslam;

namespace {

constexpr int S3_LANES = RANSAC_LANES;
constexpr int S3_MAX_LEVELS = 64;
constexpr int S3_TAP_FLOATS = 13;     // s12, R12, t12
static_assert(sizeof(s3::Row) == SIM3_ROW_BYTES, "a correspondence is three 16-byte words: sim3_plan (match_plan.h) sizes this kernel's LDS");
static_assert(sizeof(sslam_sim3_state) == 84, "sslam_sim3_state has no padding");

struct Sim3Args {
    const sslam_keypoint* kp; const float* x3dc; const uint8_t* valid; const int32_t* n;
    const float* K; const int32_t* pairs; const int32_t* m12; const int32_t* table; const int32_t* sets;
    int cap, nkeyframes, nlevels, fixScale, minInliers, maxIterations, newIterations, pair0;
    uint32_t seed;
    sslam_sim3_state* state; uint8_t* inl;
    int32_t* tapSets; float* tapMats; int32_t* tapCounts;      // sslam_testing_sim3_hypotheses only
    float maxErr[S3_MAX_LEVELS];                                  // s3::max_error of every level, from the host's level_sigma2
};

struct LdsRows {
    const float4* r;
    __device__ __forceinline__ s3::Row operator()(int i) const {
        const float4 a = r[3 * i], b = r[3 * i + 1], c = r[3 * i + 2];
        return s3::Row{{a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w}, {c.x, c.y}, c.z, c.w};
    }
};

// the constructor's filters for keyframe-1 row i (:64-79 with the rows standing for GetIndexInKeyFrame): the keyframe-2 row, or -1
struct Pair {
    const sslam_keypoint* kp1; const sslam_keypoint* kp2; const uint8_t* v1; const uint8_t* v2; const int32_t* m12;
    int n1, n2, nlevels;
    __device__ __forceinline__ int operator()(int i) const {
        if (i >= n1) return -1;
        const int m = m12[i];
        if (m < 0 || m >= n2) return -1;
        if (v1 && (!v1[i] || !v2[m])) return -1;
        const int o1 = kp1[i].octave, o2 = kp2[m].octave;
        return (o1 >= 0 && o1 < nlevels && o2 >= 0 && o2 < nlevels) ? m : -1;
    }
};

__device__ __forceinline__ void broadcast(s3::Sim3& h, int src) {
    h.s = __shfl(h.s, src, 64);
#pragma unroll
    for (int k = 0; k < 9; ++k) h.R[k] = __shfl(h.R[k], src, 64);
#pragma unroll
    for (int k = 0; k < 3; ++k) h.t[k] = __shfl(h.t[k], src, 64);
}

template <bool TAP>
__global__ __launch_bounds__(S3_LANES) void k_sim3_ransac(Sim3Args A) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = threadIdx.x, p = blockIdx.x, cap = A.cap;
    const int kf1 = A.pairs[2 * p], kf2 = A.pairs[2 * p + 1];
    sslam_sim3_state* S = A.state + p;
    if (kf1 < 0 || kf1 >= A.nkeyframes || kf2 < 0 || kf2 >= A.nkeyframes) {      // a skipped pair
        if (lane == 0) { S->n = 0; S->max_its = 0; S->found_it = -1; S->n_inliers = 0; S->no_more = 1; }
        return;
    }
    const size_t b1 = (size_t)kf1 * cap, b2 = (size_t)kf2 * cap, bp = (size_t)p * cap;
    Pair P;
    P.kp1 = A.kp + b1; P.kp2 = A.kp + b2; P.v1 = A.valid ? A.valid + b1 : nullptr; P.v2 = A.valid ? A.valid + b2 : nullptr; P.m12 = A.m12 + bp;
    P.n1 = slot_count(A.n, kf1, cap); P.n2 = slot_count(A.n, kf2, cap); P.nlevels = A.nlevels;
    const float* X1 = A.x3dc + 3 * b1;
    const float* X2 = A.x3dc + 3 * b2;
    const s3::Cam K1{A.K[4 * kf1], A.K[4 * kf1 + 1], A.K[4 * kf1 + 2], A.K[4 * kf1 + 3]}, K2{A.K[4 * kf2], A.K[4 * kf2 + 1], A.K[4 * kf2 + 2], A.K[4 * kf2 + 3]};
    float4* rows = (float4*)lds;

    // 1. mvX3Dc1 / 2, mvP1im1 / mvP2im2, mvnMaxError1 / 2 in mvnIndices1's order
    const int N = for_rows(P.n1, lane, P, [&](int i, int m, int slot) {
        if (slot < 0) return;
        const float x1[3] = {X1[3 * (size_t)i], X1[3 * (size_t)i + 1], X1[3 * (size_t)i + 2]}, x2[3] = {X2[3 * (size_t)m], X2[3 * (size_t)m + 1], X2[3 * (size_t)m + 2]};
        float p1[2], p2[2];
        s3::camera_to_image(x1, K1, p1);
        s3::camera_to_image(x2, K2, p2);
        float4* r = rows + 3 * slot;
        r[0] = make_float4(x1[0], x1[1], x1[2], x2[0]);
        r[1] = make_float4(x2[1], x2[2], p1[0], p1[1]);
        r[2] = make_float4(p2[0], p2[1], A.maxErr[P.kp1[i].octave], A.maxErr[P.kp2[m].octave]);
    });
    __syncthreads();

    // the solver object (:37-38, :137): a zero-filled state is a new one
    int itsDone = max(S->its_done, 0), bestInliers = S->best_inliers, bestIt = itsDone == 0 ? -1 : S->best_it;      // device data nothing has checked: iterations index d_sets
    s3::Sim3 best;
    best.s = S->s12;
#pragma unroll
    for (int k = 0; k < 9; ++k) best.R[k] = S->R12[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) best.t[k] = S->t12[k];

    int found = -1, nInliers = 0, maxIts = 0, noMore = 0;
    const bool iterates = N >= A.minInliers;      // :146-150
    if (iterates) {
        maxIts = A.table[N];
        const int end = itsDone < maxIts ? itsDone + min(A.newIterations, maxIts - itsDone) : itsDone;      // :158
        const LdsRows R{rows};
        // 2. / 3.
        for (int r0 = itsDone; r0 < end && found < 0; r0 += S3_LANES) {
            const int it = r0 + lane;
            const bool active = it < end;
            int set[3] = {-1, -1, -1};
            bool valid = active;
            if (active) {
                if (A.sets) {
                    const int32_t* s = A.sets + ((size_t)p * A.maxIterations + it) * 3;
#pragma unroll
                    for (int j = 0; j < 3; ++j) { set[j] = s[j]; valid = valid && set[j] >= 0 && set[j] < N; }
                } else if (N >= 3) {
                    draw_set<3>(A.seed, (uint32_t)(A.pair0 + p), (uint32_t)it, N, set);
                } else {
                    valid = false;
                }
            }
            s3::Sim3 h;
            const int count = s3::hypothesis(R, N, K1, K2, set, valid, A.fixScale != 0, h, [](int, bool) {});
            // the running maximum in front of this lane: what mnBestInliers is when the reference reaches this iteration
            int incl = count;
#pragma unroll
            for (int o = 1; o < S3_LANES; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl = max(incl, t);
            }
            int prefix = __shfl_up(incl, 1, 64);
            prefix = lane == 0 ? bestInliers : max(prefix, bestInliers);
            const bool isBest = count >= 0 && count >= prefix;                       // :183
            const unsigned long long retMask = __ballot(isBest && count > A.minInliers);      // :192
            const unsigned long long bestMask = __ballot(isBest);
            int src = -1;
            if (retMask) { src = __ffsll((long long)retMask) - 1; found = r0 + src; }
            else if (bestMask) src = 63 - __clzll((long long)bestMask);
            if (TAP) {
                if (active && (found < 0 || it <= found)) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) A.tapSets[(size_t)it * 3 + j] = set[j];
                    float* o = A.tapMats + (size_t)it * S3_TAP_FLOATS;
                    o[0] = h.s;
#pragma unroll
                    for (int k = 0; k < 9; ++k) o[1 + k] = h.R[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) o[10 + k] = h.t[k];
                    A.tapCounts[it] = count;
                }
            }
            if (src >= 0) {
                bestInliers = __shfl(count, src, 64);
                bestIt = r0 + src;
                broadcast(h, src);
                best = h;
            }
            if (found >= 0) { itsDone = found + 1; nInliers = bestInliers; }
            else itsDone = min(r0 + S3_LANES, end);
        }
        noMore = found < 0 && itsDone >= maxIts;      // :203
    } else {
        noMore = 1;
    }

    if (lane == 0) {
        S->n = N; S->max_its = maxIts; S->found_it = found; S->n_inliers = nInliers; S->no_more = noMore;
        if (iterates) {
            S->its_done = itsDone; S->best_inliers = bestInliers; S->best_it = bestIt; S->s12 = best.s;
#pragma unroll
            for (int k = 0; k < 9; ++k) S->R12[k] = best.R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) S->t12[k] = best.t[k];
        }
    }

    // 4. vbInliers (:143, :195-197) by keyframe-1 row; rows [n1, cap) are not written
    s3::Transforms T;
    s3::transforms(best, T);
    const LdsRows R{rows};
    for_rows(P.n1, lane, P, [&](int i, int, int slot) {
        uint8_t b = 0;
        if (slot >= 0 && found >= 0) b = s3::check_row(T, K1, K2, R(slot)) ? 1 : 0;
        if (i < P.n1) A.inl[bp + i] = b;
    });
}

// mRansacMaxIts for every N in [min_inliers, cap] (SetRansacParameters, :114-138, on the host with libm), cap + 1 int32 on the device.  Rebuilt only when its key changes; a
// rebuild waits on the host for the last kernel that read the old table, the upload and the kernel that reads it are ordered by the stream, and a later call on another
// stream waits on the device for the event behind them (StreamOrderedBuf).
int sim3_table(sslam_ctx* ctx, double probability, int minInliers, int maxIterations, int cap, hipStream_t st) {
    sslam_ctx::Sim3Table& T = ctx->sim3Table;
    const bool same = T.built && T.probability == probability && T.minInliers == minInliers && T.maxIterations == maxIterations && T.cap == cap;
    const size_t bytes = sizeof(int32_t) * ((size_t)cap + 1);
    if (same) return T.dev.acquire(st, bytes);
    if (T.dev.done) SSLAM_HIP(hipEventSynchronize(T.dev.done));
    int rc;
    if ((rc = T.host.ensure(bytes)) || (rc = T.dev.acquire(st, bytes))) return rc;
    int32_t* h = T.host.as<int32_t>();
    for (int n = 0; n <= cap; ++n) h[n] = n >= minInliers ? s3::ransac_max_its(probability, minInliers, maxIterations, n) : 0;      // below min_inliers: never read
    SSLAM_HIP(hipMemcpyAsync(T.dev.as<int32_t>(), h, bytes, hipMemcpyHostToDevice, st));
    T.built = true; T.probability = probability; T.minInliers = minInliers; T.maxIterations = maxIterations; T.cap = cap;
    return SSLAM_OK;
}

int sim3_enqueue(sslam_ctx* ctx, Sim3Args& A, const float* level_sigma2, double probability, int npairs, bool tap, hipStream_t st) {
    for (int l = 0; l < S3_MAX_LEVELS; ++l) A.maxErr[l] = l < A.nlevels ? s3::max_error(level_sigma2[l]) : 0.f;
    int rc;
    if ((rc = sim3_table(ctx, probability, A.minInliers, A.maxIterations, A.cap, st))) return rc;
    A.table = ctx->sim3Table.dev.as<int32_t>();
    const RansacPlan P = sim3_plan(A.cap);
    if ((rc = launch_tapped(ctx, "k_sim3_ransac", SSLAM_WITH_TAP(k_sim3_ransac), tap, (unsigned)npairs, P.threads, P.ldsBytes, st, A))) return rc;
    return ctx->sim3Table.dev.mark(st);
}

// one host pair on the device and back, as slots 0 and 1 of a pool of two: shared by the single call and the testing tap
int sim3_host_pair(sslam_ctx* ctx, const char* fn, const sslam_keypoint* kp1, const float* x3dc1, const uint8_t* valid1, int n1, const float* K1,
                   const sslam_keypoint* kp2, const float* x3dc2, const uint8_t* valid2, int n2, const float* K2, const float* level_sigma2, int nlevels,
                   const int32_t* matches12, int fix_scale, double probability, int min_inliers, int max_iterations, int new_iterations, const int32_t* sets, uint32_t seed,
                   int pair, sslam_sim3_state* state, uint8_t* inliers, int32_t* sets_out, float* mats_out, int32_t* counts_out) {
    if (!ctx || n1 < 0 || n2 < 0 || !K1 || !K2 || !state || (n1 > 0 && (!kp1 || !x3dc1 || !matches12 || !inliers)) || (n2 > 0 && (!kp2 || !x3dc2)) ||
        ((valid1 == nullptr) != (valid2 == nullptr) && n1 > 0 && n2 > 0) || pair < 0 ||
        !sim3_params_ok(level_sigma2, nlevels, probability, min_inliers, max_iterations, new_iterations)) {
        set_error("%s: invalid arguments", fn); return SSLAM_ERR_INVALID;
    }
    const int cap = std::max(std::max(n1, n2), 1);
    if (cap > SIM3_MAX_CAP) { set_error("%s: %d rows exceed the supported %d", fn, cap, SIM3_MAX_CAP); return SSLAM_ERR_UNSUPPORTED; }
    const bool tap = sets_out != nullptr;
    const bool hasValid = valid1 || valid2;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    const size_t its = (size_t)max_iterations, setsBytes = 12 * its, matsBytes = 4 * S3_TAP_FLOATS * its, countsBytes = 4 * its;
    // a pool of two slots: slot 1 starts cap rows behind slot 0 in every array
    const size_t ks = sizeof(sslam_keypoint);
    ArenaLayout L;
    const size_t oK = L.take(ks * 2 * (size_t)cap), oX = L.take(24 * (size_t)cap), oV = L.take(2 * (size_t)cap), oHead = L.take(256), oM = L.take(4 * (size_t)cap),
                 oS = L.take(sets ? setsBytes : 0), oState = L.take(256), oI = L.take((size_t)cap),
                 oTS = L.take(tap ? setsBytes : 0), oTM = L.take(tap ? matsBytes : 0), oTC = L.take(tap ? countsBytes : 0);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* d = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging S{d, ctx->stream};
    struct { int32_t n[2]; int32_t pairs[2]; float K[8]; } head;      // counts, the pair (0, 1), fx fy cx cy of both slots
    head.n[0] = n1; head.n[1] = n2; head.pairs[0] = 0; head.pairs[1] = 1;
    memcpy(head.K, K1, 16); memcpy(head.K + 4, K2, 16);
    if ((rc = S.in(oK, kp1, ks * (size_t)n1)) || (rc = S.in(oX, x3dc1, 12 * (size_t)n1)) || (rc = S.in(oV, valid1, (size_t)n1)) || (rc = S.in(oM, matches12, 4 * (size_t)n1)) ||
        (rc = S.in(oK + ks * (size_t)cap, kp2, ks * (size_t)n2)) || (rc = S.in(oX + 12 * (size_t)cap, x3dc2, 12 * (size_t)n2)) || (rc = S.in(oV + (size_t)cap, valid2, (size_t)n2)) ||
        (rc = S.in(oHead, &head, sizeof(head))) || (rc = S.in(oS, sets, setsBytes)) || (rc = S.in(oState, state, sizeof(sslam_sim3_state)))) return rc;
    if (tap) SSLAM_HIP(hipMemsetAsync(d + oTS, 0, L.size() - oTS, S.st));      // rows of iterations the loop did not run stay zero
    Sim3Args A;
    A.kp = (const sslam_keypoint*)(d + oK); A.x3dc = (const float*)(d + oX); A.valid = hasValid ? d + oV : nullptr; A.n = (const int32_t*)(d + oHead);
    A.K = (const float*)(d + oHead + 16); A.pairs = (const int32_t*)(d + oHead + 8); A.m12 = (const int32_t*)(d + oM); A.table = nullptr;
    A.sets = sets ? (const int32_t*)(d + oS) : nullptr;
    A.cap = cap; A.nkeyframes = 2; A.nlevels = nlevels; A.fixScale = fix_scale; A.minInliers = min_inliers; A.maxIterations = max_iterations; A.newIterations = new_iterations;
    A.pair0 = pair; A.seed = seed;
    A.state = (sslam_sim3_state*)(d + oState); A.inl = d + oI;
    A.tapSets = tap ? (int32_t*)(d + oTS) : nullptr; A.tapMats = tap ? (float*)(d + oTM) : nullptr; A.tapCounts = tap ? (int32_t*)(d + oTC) : nullptr;
    if ((rc = sim3_enqueue(ctx, A, level_sigma2, probability, 1, tap, S.st)) || (rc = S.out(state, oState, sizeof(sslam_sim3_state))) || (rc = S.out(inliers, oI, (size_t)n1))) return rc;
    if (tap && ((rc = S.out(sets_out, oTS, setsBytes)) || (rc = S.out(mats_out, oTM, matsBytes)) || (rc = S.out(counts_out, oTC, countsBytes)))) return rc;
    return S.done();
}

}  // namespace

extern "C" int sslam_sim3_ransac_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp, const float* d_x3dc, const uint8_t* d_valid, const int32_t* d_n, int cap, int nkeyframes,
                                           const float* d_K, const float* level_sigma2, int nlevels, const int32_t* d_pairs, int npairs, const int32_t* d_matches12,
                                           int fix_scale, double probability, int min_inliers, int max_iterations, int new_iterations, const int32_t* d_sets, uint32_t seed,
                                           sslam_sim3_state* d_state, uint8_t* d_inliers, void* stream) {
    if (!ctx || !d_kp || !d_x3dc || !d_n || !d_K || !d_pairs || !d_matches12 || !d_state || !d_inliers || cap < 1 || nkeyframes < 0 || npairs < 0 ||
        !sim3_params_ok(level_sigma2, nlevels, probability, min_inliers, max_iterations, new_iterations) ||
        !all_aligned<4>(d_kp) || !all_aligned<4>(d_x3dc, d_K) || !all_aligned<4>(d_n, d_pairs, d_matches12, d_sets) || !all_aligned<4>(d_state) ||
        !fits_31_bits(npairs, cap) || !fits_31_bits(nkeyframes, cap) || !injected_sets_ok(d_sets, npairs, max_iterations)) {
        set_error("sslam_sim3_ransac_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (cap > SIM3_MAX_CAP) { set_error("sslam_sim3_ransac_batch_dev: cap=%d exceeds the supported %d (48 bytes of LDS per row)", cap, SIM3_MAX_CAP); return SSLAM_ERR_UNSUPPORTED; }
    if (npairs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    Sim3Args A;
    A.kp = d_kp; A.x3dc = d_x3dc; A.valid = d_valid; A.n = d_n; A.K = d_K; A.pairs = d_pairs; A.m12 = d_matches12; A.table = nullptr; A.sets = d_sets;
    A.cap = cap; A.nkeyframes = nkeyframes; A.nlevels = nlevels; A.fixScale = fix_scale; A.minInliers = min_inliers; A.maxIterations = max_iterations; A.newIterations = new_iterations;
    A.pair0 = 0; A.seed = seed; A.state = d_state; A.inl = d_inliers; A.tapSets = nullptr; A.tapMats = nullptr; A.tapCounts = nullptr;
    return sim3_enqueue(ctx, A, level_sigma2, probability, npairs, false, pick(ctx, stream));
}

extern "C" int sslam_sim3_ransac(sslam_ctx* ctx, const sslam_keypoint* kp1, const float* x3dc1, const uint8_t* valid1, int n1, const float K1[4],
                                 const sslam_keypoint* kp2, const float* x3dc2, const uint8_t* valid2, int n2, const float K2[4], const float* level_sigma2, int nlevels,
                                 const int32_t* matches12, int fix_scale, double probability, int min_inliers, int max_iterations, int new_iterations, const int32_t* sets,
                                 uint32_t seed, sslam_sim3_state* state, uint8_t* inliers) {
    return sim3_host_pair(ctx, "sslam_sim3_ransac", kp1, x3dc1, valid1, n1, K1, kp2, x3dc2, valid2, n2, K2, level_sigma2, nlevels, matches12, fix_scale, probability, min_inliers,
                          max_iterations, new_iterations, sets, seed, 0, state, inliers, nullptr, nullptr, nullptr);
}

#ifdef SSLAM_TESTING
#include "../../include/sslam_testing.h"
extern "C" int sslam_testing_sim3_hypotheses(sslam_ctx* ctx, const sslam_keypoint* kp1, const float* x3dc1, const uint8_t* valid1, int n1, const float K1[4],
                                             const sslam_keypoint* kp2, const float* x3dc2, const uint8_t* valid2, int n2, const float K2[4], const float* level_sigma2,
                                             int nlevels, const int32_t* matches12, int fix_scale, double probability, int min_inliers, int max_iterations, int new_iterations,
                                             const int32_t* sets, uint32_t seed, int pair, sslam_sim3_state* state, uint8_t* inliers,
                                             int32_t* sets_out, float* mats_out, int32_t* counts_out) {
    if (!sets_out || !mats_out || !counts_out) { set_error("sslam_testing_sim3_hypotheses: invalid arguments"); return SSLAM_ERR_INVALID; }
    return sim3_host_pair(ctx, "sslam_testing_sim3_hypotheses", kp1, x3dc1, valid1, n1, K1, kp2, x3dc2, valid2, n2, K2, level_sigma2, nlevels, matches12, fix_scale, probability,
                          min_inliers, max_iterations, new_iterations, sets, seed, pair, state, inliers, sets_out, mats_out, counts_out);
}
#endif
