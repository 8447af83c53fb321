// PnPsolver for MI355X (gfx950): the pose RANSAC of Tracking::Relocalization (reference src/Tracking.cc:2004-2030) between SearchByBoW (:1996) and SearchByProjection
// (:2071, :2085) -- device side of reference src/PnPsolver.cc.  The arithmetic is csrc/pnp_math.h, shared with the host model tests/sim/pnp_sim.cpp; this unit is the kernel
// around it and its entry points.
//
// k_pnp_ransac: one wave per (keyframe slot, frame slot) pair.
//   1. the pair's correspondences (the constructor's filters, :79-101) are compacted into 24-byte rows in LDS, ascending frame row (ballot + popcount prefix: for_rows,
//      pair_rows.h): Xw, pt, maxErr
//   2. a round is 64 iterations, its_done + lane: every lane draws or reads its set, runs EPnP on the four points (every run-time index of the solvers addresses the lane's
//      workspace in LDS, lane-interleaved, never a private array) and walks all rows in order (all lanes read the same row: a broadcast), keeping its count and its double R, t
//   3. iterate's control flow (:209-238) over the round: the qualifying lanes (count >= min_inliers) in ascending order.  One whose count is strictly greater than every
//      earlier one (the state's included) becomes the best; Refine is a pure function of the best set, so it runs only where the best changes, or where the state remembers
//      a success that has to be returned again (refine_ok); the first success is the return
//   4. Refine (:260-305): the best R, t are uniform; CheckInliers per row by all lanes gives the set as one bit per row in LDS; all lanes run EPnP on that set alike (the
//      same list order, the same bits, each in its own workspace: every branch is uniform and every row read a broadcast); CheckInliers again gives the refined set
//   5. the inlier bytes of a return are recomputed from the returned R, t by all lanes, by frame row
// Every output word has one writer; no atomics.
#include "common.h"
#include "match_check.h"
#include "pair_rows.h"
#include "pnp_math.h"
#include <algorithm>

using namespace sslam;

namespace {

constexpr int PNP_LANES = RANSAC_LANES;
constexpr int PNP_MAX_LEVELS = 64;
constexpr int PNP_SINGLE_CAP_STEP = 512;      // sslam_pnp_ransac: the capacity it runs its one pair at
static_assert(sizeof(pnp::Row) == PNP_ROW_BYTES, "a correspondence is three 8-byte words: pnp_plan (match_plan.h) sizes this kernel's LDS");
static_assert(pnp::WS_DOUBLES == PNP_WS_DOUBLES, "pnp_plan (match_plan.h) sizes the workspace of pnp_math.h");
static_assert(sizeof(sslam_pnp_state) == 192, "sslam_pnp_state has no padding");

struct PnpArgs {
    const sslam_keypoint* fkp; const int32_t* nf; const float* fK; const float* xw; const uint8_t* kfValid; const int32_t* nkf;
    const int32_t* pairKf; const int32_t* pairF; const int32_t* assigned; const int32_t* table; const int32_t* sets;
    int cap, nframes, kfcap, nkeyframes, nlevels, nsets, newIterations, pair0;
    uint32_t seed;
    sslam_pnp_state* state; uint8_t* inl;
    int tapRows; int32_t* tapSets; double* tapPoses; int32_t* tapCounts; double* tapTrace;      // sslam_testing_pnp_hypotheses only
    float maxErr[PNP_MAX_LEVELS];                                  // pnp::max_error of every level, from the host's level_sigma2
};

struct LdsRows {
    const float2* r;
    __device__ __forceinline__ pnp::Row operator()(int i) const {
        const float2 a = r[3 * i], b = r[3 * i + 1], c = r[3 * i + 2];
        return pnp::Row{{a.x, a.y, b.x}, b.y, c.x, c.y};
    }
};
struct LdsMask {
    const unsigned long long* m;
    __device__ __forceinline__ unsigned long long operator()(int w) const { return m[w]; }
};
struct LdsWs {      // pnp::WS_DOUBLES doubles of this lane, lane-interleaved
    double* base;
    __device__ __forceinline__ double& at(int k) { return base[k * PNP_LANES]; }
};

// the constructor's filters for frame row j (:81-99): the keyframe row, or -1
struct Match {
    const sslam_keypoint* kp; const int32_t* assigned; const uint8_t* valid;
    int nf, nkf, nlevels;
    __device__ __forceinline__ int operator()(int j) const {
        if (j >= nf) return -1;
        const int a = assigned[j];
        if (a < 0 || a >= nkf) return -1;
        if (valid && !valid[a]) return -1;
        const int o = kp[j].octave;
        return (o >= 0 && o < nlevels) ? a : -1;
    }
};

__device__ __forceinline__ void broadcast(pnp::Pose& h, int src) {
#pragma unroll
    for (int k = 0; k < 9; ++k) h.R[k] = __shfl(h.R[k], src, 64);
#pragma unroll
    for (int k = 0; k < 3; ++k) h.t[k] = __shfl(h.t[k], src, 64);
}

// CheckInliers (:308-339) with the uniform pose h, 64 rows a step: the count, and with `mask` the set as one bit per row
__device__ __forceinline__ int check_all(const LdsRows& R, int N, const pnp::Cam& K, const pnp::Pose& h, int lane, unsigned long long* mask) {
    int count = 0;
    for (int i0 = 0; i0 < N; i0 += PNP_LANES) {
        const int i = i0 + lane;
        const bool in = i < N && pnp::check_row(h, K, R(i));
        const unsigned long long m = __ballot(in);
        if (mask && lane == 0) mask[i0 >> 6] = m;
        count += __popcll(m);
    }
    return count;
}

template <bool TAP>
__global__ __launch_bounds__(PNP_LANES) void k_pnp_ransac(PnpArgs A) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = threadIdx.x, p = blockIdx.x, cap = A.cap;
    const int kf = A.pairKf ? A.pairKf[p] : p, f = A.pairF ? A.pairF[p] : p;
    sslam_pnp_state* S = A.state + p;
    if (kf < 0 || kf >= A.nkeyframes || f < 0 || f >= A.nframes) {      // a skipped pair
        if (lane == 0) { S->n = 0; S->min_inliers = 0; S->max_its = 0; S->found = 0; S->found_it = -1; S->n_inliers = 0; S->no_more = 1; }
        return;
    }
    const size_t bf = (size_t)f * cap, bk = (size_t)kf * A.kfcap, bp = (size_t)p * cap;
    Match M;
    M.kp = A.fkp + bf; M.assigned = A.assigned + bp; M.valid = A.kfValid ? A.kfValid + bk : nullptr;
    M.nf = slot_count(A.nf, f, cap); M.nkf = slot_count(A.nkf, kf, A.kfcap); M.nlevels = A.nlevels;
    const float* Xw = A.xw + 3 * bk;
    const pnp::Cam K{A.fK[4 * f], A.fK[4 * f + 1], A.fK[4 * f + 2], A.fK[4 * f + 3]};      // :104-107: doubles made from the frame's floats
    float2* rows = (float2*)lds;
    LdsWs ws{(double*)(lds + (size_t)PNP_ROW_BYTES * cap) + lane};
    unsigned long long* mask = (unsigned long long*)(lds + (size_t)PNP_ROW_BYTES * cap + PNP_WS_BYTES);

    // 1. mvP3Dw, mvP2D, mvMaxError in mvKeyPointIndices' order
    const int N = for_rows(M.nf, lane, M, [&](int j, int a, int slot) {
        if (slot < 0) return;
        float2* r = rows + 3 * slot;
        r[0] = make_float2(Xw[3 * (size_t)a], Xw[3 * (size_t)a + 1]);
        r[1] = make_float2(Xw[3 * (size_t)a + 2], M.kp[j].x);
        r[2] = make_float2(M.kp[j].y, A.maxErr[M.kp[j].octave]);
    });
    __syncthreads();
    const LdsRows R{rows};

    // the solver object (:67-69): a zero-filled state is a new one
    int itsDone = max(S->its_done, 0), bestInliers = S->best_inliers, bestIt = itsDone == 0 ? -1 : S->best_it, refineOk = S->refine_ok != 0;
    pnp::Pose best, ret;
#pragma unroll
    for (int k = 0; k < 9; ++k) best.R[k] = S->best_R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) best.t[k] = S->best_t[k];
    pnp::zero_pose(ret);

    const int minInliers = A.table[2 * N], maxIts = A.table[2 * N + 1];
    int found = 0, foundIt = -1, nInliers = 0, noMore = 0;
    const bool iterates = N >= minInliers;      // :173-177
    if (iterates) {
        const int end = max(maxIts, itsDone + A.newIterations);      // :182: an OR
        bool refineKnown = false;      // whether Refine of the current best ran in this call: refCount / refined are its outcome
        int refCount = 0;
        pnp::Pose refined;
        pnp::zero_pose(refined);
        // 2. / 3.
        for (int r0 = itsDone; r0 < end && !found; r0 += PNP_LANES) {
            const int it = r0 + lane;
            const bool active = it < end;
            int set[4] = {-1, -1, -1, -1};
            bool valid = active;
            if (active) {
                if (A.sets) {
                    if (it < A.nsets) {
                        const int32_t* s = A.sets + ((size_t)p * A.nsets + it) * 4;
#pragma unroll
                        for (int j = 0; j < 4; ++j) { set[j] = s[j]; valid = valid && set[j] >= 0 && set[j] < N; }
                    } else {
                        valid = false;
                    }
                } else if (N >= 4) {
                    draw_set<4>(A.seed, (uint32_t)(A.pair0 + p), (uint32_t)it, N, set);
                } else {
                    valid = false;
                }
            }
            pnp::Pose h;
            pnp::Trace tr;
            const int count = pnp::hypothesis(R, N, K, set, valid, ws, h, tr, [](int, bool) {});
            unsigned long long qual = __ballot(active && count >= minInliers);      // :209
            int last = PNP_LANES - 1;      // the last lane whose iteration the reference's loop ran
            while (qual && !found) {
                const int l = __ffsll((long long)qual) - 1;
                qual &= qual - 1;
                const int c = __shfl(count, l, 64);
                const bool newBest = c > bestInliers;      // :212
                if (newBest) {
                    bestInliers = c; bestIt = r0 + l;
                    best = h;
                    broadcast(best, l);
                    refineKnown = false;
                }
                if (!refineKnown && (newBest || refineOk || TAP)) {
                    // 4. Refine (:260-305) on the best set
                    const int n = check_all(R, N, K, best, lane, mask);
                    __syncthreads();
                    const pnp::MaskedPts<LdsRows, LdsMask> P{R, LdsMask{mask}, N, n};
                    pnp::Trace rtr;
                    pnp::compute_pose(P, K, ws, refined, rtr);
                    refCount = check_all(R, N, K, refined, lane, nullptr);
                    __syncthreads();
                    refineOk = refCount > minInliers;      // :292
                    refineKnown = true;
                }
                if (TAP) {
                    if (lane == l && it < A.tapRows) { A.tapCounts[(size_t)it * 4 + 2] = 1; A.tapCounts[(size_t)it * 4 + 3] = refCount; }
                }
                if (refineOk) { found = 1; foundIt = r0 + l; nInliers = refCount; ret = refined; last = l; }      // :226-236
            }
            if (TAP) {
                if (active && lane <= last && it < A.tapRows) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) A.tapSets[(size_t)it * 4 + j] = set[j];
                    double* o = A.tapPoses + (size_t)it * 12;
#pragma unroll
                    for (int k = 0; k < 9; ++k) o[k] = h.R[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) o[9 + k] = h.t[k];
                    A.tapCounts[(size_t)it * 4] = count; A.tapCounts[(size_t)it * 4 + 1] = tr.N | (tr.flags << 8);
                    double* q = A.tapTrace + (size_t)it * 15;
#pragma unroll
                    for (int k = 0; k < 3; ++k) q[k] = tr.rep[k];
#pragma unroll
                    for (int k = 0; k < 12; ++k) q[3 + k] = tr.betas[k / 4][k % 4];
                }
            }
            itsDone = found ? foundIt + 1 : min(r0 + PNP_LANES, end);
        }
        if (!found && itsDone >= maxIts) {      // :241-255
            noMore = 1;
            if (bestInliers >= minInliers) { found = 2; foundIt = bestIt; nInliers = bestInliers; ret = best; }
        }
    } else {
        noMore = 1;
    }

    if (lane == 0) {
        S->n = N; S->min_inliers = minInliers; S->max_its = maxIts; S->found = found; S->found_it = foundIt; S->n_inliers = nInliers; S->no_more = noMore;
        if (iterates) {
            S->its_done = itsDone; S->best_inliers = bestInliers; S->best_it = bestIt; S->refine_ok = refineOk ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) S->best_R[k] = best.R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) S->best_t[k] = best.t[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {      // :217-223 / :294-300
#pragma unroll
            for (int c = 0; c < 3; ++c) S->Tcw[k * 4 + c] = found ? (float)ret.R[k * 3 + c] : 0.f;
            S->Tcw[k * 4 + 3] = found ? (float)ret.t[k] : 0.f;
        }
    }

    // 5. vbInliers (:229-234, :247-252) by frame row; rows [nf, cap) are not written
    for_rows(M.nf, lane, M, [&](int j, int, int slot) {
        uint8_t b = 0;
        if (slot >= 0 && found) b = pnp::check_row(ret, K, R(slot)) ? 1 : 0;
        if (j < M.nf) A.inl[bp + j] = b;
    });
}

// (mRansacMinInliers, mRansacMaxIts) for every N in [0, cap] (SetRansacParameters, :121-152, on the host with libm), cap + 1 pairs of int32 on the device.  Rebuilt only when
// its key changes; ordered like the Sim3 table (sim3.hip): a rebuild waits on the host for the last kernel that read the old table, the upload and the kernel that reads it
// are ordered by the stream, and a later call on another stream waits on the device for the event behind them (StreamOrderedBuf).
int pnp_table(sslam_ctx* ctx, double probability, int minInliers, int maxIterations, float epsilon, int cap, hipStream_t st) {
    sslam_ctx::PnpTable& T = ctx->pnpTable;
    const bool same = T.built && T.probability == probability && T.minInliers == minInliers && T.maxIterations == maxIterations && T.epsilon == epsilon && T.cap == cap;
    const size_t bytes = 2 * sizeof(int32_t) * ((size_t)cap + 1);
    if (same) return T.dev.acquire(st, bytes);
    if (T.dev.done) SSLAM_HIP(hipEventSynchronize(T.dev.done));
    int rc;
    if ((rc = T.host.ensure(bytes)) || (rc = T.dev.acquire(st, bytes))) return rc;
    int32_t* h = T.host.as<int32_t>();
    for (int n = 0; n <= cap; ++n) pnp::ransac_params(probability, minInliers, maxIterations, epsilon, n, h[2 * n], h[2 * n + 1]);
    SSLAM_HIP(hipMemcpyAsync(T.dev.as<int32_t>(), h, bytes, hipMemcpyHostToDevice, st));
    T.built = true; T.probability = probability; T.minInliers = minInliers; T.maxIterations = maxIterations; T.epsilon = epsilon; T.cap = cap;
    return SSLAM_OK;
}

int pnp_enqueue(sslam_ctx* ctx, PnpArgs& A, const float* level_sigma2, double probability, int minInliers, int maxIterations, float epsilon, float th2, int npairs, bool tap,
                hipStream_t st) {
    for (int l = 0; l < PNP_MAX_LEVELS; ++l) A.maxErr[l] = l < A.nlevels ? pnp::max_error(level_sigma2[l], th2) : 0.f;
    int rc;
    if ((rc = pnp_table(ctx, probability, minInliers, maxIterations, epsilon, A.cap, st))) return rc;
    A.table = ctx->pnpTable.dev.as<int32_t>();
    const RansacPlan P = pnp_plan(A.cap);
    if ((rc = launch_tapped(ctx, "k_pnp_ransac", SSLAM_WITH_TAP(k_pnp_ransac), tap, (unsigned)npairs, P.threads, P.ldsBytes, st, A))) return rc;
    return ctx->pnpTable.dev.mark(st);
}

// one host pair on the device and back, as frame slot 0 against keyframe slot 0: shared by the single call and the testing tap
int pnp_host_pair(sslam_ctx* ctx, const char* fn, const sslam_keypoint* f_kp, int nf, const float* f_K, const float* kf_xw, const uint8_t* kf_valid, int nkf,
                  const float* level_sigma2, int nlevels, const int32_t* assigned, double probability, int min_inliers, int max_iterations, float epsilon, float th2,
                  int new_iterations, const int32_t* sets, int nsets, uint32_t seed, int pair, sslam_pnp_state* state, uint8_t* inliers,
                  int tap_rows, int32_t* sets_out, double* poses_out, int32_t* counts_out, double* trace_out) {
    if (!ctx || nf < 0 || nkf < 0 || !f_K || !state || (nf > 0 && (!f_kp || !assigned || !inliers)) || (nkf > 0 && !kf_xw) || pair < 0 || nsets < 0 || (nsets > 0 && !sets) ||
        tap_rows < 0 || !pnp_params_ok(level_sigma2, nlevels, probability, min_inliers, max_iterations, new_iterations, epsilon, th2) || (long long)nsets >= (1ll << 28)) {
        set_error("%s: invalid arguments", fn); return SSLAM_ERR_INVALID;
    }
    // the capacity is a key of the iteration table: rounded up, so that a caller who goes round its candidates with other row counts does not rebuild it every call
    const int cap = std::min((std::max(nf, 1) + PNP_SINGLE_CAP_STEP - 1) / PNP_SINGLE_CAP_STEP * PNP_SINGLE_CAP_STEP, std::max(nf, PNP_MAX_CAP)), kfcap = std::max(nkf, 1);
    if (cap > PNP_MAX_CAP) { set_error("%s: %d rows exceed the supported %d", fn, cap, PNP_MAX_CAP); return SSLAM_ERR_UNSUPPORTED; }
    const bool tap = sets_out != nullptr;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    const size_t rowsT = (size_t)tap_rows, setsBytes = 16 * (size_t)nsets;
    const size_t ks = sizeof(sslam_keypoint);
    ArenaLayout L;
    const size_t oK = L.take(ks * (size_t)cap), oX = L.take(12 * (size_t)kfcap), oV = L.take((size_t)kfcap), oHead = L.take(256), oA = L.take(4 * (size_t)cap),
                 oS = L.take(sets ? setsBytes : 0), oState = L.take(256), oI = L.take((size_t)cap),
                 oTS = L.take(tap ? 16 * rowsT : 0), oTP = L.take(tap ? 96 * rowsT : 0), oTC = L.take(tap ? 16 * rowsT : 0), oTT = L.take(tap ? 120 * rowsT : 0);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* d = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging S{d, ctx->stream};
    struct { int32_t nf, nkf; float K[4]; } head;      // the two counts, fx fy cx cy
    head.nf = nf; head.nkf = nkf;
    memcpy(head.K, f_K, 16);
    if ((rc = S.in(oK, f_kp, ks * (size_t)nf)) || (rc = S.in(oX, kf_xw, 12 * (size_t)nkf)) || (rc = S.in(oV, kf_valid, (size_t)nkf)) || (rc = S.in(oA, assigned, 4 * (size_t)nf)) ||
        (rc = S.in(oHead, &head, sizeof(head))) || (rc = S.in(oS, sets, setsBytes)) || (rc = S.in(oState, state, sizeof(sslam_pnp_state)))) return rc;
    if (tap && L.size() > oTS) SSLAM_HIP(hipMemsetAsync(d + oTS, 0, L.size() - oTS, S.st));      // rows of iterations the loop did not run stay zero
    PnpArgs A;
    A.fkp = (const sslam_keypoint*)(d + oK); A.nf = (const int32_t*)(d + oHead); A.fK = (const float*)(d + oHead + 8); A.xw = (const float*)(d + oX);
    A.kfValid = kf_valid ? d + oV : nullptr; A.nkf = (const int32_t*)(d + oHead + 4); A.pairKf = nullptr; A.pairF = nullptr; A.assigned = (const int32_t*)(d + oA);
    A.table = nullptr; A.sets = sets ? (const int32_t*)(d + oS) : nullptr;
    A.cap = cap; A.nframes = 1; A.kfcap = kfcap; A.nkeyframes = 1; A.nlevels = nlevels; A.nsets = nsets; A.newIterations = new_iterations; A.pair0 = pair; A.seed = seed;
    A.state = (sslam_pnp_state*)(d + oState); A.inl = d + oI;
    A.tapRows = tap ? tap_rows : 0; A.tapSets = tap ? (int32_t*)(d + oTS) : nullptr; A.tapPoses = tap ? (double*)(d + oTP) : nullptr;
    A.tapCounts = tap ? (int32_t*)(d + oTC) : nullptr; A.tapTrace = tap ? (double*)(d + oTT) : nullptr;
    if ((rc = pnp_enqueue(ctx, A, level_sigma2, probability, min_inliers, max_iterations, epsilon, th2, 1, tap, S.st)) || (rc = S.out(state, oState, sizeof(sslam_pnp_state))) ||
        (rc = S.out(inliers, oI, (size_t)nf))) return rc;
    if (tap && ((rc = S.out(sets_out, oTS, 16 * rowsT)) || (rc = S.out(poses_out, oTP, 96 * rowsT)) || (rc = S.out(counts_out, oTC, 16 * rowsT)) ||
                (rc = S.out(trace_out, oTT, 120 * rowsT)))) return rc;
    return S.done();
}

}  // namespace

extern "C" int sslam_pnp_ransac_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_f_kp, const int32_t* d_nf, int cap, int nframes, const float* d_f_K,
                                          const float* d_kf_xw, const uint8_t* d_kf_valid, const int32_t* d_nkf, int kfcap, int nkeyframes,
                                          const float* level_sigma2, int nlevels, const int32_t* d_pair_kf, const int32_t* d_pair_f, int npairs, const int32_t* d_assigned,
                                          double probability, int min_inliers, int max_iterations, float epsilon, float th2, int new_iterations,
                                          const int32_t* d_sets, int nsets, uint32_t seed, sslam_pnp_state* d_state, uint8_t* d_inliers, void* stream) {
    if (!ctx || !d_f_kp || !d_nf || !d_f_K || !d_kf_xw || !d_nkf || !d_assigned || !d_state || !d_inliers ||
        !pnp_params_ok(level_sigma2, nlevels, probability, min_inliers, max_iterations, new_iterations, epsilon, th2) ||
        !pnp_sizes_ok(npairs, cap, nframes, nkeyframes, kfcap, d_sets, nsets) || (!d_pair_kf && nkeyframes != npairs) || (!d_pair_f && nframes != npairs) ||
        !all_aligned<4>(d_f_kp) || !all_aligned<4>(d_f_K, d_kf_xw) || !all_aligned<4>(d_nf, d_nkf, d_pair_kf, d_pair_f, d_assigned, d_sets) || !all_aligned<8>(d_state)) {
        set_error("sslam_pnp_ransac_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (cap > PNP_MAX_CAP) { set_error("sslam_pnp_ransac_batch_dev: cap=%d exceeds the supported %d (24 bytes of LDS per row beside the EPnP workspace)", cap, PNP_MAX_CAP); return SSLAM_ERR_UNSUPPORTED; }
    if (npairs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    PnpArgs A;
    A.fkp = d_f_kp; A.nf = d_nf; A.fK = d_f_K; A.xw = d_kf_xw; A.kfValid = d_kf_valid; A.nkf = d_nkf; A.pairKf = d_pair_kf; A.pairF = d_pair_f; A.assigned = d_assigned;
    A.table = nullptr; A.sets = d_sets;
    A.cap = cap; A.nframes = nframes; A.kfcap = kfcap; A.nkeyframes = nkeyframes; A.nlevels = nlevels; A.nsets = d_sets ? nsets : 0; A.newIterations = new_iterations;
    A.pair0 = 0; A.seed = seed; A.state = d_state; A.inl = d_inliers;
    A.tapRows = 0; A.tapSets = nullptr; A.tapPoses = nullptr; A.tapCounts = nullptr; A.tapTrace = nullptr;
    return pnp_enqueue(ctx, A, level_sigma2, probability, min_inliers, max_iterations, epsilon, th2, npairs, false, pick(ctx, stream));
}

extern "C" int sslam_pnp_ransac(sslam_ctx* ctx, const sslam_keypoint* f_kp, int nf, const float f_K[4], const float* kf_xw, const uint8_t* kf_valid, int nkf,
                                const float* level_sigma2, int nlevels, const int32_t* assigned, double probability, int min_inliers, int max_iterations, float epsilon,
                                float th2, int new_iterations, const int32_t* sets, int nsets, uint32_t seed, sslam_pnp_state* state, uint8_t* inliers) {
    return pnp_host_pair(ctx, "sslam_pnp_ransac", f_kp, nf, f_K, kf_xw, kf_valid, nkf, level_sigma2, nlevels, assigned, probability, min_inliers, max_iterations, epsilon, th2,
                         new_iterations, sets, nsets, seed, 0, state, inliers, 0, nullptr, nullptr, nullptr, nullptr);
}

#ifdef SSLAM_TESTING
#include "../../include/sslam_testing.h"
extern "C" int sslam_testing_pnp_hypotheses(sslam_ctx* ctx, const sslam_keypoint* f_kp, int nf, const float f_K[4], const float* kf_xw, const uint8_t* kf_valid, int nkf,
                                            const float* level_sigma2, int nlevels, const int32_t* assigned, double probability, int min_inliers, int max_iterations,
                                            float epsilon, float th2, int new_iterations, const int32_t* sets, int nsets, uint32_t seed, int pair, sslam_pnp_state* state,
                                            uint8_t* inliers, int tap_rows, int32_t* sets_out, double* poses_out, int32_t* counts_out, double* trace_out) {
    if (!sets_out || !poses_out || !counts_out || !trace_out || tap_rows < 1) { set_error("sslam_testing_pnp_hypotheses: invalid arguments"); return SSLAM_ERR_INVALID; }
    return pnp_host_pair(ctx, "sslam_testing_pnp_hypotheses", f_kp, nf, f_K, kf_xw, kf_valid, nkf, level_sigma2, nlevels, assigned, probability, min_inliers, max_iterations,
                         epsilon, th2, new_iterations, sets, nsets, seed, pair, state, inliers, tap_rows, sets_out, poses_out, counts_out, trace_out);
}
#endif
