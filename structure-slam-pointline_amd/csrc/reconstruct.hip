// The second half of Initializer::Initialize for MI355X (gfx950): ReconstructH / ReconstructF with CheckRT and Triangulate, and ReconstructLine with LineTriangulate --
// device side of reference src/Initializer.cc:143-152, :499-782 and :833-1171, behind sslam_two_view_ransac_batch_dev's H21 / F21 and inlier bits.  The arithmetic is
// csrc/reconstruct_math.h, shared with the host model tests/sim/reconstruct_sim.cpp; this unit is the kernel around it and its entry points.
//
// k_reconstruct: one workgroup of RECON_WAVES waves per frame pair.
//   1. wave 0 compacts matches12 into (u1, v1, u2, v2) rows and the inlier byte of the pair's model in LDS, ascending keypoint-1 index (for_rows, pair_rows.h), and counts N
//   2. lane 0 decomposes E or A into the four or eight hypotheses (the one-sided Jacobi of the 3 x 3 on 18 doubles of LDS); lane h completes hypothesis h (P2, O2)
//   3. hypothesis after hypothesis, all lanes walk the rows: Triangulate's 4 x 4 goes through the lane's Jacobi workspace in LDS (lane-interleaved: double k of lane l is
//      word k * RECON_THREADS + l, so run-time indices make no private array and a half wave's 8-byte accesses hit 64 distinct banks), the accepted cosine is left as an
//      order-preserving key in the row's word of the key strip, nGood comes from ballots; wave 0 then selects element min(50, nGood - 1) of the strip by value
//      (rc::kth_key: 32 rounds of ballots over the strip) -- no sort, no per-hypothesis point buffers
//   4. lane 0 makes the reference's choice; the winner's CheckRT runs once more and leaves (x, y, z, good) in the row's own LDS words; wave 0 walks keypoint 1 again and
//      writes p3d and the triangulated byte of every row [0, n1)
//   5. the line tail with the winning R21 / t21: lanes over the pair's line pairs (two 4 x 4 solves each), the errors in LDS, wave 0 and wave 1 select the two medians of
//      one error each (64 rounds of ballots), then the flags
// Every output word has one writer; no atomics.
#include "common.h"
#include "match_check.h"
#include "pair_rows.h"
#include "reconstruct_math.h"
#include <algorithm>

using namespace sslam;

namespace {

constexpr int RC_THREADS = RECON_THREADS, RC_WAVES = RECON_WAVES;
static_assert(rc::WS4_DOUBLES == RECON_WS_DOUBLES && sizeof(float4) + sizeof(uint32_t) + 1 == RECON_ROW_BYTES && 2 * sizeof(double) == RECON_LINE_ROW_BYTES && RC_WAVES >= 2,
              "reconstruct_plan (match_plan.h) sizes this kernel's LDS; the two medians take two waves");

struct ReconArgs {
    const sslam_keypoint* kp1; const int32_t* n1;
    const sslam_keypoint* kp2; const int32_t* n2;
    const int32_t* m12; const sslam_two_view_result* res; const uint8_t* inl; const float* K;
    int cap, lcap, minTri; float sigma, minParallax;
    const sslam_keyline* kl1; const int32_t* nl1; const int32_t* nl2; const double* fn1; const double* fn2; const int32_t* lpairs; const int32_t* lnp;      // lpairs NULL: no lines
    sslam_two_view_pose* pose; float* p3d; uint8_t* tri; float* ls3d; float* le3d; uint8_t* ltri;
    size_t wsOff, lineOff, rowOff, keyOff, flagOff;      // reconstruct_plan's offsets
    float* tapHyp; float* tapSel; int32_t* tapStage; float* tapP3d; float* tapCos; double* tapLineErr;      // sslam_testing_two_view_reconstruct only
};

struct ReconShared {      // static LDS of the workgroup
    double ws3[rc::WS3_DOUBLES];
    rc::Hyp hyp[8];
    float nrm[8][3];
    int nGood[8]; float par[8], sel[8];
    int cntH[RC_WAVES], cntTri[RC_WAVES], cntLv[RC_WAVES], cntLt[RC_WAVES];
    double thr[2];
    int nm, N, nh, reason, ok, hypothesis;
};
static_assert(sizeof(ReconShared) <= RECON_STATIC_LDS, "reconstruct_plan (match_plan.h) leaves this much for the static words");

struct LdsWs4 {      // rc::WS4_DOUBLES doubles of this lane, lane-interleaved
    double* base;
    __device__ __forceinline__ double& at(int k) { return base[k * RC_THREADS]; }
};
struct LdsWs3 {
    double* base;
    __device__ __forceinline__ double& at(int k) { return base[k - pnp::WS_S]; }
};
struct Matches12 {      // mvMatches12 (:67-76) for keypoint-1 row i, as k_two_view reads it
    const int32_t* m12; int n1, n2;
    __device__ __forceinline__ int operator()(int i) const { const int m = i < n1 ? m12[i] : -1; return m >= 0 && m < n2 ? m : -1; }
};

// how many of the n keys are below t: the wave's ballots over the strip
template <class Key, class Get>
__device__ __forceinline__ int wave_count_below(int n, int lane, Key t, Get get) {
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool below = i < n && get(i) < t;
        c += __popcll(__ballot(below));
    }
    return c;
}

template <bool TAP>
__global__ __launch_bounds__(RC_THREADS) void k_reconstruct(ReconArgs A) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ ReconShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x, cap = A.cap;
    const size_t base = (size_t)p * cap;
    const int n1 = slot_count(A.n1, p, cap), n2 = slot_count(A.n2, p, cap);
    const sslam_keypoint* kp1 = A.kp1 + base;
    const sslam_keypoint* kp2 = A.kp2 + base;
    LdsWs4 ws{(double*)(lds + A.wsOff) + tid};
    double2* lerr = (double2*)(lds + A.lineOff);
    float4* rows = (float4*)(lds + A.rowOff);
    uint32_t* keys = (uint32_t*)(lds + A.keyOff);
    uint8_t* flags = lds + A.flagOff;
    const sslam_two_view_result* res = A.res + p;
    const int rm = res->model, model = rm == 1 || rm == 2 ? rm : 0;
    const rc::Cam K{A.K[(size_t)p * 4], A.K[(size_t)p * 4 + 1], A.K[(size_t)p * 4 + 2], A.K[(size_t)p * 4 + 3]};
    const Matches12 M{A.m12 + base, n1, n2};

    // 1. mvMatches12 (:67-76) and vbMatchesInliers of the model, by match; N (:504-507, :615-618)
    if (wave == 0) {
        const int bit = model == 1 ? 1 : 2;
        int N = 0;
        const int nm = for_rows(n1, lane, M, [&](int i, int m, int slot) {
            bool in = false;
            if (slot >= 0) {
                in = model != 0 && (A.inl[base + i] & bit);
                rows[slot] = make_float4(kp1[i].x, kp1[i].y, kp2[m].x, kp2[m].y);
                flags[slot] = in ? 1 : 0;
            }
            N += __popcll(__ballot(in));
        });
        if (lane == 0) { S.nm = nm; S.N = N; }
    }
    // 2. the hypotheses
    if (tid == 0) {
        LdsWs3 w3{S.ws3};
        int nh = 0, reason = rc::REASON_OK;
        if (model == 0) reason = rc::REASON_SKIPPED;
        else if (model == 1) { if (rc::hypotheses_h(w3, res->H21, K, S.hyp, S.nrm)) nh = 8; else reason = rc::REASON_NOT_SEPARATED; }
        else { rc::hypotheses_f(w3, res->F21, K, S.hyp); nh = 4; }
        S.nh = nh; S.reason = reason; S.ok = 0; S.hypothesis = -1;
        if (model != 1) for (int h = 0; h < 8; ++h) for (int k = 0; k < 3; ++k) S.nrm[h][k] = 0.f;
        if (model == 0) for (int h = 0; h < 8; ++h) { for (int k = 0; k < 9; ++k) S.hyp[h].R[k] = 0.f; for (int k = 0; k < 3; ++k) S.hyp[h].t[k] = 0.f; }
        if (model == 2) for (int h = 4; h < 8; ++h) { for (int k = 0; k < 9; ++k) S.hyp[h].R[k] = 0.f; for (int k = 0; k < 3; ++k) S.hyp[h].t[k] = 0.f; }
    }
    if (tid < 8) { S.nGood[tid] = 0; S.par[tid] = 0.f; S.sel[tid] = 0.f; }
    __syncthreads();
    const int nm = S.nm, nh = S.nh;
    if (tid < nh) rc::hyp_setup(K, S.hyp[tid]);
    __syncthreads();

    // 3. CheckRT (:833-961) per hypothesis
    const float th2 = rc::th2_of(A.sigma);
    for (int h = 0; h < nh; ++h) {
        const rc::Hyp H = S.hyp[h];
        int cnt = 0;
        for (int s0 = 0; s0 < nm; s0 += RC_THREADS) {
            const int slot = s0 + tid;
            rc::RowOut o;
            o.stage = rc::STAGE_NOT_INLIER; o.cosv = 0.f; o.p3d[0] = o.p3d[1] = o.p3d[2] = 0.f;
            if (slot < nm && flags[slot]) {
                const float4 r = rows[slot];
                rc::check_row(K, H, r.x, r.y, r.z, r.w, th2, ws, o);
            }
            const bool good = o.stage == rc::STAGE_GOOD;
            if (slot < nm) keys[slot] = good ? rc::key_of(o.cosv) : rc::KEY32_ABSENT;
            cnt += __popcll(__ballot(good));
            if (TAP && slot < nm) {
                const size_t q = (size_t)h * cap + slot;
                A.tapStage[q] = o.stage; A.tapCos[q] = o.stage >= rc::STAGE_Z1 ? o.cosv : 0.f;
                for (int k = 0; k < 3; ++k) A.tapP3d[q * 3 + k] = o.stage >= rc::STAGE_NOT_FINITE ? o.p3d[k] : 0.f;
            }
        }
        if (lane == 0) S.cntH[wave] = cnt;
        __syncthreads();
        if (wave == 0) {
            int nGood = 0;
            for (int w = 0; w < RC_WAVES; ++w) nGood += S.cntH[w];
            float sel = 0.f, par = 0.f;
            if (nGood > 0) {      // :947-956
                const int k = nGood - 1 < 50 ? nGood - 1 : 50;
                sel = rc::value_of(rc::kth_key<uint32_t>(k, [&](uint32_t t) { return wave_count_below(nm, lane, t, [&](int i) { return keys[i]; }); }));
                par = rc::parallax_of(sel);
            }
            if (lane == 0) { S.nGood[h] = nGood; S.sel[h] = sel; S.par[h] = par; }
        }
        __syncthreads();
    }

    // 4. the choice (:532-607, :731-780), the winner's points
    if (tid == 0) {
        rc::Choice c{0, S.reason, -1};
        if (nh == 4) c = rc::choose_f(S.nGood, S.par, S.N, A.minParallax, A.minTri);
        if (nh == 8) c = rc::choose_h(S.nGood, S.par, S.N, A.minParallax, A.minTri);
        S.ok = c.ok; S.reason = c.reason; S.hypothesis = c.hypothesis;
    }
    __syncthreads();
    const int ok = S.ok, win = ok ? S.hypothesis : 0;
    const rc::Hyp H = S.hyp[win];
    {
        int cnt = 0;
        for (int s0 = 0; s0 < nm; s0 += RC_THREADS) {
            const int slot = s0 + tid;
            bool good = false;
            if (ok && slot < nm && flags[slot]) {
                const float4 r = rows[slot];
                rc::RowOut o;
                rc::check_row(K, H, r.x, r.y, r.z, r.w, th2, ws, o);
                good = o.stage == rc::STAGE_GOOD;
                if (good) rows[slot] = make_float4(o.p3d[0], o.p3d[1], o.p3d[2], 1.f);
            }
            if (slot < nm && !good) rows[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
            cnt += __popcll(__ballot(good));
        }
        if (lane == 0) S.cntTri[wave] = cnt;
    }
    __syncthreads();
    if (wave == 0) {      // vP3D / vbTriangulated by keypoint 1: rows [0, n1)
        float* p3d = A.p3d + base * 3;
        uint8_t* tri = A.tri + base;
        for_rows(n1, lane, M, [&](int i, int, int slot) {
            if (i >= n1) return;
            const float4 r = slot >= 0 ? rows[slot] : make_float4(0.f, 0.f, 0.f, 0.f);
            p3d[(size_t)i * 3] = r.x; p3d[(size_t)i * 3 + 1] = r.y; p3d[(size_t)i * 3 + 2] = r.z;
            tri[i] = r.w != 0.f ? 1 : 0;
        });
    }

    // 5. ReconstructLine (:1059-1171)
    int nLines = 0, nLinesTri = 0;
    if (A.lpairs) {
        const int lcap = A.lcap;
        const size_t lbase = (size_t)p * lcap;
        const int nl1 = slot_count(A.nl1, p, lcap), nl2 = slot_count(A.nl2, p, lcap), nlp = slot_count(A.lnp, p, lcap);
        const int32_t* lp = A.lpairs + lbase * 2;
        int cnt = 0;
        for (int r0 = 0; r0 < nlp; r0 += RC_THREADS) {
            const int r = r0 + tid;
            bool valid = false;
            if (r < nlp) {
                const int a = lp[(size_t)r * 2], b = lp[(size_t)r * 2 + 1];
                valid = a >= 0 && a < nl1 && b >= 0 && b < nl2;
                rc::LineOut o;
                o.err1 = o.err2 = 0.0;
                for (int k = 0; k < 3; ++k) o.s3d[k] = o.e3d[k] = 0.f;
                if (valid && ok) {
                    const sslam_keyline& kl = A.kl1[lbase + a];
                    const float e[4] = {kl.startPointX, kl.startPointY, kl.endPointX, kl.endPointY};
                    const double* f1 = A.fn1 + (lbase + a) * 3;
                    const double* f2 = A.fn2 + (lbase + b) * 3;
                    const double g1[3] = {f1[0], f1[1], f1[2]}, g2[3] = {f2[0], f2[1], f2[2]};
                    rc::line_row(K, H, e, g1, g2, ws, o);
                }
                lerr[r] = valid ? make_double2(o.err1, o.err2) : make_double2(-1.0, -1.0);      // an error is a norm or a NaN: -1 marks a row that is not in the list
                for (int k = 0; k < 3; ++k) { A.ls3d[(lbase + r) * 3 + k] = o.s3d[k]; A.le3d[(lbase + r) * 3 + k] = o.e3d[k]; }
                if (TAP) { A.tapLineErr[(size_t)r * 2] = o.err1; A.tapLineErr[(size_t)r * 2 + 1] = o.err2; }
            }
            cnt += __popcll(__ballot(valid));
        }
        if (lane == 0) S.cntLv[wave] = cnt;
        __syncthreads();
        for (int w = 0; w < RC_WAVES; ++w) nLines += S.cntLv[w];
        if (wave < 2) {      // vector_mad of errorC1 (wave 0) and errorC2 (wave 1)
            double thr = 0.0;
            if (ok && nLines > 0) {
                const int k = nLines / 2;
                auto err = [&](int i) { const double2 e = lerr[i]; return wave == 0 ? e.x : e.y; };
                const double med = rc::value_of(rc::kth_key<uint64_t>(k, [&](uint64_t t) {
                    return wave_count_below(nlp, lane, t, [&](int i) { const double e = err(i); return e < 0.0 ? rc::KEY64_ABSENT : rc::key_of(e); }); }));
                const double mad = rc::value_of(rc::kth_key<uint64_t>(k, [&](uint64_t t) {
                    return wave_count_below(nlp, lane, t, [&](int i) { const double e = err(i); return e < 0.0 ? rc::KEY64_ABSENT : rc::key_of(rc::abs_dev(e, med)); }); }));
                thr = rc::inlier_threshold(mad);
            }
            if (lane == 0) S.thr[wave] = thr;
        }
        __syncthreads();
        const double thr1 = S.thr[0], thr2 = S.thr[1];
        cnt = 0;
        for (int r0 = 0; r0 < nlp; r0 += RC_THREADS) {
            const int r = r0 + tid;
            bool t = false;
            if (r < nlp) {
                const double2 e = lerr[r];
                t = ok && !(e.x < 0.0) && !(e.x > thr1 || e.y > thr2);
                A.ltri[lbase + r] = t ? 1 : 0;
            }
            cnt += __popcll(__ballot(t));
        }
        if (lane == 0) S.cntLt[wave] = cnt;
        __syncthreads();
        for (int w = 0; w < RC_WAVES; ++w) nLinesTri += S.cntLt[w];
    }

    if (tid == 0) {
        sslam_two_view_pose o;
        o.ok = ok; o.reason = S.reason; o.model = model; o.hypothesis = S.hypothesis; o.n_inliers = S.N;
        for (int h = 0; h < 8; ++h) { o.n_good[h] = S.nGood[h]; o.parallax[h] = S.par[h]; }
        for (int k = 0; k < 9; ++k) o.R21[k] = ok ? H.R[k] : 0.f;
        for (int k = 0; k < 3; ++k) o.t21[k] = ok ? H.t[k] : 0.f;
        int nTri = 0;
        for (int w = 0; w < RC_WAVES; ++w) nTri += S.cntTri[w];
        o.n_triangulated = nTri; o.n_lines = nLines; o.n_lines_triangulated = nLinesTri;
        A.pose[p] = o;
        if (TAP) {
            for (int h = 0; h < 8; ++h) {
                for (int k = 0; k < 9; ++k) A.tapHyp[h * 15 + k] = S.hyp[h].R[k];
                for (int k = 0; k < 3; ++k) { A.tapHyp[h * 15 + 9 + k] = S.hyp[h].t[k]; A.tapHyp[h * 15 + 12 + k] = S.nrm[h][k]; }
                A.tapSel[h] = S.sel[h];
            }
        }
    }
}

int reconstruct_launch(sslam_ctx* ctx, ReconArgs& A, int npairs, bool tap, hipStream_t st) {
    const ReconstructPlan P = reconstruct_plan(A.cap, A.lpairs ? A.lcap : 0);
    A.wsOff = P.wsOff; A.lineOff = P.lineOff; A.rowOff = P.rowOff; A.keyOff = P.keyOff; A.flagOff = P.flagOff;
    return launch_tapped(ctx, "k_reconstruct", SSLAM_WITH_TAP(k_reconstruct), tap, (unsigned)npairs, P.threads, P.ldsBytes, st, A);
}

struct ReconTap { float* hyp; float* sel; int32_t* stage; float* p3dRows; float* cosv; double* lineErr; };

// one host pair on the device and back: shared by the single call and the testing tap
int reconstruct_host_pair(sslam_ctx* ctx, const char* fn, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12,
                          const sslam_two_view_result* result, const uint8_t* inliers, const float* K, float sigma, float minParallax, int minTri,
                          const sslam_keyline* kl1, int nl1, const sslam_keyline* kl2, int nl2, const double* fn1, const double* fn2, const int32_t* lpairs, int nlp,
                          sslam_two_view_pose* pose, float* p3d, uint8_t* tri, float* ls3d, float* le3d, uint8_t* ltri, const ReconTap* T) {
    const bool lines = lpairs != nullptr;
    bool okArgs = ctx && n1 >= 0 && n2 >= 0 && result && K && pose && reconstruct_params_ok(sigma, minTri) && !(n1 > 0 && (!kp1 || !matches12 || !inliers || !p3d || !tri)) &&
                  !(n2 > 0 && !kp2);
    if (lines) okArgs = okArgs && nl1 >= 0 && nl2 >= 0 && nlp >= 0 && !(nl1 > 0 && (!kl1 || !fn1)) && !(nl2 > 0 && !fn2) && !(nlp > 0 && (!ls3d || !le3d || !ltri));
    else okArgs = okArgs && !kl1 && !kl2 && !fn1 && !fn2 && !ls3d && !le3d && !ltri && nl1 == 0 && nl2 == 0 && nlp == 0;
    if (T) okArgs = okArgs && T->hyp && T->sel && T->stage && T->p3dRows && T->cosv && (!lines || nlp == 0 || T->lineErr);
    if (!okArgs) { set_error("%s: invalid arguments", fn); return SSLAM_ERR_INVALID; }
    const int cap = std::max(std::max(n1, n2), 1), lcap = std::max(std::max(nl1, nl2), std::max(nlp, 1));
    if (cap > RECON_MAX_CAP || (lines && lcap > RECON_MAX_LCAP)) {
        set_error("%s: %d keypoints / %d lines exceed the supported %d / %d", fn, cap, lines ? lcap : 0, RECON_MAX_CAP, RECON_MAX_LCAP); return SSLAM_ERR_UNSUPPORTED;
    }
    const bool tap = T != nullptr;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    const size_t c = (size_t)cap, l = lines ? (size_t)lcap : 0, ks = sizeof(sslam_keypoint), ls = sizeof(sslam_keyline);
    ArenaLayout L;
    const size_t oK1 = L.take(ks * c), oK2 = L.take(ks * c), oN = L.take(256), oM = L.take(4 * c), oR = L.take(sizeof(sslam_two_view_result)), oI = L.take(c), oK = L.take(16),
                 oL1 = L.take(ls * l), oF1 = L.take(24 * l), oF2 = L.take(24 * l), oLP = L.take(8 * l),
                 oPose = L.take(sizeof(sslam_two_view_pose)), oP3 = L.take(12 * c), oT = L.take(c), oS3 = L.take(12 * l), oE3 = L.take(12 * l), oLT = L.take(l),
                 oTH = L.take(tap ? 4 * 8 * 15 : 0), oTS = L.take(tap ? 4 * 8 : 0), oTG = L.take(tap ? 4 * 8 * c : 0), oTP = L.take(tap ? 12 * 8 * c : 0),
                 oTC = L.take(tap ? 4 * 8 * c : 0), oTL = L.take(tap ? 16 * l : 0);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* d = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging St{d, ctx->stream};
    const int hn[5] = {n1, n2, nl1, nl2, nlp};
    if ((rc = St.in(oK1, kp1, ks * (size_t)n1)) || (rc = St.in(oK2, kp2, ks * (size_t)n2)) || (rc = St.in(oN, hn, sizeof(hn))) || (rc = St.in(oM, matches12, 4 * (size_t)n1)) ||
        (rc = St.in(oR, result, sizeof(sslam_two_view_result))) || (rc = St.in(oI, inliers, (size_t)n1)) || (rc = St.in(oK, K, 16))) return rc;
    if (lines && ((rc = St.in(oL1, kl1, ls * (size_t)nl1)) || (rc = St.in(oF1, fn1, 24 * (size_t)nl1)) || (rc = St.in(oF2, fn2, 24 * (size_t)nl2)) ||
                  (rc = St.in(oLP, lpairs, 8 * (size_t)nlp)))) return rc;
    if (tap) SSLAM_HIP(hipMemsetAsync(d + oTH, 0, L.size() - oTH, St.st));      // rows past the match list, hypotheses that were not run
    ReconArgs A{};
    A.kp1 = (const sslam_keypoint*)(d + oK1); A.kp2 = (const sslam_keypoint*)(d + oK2); A.n1 = (const int32_t*)(d + oN); A.n2 = A.n1 + 1;
    A.m12 = (const int32_t*)(d + oM); A.res = (const sslam_two_view_result*)(d + oR); A.inl = d + oI; A.K = (const float*)(d + oK);
    A.cap = cap; A.lcap = lcap; A.minTri = minTri; A.sigma = sigma; A.minParallax = minParallax;
    if (lines) {
        A.kl1 = (const sslam_keyline*)(d + oL1); A.nl1 = A.n1 + 2; A.nl2 = A.n1 + 3; A.fn1 = (const double*)(d + oF1); A.fn2 = (const double*)(d + oF2);
        A.lpairs = (const int32_t*)(d + oLP); A.lnp = A.n1 + 4;
        A.ls3d = (float*)(d + oS3); A.le3d = (float*)(d + oE3); A.ltri = d + oLT;
    }
    A.pose = (sslam_two_view_pose*)(d + oPose); A.p3d = (float*)(d + oP3); A.tri = d + oT;
    if (tap) {
        A.tapHyp = (float*)(d + oTH); A.tapSel = (float*)(d + oTS); A.tapStage = (int32_t*)(d + oTG); A.tapP3d = (float*)(d + oTP); A.tapCos = (float*)(d + oTC);
        A.tapLineErr = (double*)(d + oTL);
    }
    if ((rc = reconstruct_launch(ctx, A, 1, tap, St.st)) || (rc = St.out(pose, oPose, sizeof(sslam_two_view_pose))) || (rc = St.out(p3d, oP3, 12 * (size_t)n1)) ||
        (rc = St.out(tri, oT, (size_t)n1))) return rc;
    if (lines && ((rc = St.out(ls3d, oS3, 12 * (size_t)nlp)) || (rc = St.out(le3d, oE3, 12 * (size_t)nlp)) || (rc = St.out(ltri, oLT, (size_t)nlp)))) return rc;
    if (tap && ((rc = St.out(T->hyp, oTH, 4 * 8 * 15)) || (rc = St.out(T->sel, oTS, 4 * 8)) || (rc = St.out(T->stage, oTG, 4 * 8 * c)) || (rc = St.out(T->p3dRows, oTP, 12 * 8 * c)) ||
                (rc = St.out(T->cosv, oTC, 4 * 8 * c)) || (lines && (rc = St.out(T->lineErr, oTL, 16 * (size_t)nlp))))) return rc;
    return St.done();
}

}  // namespace

extern "C" int sslam_two_view_reconstruct_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp1, const int32_t* d_n1, const sslam_keypoint* d_kp2, const int32_t* d_n2,
                                                    int cap, int npairs, const int32_t* d_matches12, const sslam_two_view_result* d_result, const uint8_t* d_inliers,
                                                    const float* d_K, float sigma, float min_parallax, int min_triangulated,
                                                    const sslam_keyline* d_kl1, const int32_t* d_nl1, const sslam_keyline* d_kl2, const int32_t* d_nl2, const double* d_linefn1,
                                                    const double* d_linefn2, int lcap, const int32_t* d_line_pairs, const int32_t* d_line_npairs,
                                                    sslam_two_view_pose* d_pose, float* d_p3d, uint8_t* d_triangulated, float* d_line_s3d, float* d_line_e3d,
                                                    uint8_t* d_line_triangulated, void* stream) {
    const char* fn = "sslam_two_view_reconstruct_batch_dev";
    const int lines = reconstruct_lines_given(d_kl1, d_nl1, d_kl2, d_nl2, d_linefn1, d_linefn2, d_line_pairs, d_line_npairs, d_line_s3d, d_line_e3d, d_line_triangulated, lcap);
    if (!ctx || !d_kp1 || !d_n1 || !d_kp2 || !d_n2 || !d_matches12 || !d_result || !d_inliers || !d_K || !d_pose || !d_p3d || !d_triangulated || lines < 0 ||
        !reconstruct_params_ok(sigma, min_triangulated) || !reconstruct_sizes_ok(npairs, cap, lines ? lcap : 0) || !all_aligned<4>(d_kp1, d_kp2) || !all_aligned<4>(d_kl1, d_kl2) ||
        !all_aligned<4>(d_n1, d_n2, d_matches12, d_nl1, d_nl2, d_line_pairs, d_line_npairs) || !all_aligned<4>(d_K, d_p3d, d_line_s3d, d_line_e3d) ||
        !all_aligned<4>(d_result) || !all_aligned<4>(d_pose) || !all_aligned<8>(d_linefn1, d_linefn2)) {
        set_error("%s: invalid arguments", fn); return SSLAM_ERR_INVALID;
    }
    if (cap > RECON_MAX_CAP || (lines && lcap > RECON_MAX_LCAP)) {
        set_error("%s: cap=%d / lcap=%d exceed the supported %d / %d (a pair's rows sit in LDS)", fn, cap, lines ? lcap : 0, RECON_MAX_CAP, RECON_MAX_LCAP); return SSLAM_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    ReconArgs A{};
    A.kp1 = d_kp1; A.n1 = d_n1; A.kp2 = d_kp2; A.n2 = d_n2; A.m12 = d_matches12; A.res = d_result; A.inl = d_inliers; A.K = d_K;
    A.cap = cap; A.lcap = lines ? lcap : 0; A.minTri = min_triangulated; A.sigma = sigma; A.minParallax = min_parallax;
    A.kl1 = d_kl1; A.nl1 = d_nl1; A.nl2 = d_nl2; A.fn1 = d_linefn1; A.fn2 = d_linefn2; A.lpairs = d_line_pairs; A.lnp = d_line_npairs;
    A.pose = d_pose; A.p3d = d_p3d; A.tri = d_triangulated; A.ls3d = d_line_s3d; A.le3d = d_line_e3d; A.ltri = d_line_triangulated;
    return reconstruct_launch(ctx, A, npairs, false, pick(ctx, stream));
}

extern "C" int sslam_two_view_reconstruct(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12,
                                          const sslam_two_view_result* result, const uint8_t* inliers, const float K[4], float sigma, float min_parallax, int min_triangulated,
                                          const sslam_keyline* kl1, int nl1, const sslam_keyline* kl2, int nl2, const double* linefn1, const double* linefn2,
                                          const int32_t* line_pairs, int line_npairs, sslam_two_view_pose* pose, float* p3d, uint8_t* triangulated,
                                          float* line_s3d, float* line_e3d, uint8_t* line_triangulated) {
    return reconstruct_host_pair(ctx, "sslam_two_view_reconstruct", kp1, n1, kp2, n2, matches12, result, inliers, K, sigma, min_parallax, min_triangulated, kl1, nl1, kl2, nl2,
                                 linefn1, linefn2, line_pairs, line_npairs, pose, p3d, triangulated, line_s3d, line_e3d, line_triangulated, nullptr);
}

#ifdef SSLAM_TESTING
#include "../../include/sslam_testing.h"
extern "C" int sslam_testing_two_view_reconstruct(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const int32_t* matches12,
                                                  const sslam_two_view_result* result, const uint8_t* inliers, const float K[4], float sigma, float min_parallax,
                                                  int min_triangulated, const sslam_keyline* kl1, int nl1, const sslam_keyline* kl2, int nl2, const double* linefn1,
                                                  const double* linefn2, const int32_t* line_pairs, int line_npairs, sslam_two_view_pose* pose, float* p3d, uint8_t* triangulated,
                                                  float* line_s3d, float* line_e3d, uint8_t* line_triangulated,
                                                  float* hyp_out, float* sel_out, int32_t* stage_out, float* p3d_rows_out, float* cos_out, double* line_err_out) {
    const ReconTap T{hyp_out, sel_out, stage_out, p3d_rows_out, cos_out, line_err_out};
    return reconstruct_host_pair(ctx, "sslam_testing_two_view_reconstruct", kp1, n1, kp2, n2, matches12, result, inliers, K, sigma, min_parallax, min_triangulated, kl1, nl1, kl2,
                                 nl2, linefn1, linefn2, line_pairs, line_npairs, pose, p3d, triangulated, line_s3d, line_e3d, line_triangulated, &T);
}
#endif
