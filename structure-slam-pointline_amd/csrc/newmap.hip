// The map-creation step of LocalMapping for MI355X (gfx950): the loop bodies of CreateNewMapPoints (reference src/LocalMapping.cc:456-635) and CreateNewMapLines2
// (:1005-1170) with the first UpdateNormalAndDepth / UpdateAverageDir of the new object, behind sslam_orb_search_for_triangulation_batch_dev's d_matches12 and
// sslam_line_match_batch_dev's d_pairs, on the device-resident pool of keyframe slots.  The arithmetic is csrc/newmap_math.h, shared with the host model
// tests/sim/newmap_sim.cpp; this unit is the two kernels around it and their entry points.
//
// k_newmap_points / k_newmap_lines: one workgroup of NM_THREADS threads per pair; the lanes stride over the rows of the pair, one row per lane and turn (rows are
// independent).  The Jacobi workspace of rc::svd4_last is rc::WS4_DOUBLES doubles per lane, lane-interleaved in static LDS as reconstruct.hip's LdsWs4 holds it, so
// that run-time indices make no private array.  The level tables travel in the kernel's arguments and are staged in LDS.  Created rows are counted with ballot +
// popcount per wave and one LDS sum.  Every output word has one writer; no atomics.  The free flags are plain byte stores of 0: two rows or two pairs naming one
// slot only ever store the same value.  k_newmap_lines reads the free flags of ALL rows of its pair (leaving LN_NOT_FREE in the row's stage byte) before any row
// clears one, which is the order of src/LSDmatcher.cpp:398-413 before the loop of :1007.
#include "common.h"
#include "match_check.h"
#include "newmap_math.h"
#include <algorithm>

using namespace sslam;

namespace {

constexpr int NM_THREADS = 256, NM_WAVES = NM_THREADS / 64, NM_MAX_LEVELS = 64;
constexpr size_t NM_WS_BYTES = (size_t)rc::WS4_DOUBLES * sizeof(double) * NM_THREADS;
static_assert(NM_WS_BYTES == 53248 && NM_WS_BYTES + 1024 <= 64 * 1024, "the lane-interleaved Jacobi workspace and the level tables are static LDS below the 64 KB a workgroup gets without an opt-in");
static_assert(sizeof(sslam_kf_pose) == 84 && sizeof(sslam_newmap_pair) == 12, "include/sslam_frontend.h states these sizes");

struct LdsWs4 {      // rc::WS4_DOUBLES doubles of this lane, lane-interleaved
    double* base;
    __device__ __forceinline__ double& at(int k) { return base[k * NM_THREADS]; }
};

struct PointArgs {
    const sslam_keypoint* kp; const int32_t* n; const sslam_kf_pose* pose; const sslam_newmap_pair* pairs; const int32_t* m12;
    int cap, nkf, nlevels; float ratioFactor;
    uint8_t* freeFlags; float* x3d; uint8_t* stage; float* normal; float* dist; int32_t* nnew;
    float* tapCos; float* tapHom;      // sslam_testing_new_map_points only: [cap], [cap * 4]
    float sf[NM_MAX_LEVELS], sigma2[NM_MAX_LEVELS];
};
struct LineArgs {
    const sslam_keyline* kl; const double* fn; const int32_t* nl; const sslam_kf_pose* pose; const sslam_newmap_pair* pairs; const int32_t* lpairs; const int32_t* lnp;
    int lcap, nkf, nlevels;
    uint8_t* freeFlags; float* s3d; float* e3d; uint8_t* stage; double* normal; float* dist; int32_t* nnew;
    float* tapCos; float* tapHom;      // sslam_testing_new_map_lines only: [lcap], [lcap * 8]
    float sf[NM_MAX_LEVELS];
};

__device__ __forceinline__ bool pair_ok(int kf1, int kf2, int nkf) { return kf1 >= 0 && kf1 < nkf && kf2 >= 0 && kf2 < nkf && kf1 != kf2; }

// the workgroup's sum of the waves' counts -> out[0] (thread 0)
__device__ __forceinline__ void store_count(int* cnt, int c, int32_t* out) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) cnt[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) { int s = 0; for (int w = 0; w < NM_WAVES; ++w) s += cnt[w]; out[0] = s; }
}

template <bool TAP>
__global__ __launch_bounds__(NM_THREADS) void k_newmap_points(PointArgs A) {
    __shared__ double wsmem[rc::WS4_DOUBLES * NM_THREADS];
    __shared__ float sf[NM_MAX_LEVELS], sigma2[NM_MAX_LEVELS];
    __shared__ int cnt[NM_WAVES];
    const int tid = threadIdx.x, p = blockIdx.x, cap = A.cap;
    const sslam_newmap_pair pr = A.pairs[p];
    const int kf1 = pr.kf1, kf2 = pr.kf2;
    if (!pair_ok(kf1, kf2, A.nkf)) { if (tid == 0) A.nnew[p] = -1; return; }
    if (tid < NM_MAX_LEVELS) { sf[tid] = tid < A.nlevels ? A.sf[tid] : 0.f; sigma2[tid] = tid < A.nlevels ? A.sigma2[tid] : 0.f; }
    __syncthreads();
    const int n1 = slot_count(A.n, kf1, cap), n2 = slot_count(A.n, kf2, cap);
    const size_t b1 = (size_t)kf1 * cap, b2 = (size_t)kf2 * cap, ob = (size_t)p * cap;
    const sslam_kf_pose P1 = A.pose[kf1], P2 = A.pose[kf2];
    LdsWs4 ws{wsmem + tid};
    int c = 0;
    for (int i0 = 0; i0 < n1; i0 += NM_THREADS) {
        const int i = i0 + tid;
        bool created = false;
        if (i < n1) {
            const int m = A.m12[ob + i];
            nm::PointOut o;
            if (m < 0 || m >= n2) {
                o.stage = nm::PT_NO_MATCH; o.cosv = o.max_dist = o.min_dist = 0.f;
                for (int k = 0; k < 3; ++k) o.x3d[k] = o.normal[k] = 0.f;
                for (int k = 0; k < 4; ++k) o.hom[k] = 0.f;
                o.err1 = o.err2 = o.ratio_dist = o.ratio_octave = 0.f;
            } else {
                const sslam_keypoint k1 = A.kp[b1 + i], k2 = A.kp[b2 + m];
                nm::point_row(P1, P2, k1.x, k1.y, k1.octave, k2.x, k2.y, k2.octave, sf, sigma2, A.nlevels, A.ratioFactor, ws, o);
            }
            created = o.stage == nm::PT_CREATED;
            const size_t q = ob + i;
            for (int k = 0; k < 3; ++k) { A.x3d[q * 3 + k] = o.x3d[k]; A.normal[q * 3 + k] = o.normal[k]; }
            A.stage[q] = (uint8_t)o.stage;
            A.dist[q * 2] = o.max_dist; A.dist[q * 2 + 1] = o.min_dist;
            if (created && A.freeFlags) { A.freeFlags[b1 + i] = 0; A.freeFlags[b2 + m] = 0; }      // AddMapPoint on both keyframes (:624-625)
            if (TAP) { A.tapCos[i] = o.cosv; for (int k = 0; k < 4; ++k) A.tapHom[(size_t)i * 4 + k] = o.hom[k]; }
        }
        c += __popcll(__ballot(created));
    }
    store_count(cnt, c, A.nnew + p);
}

template <bool TAP>
__global__ __launch_bounds__(NM_THREADS) void k_newmap_lines(LineArgs A) {
    __shared__ double wsmem[rc::WS4_DOUBLES * NM_THREADS];
    __shared__ float sf[NM_MAX_LEVELS];
    __shared__ int cnt[NM_WAVES];
    const int tid = threadIdx.x, p = blockIdx.x, lcap = A.lcap;
    const sslam_newmap_pair pr = A.pairs[p];
    const int kf1 = pr.kf1, kf2 = pr.kf2;
    if (!pair_ok(kf1, kf2, A.nkf)) { if (tid == 0) A.nnew[p] = -1; return; }
    if (tid < NM_MAX_LEVELS) sf[tid] = tid < A.nlevels ? A.sf[tid] : 0.f;
    const int nl1 = slot_count(A.nl, kf1, lcap), nl2 = slot_count(A.nl, kf2, lcap), nrows = slot_count(A.lnp, p, lcap);
    const size_t b1 = (size_t)kf1 * lcap, b2 = (size_t)kf2 * lcap, ob = (size_t)p * lcap;
    const int32_t* lp = A.lpairs + ob * 2;
    // GetMapLine(qdx) || GetMapLine(tdx) of every row, as the flags stand before this pair creates anything
    for (int r0 = 0; r0 < nrows; r0 += NM_THREADS) {
        const int r = r0 + tid;
        if (r < nrows) {
            const int a = lp[(size_t)r * 2], b = lp[(size_t)r * 2 + 1];
            int st = nm::LN_CREATED;
            if (a < 0 || a >= nl1 || b < 0 || b >= nl2) st = nm::LN_NO_MATCH;
            else if (A.freeFlags && (!A.freeFlags[b1 + a] || !A.freeFlags[b2 + b])) st = nm::LN_NOT_FREE;
            A.stage[ob + r] = (uint8_t)st;
        }
    }
    __syncthreads();
    const sslam_kf_pose P1 = A.pose[kf1], P2 = A.pose[kf2];
    LdsWs4 ws{wsmem + tid};
    int c = 0;
    for (int r0 = 0; r0 < nrows; r0 += NM_THREADS) {
        const int r = r0 + tid;
        bool created = false;
        if (r < nrows) {
            const size_t q = ob + r;
            const int a = lp[(size_t)r * 2], b = lp[(size_t)r * 2 + 1];
            nm::LineOut o;
            o.stage = A.stage[q];      // this lane's own store of the first pass
            if (o.stage != nm::LN_CREATED) {
                o.cosv = o.max_dist = o.min_dist = 0.f;
                for (int k = 0; k < 3; ++k) { o.s3d[k] = o.e3d[k] = 0.f; o.normal[k] = 0.0; }
                for (int k = 0; k < 4; ++k) o.shom[k] = o.ehom[k] = 0.f;
                for (int k = 0; k < 5; ++k) o.ratio[k] = 0.f;
            } else {
                const sslam_keyline& l1 = A.kl[b1 + a];
                const sslam_keyline& l2 = A.kl[b2 + b];
                const float e1[4] = {l1.startPointX, l1.startPointY, l1.endPointX, l1.endPointY}, e2[4] = {l2.startPointX, l2.startPointY, l2.endPointX, l2.endPointY};
                const double* g1 = A.fn + (b1 + a) * 3;
                const double* g2 = A.fn + (b2 + b) * 3;
                const double f1[3] = {g1[0], g1[1], g1[2]}, f2[3] = {g2[0], g2[1], g2[2]};
                nm::line_row(P1, P2, e1, f1, l1.octave, e2, f2, pr.median_depth2, sf, A.nlevels, ws, o);
            }
            created = o.stage == nm::LN_CREATED;
            for (int k = 0; k < 3; ++k) { A.s3d[q * 3 + k] = o.s3d[k]; A.e3d[q * 3 + k] = o.e3d[k]; A.normal[q * 3 + k] = o.normal[k]; }
            A.stage[q] = (uint8_t)o.stage;
            A.dist[q * 2] = o.max_dist; A.dist[q * 2 + 1] = o.min_dist;
            if (created && A.freeFlags) { A.freeFlags[b1 + a] = 0; A.freeFlags[b2 + b] = 0; }      // AddMapLine on both keyframes (:1159-1160)
            if (TAP) {
                A.tapCos[r] = o.cosv;
                for (int k = 0; k < 4; ++k) { A.tapHom[(size_t)r * 8 + k] = o.shom[k]; A.tapHom[(size_t)r * 8 + 4 + k] = o.ehom[k]; }
            }
        }
        c += __popcll(__ballot(created));
    }
    store_count(cnt, c, A.nnew + p);
}

bool levels_ok(const float* table, int nlevels) { return table && nlevels >= 1 && nlevels <= NM_MAX_LEVELS; }

int points_launch(sslam_ctx* ctx, PointArgs& A, const float* scale_factors, const float* level_sigma2, float scale_factor, int npairs, bool tap, hipStream_t st) {
    for (int l = 0; l < NM_MAX_LEVELS; ++l) { A.sf[l] = l < A.nlevels ? scale_factors[l] : 0.f; A.sigma2[l] = l < A.nlevels ? level_sigma2[l] : 0.f; }
    A.ratioFactor = 1.5f * scale_factor;      // :400
    return launch_tapped(ctx, "k_newmap_points", SSLAM_WITH_TAP(k_newmap_points), tap, (unsigned)npairs, NM_THREADS, 0, st, A);
}
int lines_launch(sslam_ctx* ctx, LineArgs& A, const float* scale_factors, int npairs, bool tap, hipStream_t st) {
    for (int l = 0; l < NM_MAX_LEVELS; ++l) A.sf[l] = l < A.nlevels ? scale_factors[l] : 0.f;
    return launch_tapped(ctx, "k_newmap_lines", SSLAM_WITH_TAP(k_newmap_lines), tap, (unsigned)npairs, NM_THREADS, 0, st, A);
}

// one host pair on the device and back as pair 0 of a pool of two slots: shared by the single calls and the testing taps
int points_host_pair(sslam_ctx* ctx, const char* fn, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const sslam_kf_pose* pose1, const sslam_kf_pose* pose2,
                     const int32_t* matches12, const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                     float* x3d, uint8_t* stage, float* normal, float* dist, int* nnew, float* tapCos, float* tapHom, bool tap) {
    if (!ctx || n1 < 0 || n2 < 0 || !pose1 || !pose2 || !nnew || !levels_ok(scale_factors, nlevels) || !level_sigma2 || (n1 > 0 && (!kp1 || !matches12 || !x3d || !stage || !normal || !dist)) ||
        (n2 > 0 && !kp2) || (tap && n1 > 0 && (!tapCos || !tapHom))) {
        set_error("%s: invalid arguments", fn); return SSLAM_ERR_INVALID;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    const size_t c = (size_t)std::max(std::max(n1, n2), 1), ks = sizeof(sslam_keypoint);
    ArenaLayout L;
    const size_t oK = L.take(ks * 2 * c), oN = L.take(8), oP = L.take(2 * sizeof(sslam_kf_pose)), oPr = L.take(sizeof(sslam_newmap_pair)), oM = L.take(4 * c),
                 oX = L.take(12 * c), oS = L.take(c), oNo = L.take(12 * c), oD = L.take(8 * c), oC = L.take(4), oTC = L.take(tap ? 4 * c : 0), oTH = L.take(tap ? 16 * c : 0);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* d = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging St{d, ctx->stream};
    const int32_t hn[2] = {n1, n2};
    const sslam_newmap_pair pr{0, 1, 0.f};
    if ((rc = St.in(oK, kp1, ks * (size_t)n1)) || (rc = St.in(oK + ks * c, kp2, ks * (size_t)n2)) || (rc = St.in(oN, hn, sizeof(hn))) || (rc = St.in(oP, pose1, sizeof(sslam_kf_pose))) ||
        (rc = St.in(oP + sizeof(sslam_kf_pose), pose2, sizeof(sslam_kf_pose))) || (rc = St.in(oPr, &pr, sizeof(pr))) || (rc = St.in(oM, matches12, 4 * (size_t)n1))) return rc;
    PointArgs A{};
    A.kp = (const sslam_keypoint*)(d + oK); A.n = (const int32_t*)(d + oN); A.pose = (const sslam_kf_pose*)(d + oP); A.pairs = (const sslam_newmap_pair*)(d + oPr);
    A.m12 = (const int32_t*)(d + oM); A.cap = (int)c; A.nkf = 2; A.nlevels = nlevels;
    A.x3d = (float*)(d + oX); A.stage = d + oS; A.normal = (float*)(d + oNo); A.dist = (float*)(d + oD); A.nnew = (int32_t*)(d + oC);
    if (tap) { A.tapCos = (float*)(d + oTC); A.tapHom = (float*)(d + oTH); }
    int32_t count = 0;
    if ((rc = points_launch(ctx, A, scale_factors, level_sigma2, scale_factor, 1, tap, St.st)) || (rc = St.out(x3d, oX, 12 * (size_t)n1)) || (rc = St.out(stage, oS, (size_t)n1)) ||
        (rc = St.out(normal, oNo, 12 * (size_t)n1)) || (rc = St.out(dist, oD, 8 * (size_t)n1)) || (rc = St.out(&count, oC, 4))) return rc;
    if (tap && ((rc = St.out(tapCos, oTC, 4 * (size_t)n1)) || (rc = St.out(tapHom, oTH, 16 * (size_t)n1)))) return rc;
    if ((rc = St.done())) return rc;
    *nnew = count;
    return SSLAM_OK;
}

int lines_host_pair(sslam_ctx* ctx, const char* fn, const sslam_keyline* kl1, const double* linefn1, int nl1, const sslam_keyline* kl2, const double* linefn2, int nl2,
                    const sslam_kf_pose* pose1, const sslam_kf_pose* pose2, float median_depth2, const int32_t* line_pairs, int line_npairs, const float* scale_factors, int nlevels,
                    float* s3d, float* e3d, uint8_t* stage, double* normal, float* dist, int* nnew, float* tapCos, float* tapHom, bool tap) {
    const int nr = line_npairs;
    if (!ctx || nl1 < 0 || nl2 < 0 || nr < 0 || !pose1 || !pose2 || !nnew || !levels_ok(scale_factors, nlevels) || (nl1 > 0 && (!kl1 || !linefn1)) || (nl2 > 0 && (!kl2 || !linefn2)) ||
        (nr > 0 && (!line_pairs || !s3d || !e3d || !stage || !normal || !dist)) || (tap && nr > 0 && (!tapCos || !tapHom))) {
        set_error("%s: invalid arguments", fn); return SSLAM_ERR_INVALID;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    const size_t c = (size_t)std::max(std::max(nl1, nl2), std::max(nr, 1)), ls = sizeof(sslam_keyline);
    ArenaLayout L;
    const size_t oK = L.take(ls * 2 * c), oF = L.take(24 * 2 * c), oN = L.take(12), oP = L.take(2 * sizeof(sslam_kf_pose)), oPr = L.take(sizeof(sslam_newmap_pair)), oLP = L.take(8 * c),
                 oS3 = L.take(12 * c), oE3 = L.take(12 * c), oS = L.take(c), oNo = L.take(24 * c), oD = L.take(8 * c), oC = L.take(4), oTC = L.take(tap ? 4 * c : 0),
                 oTH = L.take(tap ? 32 * c : 0);
    int rc;
    if ((rc = ctx->scratch[SCR_CALL].ensure(L.size()))) return rc;
    uint8_t* d = ctx->scratch[SCR_CALL].as<uint8_t>();
    const Staging St{d, ctx->stream};
    const int32_t hn[3] = {nl1, nl2, nr};
    const sslam_newmap_pair pr{0, 1, median_depth2};
    if ((rc = St.in(oK, kl1, ls * (size_t)nl1)) || (rc = St.in(oK + ls * c, kl2, ls * (size_t)nl2)) || (rc = St.in(oF, linefn1, 24 * (size_t)nl1)) ||
        (rc = St.in(oF + 24 * c, linefn2, 24 * (size_t)nl2)) || (rc = St.in(oN, hn, sizeof(hn))) || (rc = St.in(oP, pose1, sizeof(sslam_kf_pose))) ||
        (rc = St.in(oP + sizeof(sslam_kf_pose), pose2, sizeof(sslam_kf_pose))) || (rc = St.in(oPr, &pr, sizeof(pr))) || (rc = St.in(oLP, line_pairs, 8 * (size_t)nr))) return rc;
    LineArgs A{};
    A.kl = (const sslam_keyline*)(d + oK); A.fn = (const double*)(d + oF); A.nl = (const int32_t*)(d + oN); A.pose = (const sslam_kf_pose*)(d + oP);
    A.pairs = (const sslam_newmap_pair*)(d + oPr); A.lpairs = (const int32_t*)(d + oLP); A.lnp = A.nl + 2; A.lcap = (int)c; A.nkf = 2; A.nlevels = nlevels;
    A.s3d = (float*)(d + oS3); A.e3d = (float*)(d + oE3); A.stage = d + oS; A.normal = (double*)(d + oNo); A.dist = (float*)(d + oD); A.nnew = (int32_t*)(d + oC);
    if (tap) { A.tapCos = (float*)(d + oTC); A.tapHom = (float*)(d + oTH); }
    int32_t count = 0;
    if ((rc = lines_launch(ctx, A, scale_factors, 1, tap, St.st)) || (rc = St.out(s3d, oS3, 12 * (size_t)nr)) || (rc = St.out(e3d, oE3, 12 * (size_t)nr)) || (rc = St.out(stage, oS, (size_t)nr)) ||
        (rc = St.out(normal, oNo, 24 * (size_t)nr)) || (rc = St.out(dist, oD, 8 * (size_t)nr)) || (rc = St.out(&count, oC, 4))) return rc;
    if (tap && ((rc = St.out(tapCos, oTC, 4 * (size_t)nr)) || (rc = St.out(tapHom, oTH, 32 * (size_t)nr)))) return rc;
    if ((rc = St.done())) return rc;
    *nnew = count;
    return SSLAM_OK;
}

// rows are indexed slot * cap + i and pair * cap + i in 31 bits
bool sizes_ok(int cap, int nkeyframes, int npairs) { return cap >= 0 && nkeyframes >= 0 && npairs >= 0 && fits_31_bits(npairs, cap) && fits_31_bits(nkeyframes, cap); }

}  // namespace

extern "C" int sslam_new_map_points_batch_dev(sslam_ctx* ctx, const sslam_keypoint* d_kp, const int32_t* d_n, int cap, int nkeyframes, const sslam_kf_pose* d_pose,
                                              const sslam_newmap_pair* d_pairs, int npairs, const int32_t* d_matches12, const float* scale_factors, const float* level_sigma2,
                                              int nlevels, float scale_factor, uint8_t* d_free, float* d_x3d, uint8_t* d_stage, float* d_normal, float* d_dist, int32_t* d_nnew,
                                              void* stream) {
    if (!ctx || !d_kp || !d_n || !d_pose || !d_pairs || !d_matches12 || !levels_ok(scale_factors, nlevels) || !level_sigma2 || !d_x3d || !d_stage || !d_normal || !d_dist || !d_nnew ||
        !sizes_ok(cap, nkeyframes, npairs) || !all_aligned<4>(d_kp) || !all_aligned<4>(d_pose) || !all_aligned<4>(d_pairs) ||
        !all_aligned<4>(d_n, d_matches12, d_nnew) || !all_aligned<4>(d_x3d, d_normal, d_dist)) {
        set_error("sslam_new_map_points_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (npairs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    PointArgs A{};
    A.kp = d_kp; A.n = d_n; A.pose = d_pose; A.pairs = d_pairs; A.m12 = d_matches12; A.cap = cap; A.nkf = nkeyframes; A.nlevels = nlevels;
    A.freeFlags = d_free; A.x3d = d_x3d; A.stage = d_stage; A.normal = d_normal; A.dist = d_dist; A.nnew = d_nnew;
    return points_launch(ctx, A, scale_factors, level_sigma2, scale_factor, npairs, false, pick(ctx, stream));
}

extern "C" int sslam_new_map_lines_batch_dev(sslam_ctx* ctx, const sslam_keyline* d_kl, const double* d_linefn, const int32_t* d_nl, int lcap, int nkeyframes,
                                             const sslam_kf_pose* d_pose, const sslam_newmap_pair* d_pairs, int npairs, const int32_t* d_line_pairs, const int32_t* d_line_npairs,
                                             const float* scale_factors, int nlevels, uint8_t* d_lfree, float* d_s3d, float* d_e3d, uint8_t* d_stage, double* d_normal,
                                             float* d_dist, int32_t* d_nnew, void* stream) {
    if (!ctx || !d_kl || !d_linefn || !d_nl || !d_pose || !d_pairs || !d_line_pairs || !d_line_npairs || !levels_ok(scale_factors, nlevels) || !d_s3d || !d_e3d || !d_stage ||
        !d_normal || !d_dist || !d_nnew || !sizes_ok(lcap, nkeyframes, npairs) || !all_aligned<4>(d_kl) || !all_aligned<4>(d_pose) || !all_aligned<4>(d_pairs) ||
        !all_aligned<4>(d_nl, d_line_pairs, d_line_npairs, d_nnew) || !all_aligned<4>(d_s3d, d_e3d, d_dist) || !all_aligned<8>(d_linefn, d_normal)) {
        set_error("sslam_new_map_lines_batch_dev: invalid arguments"); return SSLAM_ERR_INVALID;
    }
    if (npairs == 0) return SSLAM_OK;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    SSLAM_HIP(hipSetDevice(ctx->device));
    LineArgs A{};
    A.kl = d_kl; A.fn = d_linefn; A.nl = d_nl; A.pose = d_pose; A.pairs = d_pairs; A.lpairs = d_line_pairs; A.lnp = d_line_npairs; A.lcap = lcap; A.nkf = nkeyframes; A.nlevels = nlevels;
    A.freeFlags = d_lfree; A.s3d = d_s3d; A.e3d = d_e3d; A.stage = d_stage; A.normal = d_normal; A.dist = d_dist; A.nnew = d_nnew;
    return lines_launch(ctx, A, scale_factors, npairs, false, pick(ctx, stream));
}

extern "C" int sslam_new_map_points(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const sslam_kf_pose* pose1, const sslam_kf_pose* pose2,
                                    const int32_t* matches12, const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                                    float* x3d, uint8_t* stage, float* normal, float* dist, int* nnew) {
    return points_host_pair(ctx, "sslam_new_map_points", kp1, n1, kp2, n2, pose1, pose2, matches12, scale_factors, level_sigma2, nlevels, scale_factor, x3d, stage, normal, dist, nnew,
                            nullptr, nullptr, false);
}

extern "C" int sslam_new_map_lines(sslam_ctx* ctx, const sslam_keyline* kl1, const double* linefn1, int nl1, const sslam_keyline* kl2, const double* linefn2, int nl2,
                                   const sslam_kf_pose* pose1, const sslam_kf_pose* pose2, float median_depth2, const int32_t* line_pairs, int line_npairs,
                                   const float* scale_factors, int nlevels, float* s3d, float* e3d, uint8_t* stage, double* normal, float* dist, int* nnew) {
    return lines_host_pair(ctx, "sslam_new_map_lines", kl1, linefn1, nl1, kl2, linefn2, nl2, pose1, pose2, median_depth2, line_pairs, line_npairs, scale_factors, nlevels, s3d, e3d,
                           stage, normal, dist, nnew, nullptr, nullptr, false);
}

#ifdef SSLAM_TESTING
#include "../../include/sslam_testing.h"
extern "C" int sslam_testing_new_map_points(sslam_ctx* ctx, const sslam_keypoint* kp1, int n1, const sslam_keypoint* kp2, int n2, const sslam_kf_pose* pose1,
                                            const sslam_kf_pose* pose2, const int32_t* matches12, const float* scale_factors, const float* level_sigma2, int nlevels,
                                            float scale_factor, float* x3d, uint8_t* stage, float* normal, float* dist, int* nnew, float* cos_out, float* hom_out) {
    return points_host_pair(ctx, "sslam_testing_new_map_points", kp1, n1, kp2, n2, pose1, pose2, matches12, scale_factors, level_sigma2, nlevels, scale_factor, x3d, stage, normal, dist,
                            nnew, cos_out, hom_out, true);
}
extern "C" int sslam_testing_new_map_lines(sslam_ctx* ctx, const sslam_keyline* kl1, const double* linefn1, int nl1, const sslam_keyline* kl2, const double* linefn2, int nl2,
                                           const sslam_kf_pose* pose1, const sslam_kf_pose* pose2, float median_depth2, const int32_t* line_pairs, int line_npairs,
                                           const float* scale_factors, int nlevels, float* s3d, float* e3d, uint8_t* stage, double* normal, float* dist, int* nnew,
                                           float* cos_out, float* hom_out) {
    return lines_host_pair(ctx, "sslam_testing_new_map_lines", kl1, linefn1, nl1, kl2, linefn2, nl2, pose1, pose2, median_depth2, line_pairs, line_npairs, scale_factors, nlevels, s3d,
                           e3d, stage, normal, dist, nnew, cos_out, hom_out, true);
}
#endif
