// Matchers whose queries do not interact: Fuse / Sim3 candidate search, SearchForTriangulation, DBoW2 vocabulary descent,
// distinctive-descriptor selection.
// Part of match.hip (included there, inside its anonymous namespace: one translation unit).  Not a standalone header.
#pragma once

// ------------------------------------------------------------------ Fuse: independent best match per projected point / line
// ORBmatcher::Fuse (src/ORBmatcher.cc:897-948 with the chi-square gates, :1055-1080 without) and LSDmatcher::Fuse
// (src/LSDmatcher.cpp:497-523): every query keeps the candidate with the smallest Hamming distance, the first one in
// KeyFrame::GetFeaturesInArea / GetLinesInArea order on ties.  Queries do not interact, so one wave takes one query and scans
// the keyframe's features lane-parallel; the candidate order travels in the low bits of the min-reduction key.
struct FuseArgs {
    int kind, chi2;
    const void* feats; const uint8_t* desc; int n;
    float minX, maxX, minY, maxY;
    const float* uright; const float* invSigma2; int nlevels;
    const sslam_proj_query* q; const uint8_t* qdesc; int nq;
    int* bestIdx; int* bestDist;
};
__global__ __launch_bounds__(64) void k_fuse_search(FuseArgs A) {
    const int lane = threadIdx.x;
    const sslam_keypoint* kps = (const sslam_keypoint*)A.feats;
    const sslam_keyline* kls = (const sslam_keyline*)A.feats;
    const float invW = __fdiv_rn((float)GRID_COLS, __fsub_rn(A.maxX, A.minX));
    const float invH = __fdiv_rn((float)GRID_ROWS, __fsub_rn(A.maxY, A.minY));
    for (int iq = blockIdx.x; iq < A.nq; iq += gridDim.x) {
        const sslam_proj_query Q = A.q[iq];
        unsigned long long b = ~0ull;
        if (Q.valid) {
            const uint4 q0 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[0], q1 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[1];
            for (int i = lane; i < A.n; i += 64) {
                int key = i, lvl;
                if (A.kind == 0) {
                    const sslam_keypoint kp = kps[i];
                    const int px = (int)roundf(__fmul_rn(__fsub_rn(kp.x, A.minX), invW));
                    const int py = (int)roundf(__fmul_rn(__fsub_rn(kp.y, A.minY), invH));
                    if (!(px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS)) continue;      // not in the grid at all
                    key = ((px * GRID_ROWS + py) << 19) | i;
                    const float dx = __fsub_rn(kp.x, Q.u), dy = __fsub_rn(kp.y, Q.v);
                    if (!(fabsf(dx) < Q.radius && fabsf(dy) < Q.radius)) continue;
                    lvl = kp.octave;
                    if (lvl < Q.min_level || lvl > Q.max_level) continue;
                    if (A.chi2) {
                        const float ex = __fsub_rn(Q.u, kp.x), ey = __fsub_rn(Q.v, kp.y);
                        const float inv = (lvl >= 0 && lvl < A.nlevels) ? A.invSigma2[lvl] : 0.f;
                        const float ur = A.uright ? A.uright[i] : -1.f;
                        if (ur >= 0) {
                            const float er = __fsub_rn(Q.ur, ur);
                            const float e2 = __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(er, er));
                            if ((double)__fmul_rn(e2, inv) > 7.8) continue;
                        } else {
                            const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                            if ((double)__fmul_rn(e2, inv) > 5.99) continue;
                        }
                    }
                } else {
                    const sslam_keyline kl = kls[i];
                    const double mxp = 0.5 * (double)__fadd_rn(Q.u, Q.u2) - (double)kl.pt_x, myp = 0.5 * (double)__fadd_rn(Q.v, Q.v2) - (double)kl.pt_y;
                    const float distance = (float)(mxp * mxp + myp * myp);
                    if (distance > __fmul_rn(Q.radius, Q.radius)) continue;
                    const float slope = __fsub_rn(__fdiv_rn(__fsub_rn(Q.v, Q.v2), __fsub_rn(Q.u, Q.u2)), kl.angle);
                    if ((double)slope > (double)Q.radius * 0.01) continue;
                    lvl = kl.octave;
                    if (lvl < Q.min_level || lvl > Q.max_level) continue;
                }
                const uint4* tp = (const uint4*)(A.desc + (size_t)i * 32);
                const unsigned long long kk = ((unsigned long long)hamming256(q0, q1, tp[0], tp[1]) << 32) | (unsigned)key;
                b = kk < b ? kk : b;
            }
        }
        b = wave_min_u64(b);
        if (lane == 0) {
            A.bestIdx[iq] = b == ~0ull ? -1 : (int)(b & 0x7FFFF);
            A.bestDist[iq] = b == ~0ull ? 0x7fffffff : (int)(b >> 32);
        }
    }
}

// ------------------------------------------------------------------ ORBmatcher::SearchForTriangulation
// src/ORBmatcher.cc:660-826 (+ CheckDistEpipolarLine :140-157).  The reference never sets vbMatched2, so every keyframe-1
// feature is an independent query over the keyframe-2 features of its vocabulary node: one wave per query, candidates
// lane-parallel.  `dist > bestDist` (not >=) lets a later candidate with an equal distance win, hence the inverted position
// in the min-reduction key.  k_rot_finish (match_rot.h) applies the rotation-histogram pruning and counts.
// The rules of one candidate exist once, here, for the single call's kernel and the batch's:
//   tri_side_ok     a keypoint of either keyframe takes part when it holds no map point and, under bOnlyStereo, has a right coordinate (:697-711, :738-747)
//   tri_query       the epipolar line of a keyframe-1 keypoint in image 2 (CheckDistEpipolarLine :143-147) beside its descriptor
//   tri_candidate   the descriptor distance of an admissible keyframe-2 keypoint, -1 where TH_LOW (:749), the epipole gate of two monocular keypoints
//                   (:757-763) or the epipolar distance against 3.84 sigma2 (:149-156) rejects it
// The float operations and their order are k_tri_search's own; scale2 / sigma2 are read only where the original read them.
struct TriQuery { uint4 q0, q1; float la, lb, lc, den; bool st1; };
__device__ __forceinline__ bool tri_side_ok(bool isFree, bool stereo, int onlyStereo) { return isFree && !(onlyStereo && !stereo); }
__device__ __forceinline__ TriQuery tri_query(const sslam_keypoint& k1, const uint8_t* d1row, const float* F, bool st1) {
    TriQuery Q;
    Q.q0 = ((const uint4*)d1row)[0]; Q.q1 = ((const uint4*)d1row)[1];
    Q.la = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, F[0]), __fmul_rn(k1.y, F[3])), F[6]);
    Q.lb = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, F[1]), __fmul_rn(k1.y, F[4])), F[7]);
    Q.lc = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, F[2]), __fmul_rn(k1.y, F[5])), F[8]);
    Q.den = __fadd_rn(__fmul_rn(Q.la, Q.la), __fmul_rn(Q.lb, Q.lb));
    Q.st1 = st1;
    return Q;
}
// oct: the keypoint's octave clamped to the level tables
__device__ __forceinline__ int tri_octave(int octave, int nlevels) { return min(max(octave, 0), nlevels - 1); }
__device__ __forceinline__ int tri_candidate(const TriQuery& Q, uint4 t0, uint4 t1, float x2, float y2, int oct, bool st2, float ex, float ey,
                                             const float* scale2, const float* sigma2_2) {
    const int dist = hamming256(Q.q0, Q.q1, t0, t1);
    if (dist > TH_LOW) return -1;
    if (!Q.st1 && !st2) {
        const float dx = __fsub_rn(ex, x2), dy = __fsub_rn(ey, y2);
        if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < __fmul_rn(100.f, scale2[oct])) return -1;
    }
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(Q.la, x2), __fmul_rn(Q.lb, y2)), Q.lc);
    if (Q.den == 0.f) return -1;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), Q.den);
    if (!((double)dsqr < 3.84 * (double)sigma2_2[oct])) return -1;
    return dist;
}
// `dist > bestDist` keeps the LATER of two candidates at one distance: the smallest key is the smallest distance at the highest position
__device__ __forceinline__ unsigned long long tri_key(int dist, int pos) { return ((unsigned long long)dist << 32) | (unsigned)(0x7FFFFFFF - pos); }
__device__ __forceinline__ int tri_key_pos(unsigned long long key) { return 0x7FFFFFFF - (int)(unsigned)key; }

struct TriArgs {
    const sslam_keypoint* kp1; const uint8_t* d1; const float* ur1; const uint8_t* free1; int n1;
    const sslam_keypoint* kp2; const uint8_t* d2; const float* ur2; const uint8_t* free2;
    const int* ptr1; const int* ptr2; int nnodes; const int* idx1; const int* idx2; const int* nodeOf; int total1;
    float F[9]; float ex, ey; const float* scale2; const float* sigma2_2; int nlevels;
    int onlyStereo, checkOri;
    int* m12; int* qbin; int* nmatches;
};
__global__ __launch_bounds__(64) void k_tri_search(TriArgs A) {
    const int lane = threadIdx.x;
    for (int a = blockIdx.x; a < A.total1; a += gridDim.x) {
        const int i1 = A.idx1[a];
        const bool st1 = A.ur1 && A.ur1[i1] >= 0;
        if (!tri_side_ok(A.free1[i1] != 0, st1, A.onlyStereo)) continue;
        const int nd = A.nodeOf[a];
        const int f0 = A.ptr2[nd], f1 = A.ptr2[nd + 1];
        const sslam_keypoint k1 = A.kp1[i1];
        const TriQuery Q = tri_query(k1, A.d1 + (size_t)i1 * 32, A.F, st1);
        unsigned long long b = ~0ull;
        for (int p = f0 + lane; p < f1; p += 64) {
            const int i2 = A.idx2[p];
            const bool st2 = A.ur2 && A.ur2[i2] >= 0;
            if (!tri_side_ok(A.free2[i2] != 0, st2, A.onlyStereo)) continue;
            const uint4* tp = (const uint4*)(A.d2 + (size_t)i2 * 32);
            const sslam_keypoint k2 = A.kp2[i2];
            const int dist = tri_candidate(Q, tp[0], tp[1], k2.x, k2.y, tri_octave(k2.octave, A.nlevels), st2, A.ex, A.ey, A.scale2, A.sigma2_2);
            if (dist < 0) continue;
            const unsigned long long kk = tri_key(dist, p - f0);
            b = kk < b ? kk : b;
        }
        b = wave_min_u64(b);
        if (b != ~0ull && lane == 0) {
            const int i2 = A.idx2[f0 + tri_key_pos(b)];
            A.m12[i1] = i2;
            if (A.checkOri) A.qbin[i1] = rot_bin(k1.angle, A.kp2[i2].angle);
        }
    }
}

// ------------------------------------------------------------------ SearchForTriangulation of a batch (sslam_orb_search_for_triangulation_batch_dev)
// The same matcher on per-feature NODE IDS instead of CSR lists, for pairs of keyframe slots of one device-resident pool: no sort, no scratch, no
// traffic between workgroups.  One workgroup of TRI_BATCH_WAVES waves per pair (match_plan.h).  The queries do not interact, so there is no chain and
// no ownership of nodes: wave w takes the keyframe-1 rows [64 (w + k TRI_BATCH_WAVES), +64), k = 0, 1, .., one row per lane, ballots the rows that
// take part (tri_side_ok, node id >= 0) and serves them in bit order; for each it scans the keyframe-2 rows lane-parallel for rows of that node and
// reduces tri_key over tri_candidate.  The position in the key is the keyframe-2 row index: inside a node the list FeatureVector::addFeature builds is
// in ascending feature index, so the later list entry is the higher row.  The lane that loaded a row writes its match (or -1) once, behind the
// ballot's loop.  After the one barrier behind the walk the workgroup builds the rotation histogram of ITS pair -- the bin is recomputed from
// matches12[i] and the two angles -- prunes (three_maxima / rot_kept, match_rot.h), counts and writes.
// Every loop is bounded by a clamped count, a ballot's set bits or a constant: node ids, free flags and uright past a count are never read.
struct TriBatchArgs {
    const sslam_keypoint* kp; const uint8_t* desc; const int* node; const uint8_t* isFree; const float* uright; const int* n; int cap, nkeyframes;
    const sslam_tri_pair* pairs;
    int nlevels, onlyStereo, checkOri;
    int* m12; int* nmatches;
    float scale2[64], sigma2_2[64];          // the level tables travel in the kernel's arguments: read from the caller's host arrays before the call returns
};
constexpr unsigned TRI_PACK_FREE = 0x100u, TRI_PACK_STEREO = 0x200u;      // beside the clamped octave (< 64) in a row's packed word
// kLds: keyframe 2 of the pair in dynamic LDS -- descriptors [2 cap] uint4, node ids [cap], x [cap], y [cap], octave | free | stereo [cap]
// (TRI_BATCH_ROW_BYTES per row); otherwise the scan reads the caller's buffers
template <bool kLds>
__global__ __launch_bounds__(64 * TRI_BATCH_WAVES) void k_tri_search_batch(TriBatchArgs A) {
    extern __shared__ __align__(16) unsigned trl[];
    __shared__ float scale2[64], sigma2_2[64];
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int keep[3];
    __shared__ int total;
    constexpr int NT = 64 * TRI_BATCH_WAVES;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sslam_tri_pair P = A.pairs[p];
    if (P.kf1 < 0 || P.kf1 >= A.nkeyframes || P.kf2 < 0 || P.kf2 >= A.nkeyframes) {      // (uniform over the workgroup, ahead of every barrier)
        if (tid == 0) A.nmatches[p] = 0;
        return;
    }
    const int n1 = min(max(A.n[P.kf1], 0), A.cap), n2 = min(max(A.n[P.kf2], 0), A.cap);
    const size_t r1 = (size_t)P.kf1 * (size_t)A.cap, r2 = (size_t)P.kf2 * (size_t)A.cap;
    const sslam_keypoint* kp1 = A.kp + r1; const uint8_t* d1 = A.desc + r1 * 32; const int* node1 = A.node + r1;
    const uint8_t* free1 = A.isFree ? A.isFree + r1 : nullptr; const float* ur1 = A.uright ? A.uright + r1 : nullptr;
    const sslam_keypoint* kp2 = A.kp + r2; const uint4* d2 = (const uint4*)(A.desc + r2 * 32); const int* node2 = A.node + r2;
    const uint8_t* free2 = A.isFree ? A.isFree + r2 : nullptr; const float* ur2 = A.uright ? A.uright + r2 : nullptr;
    int* out = A.m12 + (size_t)p * (size_t)A.cap;
    uint4* ld = (uint4*)trl; int* ln = (int*)(ld + 2 * (size_t)A.cap); float* lx = (float*)(ln + A.cap); float* ly = lx + A.cap; unsigned* lp = (unsigned*)(ly + A.cap);
    if (kLds) {
        for (int j = tid; j < 2 * n2; j += NT) ld[j] = d2[j];
        for (int j = tid; j < n2; j += NT) {
            const sslam_keypoint k2 = kp2[j];
            ln[j] = node2[j]; lx[j] = k2.x; ly[j] = k2.y;
            lp[j] = (unsigned)tri_octave(k2.octave, A.nlevels) | ((!free2 || free2[j]) ? TRI_PACK_FREE : 0u) | ((ur2 && ur2[j] >= 0) ? TRI_PACK_STEREO : 0u);
        }
    }
    if (tid < 64) { scale2[tid] = tid < A.nlevels ? A.scale2[tid] : 0.f; sigma2_2[tid] = tid < A.nlevels ? A.sigma2_2[tid] : 0.f; }
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    // the walk: no workgroup barrier in here (the waves' trip counts differ)
    for (int i0 = 64 * wave; i0 < n1; i0 += NT) {
        const int i = i0 + lane;
        int nd = -1; bool st = false, take = false;
        if (i < n1) {
            nd = node1[i]; st = ur1 && ur1[i] >= 0;
            take = nd >= 0 && tri_side_ok(!free1 || free1[i], st, A.onlyStereo);
        }
        int res = -1;
        const unsigned long long stereo = __ballot(st);
        unsigned long long todo = __ballot(take);
        while (todo) {
            const int bit = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int i1 = i0 + bit;
            const int nodeQ = __builtin_amdgcn_readlane(nd, bit);
            const TriQuery Q = tri_query(kp1[i1], d1 + (size_t)i1 * 32, P.F12, (stereo >> bit) & 1);
            unsigned long long b = ~0ull;
            for (int j = lane; j < n2; j += 64) {
                if ((kLds ? ln[j] : node2[j]) != nodeQ) continue;
                bool st2; int oct; float x2, y2; uint4 t0, t1;
                if (kLds) {
                    const unsigned pk = lp[j];
                    st2 = pk & TRI_PACK_STEREO;
                    if (!tri_side_ok(pk & TRI_PACK_FREE, st2, A.onlyStereo)) continue;
                    oct = (int)(pk & 0xFFu); x2 = lx[j]; y2 = ly[j]; t0 = ld[2 * j]; t1 = ld[2 * j + 1];
                } else {
                    st2 = ur2 && ur2[j] >= 0;
                    if (!tri_side_ok(!free2 || free2[j], st2, A.onlyStereo)) continue;
                    const sslam_keypoint k2 = kp2[j];
                    oct = tri_octave(k2.octave, A.nlevels); x2 = k2.x; y2 = k2.y; t0 = d2[2 * j]; t1 = d2[2 * j + 1];
                }
                const int dist = tri_candidate(Q, t0, t1, x2, y2, oct, st2, P.ex, P.ey, scale2, sigma2_2);
                if (dist < 0) continue;
                const unsigned long long kk = tri_key(dist, j);
                b = kk < b ? kk : b;
            }
            b = wave_min_u64(b);
            if (b != ~0ull && lane == bit) res = tri_key_pos(b);
        }
        if (i < n1) out[i] = res;
    }
    __syncthreads();
    if (A.checkOri) {
        for (int i = tid; i < n1; i += NT) {
            const int m = out[i];
            if (m >= 0) atomicAdd(&hist[min(max(rot_bin(kp1[i].angle, kp2[m].angle), 0), HISTO_LENGTH - 1)], 1);      // angles of [0, 360) never need the clamp; the histogram index stays in range whatever a row holds
        }
        __syncthreads();
        if (tid == 0) three_maxima(hist, keep[0], keep[1], keep[2]);
        __syncthreads();
    }
    int cnt = 0;
    for (int i = tid; i < n1; i += NT) {
        const int m = out[i];
        if (m < 0) continue;
        if (A.checkOri && !rot_kept(min(max(rot_bin(kp1[i].angle, kp2[m].angle), 0), HISTO_LENGTH - 1), keep[0], keep[1], keep[2])) { out[i] = -1; continue; }
        ++cnt;
    }
    cnt = wave_sum(cnt);
    if (lane == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) A.nmatches[p] = total;
}

// ------------------------------------------------------------------ DBoW2 vocabulary descent (Frame::ComputeBoW)
// TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup), Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1216-1259:
// from the root, move to the child with the smallest Hamming distance (the FIRST such child: `d < best_d`) until a leaf;
// remember the node passed at level L - levelsup.  Features are independent: one lane per feature.
// n rows in all (< 2^31).  The batch call (sslam_bow_transform_batch_dev) passes the per-frame counts: row i is row i % cap of frame i / cap, and
// the rows at or past the frame's count (clamped to [0, cap]) are left alone; counts == nullptr: the single call, every row < n is a feature.
// wordOut / weightOut may be null (the batch call's optional outputs).
__global__ __launch_bounds__(256) void k_bow_transform(const uint8_t* __restrict__ feat, int n, const int* __restrict__ counts, int cap,
                                                       const int* __restrict__ childPtr, const int* __restrict__ children,
                                                       const uint8_t* __restrict__ nodeDesc, const int* __restrict__ wordId, const double* __restrict__ weight,
                                                       int nidLevel, int* __restrict__ wordOut, double* __restrict__ weightOut, int* __restrict__ nodeOut) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    if (counts) {
        const unsigned f = i / (unsigned)cap;
        if ((int)(i - f * (unsigned)cap) >= min(max(counts[f], 0), cap)) return;
    }
    const uint4 q0 = ((const uint4*)(feat + (size_t)i * 32))[0], q1 = ((const uint4*)(feat + (size_t)i * 32))[1];
    int node = 0, level = 0, nid = 0;
    while (childPtr[node + 1] > childPtr[node]) {
        ++level;
        const int c0 = childPtr[node], c1 = childPtr[node + 1];
        int best = children[c0];
        const uint4* bp = (const uint4*)(nodeDesc + (size_t)best * 32);
        int bestD = hamming256(q0, q1, bp[0], bp[1]);
        for (int c = c0 + 1; c < c1; ++c) {
            const int id = children[c];
            const uint4* tp = (const uint4*)(nodeDesc + (size_t)id * 32);
            const int d = hamming256(q0, q1, tp[0], tp[1]);
            if (d < bestD) { bestD = d; best = id; }
        }
        node = best;
        if (level == nidLevel) nid = node;
    }
    if (wordOut) wordOut[i] = wordId[node];
    if (weightOut) weightOut[i] = weight[node];
    nodeOut[i] = nid;
}

// ------------------------------------------------------------------ distinctive descriptor of an observation set
// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:247-312) == MapLine::ComputeDistinctiveDescriptors
// (src/MapLine.cpp:246-317): all-pairs Hamming distances of the N observed descriptors, per row the median
// `sorted[int(0.5*(N-1))]`, and the FIRST row with the smallest median wins.  One wave per set: the descriptors sit in LDS,
// lane i owns row i (rows i+64, ... in turn); the k-th smallest of a row is found by bisection on the value
// (distances are integers in [0,256]: nine counting passes) instead of sorting.
constexpr int DISTINCT_MAXN = 1024;
__global__ __launch_bounds__(64) void k_distinctive(const uint8_t* __restrict__ desc, const int32_t* __restrict__ ptr, int nsets, int32_t* __restrict__ best) {
    __shared__ __align__(16) unsigned d[DISTINCT_MAXN * 8];
    const int lane = threadIdx.x;
    for (int sIdx = blockIdx.x; sIdx < nsets; sIdx += gridDim.x) {
        const int beg = ptr[sIdx], n = ptr[sIdx + 1] - beg;
        if (n <= 0) { if (lane == 0) best[sIdx] = -1; continue; }
        __syncthreads();
        for (int i = lane; i < n * 8; i += 64) d[i] = ((const unsigned*)(desc + (size_t)beg * 32))[i];
        __syncthreads();
        const int k = (int)(0.5 * (double)(n - 1));              // index of the median in the sorted row
        unsigned long long bestKey = ~0ull;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            int lo = 0, hi = 256;                                  // smallest v with #{j : dist(i,j) <= v} >= k+1
            if (i < n) {
                unsigned a[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) a[w] = d[i * 8 + w];
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    int cnt = 0;
                    for (int j = 0; j < n; ++j) {
                        int dist = 0;
#pragma unroll
                        for (int w = 0; w < 8; ++w) dist += __popc(a[w] ^ d[j * 8 + w]);
                        cnt += dist <= mid ? 1 : 0;
                    }
                    if (cnt >= k + 1) hi = mid; else lo = mid + 1;
                }
                const unsigned long long key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)i;
                bestKey = key < bestKey ? key : bestKey;
            }
        }
        bestKey = wave_min_u64(bestKey);
        if (lane == 0) best[sIdx] = (int)(unsigned)bestKey;
    }
}
