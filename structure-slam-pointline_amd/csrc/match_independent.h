// Matchers whose queries do not interact: Fuse / Sim3 candidate search, SearchForTriangulation, DBoW2 vocabulary descent,
// distinctive-descriptor selection.
// Part of match.hip (included there, inside its anonymous namespace: one translation unit).  Not a standalone header.
#pragma once

// ------------------------------------------------------------------ Fuse: independent best match per projected point / line
// ORBmatcher::Fuse (src/ORBmatcher.cc:897-948 with the chi-square gates, :1055-1080 without) and LSDmatcher::Fuse
// (src/LSDmatcher.cpp:497-523): every query keeps the candidate with the smallest Hamming distance, the first one in
// KeyFrame::GetFeaturesInArea / GetLinesInArea order on ties.  Queries do not interact, so one wave takes one query and scans
// the keyframe's features lane-parallel; the candidate order travels in the low bits of the min-reduction key.
// The rules of one candidate exist once, here, for the single call's kernel and the batch's:
//   fuse_grid / fuse_cell   the 64 x 48 grid Frame::AssignFeaturesToGrid files a keypoint in (PosInGrid, src/Frame.cc:133-148, :462-472; the keyframe copies it): -1 for a keypoint
//                           that is in no cell and so in no GetFeaturesInArea result, else the cell's rank in the column-major walk of the window
//   fuse_point_window       |dx| < r, |dy| < r (KeyFrame::GetFeaturesInArea, src/KeyFrame.cc:610-649) and the level test of src/ORBmatcher.cc:912-915
//   fuse_inv_sigma2         mvInvLevelSigma2[level]; a level outside the table weighs 0, so that nothing beyond the table is read
//   fuse_point_chi2         the 7.8 (stereo) / 5.99 (monocular) gates of src/ORBmatcher.cc:917-941
//   fuse_line_ok            midpoint distance, slope against the keyline's angle (KeyFrame::GetLinesInArea, src/KeyFrame.cc:652-683) and the level test
//   fuse_key                smallest distance first, then GetFeaturesInArea order: cell by cell, inside a cell by ascending index (lines: the index alone)
// The float operations and their order are k_fuse_search's own.
struct FuseGrid { float minX, minY, invW, invH; };
__device__ __forceinline__ FuseGrid fuse_grid(float minX, float maxX, float minY, float maxY) {
    return {minX, minY, __fdiv_rn((float)GRID_COLS, __fsub_rn(maxX, minX)), __fdiv_rn((float)GRID_ROWS, __fsub_rn(maxY, minY))};
}
__device__ __forceinline__ int fuse_cell(const FuseGrid& G, float x, float y) {
    const int px = (int)roundf(__fmul_rn(__fsub_rn(x, G.minX), G.invW));
    const int py = (int)roundf(__fmul_rn(__fsub_rn(y, G.minY), G.invH));
    if (!(px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS)) return -1;      // not in the grid at all
    return px * GRID_ROWS + py;
}
__device__ __forceinline__ bool fuse_point_window(const sslam_proj_query& Q, float x, float y, int lvl) {
    const float dx = __fsub_rn(x, Q.u), dy = __fsub_rn(y, Q.v);
    if (!(fabsf(dx) < Q.radius && fabsf(dy) < Q.radius)) return false;
    return !(lvl < Q.min_level || lvl > Q.max_level);
}
__device__ __forceinline__ float fuse_inv_sigma2(const float* table, int nlevels, int lvl) { return (lvl >= 0 && lvl < nlevels) ? table[lvl] : 0.f; }
// ur: the keypoint's right coordinate, below 0 for a monocular keypoint (and for a keyframe without right coordinates)
__device__ __forceinline__ bool fuse_point_chi2(const sslam_proj_query& Q, float x, float y, float ur, float inv) {
    const float ex = __fsub_rn(Q.u, x), ey = __fsub_rn(Q.v, y);
    if (ur >= 0) {
        const float er = __fsub_rn(Q.ur, ur);
        const float e2 = __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(er, er));
        return !((double)__fmul_rn(e2, inv) > 7.8);
    }
    const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    return !((double)__fmul_rn(e2, inv) > 5.99);
}
__device__ __forceinline__ bool fuse_line_ok(const sslam_proj_query& Q, float pt_x, float pt_y, float angle, int lvl) {
    const double mxp = 0.5 * (double)__fadd_rn(Q.u, Q.u2) - (double)pt_x, myp = 0.5 * (double)__fadd_rn(Q.v, Q.v2) - (double)pt_y;
    const float distance = (float)(mxp * mxp + myp * myp);
    if (distance > __fmul_rn(Q.radius, Q.radius)) return false;
    const float slope = __fsub_rn(__fdiv_rn(__fsub_rn(Q.v, Q.v2), __fsub_rn(Q.u, Q.u2)), angle);
    if ((double)slope > (double)Q.radius * 0.01) return false;
    return !(lvl < Q.min_level || lvl > Q.max_level);
}
// cell < 2^12 and i < 2^19: 31 bits; lines pass cell 0
__device__ __forceinline__ unsigned long long fuse_key(int dist, int cell, int i) { return ((unsigned long long)dist << 32) | (unsigned)((cell << 19) | i); }
__device__ __forceinline__ int fuse_key_idx(unsigned long long key) { return key == ~0ull ? -1 : (int)(key & 0x7FFFF); }
__device__ __forceinline__ int fuse_key_dist(unsigned long long key) { return key == ~0ull ? 0x7fffffff : (int)(key >> 32); }

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
    const FuseGrid G = fuse_grid(A.minX, A.maxX, A.minY, A.maxY);
    for (int iq = blockIdx.x; iq < A.nq; iq += gridDim.x) {
        const sslam_proj_query Q = A.q[iq];
        unsigned long long b = ~0ull;
        if (Q.valid) {
            const uint4 q0 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[0], q1 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[1];
            for (int i = lane; i < A.n; i += 64) {
                int cell = 0;
                if (A.kind == 0) {
                    const sslam_keypoint kp = kps[i];
                    cell = fuse_cell(G, kp.x, kp.y);
                    if (cell < 0) continue;
                    if (!fuse_point_window(Q, kp.x, kp.y, kp.octave)) continue;
                    if (A.chi2 && !fuse_point_chi2(Q, kp.x, kp.y, A.uright ? A.uright[i] : -1.f, fuse_inv_sigma2(A.invSigma2, A.nlevels, kp.octave))) continue;
                } else {
                    const sslam_keyline kl = kls[i];
                    if (!fuse_line_ok(Q, kl.pt_x, kl.pt_y, kl.angle, kl.octave)) continue;
                }
                const uint4* tp = (const uint4*)(A.desc + (size_t)i * 32);
                const unsigned long long kk = fuse_key(hamming256(q0, q1, tp[0], tp[1]), cell, i);
                b = kk < b ? kk : b;
            }
        }
        b = wave_min_u64(b);
        if (lane == 0) {
            A.bestIdx[iq] = fuse_key_idx(b);
            A.bestDist[iq] = fuse_key_dist(b);
        }
    }
}

// ------------------------------------------------------------------ Fuse / SearchBySim3 candidate search of a batch (sslam_fuse_search_batch_dev)
// The same search for jobs (keyframe slot, block of queries) on one device-resident pool of keyframe slots.  One workgroup of BATCH_WAVES waves
// per (job, chunk of FUSE_BATCH_CHUNK queries), the grid flattened job-major (match_plan.h).  Where k_fuse_search recomputes every feature's grid cell
// for every (query, feature) pair and reads 28 or 68 bytes of a row to test 12, the workgroup stages the keyframe's GEOMETRY once, as four arrays of
// cap words in dynamic LDS (FUSE_BATCH_ROW_BYTES per row): x, y, uright, octave of a keypoint, pt_x, pt_y, angle, octave of a keyline.  A keypoint in
// no grid cell is staged with x = NaN: every window test rejects it, which is what the single kernel's first gate does.  Consecutive lanes read
// consecutive words of one array: no bank conflicts.  Wave w takes the chunk's queries w, w + BATCH_WAVES, .. in turn and scans the rows
// lane-parallel; only a row that passed every gate -- a handful of a thousand under a window of 3 x scale -- has its cell computed and its 32-byte
// descriptor read, from global memory.  fuse_key and wave_min_u64 reduce as in the single kernel.
// d_nfound: the host zeroes it ahead of the launch; every workgroup adds the candidates of its chunk with ONE agent-scope atomic (none where it found
// nothing).  A skipped job gets -1 from its chunk 0 alone and its other chunks leave without adding, so no workgroup races with that store.
// Every loop is bounded by a clamped count or a constant; the two barriers sit behind conditions that are uniform over the workgroup (the job, its
// clamped query count and the chunk).  Rows at or past a keyframe's count, queries at or past a job's count and right coordinates of a NULL d_uright
// are never read.
struct FuseBatchArgs {
    int chi2;
    const void* feats; const uint8_t* desc; const float* uright; const int* n; int cap, nkeyframes;
    float minX, maxX, minY, maxY;
    int nlevels;
    const sslam_proj_query* q; int qcap; const uint8_t* qdesc; int nqdesc;
    const sslam_fuse_job* jobs; unsigned chunks;
    int* bestIdx; int* bestDist; int* nfound;
    float invSigma2[64];                     // the level table travels in the kernel's arguments: read from the caller's host array before the call returns; 0 past nlevels
};
// kLds: the keyframe's geometry in dynamic LDS; otherwise the scan reads the caller's buffers, with the single kernel's grid gate per row
template <int kind, bool kLds>
__global__ __launch_bounds__(64 * BATCH_WAVES) void k_fuse_search_batch(FuseBatchArgs A) {
    extern __shared__ __align__(16) unsigned fsl[];
    __shared__ float invS[64];
    __shared__ int total;
    constexpr int NT = 64 * BATCH_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned j = blockIdx.x / A.chunks, chunk = blockIdx.x - j * A.chunks;
    const sslam_fuse_job J = A.jobs[j];
    const int nq = min(max(J.nq, 0), A.qcap);
    // (uniform over the workgroup, ahead of every barrier)
    if (J.kf < 0 || J.kf >= A.nkeyframes || J.qdesc0 < 0 || (long long)J.qdesc0 + nq > (long long)A.nqdesc) {
        if (chunk == 0 && tid == 0) A.nfound[j] = -1;
        return;
    }
    const int q0 = (int)chunk * FUSE_BATCH_CHUNK, q1 = min(nq, q0 + FUSE_BATCH_CHUNK);
    if (q0 >= nq) return;                                        // d_nfound[j] keeps the host's 0 where the job has no query
    const int n = min(max(A.n[J.kf], 0), A.cap);      // slot_count (common.h), written out: through the helper the capacity is loaded ahead of the count and the LDS forms schedule differently
    const size_t r = (size_t)J.kf * (size_t)A.cap;
    const sslam_keypoint* kps = (const sslam_keypoint*)A.feats + r;
    const sslam_keyline* kls = (const sslam_keyline*)A.feats + r;
    const uint8_t* desc = A.desc + r * 32;
    const float* uright = A.uright ? A.uright + r : nullptr;
    const sslam_proj_query* qs = A.q + (size_t)j * (size_t)A.qcap;
    const uint8_t* qdesc = A.qdesc + (size_t)J.qdesc0 * 32;
    int* outIdx = A.bestIdx + (size_t)j * (size_t)A.qcap; int* outDist = A.bestDist + (size_t)j * (size_t)A.qcap;
    const FuseGrid G = fuse_grid(A.minX, A.maxX, A.minY, A.maxY);
    float* la = (float*)fsl; float* lb = la + A.cap; float* lc = lb + A.cap; int* lo = (int*)(lc + A.cap);
    if (kLds) {
        for (int i = tid; i < n; i += NT) {
            if (kind == 0) {
                const sslam_keypoint kp = kps[i];
                la[i] = fuse_cell(G, kp.x, kp.y) < 0 ? __int_as_float(0x7fc00000) : kp.x; lb[i] = kp.y;
                lc[i] = (A.chi2 && uright) ? uright[i] : -1.f; lo[i] = kp.octave;
            } else {
                const sslam_keyline kl = kls[i];
                la[i] = kl.pt_x; lb[i] = kl.pt_y; lc[i] = kl.angle; lo[i] = kl.octave;
            }
        }
    }
    if (tid < 64) invS[tid] = A.invSigma2[tid];
    if (tid == 0) total = 0;
    __syncthreads();
    // the scan: no workgroup barrier in here
    int found = 0;
    for (int iq = q0 + wave; iq < q1; iq += BATCH_WAVES) {
        const sslam_proj_query Q = qs[iq];
        unsigned long long b = ~0ull;
        if (Q.valid) {
            const uint4 d0 = ((const uint4*)(qdesc + (size_t)iq * 32))[0], d1 = ((const uint4*)(qdesc + (size_t)iq * 32))[1];
            for (int i = lane; i < n; i += 64) {
                int cell = 0;
                if (kind == 0) {
                    float x, y; int lvl;
                    if (kLds) { x = la[i]; y = lb[i]; lvl = lo[i]; }
                    else {
                        const sslam_keypoint kp = kps[i];
                        x = kp.x; y = kp.y; lvl = kp.octave;
                        if (fuse_cell(G, x, y) < 0) continue;
                    }
                    if (!fuse_point_window(Q, x, y, lvl)) continue;
                    if (A.chi2 && !fuse_point_chi2(Q, x, y, kLds ? lc[i] : (uright ? uright[i] : -1.f), fuse_inv_sigma2(invS, A.nlevels, lvl))) continue;
                    cell = fuse_cell(G, x, y);                   // survivors only: k_fuse_search's expression on the same two floats
                } else {
                    float px, py, ang; int lvl;
                    if (kLds) { px = la[i]; py = lb[i]; ang = lc[i]; lvl = lo[i]; }
                    else { const sslam_keyline* kl = kls + i; px = kl->pt_x; py = kl->pt_y; ang = kl->angle; lvl = kl->octave; }
                    if (!fuse_line_ok(Q, px, py, ang, lvl)) continue;
                }
                const uint4* tp = (const uint4*)(desc + (size_t)i * 32);
                const unsigned long long kk = fuse_key(hamming256(d0, d1, tp[0], tp[1]), cell, i);
                b = kk < b ? kk : b;
            }
        }
        b = wave_min_u64(b);
        if (lane == 0) { outIdx[iq] = fuse_key_idx(b); outDist[iq] = fuse_key_dist(b); }
        found += b != ~0ull ? 1 : 0;
    }
    if (lane == 0 && found) atomicAdd(&total, found);
    __syncthreads();
    if (tid == 0 && total) atomicAdd(&A.nfound[j], total);
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
// traffic between workgroups.  One workgroup of BATCH_WAVES waves per pair (match_plan.h).  The queries do not interact, so there is no chain and
// no ownership of nodes: wave w takes the keyframe-1 rows [64 (w + k BATCH_WAVES), +64), k = 0, 1, .., one row per lane, ballots the rows that
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
__global__ __launch_bounds__(64 * BATCH_WAVES) void k_tri_search_batch(TriBatchArgs A) {
    extern __shared__ __align__(16) unsigned trl[];
    __shared__ float scale2[64], sigma2_2[64];
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int keep[3];
    __shared__ int total;
    constexpr int NT = 64 * BATCH_WAVES;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sslam_tri_pair P = A.pairs[p];
    if (P.kf1 < 0 || P.kf1 >= A.nkeyframes || P.kf2 < 0 || P.kf2 >= A.nkeyframes) {      // (uniform over the workgroup, ahead of every barrier)
        if (tid == 0) A.nmatches[p] = 0;
        return;
    }
    const int n1 = slot_count(A.n, P.kf1, A.cap), n2 = slot_count(A.n, P.kf2, A.cap);
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
            if (m >= 0) atomicAdd(&hist[rot_hist_bin(kp1[i].angle, kp2[m].angle)], 1);
        }
        __syncthreads();
        if (tid == 0) three_maxima(hist, keep[0], keep[1], keep[2]);
        __syncthreads();
    }
    int cnt = 0;
    for (int i = tid; i < n1; i += NT) {
        const int m = out[i];
        if (m < 0) continue;
        if (A.checkOri && !rot_kept(rot_hist_bin(kp1[i].angle, kp2[m].angle), keep[0], keep[1], keep[2])) { out[i] = -1; continue; }
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
        if ((int)(i - f * (unsigned)cap) >= slot_count(counts, f, cap)) return;
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
