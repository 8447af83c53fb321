// Order-dependent matchers (an accepted match changes what later queries may take): SearchForInitialization, the
// projection-window family (two-kernel form and one-wave form), SearchByBoW (KeyFrame -> Frame and KeyFrame -> KeyFrame).
// Part of match.hip (included there, inside its anonymous namespace: one translation unit).  Not a standalone header.
#pragma once

// ---------------------------------------------------------------- SearchForInitialization
// One wave per frame pair.  The i1 loop is sequential (vMatchedDistance / un-match
// semantics); the candidate scan of each step is wave-parallel.  The
// GetFeaturesInArea order (grid cell x-major, then y, then index — D.4) is carried in
// the reduction key so "first strictly smaller distance wins" is reproduced.
struct SfiArgs {
    const sslam_keypoint* kp1; const uint8_t* d1; const int* n1;
    const sslam_keypoint* kp2; const uint8_t* d2; const int* n2;
    int cap, n1s, n2s;             // n1s/n2s used when n1/n2 pointers are null
    float* prevMatched; int* m12; int* nmatches;
    int* scratch;                  // per pair: matchedDist[cap], m21[cap], cand[cap], key[cap], bin[cap]
    int window; float nnratio; int checkOri;
    float minX, maxX, minY, maxY;
    int ccap;                      // k_search_init_lds: LDS capacity in level-0 candidates / level-0 keypoints of F1, always > 0 (SfiPlan::ccap; the kernel's 0 = "the pair's own counts" has no caller)
};

// the two ends every form of the matcher shares.  rot_prune_wave's un-match: an F1 keypoint whose match a later one took over is no match any more
__device__ __forceinline__ bool sfi_unmatch(int* m12, int i) {
    if (m12[i] < 0) return false;
    m12[i] = -1;
    return true;
}
// the epilogue, by nt threads of which this is tid: vbPrevMatched takes the matched keypoints' positions (src/ORBmatcher.cc:519-521), then the count
__device__ __forceinline__ void sfi_write_back(const SfiArgs& A, int p, int n1, const sslam_keypoint* kp2, float* pm, const int* m12, int nmatches, int tid, int nt) {
    for (int i = tid; i < n1; i += nt) {
        const int m = m12[i];
        if (m >= 0) { pm[i * 2] = kp2[m].x; pm[i * 2 + 1] = kp2[m].y; }
    }
    if (tid == 0) A.nmatches[p] = nmatches;
}

// the pair's state in global memory (what a pair falls back to when its level-0 features do not fit the LDS capacity of the batch launch)
__device__ __forceinline__ void sfi_global_body(const SfiArgs& A, int p, int lane, int* __restrict__ hist) {
    const int n1 = A.n1 ? A.n1[p] : A.n1s, n2 = A.n2 ? A.n2[p] : A.n2s;
    const sslam_keypoint* kp1 = A.kp1 + (size_t)p * A.cap;
    const sslam_keypoint* kp2 = A.kp2 + (size_t)p * A.cap;
    const uint8_t* d1 = A.d1 + (size_t)p * A.cap * 32;
    const uint8_t* d2 = A.d2 + (size_t)p * A.cap * 32;
    float* pm = A.prevMatched + (size_t)p * A.cap * 2;
    int* m12 = A.m12 + (size_t)p * A.cap;
    int* matchedDist = A.scratch + (size_t)p * A.cap * 5;
    int* m21 = matchedDist + A.cap;
    int* cand = m21 + A.cap;       // compact list of F2 level-0, in-grid keypoints
    int* ckey = cand + A.cap;      // their GetFeaturesInArea order key
    int* binOf = ckey + A.cap;     // rotation bin of i1 (or -1)

    const float invW = __fdiv_rn((float)GRID_COLS, __fsub_rn(A.maxX, A.minX));
    const float invH = __fdiv_rn((float)GRID_ROWS, __fsub_rn(A.maxY, A.minY));
    for (int i = lane; i < n1; i += 64) { m12[i] = -1; binOf[i] = -1; }
    for (int i = lane; i < n2; i += 64) { matchedDist[i] = 0x7FFFFFFF; m21[i] = -1; }
    if (lane < HISTO_LENGTH) hist[lane] = 0;
    // candidates of level 0 that sit in the 64x48 grid (PosInGrid, src/Frame.cc:462-472)
    int nc = 0;
    for (int j0 = 0; j0 < n2; j0 += 64) {
        int j = j0 + lane;
        bool ok = false; int key = 0;
        if (j < n2) {
            const sslam_keypoint k = kp2[j];
            int px = (int)roundf(__fmul_rn(__fsub_rn(k.x, A.minX), invW));
            int py = (int)roundf(__fmul_rn(__fsub_rn(k.y, A.minY), invH));
            ok = k.octave == 0 && px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS;     // level1 == 0 -> minLevel=maxLevel=0
            key = ((px * GRID_ROWS + py) << 19) | j;
        }
        unsigned long long m = __ballot(ok);
        if (ok) { int o = nc + mbcnt(m); cand[o] = j; ckey[o] = key; }
        nc += __popcll(m);
    }
    __syncthreads();
    int nmatches = 0;
    const float r = (float)A.window;
    for (int i1 = 0; i1 < n1; ++i1) {
        const int level1 = kp1[i1].octave;
        if (level1 > 0) continue;
        const float cx = pm[i1 * 2], cy = pm[i1 * 2 + 1];
        const uint4 q0 = ((const uint4*)(d1 + (size_t)i1 * 32))[0], q1 = ((const uint4*)(d1 + (size_t)i1 * 32))[1];
        unsigned long long b = ~0ull; unsigned s2 = 0x7FFFFFFFu;    // best key (dist<<32|orderkey), second-best distance
        for (int c = lane; c < nc; c += 64) {
            const int j = cand[c];
            const float dx = __fsub_rn(kp2[j].x, cx), dy = __fsub_rn(kp2[j].y, cy);
            if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
            const uint4* tp = (const uint4*)(d2 + (size_t)j * 32);
            const int dist = hamming256(q0, q1, tp[0], tp[1]);
            if (matchedDist[j] <= dist) continue;
            unsigned long long k = ((unsigned long long)dist << 32) | (unsigned)ckey[c];
            if (k < b) { if (b != ~0ull) s2 = min(s2, (unsigned)(b >> 32)); b = k; }
            else s2 = min(s2, (unsigned)dist);
        }
        const unsigned long long best = wave_min_u64(b);
        if (best == ~0ull) continue;                   // vIndices2 empty, or every candidate suppressed: bestDist stays INT_MAX
        unsigned other = (b == best) ? s2 : min(s2, (unsigned)(b >> 32));
        if (b == ~0ull) other = 0x7FFFFFFFu;
        const unsigned second = wave_min_u32(other);
        const int bestDist = (int)(best >> 32);
        const int bestIdx2 = (int)(best & 0x7FFFF);
        if (bestDist <= TH_LOW && (float)bestDist < __fmul_rn((float)(int)second, A.nnratio)) {
            const int prev = m21[bestIdx2];
            if (prev >= 0) { if (lane == 0) m12[prev] = -1; nmatches--; }
            if (lane == 0) { m12[i1] = bestIdx2; m21[bestIdx2] = i1; matchedDist[bestIdx2] = bestDist; }
            nmatches++;
            if (A.checkOri) {
                const int bin = rot_bin(kp1[i1].angle, kp2[bestIdx2].angle);
                if (lane == 0) { binOf[i1] = bin; hist[bin]++; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (A.checkOri) nmatches -= rot_prune_wave(hist, n1, lane, [&](int i) { return binOf[i]; }, [&](int i) { return sfi_unmatch(m12, i); });
    __syncthreads();
    sfi_write_back(A, p, n1, kp2, pm, m12, nmatches, lane, 64);
}

__global__ __launch_bounds__(64) void k_search_init(SfiArgs A) {
    __shared__ int hist[HISTO_LENGTH];
    sfi_global_body(A, xcd_mix_frame(blockIdx.x, gridDim.x), threadIdx.x, hist);      // one wave per frame pair: see xcd_mix_frame
}


// The LDS form, one wave per pair (written for the single call, which k_search_init_spec below serves now; launched for batches): the same
// sequential i1 loop, but everything an iteration touches lives in LDS -- the level-0 keypoints of F1 as a compact list, and per candidate of F2 its
// position, GetFeaturesInArea order key, descriptor, matched distance and owner -- so a step is LDS reads plus one prefetched query
// descriptor instead of a chain of dependent global loads (~1 us each with one wave on the chip).  Semantics identical to k_search_init:
// candidates are compacted in ascending index, so (cell, slot) orders like (cell, index).
// dynamic LDS: per candidate 14 words (x, y, key, index, matchedDist, owner, 8 descriptor words) + per F1 keypoint 2 words (level-0 list, bin)
__global__ __launch_bounds__(64) void k_search_init_lds(SfiArgs A) {
    extern __shared__ __align__(16) unsigned sfi[];
    const int p = A.ccap > 0 ? xcd_mix_frame(blockIdx.x, gridDim.x) : blockIdx.x, lane = threadIdx.x;
    const int n1 = A.n1 ? A.n1[p] : A.n1s, n2 = A.n2 ? A.n2[p] : A.n2s;
    // Round 4: also the batch form.  Only LEVEL-0 features enter the search (a fifth of a frame's keypoints), so the arrays are sized by a
    // capacity in level-0 features chosen by the host (ccap; 0 = the pair's own counts, the single call) -- ~25 KB for 1000-keypoint frames, six
    // pairs per compute unit -- and a pair that exceeds it takes the global-memory body.  The batch kernel before gathered every candidate's
    // position, key, descriptor and matched distance from global memory for every query: 2.45 MB of HBM traffic per pair for 72 KB of inputs.
    const int cc = A.ccap > 0 ? A.ccap : n2, lc = A.ccap > 0 ? A.ccap : n1;
    const sslam_keypoint* kp1 = A.kp1 + (size_t)p * A.cap;
    const sslam_keypoint* kp2 = A.kp2 + (size_t)p * A.cap;
    const uint8_t* d1 = A.d1 + (size_t)p * A.cap * 32;
    const uint8_t* d2 = A.d2 + (size_t)p * A.cap * 32;
    float* pm = A.prevMatched + (size_t)p * A.cap * 2;
    int* m12 = A.m12 + (size_t)p * A.cap;
    uint4* cdesc = (uint4*)sfi;                              // [2 * cc]
    float* cxs = (float*)(cdesc + 2 * (size_t)cc);            // [cc]
    float* cys = cxs + cc;
    int* ckey = (int*)(cys + cc);
    int* cj = ckey + cc;
    int* md = cj + cc;                                       // matched distance per candidate slot
    int* owner = md + cc;                                    // m21 per candidate slot
    int* list1 = owner + cc;                                 // level-0 keypoints of F1, ascending  [lc]
    int* binOf = list1 + lc;                                 // rotation bin per entry of list1, -1  [lc]
    __shared__ int hist[HISTO_LENGTH];
    const float invW = __fdiv_rn((float)GRID_COLS, __fsub_rn(A.maxX, A.minX));
    const float invH = __fdiv_rn((float)GRID_ROWS, __fsub_rn(A.maxY, A.minY));
    if (lane < HISTO_LENGTH) hist[lane] = 0;
    int nl = 0;
    for (int i0 = 0; i0 < n1; i0 += 64) {
        const int i = i0 + lane;
        const bool l0 = i < n1 && kp1[i].octave == 0;
        if (i < n1) m12[i] = -1;
        const unsigned long long m = __ballot(l0);
        if (l0) { const int o = nl + mbcnt(m); if (o < lc) { list1[o] = i; binOf[o] = -1; } }
        nl += __popcll(m);
    }
    int nc = 0;
    for (int j0 = 0; j0 < n2; j0 += 64) {
        const int j = j0 + lane;
        bool ok = false; int cell = 0; float x = 0, y = 0;
        if (j < n2) {
            const sslam_keypoint k = kp2[j];
            const int px = (int)roundf(__fmul_rn(__fsub_rn(k.x, A.minX), invW));
            const int py = (int)roundf(__fmul_rn(__fsub_rn(k.y, A.minY), invH));
            ok = k.octave == 0 && px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS;
            cell = px * GRID_ROWS + py; x = k.x; y = k.y;
        }
        const unsigned long long m = __ballot(ok);
        if (ok && nc + mbcnt(m) < cc) {
            const int o = nc + mbcnt(m);
            cxs[o] = x; cys[o] = y; ckey[o] = (cell << 19) | o; cj[o] = j; md[o] = 0x7FFFFFFF; owner[o] = -1;
            const uint4* tp = (const uint4*)(d2 + (size_t)j * 32);
            cdesc[2 * o] = tp[0]; cdesc[2 * o + 1] = tp[1];
        }
        nc += __popcll(m);
    }
    __syncthreads();
    if (nl > lc || nc > cc) { sfi_global_body(A, p, lane, hist); return; }      // (wave-uniform) more level-0 features than the launch planned for
    int nmatches = 0;
    const float r = (float)A.window;
    uint4 q0n = make_uint4(0, 0, 0, 0), q1n = q0n; float cxn = 0, cyn = 0;
    if (nl > 0) { const int i = list1[0]; q0n = ((const uint4*)(d1 + (size_t)i * 32))[0]; q1n = ((const uint4*)(d1 + (size_t)i * 32))[1]; cxn = pm[i * 2]; cyn = pm[i * 2 + 1]; }
    for (int t = 0; t < nl; ++t) {
        const int i1 = list1[t];
        const uint4 q0 = q0n, q1 = q1n; const float cx = cxn, cy = cyn;
        if (t + 1 < nl) { const int i = list1[t + 1]; q0n = ((const uint4*)(d1 + (size_t)i * 32))[0]; q1n = ((const uint4*)(d1 + (size_t)i * 32))[1]; cxn = pm[i * 2]; cyn = pm[i * 2 + 1]; }
        unsigned long long b = ~0ull; unsigned s2 = 0x7FFFFFFFu;
        for (int c = lane; c < nc; c += 64) {
            const float dx = __fsub_rn(cxs[c], cx), dy = __fsub_rn(cys[c], cy);
            if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
            const int dist = hamming256(q0, q1, cdesc[2 * c], cdesc[2 * c + 1]);
            if (md[c] <= dist) continue;
            const unsigned long long k = ((unsigned long long)dist << 32) | (unsigned)ckey[c];
            if (k < b) { if (b != ~0ull) s2 = min(s2, (unsigned)(b >> 32)); b = k; }
            else s2 = min(s2, (unsigned)dist);
        }
        const unsigned long long best = wave_min_u64(b);
        if (best == ~0ull) continue;
        unsigned other = (b == best) ? s2 : min(s2, (unsigned)(b >> 32));
        if (b == ~0ull) other = 0x7FFFFFFFu;
        const unsigned second = wave_min_u32(other);
        const int bestDist = (int)(best >> 32);
        const int slot = (int)(best & 0x7FFFF);
        if (bestDist <= TH_LOW && (float)bestDist < __fmul_rn((float)(int)second, A.nnratio)) {
            const int bestIdx2 = cj[slot];
            const int prev = owner[slot];
            if (prev >= 0) { if (lane == 0) m12[prev] = -1; nmatches--; }
            if (lane == 0) { m12[i1] = bestIdx2; owner[slot] = i1; md[slot] = bestDist; }
            nmatches++;
            if (A.checkOri) {
                const int bin = rot_bin(kp1[i1].angle, kp2[bestIdx2].angle);
                if (lane == 0) { binOf[t] = bin; hist[bin]++; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (A.checkOri) nmatches -= rot_prune_wave(hist, nl, lane, [&](int t) { return binOf[t]; }, [&](int t) { return sfi_unmatch(m12, list1[t]); });      // bins per entry of list1
    __syncthreads();
    sfi_write_back(A, p, n1, kp2, pm, m12, nmatches, lane, 64);
}

// Speculative form of the single call (round 3): sixteen waves evaluate sixteen consecutive level-0 keypoints of F1 against the state at the
// start of a round; wave 0 then commits them.  A match only ever LOWERS the matched distance of its candidate slot (a candidate is eligible
// while matchedDist > dist), so an earlier keypoint of the round can change a later one's result only through that slot being the later
// one's best or second-best candidate (removing any OTHER candidate cannot change best / second, so checking these two is exact).  Every
// accepting wave stamps its slot with (round, wave); if no
// wave finds an earlier stamp of the round on its best / second, all sixteen commit at once (un-matching the slots' previous owners, which
// are then keypoints of earlier rounds: distinct slots, distinct owners); otherwise the round is replayed serially with re-evaluation.
// Same LDS layout as k_search_init_lds plus the stamps; same results (tests/test_match_gpu.py runs contended pairs through this kernel,
// k_search_init_lds and k_search_init and compares each with the oracle).
constexpr int SFI_WAVES = 16;
struct SfiLds { uint4* cdesc; float* cxs; float* cys; int* ckey; int* cj; int* md; int* owner; int* stamp; };
__device__ __forceinline__ void sfi_scan(const SfiLds& S, int nc, float cx, float cy, float r, const uint4& q0, const uint4& q1, int lane,
                                         unsigned long long& best, unsigned long long& second) {
    unsigned long long b = ~0ull, s2 = ~0ull;
    for (int c = lane; c < nc; c += 64) {
        const float dx = __fsub_rn(S.cxs[c], cx), dy = __fsub_rn(S.cys[c], cy);
        if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
        const int dist = hamming256(q0, q1, S.cdesc[2 * c], S.cdesc[2 * c + 1]);
        if (S.md[c] <= dist) continue;
        const unsigned long long k = ((unsigned long long)dist << 32) | (unsigned)S.ckey[c];
        if (k < b) { s2 = b; b = k; } else if (k < s2) s2 = k;
    }
    best = wave_min_u64(b);
    second = wave_min_u64(b == best ? s2 : b);
}
__global__ __launch_bounds__(SFI_WAVES * 64) void k_search_init_spec(SfiArgs A) {
    extern __shared__ __align__(16) unsigned sfi[];
    constexpr int NT = SFI_WAVES * 64;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = A.n1 ? A.n1[p] : A.n1s, n2 = A.n2 ? A.n2[p] : A.n2s;
    const sslam_keypoint* kp1 = A.kp1 + (size_t)p * A.cap;
    const sslam_keypoint* kp2 = A.kp2 + (size_t)p * A.cap;
    const uint8_t* d1 = A.d1 + (size_t)p * A.cap * 32;
    const uint8_t* d2 = A.d2 + (size_t)p * A.cap * 32;
    float* pm = A.prevMatched + (size_t)p * A.cap * 2;
    int* m12 = A.m12 + (size_t)p * A.cap;
    SfiLds S;
    S.cdesc = (uint4*)sfi;
    S.cxs = (float*)(S.cdesc + 2 * (size_t)n2); S.cys = S.cxs + n2;
    S.ckey = (int*)(S.cys + n2); S.cj = S.ckey + n2; S.md = S.cj + n2; S.owner = S.md + n2; S.stamp = S.owner + n2;
    int* list1 = S.stamp + n2;                               // level-0 keypoints of F1, ascending  [n1]
    int* binOf = list1 + n1;                                 // rotation bin per F1 keypoint, -1   [n1]
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int sh_nl, sh_nc, sh_nm;
    __shared__ int rAcc[SFI_WAVES], rBest[SFI_WAVES], rSecond[SFI_WAVES], rDist[SFI_WAVES], rBin[SFI_WAVES];
    const float invW = __fdiv_rn((float)GRID_COLS, __fsub_rn(A.maxX, A.minX));
    const float invH = __fdiv_rn((float)GRID_ROWS, __fsub_rn(A.maxY, A.minY));
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) sh_nm = 0;
    for (int i = tid; i < n1; i += NT) { m12[i] = -1; binOf[i] = -1; }
    if (wave == 0) {                                         // the two compact lists, in ascending index (one wave: ordered compaction by ballots)
        int nl = 0;
        for (int i0 = 0; i0 < n1; i0 += 64) {
            const int i = i0 + lane;
            const bool l0 = i < n1 && kp1[i].octave == 0;
            const unsigned long long m = __ballot(l0);
            if (l0) list1[nl + mbcnt(m)] = i;
            nl += __popcll(m);
        }
        int nc = 0;
        for (int j0 = 0; j0 < n2; j0 += 64) {
            const int j = j0 + lane;
            bool ok = false; int cell = 0; float x = 0, y = 0;
            if (j < n2) {
                const sslam_keypoint k = kp2[j];
                const int px = (int)roundf(__fmul_rn(__fsub_rn(k.x, A.minX), invW));
                const int py = (int)roundf(__fmul_rn(__fsub_rn(k.y, A.minY), invH));
                ok = k.octave == 0 && px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS;
                cell = px * GRID_ROWS + py; x = k.x; y = k.y;
            }
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int o = nc + mbcnt(m);
                S.cxs[o] = x; S.cys[o] = y; S.ckey[o] = (cell << 19) | o; S.cj[o] = j; S.md[o] = 0x7FFFFFFF; S.owner[o] = -1; S.stamp[o] = 0;
            }
            nc += __popcll(m);
        }
        if (lane == 0) { sh_nl = nl; sh_nc = nc; }
    }
    __syncthreads();
    const int nl = sh_nl, nc = sh_nc;
    for (int c = tid; c < nc; c += NT) {                    // descriptors of the candidates, by all waves
        const uint4* tp = (const uint4*)(d2 + (size_t)S.cj[c] * 32);
        S.cdesc[2 * c] = tp[0]; S.cdesc[2 * c + 1] = tp[1];
    }
    __syncthreads();
    const float r = (float)A.window;
    auto decide = [&](int i1, unsigned long long best, unsigned long long second, int& acc, int& slot, int& slot2, int& dist, int& bin) {
        acc = 0; slot = -1; slot2 = -2; dist = 0; bin = -1;
        if (best == ~0ull) return;                           // vIndices2 empty, or every candidate suppressed
        slot = (int)(best & 0x7FFFF);
        if (second != ~0ull) slot2 = (int)(second & 0x7FFFF);
        const int bestDist = (int)(best >> 32);
        const unsigned sec = second == ~0ull ? 0x7FFFFFFFu : (unsigned)(second >> 32);
        if (bestDist <= TH_LOW && (float)bestDist < __fmul_rn((float)(int)sec, A.nnratio)) {
            acc = 1; dist = bestDist;
            if (A.checkOri) bin = rot_bin(kp1[i1].angle, kp2[S.cj[slot]].angle);
        }
    };
    for (int base = 0; base < nl; base += SFI_WAVES) {
        const int t = base + wave;
        int acc = 0, slot = -1, slot2 = -2, dist = 0, bin = -1;
        if (t < nl) {
            const int i1 = list1[t];
            const uint4 q0 = ((const uint4*)(d1 + (size_t)i1 * 32))[0], q1 = ((const uint4*)(d1 + (size_t)i1 * 32))[1];
            unsigned long long best, second;
            sfi_scan(S, nc, pm[i1 * 2], pm[i1 * 2 + 1], r, q0, q1, lane, best, second);
            decide(i1, best, second, acc, slot, slot2, dist, bin);
        }
        if (lane == 0) { rAcc[wave] = acc; rBest[wave] = slot; rSecond[wave] = slot2; rDist[wave] = dist; rBin[wave] = bin; }
        __syncthreads();
        if (wave == 0) {
            const int cnt = min(SFI_WAVES, nl - base);
            const int myAcc = lane < cnt ? rAcc[lane] : 0, myB = lane < cnt ? rBest[lane] : -1, myS = lane < cnt ? rSecond[lane] : -2;
            const int myDist = lane < cnt ? rDist[lane] : 0, myBin = lane < cnt ? rBin[lane] : -1;
            const int roundTag = base / SFI_WAVES + 1;
            if (lane < cnt && myAcc) atomicMax(&S.stamp[myB], (roundTag << 5) | (31 - lane));
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            bool clash = false;
            if (lane < cnt) {
                if (myB >= 0) { const int st = S.stamp[myB]; clash |= (st >> 5) == roundTag && 31 - (st & 31) < lane; }
                if (myS >= 0) { const int st = S.stamp[myS]; clash |= (st >> 5) == roundTag && 31 - (st & 31) < lane; }
            }
            int delta = 0;
            if (!__ballot(clash)) {
                bool unmatch = false;
                if (lane < cnt && myAcc) {
                    const int i1 = list1[base + lane];
                    const int prev = S.owner[myB];
                    if (prev >= 0) { m12[prev] = -1; unmatch = true; }
                    m12[i1] = S.cj[myB]; S.owner[myB] = i1; S.md[myB] = myDist;
                    if (A.checkOri) { binOf[i1] = myBin; atomicAdd(&hist[myBin], 1); }
                }
                delta = __popcll(__ballot(lane < cnt && myAcc)) - __popcll(__ballot(unmatch));
            } else {
                // serial replay of the round: a keypoint is re-evaluated when an earlier one of the round took its best or second-best slot
                int myTaken = -3, nTaken = 0;
                for (int w = 0; w < cnt; ++w) {
                    int a = __builtin_amdgcn_readlane(myAcc, w), b = __builtin_amdgcn_readlane(myB, w), ds = __builtin_amdgcn_readlane(myDist, w), bn = __builtin_amdgcn_readlane(myBin, w);
                    const int s2 = __builtin_amdgcn_readlane(myS, w);
                    const int i1 = list1[base + w];
                    if (nTaken > 0 && __ballot(lane < nTaken && (myTaken == b || myTaken == s2))) {
                        const uint4 q0 = ((const uint4*)(d1 + (size_t)i1 * 32))[0], q1 = ((const uint4*)(d1 + (size_t)i1 * 32))[1];
                        unsigned long long best, second; int sl2;
                        sfi_scan(S, nc, pm[i1 * 2], pm[i1 * 2 + 1], r, q0, q1, lane, best, second);
                        decide(i1, best, second, a, b, sl2, ds, bn);
                    }
                    if (!a) continue;
                    const int prev = S.owner[b];
                    if (prev >= 0) { if (lane == 0) m12[prev] = -1; --delta; }
                    if (lane == 0) { m12[i1] = S.cj[b]; S.owner[b] = i1; S.md[b] = ds; if (A.checkOri) { binOf[i1] = bn; hist[bn]++; } }
                    ++delta;
                    if (lane == nTaken) myTaken = b;
                    ++nTaken;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                }
            }
            if (lane == 0) sh_nm += delta;
        }
        __syncthreads();
    }
    int nmatches = sh_nm;
    __syncthreads();
    if (A.checkOri && wave == 0) nmatches -= rot_prune_wave(hist, n1, lane, [&](int i) { return binOf[i]; }, [&](int i) { return sfi_unmatch(m12, i); });      // (tid 0, which stores the count, is in wave 0)
    __syncthreads();
    sfi_write_back(A, p, n1, kp2, pm, m12, nmatches, tid, NT);
}

// ---------------------------------------------------------------- projection-window matchers
// ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th)  src/ORBmatcher.cc:45-129   (kind 0, mode 0)
// ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)  src/ORBmatcher.cc:1331-1473 (kind 0, mode 1)
// LSDmatcher::SearchByProjection(Frame&, vector<MapLine*>&, th) / (Frame&, const Frame&, ...) src/LSDmatcher.cpp:185-255,22-141 (kind 1, mode 0)
// One wave per problem.  Queries are consumed sequentially (an accepted match occupies its keypoint for
// the later queries); the candidate scan of each query is wave-parallel, with the reference's candidate
// order (GetFeaturesInArea cell order / GetLinesInArea index order) carried in the reduction key.
struct ProjArgs {
    int kind, mode;
    const void* feats; const uint8_t* desc; int n;
    float minX, maxX, minY, maxY;
    const float* uright; const uint8_t* occIn;
    const sslam_proj_query* q; const uint8_t* qdesc; int nq;
    float nnratio; int thDist, checkOri;
    int* assigned; int* nmatches;
    int* scratch;          // occ[n], key[n], qbin[nq], qidx[nq]
    long long* stats;      // SSLAM_PROJ_STATS (development aid, two-kernel form): commit steps, re-scans, cycles in re-scans, total cycles
};

// the rotation check behind the walk of either form: a query matched and then removed leaves -2 on its feature (the reference NULLs the pointer,
// src/ORBmatcher.cc:1465).  qbin[iq]: the query's rotation bin or -1, qidx[iq]: the feature it took
__device__ __forceinline__ int proj_rot_prune(const ProjArgs& A, const int* hist, const int* qbin, const int* qidx, int lane) {
    return rot_prune_wave(hist, A.nq, lane, [&](int iq) { return qbin[iq]; }, [&](int iq) { A.assigned[qidx[iq]] = -2; return true; });
}

// one frame by one wave; hist: HISTO_LENGTH ints of the workgroup's LDS
__device__ __forceinline__ void search_proj_body(const ProjArgs& A, int lane, int* __restrict__ hist) {
    const int n = A.n, nq = A.nq;
    int* occ = A.scratch; int* key = occ + n; int* qbin = key + n; int* qidx = qbin + nq;
    const sslam_keypoint* kps = (const sslam_keypoint*)A.feats;
    const sslam_keyline* kls = (const sslam_keyline*)A.feats;
    if (lane < HISTO_LENGTH) hist[lane] = 0;
    const float invW = __fdiv_rn((float)GRID_COLS, __fsub_rn(A.maxX, A.minX));
    const float invH = __fdiv_rn((float)GRID_ROWS, __fsub_rn(A.maxY, A.minY));
    for (int i = lane; i < n; i += 64) {
        occ[i] = A.occIn ? (int)A.occIn[i] : 0;
        A.assigned[i] = -1;
        int k = i;                                  // lines: GetLinesInArea scans in index order
        if (A.kind == 0) {
            const int px = (int)roundf(__fmul_rn(__fsub_rn(kps[i].x, A.minX), invW));
            const int py = (int)roundf(__fmul_rn(__fsub_rn(kps[i].y, A.minY), invH));
            k = (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) ? (((px * GRID_ROWS + py) << 19) | i) : -1;
        }
        key[i] = k;
    }
    for (int i = lane; i < nq; i += 64) qbin[i] = -1;
    __syncthreads();
    int nmatches = 0;
    for (int iq = 0; iq < nq; ++iq) {
        const sslam_proj_query Q = A.q[iq];
        if (!Q.valid) continue;
        const uint4 q0 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[0], q1 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[1];
        unsigned long long b = ~0ull, s = ~0ull;
        bool any = false;
        for (int i = lane; i < n; i += 64) {
            const int k = key[i];
            if (k < 0) continue;
            int oct;
            if (A.kind == 0) {
                const sslam_keypoint kp = kps[i];
                oct = kp.octave;
                if (Q.min_level > 0 || Q.max_level >= 0) {
                    if (oct < Q.min_level) continue;
                    if (Q.max_level >= 0 && oct > Q.max_level) continue;
                }
                const float dx = __fsub_rn(kp.x, Q.u), dy = __fsub_rn(kp.y, Q.v);
                if (!(fabsf(dx) < Q.radius && fabsf(dy) < Q.radius)) continue;
            } else {
                const sslam_keyline kl = kls[i];
                oct = kl.octave;
                const double mxp = 0.5 * (double)__fadd_rn(Q.u, Q.u2) - (double)kl.pt_x, myp = 0.5 * (double)__fadd_rn(Q.v, Q.v2) - (double)kl.pt_y;
                const float distance = (float)(mxp * mxp + myp * myp);
                if (distance > __fmul_rn(Q.radius, Q.radius)) continue;
                const float slope = __fsub_rn(__fdiv_rn(__fsub_rn(Q.v, Q.v2), __fsub_rn(Q.u, Q.u2)), kl.angle);
                if ((double)slope > (double)Q.radius * 0.01) continue;
                if (Q.min_level > 0 || Q.max_level > 0) {
                    if (oct < Q.min_level) continue;
                    if (Q.max_level >= 0 && oct > Q.max_level) continue;
                }
            }
            any = true;                              // vIndices non-empty
            if (occ[i]) continue;
            if (A.kind == 0 && A.uright) {
                const float ur = A.uright[i];
                if (ur > 0 && fabsf(__fsub_rn(Q.ur, ur)) > Q.radius) continue;
            }
            const uint4* tp = (const uint4*)(A.desc + (size_t)i * 32);
            const unsigned long long kk = ((unsigned long long)hamming256(q0, q1, tp[0], tp[1]) << 32) | (unsigned)k;
            if (kk < b) { s = b; b = kk; } else if (kk < s) s = kk;
        }
        if (!__ballot(any)) continue;
        const unsigned long long best = wave_min_u64(b);
        const unsigned long long second = wave_min_u64(b == best ? s : b);
        int bestDist = 256, bestLevel = -1, bestIdx = -1, bestDist2 = 256, bestLevel2 = -1;
        if (best != ~0ull && (int)(best >> 32) < 256) {
            bestDist = (int)(best >> 32); bestIdx = (int)(best & 0x7FFFF);
            bestLevel = A.kind == 0 ? kps[bestIdx].octave : kls[bestIdx].octave;
        }
        if (A.mode == 0 && second != ~0ull && (int)(second >> 32) < 256) {
            bestDist2 = (int)(second >> 32);
            const int i2 = (int)(second & 0x7FFFF);
            bestLevel2 = A.kind == 0 ? kps[i2].octave : kls[i2].octave;
        }
        if (bestDist <= A.thDist && bestIdx >= 0) {
            if (A.mode == 0 && bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(A.nnratio, (float)bestDist2)) continue;
            ++nmatches;
            if (lane == 0) { A.assigned[bestIdx] = iq; occ[bestIdx] = Q.obs_positive ? 1 : 0; }
            if (A.mode == 1 && A.checkOri) {
                const int bin = rot_bin(Q.angle, kps[bestIdx].angle);
                if (lane == 0) { qbin[iq] = bin; qidx[iq] = bestIdx; hist[bin]++; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (A.mode == 1 && A.checkOri) nmatches -= proj_rot_prune(A, hist, qbin, qidx, lane);
    if (lane == 0) *A.nmatches = nmatches;
}
__global__ __launch_bounds__(64) void k_search_proj(ProjArgs A) {
    __shared__ int hist[HISTO_LENGTH];
    search_proj_body(A, threadIdx.x, hist);
}


// ------------------------------------------------------------------ projection matchers, two-kernel form (round 3: the single call)
// A single workgroup with the frame in LDS and sixteen speculative queries per round (rounds 2-5, removed since) kept one CU busy: sixteen
// waves share four SIMDs, so a round of sixteen candidate scans was bound by that CU's issue rate (5.5 k cycles per round measured, 63 rounds
// per 1000 queries), and its commit fell back to a serial replay whenever two queries of a round met on a feature (62 % of the rounds on
// neighbouring keypoints): 0.43-0.51 ms per call against 0.26-0.44 ms on one CPU core.  The candidate SET of a query is static -- window, level range, stereo gate and the initial occupancy do not depend on earlier
// queries; only "taken by an earlier accepted query" does.  So:
//   k_proj_topk    one wave per query over the whole chip: scan every feature once, keep the PROJ_K smallest keys (distance, then the
//                  reference's candidate order -- GetFeaturesInArea cell order / GetLinesInArea index order --, level in the low bits) and
//                  the number of eligible candidates;
//   k_proj_commit  one wave walks the queries in order, 64 at a time: every pending query picks the first (and second) entry of its list
//                  that is still free, accepting queries stamp their feature, and the longest prefix of queries on whose picks no EARLIER
//                  pending query has a stamp commits at once (their decisions cannot influence each other); the first query with a stamp
//                  in front of it simply picks again in the next step, now as the first pending one.  A query whose list runs out of
//                  free entries although it had more candidates than PROJ_K is re-scanned against the live occupancy (rare).
// The result equals the sequential loop: a query's pick is "smallest key among its candidates that are free when its turn comes", and a
// prefix commits only when that set of free candidates is already final for every query in it.
// Measured (1000 queries against 1000 keypoints): 0.14-0.22 ms per call, CPU oracle 0.26-0.46 ms (profiles/r03_matchers.txt).
// PROJ_K, the list length, lives in match_plan.h: the scratch of a batch is sized by it
struct ProjTopArgs { ProjArgs A; unsigned long long* top; int* cnt; };

// the candidate test of one (query, feature) pair, features in global memory; returns false when the feature is no candidate.
// key = dist << 35 | order << 4 | level, order = (cell << 19 | index) for keypoints, index for lines
template <class OccFn>
__device__ __forceinline__ bool proj_candidate(const ProjArgs& A, const sslam_proj_query& Q, const uint4& q0, const uint4& q1, int i, float invW, float invH, OccFn occupied,
                                               unsigned long long& key) {
    const sslam_keypoint* kps = (const sslam_keypoint*)A.feats;
    const sslam_keyline* kls = (const sslam_keyline*)A.feats;
    int oct; unsigned order = (unsigned)i;
    if (A.kind == 0) {
        const sslam_keypoint kp = kps[i];
        oct = kp.octave;
        if (Q.min_level > 0 || Q.max_level >= 0) {
            if (oct < Q.min_level) return false;
            if (Q.max_level >= 0 && oct > Q.max_level) return false;
        }
        const float dx = __fsub_rn(kp.x, Q.u), dy = __fsub_rn(kp.y, Q.v);
        if (!(fabsf(dx) < Q.radius && fabsf(dy) < Q.radius)) return false;
        const int px = (int)roundf(__fmul_rn(__fsub_rn(kp.x, A.minX), invW));
        const int py = (int)roundf(__fmul_rn(__fsub_rn(kp.y, A.minY), invH));
        if (!(px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS)) return false;      // not in the grid: GetFeaturesInArea never returns it
        order = ((unsigned)(px * GRID_ROWS + py) << 19) | (unsigned)i;
    } else {
        const sslam_keyline kl = kls[i];
        oct = kl.octave;
        const double mxp = 0.5 * (double)__fadd_rn(Q.u, Q.u2) - (double)kl.pt_x, myp = 0.5 * (double)__fadd_rn(Q.v, Q.v2) - (double)kl.pt_y;
        const float distance = (float)(mxp * mxp + myp * myp);
        if (distance > __fmul_rn(Q.radius, Q.radius)) return false;
        const float slope = __fsub_rn(__fdiv_rn(__fsub_rn(Q.v, Q.v2), __fsub_rn(Q.u, Q.u2)), kl.angle);
        if ((double)slope > (double)Q.radius * 0.01) return false;
        if (Q.min_level > 0 || Q.max_level > 0) {
            if (oct < Q.min_level) return false;
            if (Q.max_level >= 0 && oct > Q.max_level) return false;
        }
    }
    if (occupied(i)) return false;
    if (A.kind == 0 && A.uright) {
        const float ur = A.uright[i];
        if (ur > 0 && fabsf(__fsub_rn(Q.ur, ur)) > Q.radius) return false;
    }
    const uint4* tp = (const uint4*)(A.desc + (size_t)i * 32);
    key = ((unsigned long long)hamming256(q0, q1, tp[0], tp[1]) << 35) | ((unsigned long long)order << 4) | (unsigned)(oct & 15);
    return true;
}
__device__ __forceinline__ int proj_key_feature(unsigned long long key) { return (int)((key >> 4) & 0x7FFFFu); }

// query iq (< A.nq) of one frame by one wave
__device__ __forceinline__ void proj_topk_body(const ProjTopArgs& T, int iq, int lane) {
    const ProjArgs& A = T.A;
    const sslam_proj_query Q = A.q[iq];
    unsigned long long t[PROJ_K];
#pragma unroll
    for (int k = 0; k < PROJ_K; ++k) t[k] = ~0ull;
    int cnt = 0;
    if (Q.valid) {
        const float invW = __fdiv_rn((float)GRID_COLS, __fsub_rn(A.maxX, A.minX));
        const float invH = __fdiv_rn((float)GRID_ROWS, __fsub_rn(A.maxY, A.minY));
        const uint4 q0 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[0], q1 = ((const uint4*)(A.qdesc + (size_t)iq * 32))[1];
        const uint8_t* occIn = A.occIn;
        for (int i = lane; i < A.n; i += 64) {
            unsigned long long kk;
            if (!proj_candidate(A, Q, q0, q1, i, invW, invH, [&](int f) { return occIn && occIn[f]; }, kk)) continue;
            ++cnt;
            if (kk < t[PROJ_K - 1]) {                        // the lane's own PROJ_K smallest, ascending (one insertion pass)
                t[PROJ_K - 1] = kk;
#pragma unroll
                for (int k = PROJ_K - 1; k > 0; --k) if (t[k] < t[k - 1]) { const unsigned long long x = t[k - 1]; t[k - 1] = t[k]; t[k] = x; }
            }
        }
    }
    cnt = wave_sum(cnt);
#pragma unroll
    for (int k = 0; k < PROJ_K; ++k) {                       // merge: the wave's smallest, K times (keys are unique: they carry the feature index)
        const unsigned long long m = wave_min_u64(t[0]);
        if (lane == 0) T.top[(size_t)iq * PROJ_K + k] = m;
        if (t[0] == m && m != ~0ull) {
#pragma unroll
            for (int j = 0; j + 1 < PROJ_K; ++j) t[j] = t[j + 1];
            t[PROJ_K - 1] = ~0ull;
        }
    }
    if (lane == 0) T.cnt[iq] = cnt;
}
__global__ __launch_bounds__(256) void k_proj_topk(ProjTopArgs T) {
    const int lane = threadIdx.x & 63, iq = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (iq >= T.A.nq) return;
    proj_topk_body(T, iq, lane);
}

// accept / reject on (best, second) keys of the layout above: thresholds, same-level ratio test (mode 0), rotation bin (mode 1)
__device__ __forceinline__ void proj_decide_keys(const ProjArgs& A, float qAngle, unsigned long long b, unsigned long long s2, int& acc, int& bin) {
    acc = 0; bin = -1;
    if (b == ~0ull) return;
    const int bestDist = (int)(b >> 35), bestLevel = (int)(b & 15);
    int bestDist2 = 256, bestLevel2 = -1;
    if (A.mode == 0 && s2 != ~0ull) { bestDist2 = (int)(s2 >> 35); bestLevel2 = (int)(s2 & 15); }
    if (bestDist > A.thDist || bestDist >= 256) return;
    if (A.mode == 0 && bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(A.nnratio, (float)bestDist2)) return;
    acc = 1;
    if (A.mode == 1 && A.checkOri) bin = rot_bin(qAngle, ((const sslam_keypoint*)A.feats)[proj_key_feature(b)].angle);
}

// the same test on a copy of the frame's features in LDS (k_proj_commit's re-scan); every field first, the tests afterwards: one LDS round
// trip per feature instead of one per early exit
struct ProjFeatLds { const uint4* desc; const float* x; const float* y; const float* ang; const float* ur; const int* oct; const int* order; };
__device__ __forceinline__ bool proj_candidate_lds(const ProjArgs& A, const ProjFeatLds& F, const sslam_proj_query& Q, const uint4& q0, const uint4& q1, int i, const int* __restrict__ occ,
                                                   unsigned long long& key) {
    const int order = F.order[i], oct = F.oct[i], occupied = occ[i];
    const float fx = F.x[i], fy = F.y[i], fang = F.ang[i], fur = F.ur[i];
    bool ok = order >= 0 && !occupied;                        // (order < 0: keypoint outside the grid)
    if (A.kind == 0) {
        if (Q.min_level > 0 || Q.max_level >= 0) ok = ok && oct >= Q.min_level && !(Q.max_level >= 0 && oct > Q.max_level);
        const float dx = __fsub_rn(fx, Q.u), dy = __fsub_rn(fy, Q.v);
        ok = ok && fabsf(dx) < Q.radius && fabsf(dy) < Q.radius;
        if (A.uright) ok = ok && !(fur > 0 && fabsf(__fsub_rn(Q.ur, fur)) > Q.radius);
    } else {
        const double mxp = 0.5 * (double)__fadd_rn(Q.u, Q.u2) - (double)fx, myp = 0.5 * (double)__fadd_rn(Q.v, Q.v2) - (double)fy;
        const float distance = (float)(mxp * mxp + myp * myp);
        ok = ok && !(distance > __fmul_rn(Q.radius, Q.radius));
        const float slope = __fsub_rn(__fdiv_rn(__fsub_rn(Q.v, Q.v2), __fsub_rn(Q.u, Q.u2)), fang);
        ok = ok && !((double)slope > (double)Q.radius * 0.01);
        if (Q.min_level > 0 || Q.max_level > 0) ok = ok && oct >= Q.min_level && !(Q.max_level >= 0 && oct > Q.max_level);
    }
    if (!ok) return false;
    key = ((unsigned long long)hamming256(q0, q1, F.desc[2 * i], F.desc[2 * i + 1]) << 35) | ((unsigned long long)(unsigned)order << 4) | (unsigned)(oct & 15);
    return true;
}

// dynamic LDS: occ[n], stamp[n] (+ with featsInLds the frame's features: descriptors, positions, angle, right coordinate, level, order key).
// PROJ_MAXN (match_plan.h, where the host decides featsInLds) bounds the frames that take that copy: 64 bytes per feature must fit the 160 KB
// of one compute unit next to the static arrays below.
static_assert(64 * (size_t)PROJ_MAXN + 64 + 1024 <= 160 * 1024, "k_proj_commit: PROJ_MAXN features do not fit one compute unit's LDS");
// one frame by one wave; pc: the dynamic LDS described above, hist: HISTO_LENGTH ints of the workgroup's LDS
__device__ __forceinline__ void proj_commit_body(const ProjTopArgs& T, int featsInLds, int* __restrict__ pc, int* __restrict__ hist, int lane) {
    const ProjArgs& A = T.A;
    const int n = A.n, nq = A.nq;
    ProjFeatLds F;
    uint4* fdesc = (uint4*)pc;                                  // [2n] when featsInLds
    int* rest = featsInLds ? (int*)(fdesc + 2 * (size_t)n) : pc;
    int* occ = rest; int* stamp = rest + n;
    float* fx = (float*)(stamp + n); float* fy = fx + n; float* fang = fy + n; float* fur = fang + n; int* foct = (int*)(fur + n); int* ford = foct + n;
    F.desc = fdesc; F.x = fx; F.y = fy; F.ang = fang; F.ur = fur; F.oct = foct; F.order = ford;
    int* qbin = A.scratch + 2 * n; int* qidx = qbin + nq;          // the scratch layout of k_search_proj
    if (lane < HISTO_LENGTH) hist[lane] = 0;
    const float invW = __fdiv_rn((float)GRID_COLS, __fsub_rn(A.maxX, A.minX));
    const float invH = __fdiv_rn((float)GRID_ROWS, __fsub_rn(A.maxY, A.minY));
    for (int i = lane; i < n; i += 64) { occ[i] = A.occIn ? (int)A.occIn[i] : 0; stamp[i] = 0; A.assigned[i] = -1; }
    if (featsInLds) for (int i = lane; i < n; i += 64) {
        int order = i;
        if (A.kind == 0) {
            const sslam_keypoint kp = ((const sslam_keypoint*)A.feats)[i];
            fx[i] = kp.x; fy[i] = kp.y; fang[i] = kp.angle; foct[i] = kp.octave;
            const int px = (int)roundf(__fmul_rn(__fsub_rn(kp.x, A.minX), invW)), py = (int)roundf(__fmul_rn(__fsub_rn(kp.y, A.minY), invH));
            order = (px >= 0 && px < GRID_COLS && py >= 0 && py < GRID_ROWS) ? (((px * GRID_ROWS + py) << 19) | i) : -1;
        } else {
            const sslam_keyline kl = ((const sslam_keyline*)A.feats)[i];
            fx[i] = kl.pt_x; fy[i] = kl.pt_y; fang[i] = kl.angle; foct[i] = kl.octave;
        }
        ford[i] = order; fur[i] = A.uright ? A.uright[i] : -1.f;
        fdesc[2 * i] = ((const uint4*)A.desc)[2 * i]; fdesc[2 * i + 1] = ((const uint4*)A.desc)[2 * i + 1];
    }
    for (int i = lane; i < nq; i += 64) qbin[i] = -1;
    __syncthreads();
    int nmatches = 0, it = 0;
    long long stRescan = 0, cyRescan = 0; const long long tK0 = __builtin_readcyclecounter();
    for (int base = 0; base < nq; base += 64) {
        const int qi = base + lane, end = min(64, nq - base);
        unsigned long long ks[PROJ_K];
#pragma unroll
        for (int k = 0; k < PROJ_K; ++k) ks[k] = ~0ull;
        int cnt = 0, valid = 0, obs = 0; float qAngle = 0.f;
        if (lane < end) {
            const sslam_proj_query* Qp = A.q + qi;
            valid = Qp->valid; obs = Qp->obs_positive; qAngle = Qp->angle; cnt = T.cnt[qi];
            const unsigned long long* tp = T.top + (size_t)qi * PROJ_K;
#pragma unroll
            for (int k = 0; k < PROJ_K; ++k) ks[k] = tp[k];
        }
        int start = 0;
        while (start < end) {
            ++it;
            const bool active = lane >= start && lane < end && valid != 0;
            // first and second list entry whose feature is free now
            unsigned long long b = ~0ull, s2 = ~0ull; int nfree = 0;
            if (active) {
#pragma unroll
                for (int k = 0; k < PROJ_K; ++k) {
                    if (ks[k] == ~0ull) continue;
                    if (occ[proj_key_feature(ks[k])]) continue;
                    if (nfree == 0) b = ks[k]; else if (nfree == 1) s2 = ks[k];
                    ++nfree;
                }
            }
            const int need = A.mode == 0 ? 2 : 1;
            const bool exhausted = active && nfree < need && cnt > PROJ_K;      // the list ran dry although more candidates exist
            int acc = 0, bin = -1;
            if (active && !exhausted) proj_decide_keys(A, qAngle, b, s2, acc, bin);
            const int fb = b != ~0ull ? proj_key_feature(b) : -1, fs = (A.mode == 0 && s2 != ~0ull) ? proj_key_feature(s2) : -1;
            const int tag = (it << 6) | (63 - lane);
            if (active && acc) atomicMax(&stamp[fb], tag);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            bool clash = exhausted;
            if (active && !exhausted) {
                if (fb >= 0) { const int st = stamp[fb]; clash |= (st >> 6) == it && 63 - (st & 63) < lane; }
                if (fs >= 0) { const int st = stamp[fs]; clash |= (st >> 6) == it && 63 - (st & 63) < lane; }
            }
            const unsigned long long cm = __ballot(clash);
            const int c = cm ? __ffsll((long long)cm) - 1 : end;          // lanes below `start` are inactive: never set
            const bool commit = active && lane < c && acc;
            if (commit) {
                A.assigned[fb] = qi;
                if (obs) occ[fb] = 1;
                if (A.mode == 1 && A.checkOri) { qbin[qi] = bin; qidx[qi] = fb; atomicAdd(&hist[bin], 1); }
            }
            nmatches += __popcll(__ballot(commit));
            start = c;
            if (c < end && ((__ballot(exhausted) >> c) & 1ull)) {
                // query base + c is the first pending one and its list is spent: scan its candidates against the live occupancy
                ++stRescan; const long long tr0 = A.stats ? __builtin_readcyclecounter() : 0;
                const int jq = base + c;
                const sslam_proj_query Q = A.q[jq];
                const uint4 q0 = ((const uint4*)(A.qdesc + (size_t)jq * 32))[0], q1 = ((const uint4*)(A.qdesc + (size_t)jq * 32))[1];
                unsigned long long lb = ~0ull, ls = ~0ull;
                for (int i = lane; i < n; i += 64) {
                    unsigned long long kk;
                    if (!(featsInLds ? proj_candidate_lds(A, F, Q, q0, q1, i, occ, kk) : proj_candidate(A, Q, q0, q1, i, invW, invH, [&](int f) { return occ[f] != 0; }, kk))) continue;
                    if (kk < lb) { ls = lb; lb = kk; } else if (kk < ls) ls = kk;
                }
                const unsigned long long best = wave_min_u64(lb);
                const unsigned long long second = wave_min_u64(lb == best ? ls : lb);
                int a2 = 0, bn2 = -1;
                proj_decide_keys(A, Q.angle, best, A.mode == 0 ? second : ~0ull, a2, bn2);
                if (a2) {
                    const int f = proj_key_feature(best);
                    if (lane == 0) {
                        A.assigned[f] = jq;
                        if (Q.obs_positive) occ[f] = 1;
                        if (A.mode == 1 && A.checkOri) { qbin[jq] = bn2; qidx[jq] = f; atomicAdd(&hist[bn2], 1); }
                    }
                    ++nmatches;
                }
                start = c + 1;
                if (A.stats) cyRescan += __builtin_readcyclecounter() - tr0;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    __syncthreads();
    if (A.mode == 1 && A.checkOri) nmatches -= proj_rot_prune(A, hist, qbin, qidx, lane);
    if (lane == 0) *A.nmatches = nmatches;
    if (lane == 0 && A.stats) { A.stats[0] = it; A.stats[1] = stRescan; A.stats[2] = cyRescan; A.stats[3] = __builtin_readcyclecounter() - tK0; }
}
__global__ __launch_bounds__(64) void k_proj_commit(ProjTopArgs T, int featsInLds) {
    extern __shared__ __align__(16) int pc[];
    __shared__ int hist[HISTO_LENGTH];
    proj_commit_body(T, featsInLds, pc, hist, threadIdx.x);
}

// ------------------------------------------------------------------ projection matchers of a batch (sslam_search_by_projection_batch_dev)
// B independent frames in cap / qcap strided buffers, a slice of them per launch (match_plan.h: proj_batch_plan).  Every kernel builds the ProjArgs of
// its frame from the batch arguments and runs the single-frame body above on it: the matching rules exist once.  All per-frame state -- occupancy,
// stamps and rotation histogram in the LDS of the frame's own workgroup, rotation bins, lists and counts in the frame's rows of the slice's scratch --
// belongs to one workgroup (commit, one-wave form) or to the waves of one blockIdx.y (candidates): no two frames of a launch share any of it.
struct ProjBatchArgs {
    ProjArgs A;                    // the shared arguments; its pointers are the batch buffers (row 0 of frame 0); n, nq, scratch and stats are per frame
    const int* n; const int* nq;   // per-frame counts, clamped to [0, cap] / [0, qcap] here
    int cap, qcap;
    int frame0;                    // first frame of the slice
    int* scratch; unsigned long long* top; int* cnt;      // per frame of the SLICE: scratch[2 cap + 2 qcap], top[PROJ_K qcap], cnt[qcap]
};
__device__ __forceinline__ ProjTopArgs proj_batch_frame(const ProjBatchArgs& B, int s) {
    const int f = B.frame0 + s;
    const size_t r = (size_t)f * (size_t)B.cap, rq = (size_t)f * (size_t)B.qcap;
    ProjTopArgs T;
    T.A = B.A;
    ProjArgs& A = T.A;
    A.n = slot_count(B.n, f, B.cap); A.nq = slot_count(B.nq, f, B.qcap);
    A.feats = (const uint8_t*)B.A.feats + r * (B.A.kind == 0 ? sizeof(sslam_keypoint) : sizeof(sslam_keyline));
    A.desc = B.A.desc + r * 32;
    A.uright = B.A.uright ? B.A.uright + r : nullptr;
    A.occIn = B.A.occIn ? B.A.occIn + r : nullptr;
    A.q = B.A.q + rq; A.qdesc = B.A.qdesc + rq * 32;
    A.assigned = B.A.assigned + r; A.nmatches = B.A.nmatches + f;
    A.scratch = B.scratch + (size_t)s * 2 * ((size_t)B.cap + (size_t)B.qcap);
    A.stats = nullptr;
    T.top = B.top + (size_t)s * PROJ_K * (size_t)B.qcap; T.cnt = B.cnt + (size_t)s * (size_t)B.qcap;
    return T;
}
// grid (topkGrid, frames of the slice): one wave per (frame, query)
__global__ __launch_bounds__(256) void k_proj_topk_batch(ProjBatchArgs B) {
    const ProjTopArgs T = proj_batch_frame(B, blockIdx.y);
    const int lane = threadIdx.x & 63, iq = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (iq >= T.A.nq) return;
    proj_topk_body(T, iq, lane);
}
// grid (frames of the slice): one wave per frame, one frame per workgroup -- the frames of a slice commit concurrently
__global__ __launch_bounds__(64) void k_proj_commit_batch(ProjBatchArgs B, int featsInLds) {
    extern __shared__ __align__(16) int pc[];
    __shared__ int hist[HISTO_LENGTH];
    const ProjTopArgs T = proj_batch_frame(B, blockIdx.x);
    proj_commit_body(T, featsInLds, pc, hist, threadIdx.x);
}
// rows beyond PROJ_TWO_KERNEL_MAXN: the one-wave kernel, one workgroup per frame
__global__ __launch_bounds__(64) void k_search_proj_batch(ProjBatchArgs B) {
    __shared__ int hist[HISTO_LENGTH];
    const ProjTopArgs T = proj_batch_frame(B, blockIdx.x);
    search_proj_body(T.A, threadIdx.x, hist);
}

// ---------------------------------------------------------------- SearchByBoW(KeyFrame*, Frame&)
// src/ORBmatcher.cc:159-291.  One wave: the shared vocabulary nodes are walked in ascending id, the keyframe features
// of a node sequentially (a matched frame feature is skipped by the later ones), the node's frame features lane-parallel
// with the list position in the reduction key (first strictly smaller distance wins).
struct BowArgs {
    const sslam_keypoint* kpKF; const uint8_t* dKF; const uint8_t* validKF;
    const sslam_keypoint* kpF; const uint8_t* dF; int nF;
    const int* ptrKF; const int* ptrF; int nnodes; const int* idxKF; const int* idxF;
    float nnratio; int checkOri; int* assigned; int* nmatches; int* qbin;   // qbin[nF]: rotation bin recorded for a frame feature
    const uint8_t* validF; int strictTh;     // KeyFrame-KeyFrame form (:525-658): candidates need a good map point of their own, and the gate is dist < TH_LOW
};

// A frame feature belongs to one vocabulary node, so the only order dependence of SearchByBoW -- a frame feature that is
// already matched is skipped (:216-217) -- stays inside a node: one wave per node walks that node's keyframe features in order
// (grid = 1 replays all nodes in order, used when a caller's lists share a feature between nodes).  The rotation histogram
// only needs counts; k_rot_finish (match_rot.h) builds it, prunes and counts.  assigned / qbin arrive as -1, *nmatches as 0.
__global__ __launch_bounds__(64) void k_search_bow(BowArgs A) {
    const int lane = threadIdx.x;
    for (int nd = blockIdx.x; nd < A.nnodes; nd += gridDim.x) {
        const int f0 = A.ptrF[nd], f1 = A.ptrF[nd + 1];
        for (int a = A.ptrKF[nd]; a < A.ptrKF[nd + 1]; ++a) {
            const int ik = A.idxKF[a];
            if (!A.validKF[ik]) continue;
            const uint4 q0 = ((const uint4*)(A.dKF + (size_t)ik * 32))[0], q1 = ((const uint4*)(A.dKF + (size_t)ik * 32))[1];
            unsigned long long b = ~0ull, s = ~0ull;
            for (int p = f0 + lane; p < f1; p += 64) {
                const int jf = A.idxF[p];
                if (A.assigned[jf] >= 0 || (A.validF && !A.validF[jf])) continue;
                const uint4* tp = (const uint4*)(A.dF + (size_t)jf * 32);
                const unsigned long long kk = ((unsigned long long)hamming256(q0, q1, tp[0], tp[1]) << 32) | (unsigned)(p - f0);
                if (kk < b) { s = b; b = kk; } else if (kk < s) s = kk;
            }
            const unsigned long long best = wave_min_u64(b);
            const unsigned long long second = wave_min_u64(b == best ? s : b);
            int bestDist1 = 256, bestDist2 = 256, bestIdxF = -1;
            if (best != ~0ull && (int)(best >> 32) < 256) { bestDist1 = (int)(best >> 32); bestIdxF = A.idxF[f0 + (int)(unsigned)best]; }
            if (second != ~0ull && (int)(second >> 32) < 256) bestDist2 = (int)(second >> 32);
            if ((A.strictTh ? bestDist1 < TH_LOW : bestDist1 <= TH_LOW) && (float)bestDist1 < __fmul_rn(A.nnratio, (float)bestDist2)) {
                if (lane == 0) {
                    if (A.checkOri) A.qbin[bestIdxF] = rot_bin(A.kpKF[ik].angle, A.kpF[bestIdxF].angle);
                    A.assigned[bestIdxF] = ik;
                }
                __syncthreads();          // the next keyframe feature of this node must see the assignment
            }
        }
    }
}

// ---------------------------------------------------------------- SearchByBoW of a batch (sslam_orb_search_by_bow_batch_dev)
// The same matcher on per-feature NODE IDS instead of CSR lists, for pairs of device-resident frames: no sort, no scratch, no traffic between
// workgroups.  One workgroup of BATCH_WAVES waves per pair (match_plan.h); wave w owns the nodes with node % BATCH_WAVES == w, so
// every frame row -- it has one node -- is read and written as "taken" by one wave only, and the waves never wait for each other while they walk.
// A wave walks the keyframe rows in ascending index, 64 node ids per ballot, and takes the rows that are valid and of a node it owns in
// bit order; for each it scans the frame side for rows of that node that are still free, with the frame index in the reduction key: inside a
// node both sides are visited in ascending index, which is the order of the lists FeatureVector::addFeature builds.  A node id below 0 is in no
// node on either side.  After the one barrier behind the walk the workgroup builds the rotation histogram -- the bin is recomputed from
// assigned[j] and the two angles -- prunes, counts and writes the pair's rows.
// Every loop is bounded by a clamped count, a ballot's set bits or a constant: bytes past a count are never read.
struct BowBatchArgs {
    const sslam_keypoint* kpKF; const uint8_t* dKF; const int* nodeKF; const uint8_t* validKF; const int* nKF; int kfcap, nkeyframes;
    const sslam_keypoint* kpF; const uint8_t* dF; const int* nodeF; const int* nF; int cap, nframes;
    const int* pairKF; const int* pairF;      // null: slot p
    float nnratio; int checkOri;
    int* assigned; int* nmatches;
};
// kLds: the frame side in dynamic LDS -- descriptors [2 cap] uint4, node ids [cap], live assignment [cap] (BOW_BATCH_ROW_BYTES per row);
// otherwise descriptors and node ids in the caller's buffers and the live assignment in the pair's output rows
template <bool kLds>
__global__ __launch_bounds__(64 * BATCH_WAVES) void k_search_bow_batch(BowBatchArgs A) {
    extern __shared__ __align__(16) unsigned bwl[];
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int keep[3];
    __shared__ int total;
    constexpr int NT = 64 * BATCH_WAVES;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = A.pairKF ? A.pairKF[p] : p, f = A.pairF ? A.pairF[p] : p;
    if (k < 0 || k >= A.nkeyframes || f < 0 || f >= A.nframes) {      // (uniform over the workgroup, ahead of every barrier)
        if (tid == 0) A.nmatches[p] = 0;
        return;
    }
    const int nkf = slot_count(A.nKF, k, A.kfcap), nf = slot_count(A.nF, f, A.cap);
    const size_t rk = (size_t)k * (size_t)A.kfcap, rf = (size_t)f * (size_t)A.cap;
    const sslam_keypoint* kpKF = A.kpKF + rk; const uint8_t* dKF = A.dKF + rk * 32; const int* nodeKF = A.nodeKF + rk; const uint8_t* validKF = A.validKF + rk;
    const sslam_keypoint* kpF = A.kpF + rf;
    int* out = A.assigned + (size_t)p * (size_t)A.cap;
    const uint4* fdesc; const int* fnode; int* asg;
    if (kLds) {
        uint4* ld = (uint4*)bwl; int* ln = (int*)(ld + 2 * (size_t)A.cap); int* la = ln + A.cap;
        const uint4* gd = (const uint4*)(A.dF + rf * 32);
        for (int j = tid; j < 2 * nf; j += NT) ld[j] = gd[j];
        for (int j = tid; j < nf; j += NT) { ln[j] = A.nodeF[rf + j]; la[j] = -1; }
        fdesc = ld; fnode = ln; asg = la;
    } else {
        for (int j = tid; j < nf; j += NT) out[j] = -1;
        fdesc = (const uint4*)(A.dF + rf * 32); fnode = A.nodeF + rf; asg = out;
    }
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    // the walk: no workgroup barrier in here (the waves' trip counts differ); a taken flag is written and read by one wave only
    for (int i0 = 0; i0 < nkf; i0 += 64) {
        const int i = i0 + lane;
        int nd = -1; bool own = false;
        if (i < nkf) { nd = nodeKF[i]; own = nd >= 0 && validKF[i] != 0 && (nd % BATCH_WAVES) == wave; }
        unsigned long long todo = __ballot(own);
        while (todo) {
            const int bit = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int ik = i0 + bit;
            const int node = __builtin_amdgcn_readlane(nd, bit);
            const uint4 q0 = ((const uint4*)(dKF + (size_t)ik * 32))[0], q1 = ((const uint4*)(dKF + (size_t)ik * 32))[1];
            unsigned long long b = ~0ull, s = ~0ull;
            for (int j = lane; j < nf; j += 64) {
                if (fnode[j] != node) continue;
                if (__hip_atomic_load(&asg[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0) continue;      // already matched (:216-217)
                const unsigned long long kk = ((unsigned long long)hamming256(q0, q1, fdesc[2 * j], fdesc[2 * j + 1]) << 32) | (unsigned)j;
                if (kk < b) { s = b; b = kk; } else if (kk < s) s = kk;
            }
            const unsigned long long best = wave_min_u64(b);
            const unsigned long long second = wave_min_u64(b == best ? s : b);
            int bestDist1 = 256, bestDist2 = 256, bestIdxF = -1;
            if (best != ~0ull) { bestDist1 = (int)(best >> 32); bestIdxF = (int)(unsigned)best; }
            if (second != ~0ull) bestDist2 = (int)(second >> 32);
            if (bestIdxF >= 0 && bestDist1 <= TH_LOW && (float)bestDist1 < __fmul_rn(A.nnratio, (float)bestDist2)) {
                if (lane == 0) __hip_atomic_store(&asg[bestIdxF], ik, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // the wave's next keyframe row of this node must see the assignment
            }
        }
    }
    __syncthreads();
    if (A.checkOri) {
        for (int j = tid; j < nf; j += NT) {
            const int a = asg[j];
            if (a >= 0) atomicAdd(&hist[rot_hist_bin(kpKF[a].angle, kpF[j].angle)], 1);
        }
        __syncthreads();
        if (tid == 0) three_maxima(hist, keep[0], keep[1], keep[2]);
        __syncthreads();
    }
    int cnt = 0;
    for (int j = tid; j < nf; j += NT) {
        int a = asg[j];
        if (a >= 0 && A.checkOri && !rot_kept(rot_hist_bin(kpKF[a].angle, kpF[j].angle), keep[0], keep[1], keep[2])) a = -1;
        cnt += a >= 0;
        out[j] = a;
    }
    cnt = wave_sum(cnt);
    if (lane == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) A.nmatches[p] = total;
}

// ---------------------------------------------------------------- SearchByBoW(KeyFrame*, KeyFrame*) of a batch (sslam_orb_search_by_bow_keyframes_batch_dev)
// src/ORBmatcher.cc:525-658 for pairs of slots of ONE device-resident keyframe pool, on per-feature node ids.  The walk is k_search_bow_batch's: one
// workgroup of BATCH_WAVES waves per pair, wave w owns the nodes with node % BATCH_WAVES == w, walks the keyframe-1 rows in ascending index, 64 node
// ids per ballot, and takes the valid rows of a node it owns in bit order; a keyframe-2 row has one node, so its state word is written and read by
// one wave only and the waves never wait for each other.  What differs from the KeyFrame -> Frame matcher:
//   - keyframe 2 has validity flags: a row that is invalid or already taken is skipped BEFORE its distance is looked at (:577-583), so it is neither
//     best nor second best.  One state word per keyframe-2 row says both: BOW_KF_INVALID, BOW_KF_FREE, or the keyframe-1 row that owns it;
//   - the distance gate is strict, bestDist1 < TH_LOW (:601); the ratio test reads bestDist2 = 256 when there is no second (:603);
//   - the result is indexed by keyframe 1, and the rotation bin is that of kp1.angle - kp2.angle (:610).
// After the one barrier behind the walk the workgroup fills the rotation histogram, prunes, counts and writes both directions.  The state words are a
// one-to-one map, so walking the owned keyframe-2 rows visits every matched keyframe-1 row exactly once: the histogram holds the reference's per-row
// entries, and the bin is recomputed from the owner and the two angles.
// Every loop is bounded by a clamped count, a ballot's set bits or a constant: bytes past a count are never read, node ids and validity flags included.
struct BowKfBatchArgs {
    const sslam_keypoint* kp; const uint8_t* desc; const int* node; const uint8_t* valid; const int* n; int cap, nkeyframes;      // valid null: every row
    const int* pairs;              // (kf1, kf2) per pair
    float nnratio; int checkOri;
    int* m12; int* m21; int* nmatches;
};
constexpr int BOW_KF_FREE = -1, BOW_KF_INVALID = -2;      // a state word >= 0 is the owning keyframe-1 row
// kLds: keyframe 2 in dynamic LDS -- descriptors [2 cap] uint4, node ids [cap], state words [cap] (BOW_BATCH_ROW_BYTES per row); otherwise descriptors
// and node ids in the caller's buffers and the state words in the pair's d_matches21 rows
template <bool kLds>
__global__ __launch_bounds__(64 * BATCH_WAVES) void k_search_bow_kf_batch(BowKfBatchArgs A) {
    extern __shared__ __align__(16) unsigned bkl[];
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int keep[3];
    __shared__ int total;
    constexpr int NT = 64 * BATCH_WAVES;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k1 = A.pairs[2 * (size_t)p], k2 = A.pairs[2 * (size_t)p + 1];
    if (k1 < 0 || k1 >= A.nkeyframes || k2 < 0 || k2 >= A.nkeyframes) {      // (uniform over the workgroup, ahead of every barrier)
        if (tid == 0) A.nmatches[p] = 0;
        return;
    }
    const int n1 = slot_count(A.n, k1, A.cap), n2 = slot_count(A.n, k2, A.cap);
    const size_t r1 = (size_t)k1 * (size_t)A.cap, r2 = (size_t)k2 * (size_t)A.cap;
    const sslam_keypoint* kp1 = A.kp + r1; const uint8_t* d1 = A.desc + r1 * 32; const int* node1 = A.node + r1;
    const sslam_keypoint* kp2 = A.kp + r2; const int* node2 = A.node + r2;
    const uint8_t* valid1 = A.valid ? A.valid + r1 : nullptr; const uint8_t* valid2 = A.valid ? A.valid + r2 : nullptr;
    int* out12 = A.m12 + (size_t)p * (size_t)A.cap; int* out21 = A.m21 + (size_t)p * (size_t)A.cap;
    const uint4* fdesc; const int* fnode; int* state;
    if (kLds) {
        uint4* ld = (uint4*)bkl; int* ln = (int*)(ld + 2 * (size_t)A.cap); int* ls = ln + A.cap;
        const uint4* gd = (const uint4*)(A.desc + r2 * 32);
        for (int j = tid; j < 2 * n2; j += NT) ld[j] = gd[j];
        for (int j = tid; j < n2; j += NT) ln[j] = node2[j];
        fdesc = ld; fnode = ln; state = ls;
    } else {
        fdesc = (const uint4*)(A.desc + r2 * 32); fnode = node2; state = out21;
    }
    for (int j = tid; j < n2; j += NT) state[j] = (!valid2 || valid2[j] != 0) ? BOW_KF_FREE : BOW_KF_INVALID;
    for (int i = tid; i < n1; i += NT) out12[i] = -1;
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    // the walk: no workgroup barrier in here (the waves' trip counts differ); a state word is written and read by one wave only
    for (int i0 = 0; i0 < n1; i0 += 64) {
        const int i = i0 + lane;
        int nd = -1; bool own = false;
        if (i < n1) { nd = node1[i]; own = nd >= 0 && (!valid1 || valid1[i] != 0) && (nd % BATCH_WAVES) == wave; }
        unsigned long long todo = __ballot(own);
        while (todo) {
            const int bit = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int i1 = i0 + bit;
            const int nodeId = __builtin_amdgcn_readlane(nd, bit);
            const uint4 q0 = ((const uint4*)(d1 + (size_t)i1 * 32))[0], q1 = ((const uint4*)(d1 + (size_t)i1 * 32))[1];
            unsigned long long b = ~0ull, s = ~0ull;
            for (int j = lane; j < n2; j += 64) {
                if (fnode[j] != nodeId) continue;
                if (__hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != BOW_KF_FREE) continue;      // vbMatched2 || !pMP2 || isBad (:579-583)
                const unsigned long long kk = ((unsigned long long)hamming256(q0, q1, fdesc[2 * j], fdesc[2 * j + 1]) << 32) | (unsigned)j;
                if (kk < b) { s = b; b = kk; } else if (kk < s) s = kk;
            }
            const unsigned long long best = wave_min_u64(b);
            const unsigned long long second = wave_min_u64(b == best ? s : b);
            int bestDist1 = 256, bestDist2 = 256, bestIdx2 = -1;
            if (best != ~0ull) { bestDist1 = (int)(best >> 32); bestIdx2 = (int)(unsigned)best; }
            if (second != ~0ull) bestDist2 = (int)(second >> 32);
            if (bestIdx2 >= 0 && bestDist1 < TH_LOW && (float)bestDist1 < __fmul_rn(A.nnratio, (float)bestDist2)) {
                if (lane == 0) __hip_atomic_store(&state[bestIdx2], i1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // the wave's next keyframe-1 row of this node must see the row taken
            }
        }
    }
    __syncthreads();
    if (A.checkOri) {
        for (int j = tid; j < n2; j += NT) {
            const int a = state[j];
            if (a >= 0) atomicAdd(&hist[rot_hist_bin(kp1[a].angle, kp2[j].angle)], 1);
        }
        __syncthreads();
        if (tid == 0) three_maxima(hist, keep[0], keep[1], keep[2]);
        __syncthreads();
    }
    int cnt = 0;
    for (int j = tid; j < n2; j += NT) {
        int a = state[j];
        if (a >= 0 && A.checkOri && !rot_kept(rot_hist_bin(kp1[a].angle, kp2[j].angle), keep[0], keep[1], keep[2])) a = -1;
        if (a >= 0) { out12[a] = j; ++cnt; }
        out21[j] = a >= 0 ? a : -1;
    }
    cnt = wave_sum(cnt);
    if (lane == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) A.nmatches[p] = total;
}
