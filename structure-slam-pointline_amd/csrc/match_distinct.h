// ------------------------------------------------------------------ distinctive descriptors of a batch of observation sets on device-resident keyframes
// (sslam_distinctive_descriptors_batch_dev): MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:247-312) == MapLine::ComputeDistinctiveDescriptors
// (src/MapLine.cpp:246-317) for sets of (keyframe slot, feature row) entries.  An entry is ADMISSIBLE when its slot exists, is not bad and holds the row
// (distinct_row); the N admissible entries of a set, in entry order, are the reference's vDescriptors; per admissible entry the median
// sorted[int(0.5 * (N - 1))] of its N distances (its own 0 included), and the first entry with the least median wins: the minimum of median << 32 | entry.
// Which kernel runs a set follows its entry count (match_plan.h: distinct_class):
//   k_distinct_batch   a wave owns eight consecutive sets.  The small ones (<= 8 entries) run together, one group of eight lanes each, lane = entry: the
//                      row is gathered with two 16-byte loads into registers and handed round the group with DPP (quad_perm / row_half_mirror: lane ^ 1 .. 7),
//                      so every lane holds its 8 distances; the median is the value of rank k by counting over 8 registers, no bisection, no LDS.
//                      Then the medium ones (9 .. 64 entries) one after the other, lane = entry: the admissible rows go to the wave's LDS in entry order
//                      (distinct_compact), every lane computes its N distances ONCE into the wave's 16-bit matrix (column = lane: conflict free, two
//                      distances per word), and the nine bisection steps count on the stored values.
//   k_distinct_large   65 .. 1024 entries, the shape of k_distinctive behind the gather: rows and their entry positions in LDS, lanes take admissible
//                      rows 64 at a time and bisect with recomputed distances.
// Every set writes its own d_best / d_median; nothing at or past a slot's count and no entry outside a set's range is read.
struct DistinctArgs {
    const uint8_t* desc; const int32_t* n; int cap, nkeyframes; const uint8_t* bad;
    const sslam_observation* obs; int nobs; const int32_t* ptr; int nsets;
    int32_t* best; int32_t* median; uint8_t* outDesc; const int32_t* outRow; int nout;
};

// the class of set s from its range alone; beg / cnt are meaningful unless the set is refused
__device__ __forceinline__ DistinctClass distinct_set(const DistinctArgs& A, unsigned s, int& beg, int& cnt) {
    const int b = A.ptr[s], e = A.ptr[s + 1];
    beg = b; cnt = e - b;
    return (b < 0 || e < b || e > A.nobs) ? DistinctClass::Refused : distinct_class(e - b);
}
// pool row (kf * cap + row, below 2^31) of entry `idx` of d_obs, or -1 when the entry is not admissible: pKF->isBad() (src/MapPoint.cc:270) and what a
// caller's stale bookkeeping may hold (a slot or row that does not exist).  The count of a slot is clamped to [0, cap]
__device__ __forceinline__ int distinct_row(const DistinctArgs& A, int idx) {
    const int kf = A.obs[idx].kf, row = A.obs[idx].row;
    if ((unsigned)kf >= (unsigned)A.nkeyframes) return -1;
    if (A.bad && A.bad[kf]) return -1;
    const int n = slot_count(A.n, kf, A.cap);
    return (unsigned)row < (unsigned)n ? kf * A.cap + row : -1;
}
// THE compaction: position of this lane's entry among the admissible entries of the wave's 64, in entry order (ballot + prefix popcount), and their number.
// It is what makes N and "the first wins" right: rows sit in LDS in the order the reference pushes them into vDescriptors
__device__ __forceinline__ int distinct_compact(bool admissible, int& count) {
    const unsigned long long m = __ballot(admissible);
    count = __popcll(m);
    return mbcnt(m);
}
__device__ __forceinline__ void distinct_report(const DistinctArgs& A, unsigned s, int best, int median) {
    A.best[s] = best;
    if (A.median) A.median[s] = median;
}
// row of d_out_desc that set s writes, -1 for none
__device__ __forceinline__ int distinct_target(const DistinctArgs& A, unsigned s) {
    if (!A.outDesc) return -1;
    const int r = A.outRow ? A.outRow[s] : (int)s;
    return (unsigned)r < (unsigned)A.nout ? r : -1;
}
__device__ __forceinline__ void distinct_copy(const DistinctArgs& A, unsigned s, const uint4& q0, const uint4& q1) {
    const int t = distinct_target(A, s);
    if (t >= 0) { uint4* o = (uint4*)(A.outDesc + (size_t)t * 32); o[0] = q0; o[1] = q1; }
}
__device__ __forceinline__ void distinct_lds_order() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }

template <int CTRL>
__device__ __forceinline__ uint4 dpp_u128(const uint4& v) {
    return make_uint4((unsigned)__builtin_amdgcn_mov_dpp((int)v.x, CTRL, 0xF, 0xF, false), (unsigned)__builtin_amdgcn_mov_dpp((int)v.y, CTRL, 0xF, 0xF, false),
                      (unsigned)__builtin_amdgcn_mov_dpp((int)v.z, CTRL, 0xF, 0xF, false), (unsigned)__builtin_amdgcn_mov_dpp((int)v.w, CTRL, 0xF, 0xF, false));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_XOR3 = 0x1B, DPP_XOR7 = 0x141;      // quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0]; row_half_mirror (lane -> 7 - lane of its eight)

// the small sets of a wave's eight, all at once.  Called by the whole wave in uniform control flow (the DPP moves read every lane); a lane without an
// admissible entry carries a zero row and the key ~0
__device__ __forceinline__ void distinct_small(const DistinctArgs& A, unsigned s, bool small, int beg, int cnt, int lane) {
    const int e = lane & 7;
    const int row = (small && e < cnt) ? distinct_row(A, beg + e) : -1;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (row >= 0) { const uint4* p = (const uint4*)(A.desc + (size_t)row * 32); q0 = p[0]; q1 = p[1]; }
    const unsigned g = (unsigned)(__ballot(row >= 0) >> (lane & 56)) & 0xFFu;      // the admissible entries of this lane's set
    const int N = __popc(g), k = (N - 1) >> 1;                                      // int(0.5 * (N - 1))
    // v[m] = distance to entry e ^ m of the set, << 3 | m so that the eight values of a lane differ; an inadmissible partner sorts behind every distance
    unsigned v[8];
    v[0] = 0;
    const uint4 h0 = dpp_u128<DPP_XOR7>(q0), h1 = dpp_u128<DPP_XOR7>(q1);
    // the moves stand OUTSIDE the select: a lane whose own partner is inadmissible still has to be active as the source of another lane's move
#define SSLAM_DISTINCT_PAIR(m, T0, T1) { const uint4 t0 = T0, t1 = T1; const unsigned dd = (unsigned)hamming256(q0, q1, t0, t1); \
                                         v[m] = ((g >> (e ^ m)) & 1u) ? (dd << 3) | (unsigned)m : 0x1000u | (unsigned)m; }
    SSLAM_DISTINCT_PAIR(1, dpp_u128<DPP_XOR1>(q0), dpp_u128<DPP_XOR1>(q1));
    SSLAM_DISTINCT_PAIR(2, dpp_u128<DPP_XOR2>(q0), dpp_u128<DPP_XOR2>(q1));
    SSLAM_DISTINCT_PAIR(3, dpp_u128<DPP_XOR3>(q0), dpp_u128<DPP_XOR3>(q1));
    SSLAM_DISTINCT_PAIR(4, dpp_u128<DPP_XOR3>(h0), dpp_u128<DPP_XOR3>(h1));      // 7 ^ 3
    SSLAM_DISTINCT_PAIR(5, dpp_u128<DPP_XOR2>(h0), dpp_u128<DPP_XOR2>(h1));      // 7 ^ 2
    SSLAM_DISTINCT_PAIR(6, dpp_u128<DPP_XOR1>(h0), dpp_u128<DPP_XOR1>(h1));      // 7 ^ 1
    SSLAM_DISTINCT_PAIR(7, h0, h1);
#undef SSLAM_DISTINCT_PAIR
    unsigned med = 0;                                   // the value of rank k among the eight: counting, every index static
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        int r = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) r += (b != a && v[b] < v[a]) ? 1 : 0;
        med = r == k ? v[a] : med;
    }
    unsigned long long key = row >= 0 ? ((unsigned long long)(med >> 3) << 32) | (unsigned)e : ~0ull, w;
    w = dpp_u64<DPP_XOR1>(key); key = w < key ? w : key;
    w = dpp_u64<DPP_XOR2>(key); key = w < key ? w : key;
    w = dpp_u64<DPP_XOR7>(key); key = w < key ? w : key;      // both quads hold their minimum: the mirror lane sits in the other quad
    if (small && e == 0) distinct_report(A, s, N ? (int)(unsigned)key : -1, N ? (int)(key >> 32) : 0x7fffffff);
    if (row >= 0 && e == (int)(unsigned)key) distinct_copy(A, s, q0, q1);
}

// one medium set on one wave: rows[2 * 64] and dist[32 * 64] are the wave's own LDS
__device__ __forceinline__ void distinct_medium(const DistinctArgs& A, unsigned s, int beg, int cnt, int lane, uint4* rows, unsigned* dist) {
    const int row = lane < cnt ? distinct_row(A, beg + lane) : -1;
    int N;
    const int pos = distinct_compact(row >= 0, N);
    if (N == 0) { if (lane == 0) distinct_report(A, s, -1, 0x7fffffff); return; }
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (row >= 0) {
        const uint4* p = (const uint4*)(A.desc + (size_t)row * 32);
        q0 = p[0]; q1 = p[1];
        rows[2 * pos] = q0; rows[2 * pos + 1] = q1;
    }
    distinct_lds_order();
    unsigned long long key = ~0ull;
    if (row >= 0) {
        const int words = (N + 1) >> 1;
        for (int j = 0; j < words; ++j) {              // every pair distance once; the row is the same for all lanes: a broadcast read
            const int j0 = 2 * j, j1 = min(2 * j + 1, N - 1);
            const unsigned d0 = (unsigned)hamming256(q0, q1, rows[2 * j0], rows[2 * j0 + 1]);
            const unsigned d1 = (unsigned)hamming256(q0, q1, rows[2 * j1], rows[2 * j1 + 1]);
            dist[j * 64 + lane] = d0 | ((2 * j + 1 < N ? d1 : 0xFFFFu) << 16);
        }
        const int k = (N - 1) >> 1;
        int lo = 0, hi = 256;                            // smallest v with #{j : dist(lane, j) <= v} >= k + 1: nine steps at the most
        for (int it = 0; it < 9; ++it) {
            const unsigned mid = (unsigned)((lo + hi) >> 1);
            int c = 0;
            for (int j = 0; j < words; ++j) {
                const unsigned w = dist[j * 64 + lane];
                c += ((w & 0xFFFFu) <= mid ? 1 : 0) + ((w >> 16) <= mid ? 1 : 0);
            }
            if (lo < hi) { if (c >= k + 1) hi = (int)mid; else lo = (int)mid + 1; }
        }
        key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)lane;
    }
    key = wave_min_u64(key);
    if (lane == 0) distinct_report(A, s, (int)(unsigned)key, (int)(key >> 32));
    if (lane == (int)(unsigned)key) distinct_copy(A, s, q0, q1);
    distinct_lds_order();                                // the next set of this wave overwrites rows
}

__global__ __launch_bounds__(64 * DISTINCT_BATCH_WAVES) void k_distinct_batch(DistinctArgs A) {
    __shared__ __align__(16) uint4 rowsAll[DISTINCT_BATCH_WAVES][2 * DISTINCT_MEDIUM_MAX];
    __shared__ unsigned distAll[DISTINCT_BATCH_WAVES][DISTINCT_MEDIUM_MAX * DISTINCT_MEDIUM_MAX / 2];
    static_assert(sizeof(rowsAll) == DISTINCT_BATCH_WAVES * DISTINCT_MEDIUM_ROW_BYTES && sizeof(distAll) == DISTINCT_BATCH_WAVES * DISTINCT_MEDIUM_DIST_BYTES, "match_plan.h");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned nunits = ((unsigned)A.nsets + DISTINCT_SETS_PER_WAVE - 1) / DISTINCT_SETS_PER_WAVE;
    for (unsigned unit = blockIdx.x * DISTINCT_BATCH_WAVES + wave; unit < nunits; unit += gridDim.x * DISTINCT_BATCH_WAVES) {
        const unsigned s0 = unit * DISTINCT_SETS_PER_WAVE, s = s0 + (unsigned)(lane >> 3);
        int beg = 0, cnt = 0;
        const bool live = s < (unsigned)A.nsets;
        const DistinctClass cls = live ? distinct_set(A, s, beg, cnt) : DistinctClass::Large;      // Large: not this kernel's
        if (live && cls == DistinctClass::Refused && (lane & 7) == 0) distinct_report(A, s, -2, 0x7fffffff);
        const bool small = live && cls == DistinctClass::Small;
        if (__ballot(small)) distinct_small(A, s, small, beg, cnt, lane);
        unsigned long long todo = __ballot(live && cls == DistinctClass::Medium && (lane & 7) == 0);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            distinct_medium(A, s0 + (unsigned)(src >> 3), __shfl(beg, src, 64), __shfl(cnt, src, 64), lane, rowsAll[wave], distAll[wave]);
        }
    }
}

__global__ __launch_bounds__(64) void k_distinct_large(DistinctArgs A) {
    __shared__ __align__(16) uint4 d[2 * DISTINCT_LARGE_MAX];
    __shared__ unsigned short ent[DISTINCT_LARGE_MAX];
    static_assert(sizeof(d) + sizeof(ent) == DISTINCT_LARGE_LDS_BYTES && DISTINCT_LARGE_MAX == DISTINCT_MAXN, "match_plan.h");
    const int lane = threadIdx.x;
    const unsigned nchunks = ((unsigned)A.nsets + DISTINCT_LARGE_CHUNK - 1) / DISTINCT_LARGE_CHUNK;
    for (unsigned c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const unsigned c0 = c * DISTINCT_LARGE_CHUNK, sl = c0 + (unsigned)lane;
        int lbeg = 0, lcnt = 0;
        const bool large = sl < (unsigned)A.nsets && distinct_set(A, sl, lbeg, lcnt) == DistinctClass::Large;
        unsigned long long todo = __ballot(large);
        while (todo) {                                   // most chunks hold none: the wave leaves at once
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const unsigned s = c0 + (unsigned)src;
            const int beg = __shfl(lbeg, src, 64), cnt = __shfl(lcnt, src, 64);
            __syncthreads();
            int N = 0;
            for (int i0 = 0; i0 < cnt; i0 += 64) {       // gather: admissible rows in entry order, with the entry each came from
                const int i = i0 + lane;
                const int row = i < cnt ? distinct_row(A, beg + i) : -1;
                int add;
                const int pos = N + distinct_compact(row >= 0, add);
                if (row >= 0) {
                    const uint4* p = (const uint4*)(A.desc + (size_t)row * 32);
                    d[2 * pos] = p[0]; d[2 * pos + 1] = p[1];
                    ent[pos] = (unsigned short)i;
                }
                N += add;
            }
            __syncthreads();
            if (N == 0) { if (lane == 0) distinct_report(A, s, -1, 0x7fffffff); continue; }
            const int k = (N - 1) >> 1;
            unsigned long long mine = ~0ull;
            int minePos = 0;
            for (int p0 = 0; p0 < N; p0 += 64) {
                const int p = p0 + lane;
                if (p < N) {
                    const uint4 a0 = d[2 * p], a1 = d[2 * p + 1];
                    int lo = 0, hi = 256;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        int c2 = 0;
                        for (int j = 0; j < N; ++j) c2 += hamming256(a0, a1, d[2 * j], d[2 * j + 1]) <= mid ? 1 : 0;
                        if (c2 >= k + 1) hi = mid; else lo = mid + 1;
                    }
                    const unsigned long long key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)ent[p];
                    if (key < mine) { mine = key; minePos = p; }
                }
            }
            const unsigned long long bestKey = wave_min_u64(mine);
            if (lane == 0) distinct_report(A, s, (int)(unsigned)bestKey, (int)(bestKey >> 32));
            if (mine == bestKey) distinct_copy(A, s, d[2 * minePos], d[2 * minePos + 1]);      // entries differ, so one lane holds the key
        }
    }
}
