// The draw of the two RANSAC units (two_view_math.h: Initializer.cc:93-108, eight matches; sim3_math.h: Sim3Solver.cc:166-177, three correspondences) and the sweep count
// of their Jacobi solvers.  No HIP in here.  The reference's randi comes from rand(), seeded once per process; here randi = hash32(seed, pair, it, j) % remaining with
//   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (lowbias32)
//   hash32(seed, pair, it, j) = mix(mix(mix(mix(seed + 0x9e3779b9) ^ pair) ^ it) ^ j)
// in 32-bit unsigned arithmetic.  The reference copies all indices per iteration, takes [randi] K times and moves the back into its place; that swap-with-back is replayed
// without the copy: at most K overwritten positions are remembered, every index of the replay a compile-time constant.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RANSAC_FN __host__ __device__ inline
#define RANSAC_UNROLL _Pragma("unroll")
#define RANSAC_NOUNROLL _Pragma("nounroll")
#else
#define RANSAC_FN inline
#define RANSAC_UNROLL
#define RANSAC_NOUNROLL
#endif

namespace sslam {

constexpr int JACOBI_SWEEPS = 8;      // decisions D15 and D16: cyclic sweeps of the 9 x 9 (two_view_math.h) and of the 4 x 4 (sim3_math.h)

RANSAC_FN uint32_t mix32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
RANSAC_FN uint32_t hash32(uint32_t seed, uint32_t pair, uint32_t it, uint32_t j) { return mix32(mix32(mix32(mix32(seed + 0x9e3779b9u) ^ pair) ^ it) ^ j); }

// one iteration's K distinct indices out of n >= K; K follows from the caller's array (tv:: and s3:: name this function as their own).  pos[k] / val[k]: vAvailableIndices[pos[k]] was overwritten with val[k] in step k (the latest entry for a position holds)
template <int K>
RANSAC_FN void draw_set(uint32_t seed, uint32_t pair, uint32_t it, int n, int (&set)[K]) {
    int pos[K], val[K];
    RANSAC_UNROLL
    for (int j = 0; j < K; ++j) {
        const int remaining = n - j;
        const int randi = (int)(hash32(seed, pair, it, (uint32_t)j) % (uint32_t)remaining);
        int idx = randi, back = remaining - 1;
        RANSAC_UNROLL
        for (int k = 0; k < K; ++k) if (k < j) {
            if (pos[k] == randi) idx = val[k];
            if (pos[k] == remaining - 1) back = val[k];
        }
        set[j] = idx;
        pos[j] = randi; val[j] = back;
    }
}

}  // namespace sslam
