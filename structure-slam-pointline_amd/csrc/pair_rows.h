// The compaction walk of the one-wave-per-pair RANSAC kernels (two_view.hip, sim3.hip).  Device only: include behind common.h.
// The wave steps over the n1 rows of side 1, 64 at a time; match(i) is the row of side 2 that row i goes with, or -1 (it answers -1 past n1).  The matched rows get
// consecutive slots in ascending row order (ballot + popcount prefix): body(i, m, slot) runs on every lane of every step, slot = -1 for an unmatched lane.  The same walk
// with the same match rule finds a row's slot again later.  Returns the number of matched rows; every lane gets the same value.
#pragma once

namespace sslam {
template <class Match, class Body>
__device__ __forceinline__ int for_rows(int n1, int lane, Match match, Body body) {
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += 64) {
        const int i = i0 + lane;
        const int m = match(i);
        const unsigned long long mask = __ballot(m >= 0);
        body(i, m, m >= 0 ? base + mbcnt(mask) : -1);
        base += __popcll(mask);
    }
    return base;
}
}  // namespace sslam
