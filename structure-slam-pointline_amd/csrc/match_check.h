// The argument checks that matcher entry points share (match.hip, two_view.hip, sim3.hip, pnp.hip): the CSR lists of vocabulary nodes, observation sets and children, the
// alignment and size rules of device-resident batches, and the parameter rules of the RANSAC entry points.  Host code and no HIP in here: tests/sim/host_checks.cpp compiles it with a plain host compiler under the sanitizers and supplies its own set_error.
#pragma once
#include <cstdint>
#include "../../include/sslam_frontend.h"
#include "match_plan.h"

namespace sslam {

// List r owns idx[ptr[r] .. ptr[r + 1]).  Well formed: ptr[0] == 0 and non-decreasing offsets -- so the total ptr[nnodes] is >= 0 and no list
// reaches past it: a call sizes its arena by the total -- and 0 <= idx[i] < limit (idx == nullptr: the offsets alone).  Anything else is
// SSLAM_ERR_INVALID with the error text "<fn>: <what> ...", before the call stages or launches anything.
void set_error(const char* fmt, ...);      // ctx.hip
inline int check_csr(const char* fn, const char* what, const int32_t* ptr, int nnodes, const int32_t* idx, int limit) {
    bool ok = ptr[0] == 0;
    for (int r = 0; r < nnodes && ok; ++r) ok = ptr[r + 1] >= ptr[r];
    if (!ok) { set_error("%s: %s offsets must start at 0 and be non-decreasing", fn, what); return SSLAM_ERR_INVALID; }
    if (idx) for (int i = 0; i < ptr[nnodes]; ++i) if (idx[i] < 0 || idx[i] >= limit) { set_error("%s: %s index out of range", fn, what); return SSLAM_ERR_INVALID; }
    return SSLAM_OK;
}

// Every one of these pointers is a multiple of N bytes (a power of two); a null pointer is aligned -- whether it may be null is the caller's rule.
template <unsigned N, class... Ptr> inline bool all_aligned(const Ptr*... p) {
    static_assert(N && !(N & (N - 1)), "a power of two");
    return ((((uintptr_t)p) | ... | (uintptr_t)0) & (N - 1)) == 0;
}
// A row capacity whose indices fit the packed reduction keys (match_plan.h: MAX_ROWS); 0 is in range, an entry point that needs rows says so itself.
inline bool rows_in_range(int cap) { return cap >= 0 && cap < MAX_ROWS; }
// slots * cap rows (or jobs * queries) are indexed with a signed 32-bit int on the device
inline bool fits_31_bits(int slots, int cap) { return (long long)slots * (long long)cap < (1ll << 31); }
// The parameters sslam_sim3_ransac and sslam_sim3_ransac_batch_dev share (sim3.hip): the host table of level_sigma2 (nlevels in 1 .. 64), SetRansacParameters' arguments and
// iterate's nIterations.  probability lies strictly inside (0, 1): log(1 - probability) has to be finite and negative; a NaN fails both comparisons.
inline bool sim3_params_ok(const float* level_sigma2, int nlevels, double probability, int min_inliers, int max_iterations, int new_iterations) {
    return level_sigma2 && nlevels >= 1 && nlevels <= 64 && probability > 0.0 && probability < 1.0 && min_inliers >= 1 && max_iterations >= 1 && new_iterations >= 1;
}
// The parameters sslam_pnp_ransac and sslam_pnp_ransac_batch_dev share (pnp.hip): as above, and SetRansacParameters' epsilon in (0, 1] and th2 > 0; a NaN fails every
// comparison.  The minimal set is four.
inline bool pnp_params_ok(const float* level_sigma2, int nlevels, double probability, int min_inliers, int max_iterations, int new_iterations, float epsilon, float th2) {
    return sim3_params_ok(level_sigma2, nlevels, probability, min_inliers, max_iterations, new_iterations) && epsilon > 0.f && epsilon <= 1.f && th2 > 0.f;
}
// The sizes of a PnP batch: rows are indexed pair * cap + j, frame * cap + j and keyframe * kfcap + i in 31 bits; the caller's sets pair * nsets + it below 2^28
inline bool pnp_sizes_ok(int npairs, int cap, int nframes, int nkeyframes, int kfcap, const void* d_sets, int nsets) {
    return npairs >= 0 && cap >= 1 && nframes >= 0 && nkeyframes >= 0 && kfcap >= 1 && fits_31_bits(npairs, cap) && fits_31_bits(nframes, cap) && fits_31_bits(nkeyframes, kfcap) &&
           (!d_sets || (nsets >= 0 && (long long)npairs * (long long)nsets < (1ll << 28)));
}
// Injected sets of a RANSAC batch (d_sets: iterations sets per pair): their rows are indexed pair * iterations + it, which stays below 2^28 so that the index times the
// words of a set fits 31 bits.  Without sets the rule asks nothing.
inline bool injected_sets_ok(const void* d_sets, int npairs, int iterations) { return !d_sets || (long long)npairs * (long long)iterations < (1ll << 28); }
// The parameters sslam_two_view_reconstruct and sslam_two_view_reconstruct_batch_dev share (reconstruct.hip): mSigma above 0 (a NaN fails the comparison) and a
// minTriangulated that is a count.  minParallax is compared as the reference compares it, whatever it is.
inline bool reconstruct_params_ok(float sigma, int min_triangulated) { return sigma > 0.f && min_triangulated >= 0; }
// The line arguments of a reconstruct batch come all or none: 0 = none (every pointer NULL; lcap is not looked at), 1 = all (no pointer NULL, lcap >= 1), -1 = in part
inline int reconstruct_lines_given(const void* kl1, const void* nl1, const void* kl2, const void* nl2, const void* fn1, const void* fn2, const void* pairs, const void* npairs,
                                   const void* s3d, const void* e3d, const void* tri, int lcap) {
    const void* p[11] = {kl1, nl1, kl2, nl2, fn1, fn2, pairs, npairs, s3d, e3d, tri};
    int given = 0;
    for (const void* q : p) given += q ? 1 : 0;
    return given == 0 ? 0 : given == 11 && lcap >= 1 ? 1 : -1;
}
// The sizes of a reconstruct batch: rows are indexed pair * cap + i and line rows pair * lcap + r in 31 bits (lcap 0: a batch without lines)
inline bool reconstruct_sizes_ok(int npairs, int cap, int lcap) { return npairs >= 1 && cap >= 1 && lcap >= 0 && fits_31_bits(npairs, cap) && fits_31_bits(npairs, lcap); }

}  // namespace sslam
