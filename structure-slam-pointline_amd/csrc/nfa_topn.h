// Which candidate rectangles the NFA stage has to validate when only the maxLines lines of the largest response leave the extractor (ExtractLineSegment.cpp:42-51
// sorts the KeyLines by response = lineLength / max(w, h) and keeps the first nfeatures): the response of a segment, what is known of a candidate's response BEFORE
// rect_improve ran, and the rule that ends the validation.  No HIP in here: the line kernels (lsd_nfa.h, lbd.h) compile this text for the device and
// tests/sim/nfa_topn_sim.cpp / nfa_topn_oracle.cpp for the host with a plain compiler.  Only + - / and sqrt on float / double are used, each rounded once on both sides
// (the device side through the _rn intrinsics: its compiler contracts by default), so that the two produce the same bits.
//
// What rect_improve can do to a rectangle's end points (lsd_nfa.h stage_cand; LineSegmentDetectorImpl::rect_improve): stages 0, 1 and 4 change p and width only; a step of
// stage 2 adds 0.25 * (-dy, dx) to BOTH end points, a step of stage 3 subtracts it, five steps each at most, and stage 3 starts from what stage 2 kept.  (dx, dy) is
// (cos theta, sin theta): a unit vector.  So the final end points are the initial ones moved by ONE common vector of length <= 5 * 0.25 = 1.25 scaled pixels, i.e.
// SHIFT_PX = 1.25 / 0.8 = 1.5625 pixels of the segment (seg_coord).  A rectangle accepted at its first evaluation is not moved at all.
//   * Without checkLineExtremes acting, the length is that of the same vector difference: it changes by rounding alone.  For images of up to MAX_SIDE pixels a side a
//     float coordinate carries an error <= 2^-24 * 32768 = 0.002 px (seg_coord's rounding, the float subtraction), the length therefore < 0.02 px over both end points and
//     both evaluations, lineLength's rounding to float < 0.003 px, the division's rounding less: MARGIN_IN_PX = 0.125 px covers it several times.  checkLineExtremes leaves
//     a coordinate e alone iff 0 <= e < W; with the initial e in [2, W - 2) the moved one is in (0.43, W - 0.43): that is the `inside` test of margin().
//   * Otherwise a coordinate goes through f(e) = 0 for e < 0, W - 1 for e >= W, e else, which is NOT non-expansive: it jumps by 1 at W.  |f(a) - f(b)| <= |a - b| + 1 per
//     coordinate, so an end point moved by d (|d| <= SHIFT_PX) lands at most |d| + sqrt(2) from where it was, and the length (triangle inequality over the two end
//     points) changes by at most 2 * (1.5625 + 1.4143) = 5.954 px; with the rounding above: MARGIN_EDGE_PX = 6.125 px.
// Beyond MAX_SIDE pixels a side the rounding argument does not hold and every candidate is validated (usable()).
//
// The rule.  u(c) = r0(c) + margin(c) bounds the final response of candidate c from above (r0: the response of the rectangle as the core emitted it; it IS the final
// response when the first evaluation accepts).  Candidates are validated in the order of descending u, ties by ascending emission index (rank_key: the form of k_keylines'
// sort key).  tau = the N-th largest final response among those validated and accepted so far (N = maxLines), taken only once MORE than N are accepted: the
// reference sorts and cuts iff it holds more than N lines (ExtractLineSegment.cpp:45) and otherwise hands them out in emission order, so nothing may be left out before
// that is settled -- with N + 1 accepted it is, without them the validation goes on, slice after slice, to the last candidate.  A candidate with u < tau (strictly: a tie is validated) has N accepted candidates of a larger response in front of it whatever its own
// verdict: it cannot be among the N lines that leave, and -- the order being by u -- neither can any candidate behind it.  tau only grows as more are accepted, so an
// exclusion stays valid.  The top N of the validated subset, taken in emission order with k_keylines' stable key, are then the top N of all candidates.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TOPN_FN __host__ __device__ inline
#else
#define TOPN_FN inline
#endif

namespace sslam {
namespace topn {

constexpr double SEG_SCALE = 0.8;            // LSD's SCALE: a rectangle lives in the 0.8x image
constexpr float SHIFT_PX = 1.5625f;          // 5 * 0.25 / SEG_SCALE
constexpr float MARGIN_IN_PX = 0.125f;       // no end point can meet checkLineExtremes: rounding alone
constexpr float MARGIN_EDGE_PX = 6.125f;     // 2 * (SHIFT_PX + sqrt 2) + rounding
constexpr int MAX_SIDE = 32768;              // images beyond: validate everything
constexpr int FLAG_REJECTED = 0, FLAG_ACCEPTED = 1, FLAG_NOT_NEEDED = 2;      // a candidate's flag behind the stage; NOT_NEEDED is treated as not accepted

#if defined(__HIP_DEVICE_COMPILE__)
TOPN_FN float f_sub(float a, float b) { return __fsub_rn(a, b); }
TOPN_FN float f_add(float a, float b) { return __fadd_rn(a, b); }
TOPN_FN float f_div(float a, float b) { return __fdiv_rn(a, b); }
TOPN_FN double d_sqrt(double a) { return sqrt(a); }
#else
TOPN_FN float f_sub(float a, float b) { return a - b; }
TOPN_FN float f_add(float a, float b) { return a + b; }
TOPN_FN float f_div(float a, float b) { return a / b; }
TOPN_FN double d_sqrt(double a) { return __builtin_sqrt(a); }
#endif

// one coordinate of the output segment from the rectangle's (flsd: += 0.5, /= SCALE, then float)
TOPN_FN float seg_coord(double x) { return (float)((x + 0.5) / SEG_SCALE); }

// checkLineExtremes (LSDDetector.cpp) on a segment (x1, y1, x2, y2) of a w x h image
TOPN_FN void check_line_extremes(float& e0, float& e1, float& e2, float& e3, int w, int h) {
    const float W = (float)w, H = (float)h;
    if (e0 < 0) e0 = 0;
    if (e0 >= W) e0 = W - 1.0f;
    if (e2 < 0) e2 = 0;
    if (e2 >= W) e2 = W - 1.0f;
    if (e1 < 0) e1 = 0;
    if (e1 >= H) e1 = H - 1.0f;
    if (e3 < 0) e3 = 0;
    if (e3 >= H) e3 = H - 1.0f;
}
// KeyLine::lineLength and ::response of a segment that went through check_line_extremes (the products of two floats are exact in double)
TOPN_FN float line_length(float e0, float e1, float e2, float e3) {
    const double ddx = (double)f_sub(e0, e2), ddy = (double)f_sub(e1, e3);
    return (float)d_sqrt(ddx * ddx + ddy * ddy);
}
TOPN_FN float response_of_length(float lineLength, int w, int h) { return f_div(lineLength, (float)(w > h ? w : h)); }
TOPN_FN float seg_response(float e0, float e1, float e2, float e3, int w, int h) {
    check_line_extremes(e0, e1, e2, e3, w, h);
    return response_of_length(line_length(e0, e1, e2, e3), w, h);
}

// the response a rectangle's end points (x1, y1, x2, y2 of a RectD) would get as they are
TOPN_FN float rect_response(double x1, double y1, double x2, double y2, int w, int h) {
    return seg_response(seg_coord(x1), seg_coord(y1), seg_coord(x2), seg_coord(y2), w, h);
}
// how far rect_improve can move that response (see above), in units of the response
TOPN_FN float margin(double x1, double y1, double x2, double y2, int w, int h) {
    const float e0 = seg_coord(x1), e1 = seg_coord(y1), e2 = seg_coord(x2), e3 = seg_coord(y2);
    const float W = (float)w, H = (float)h;
    const bool inside = e0 >= 2.0f && e0 < W - 2.0f && e2 >= 2.0f && e2 < W - 2.0f && e1 >= 2.0f && e1 < H - 2.0f && e3 >= 2.0f && e3 < H - 2.0f;
    return f_div(inside ? MARGIN_IN_PX : MARGIN_EDGE_PX, (float)(w > h ? w : h));
}
// u: no final response of the candidate is above it
TOPN_FN float upper(float r0, float m) { return f_add(r0, m); }
TOPN_FN bool usable(int w, int h) { return w <= MAX_SIDE && h <= MAX_SIDE; }

TOPN_FN uint32_t f_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
// ascending keys = descending value (values >= 0: the bit patterns order as the floats), ties by ascending index: k_keylines' key on the response, the ranking's on u
TOPN_FN unsigned long long rank_key(float v, int index) { return ((unsigned long long)(~f_bits(v)) << 32) | (unsigned)index; }
TOPN_FN int key_index(unsigned long long key) { return (int)(unsigned)key; }

// the stopping rule: a candidate that has not been validated, against the N-th largest final response accepted so far
TOPN_FN bool excluded(float u, float tau) { return u < tau; }
// candidates of a slice that is to bring `need` more accepted ones (the first slice: need = N + 1, ranked positions [0, slice_size(N + 1)); while no more than N are accepted
// nothing may be excluded, and the next slice is slice_size(N + 1 - accepted) more).  About an eighth of the candidates is rejected on real frames: an eighth more
// than needed, and a few, mostly leaves nothing for a further slice but what sits within a margin of tau
TOPN_FN int slice_size(int need) { return need + (need >> 3) + 8; }
// whether a frame of nCand candidates is ranked at all: with at most N of them everything is output (k_keylines does not even sort); rankCap: what the ranking holds
TOPN_FN bool ranks(int nCand, int N, int rankCap, int w, int h) { return N >= 1 && nCand > N && nCand <= rankCap && usable(w, h); }

}  // namespace topn
}  // namespace sslam
