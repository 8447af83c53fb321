// The reference's rotation-consistency check (src/ORBmatcher.cc: the rotHist blocks of every matcher and ComputeThreeMaxima, :1604-1666):
// the rotation bin of a match, a histogram of HISTO_LENGTH bins, the three fullest bins, and the matches outside them un-matched.
// Every matcher takes the rule from here.  The helpers hold no barrier and no fence: a caller keeps its own, where its comments place them.
// Part of match.hip (included there in front of the matcher headers, inside its anonymous namespace: one translation unit).  Not a standalone header.
#pragma once

// rot = angle1 - angle2 in [0, 360) -> bin = round(rot / HISTO_LENGTH), bin HISTO_LENGTH wraps to 0.  In range for angles of [0, 360); a
// caller whose rows may hold anything clamps the result before it indexes a histogram.
__device__ __forceinline__ int rot_bin(float angle1, float angle2) {
    float rot = __fsub_rn(angle1, angle2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, 1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// The bin as a histogram index whatever the rows hold: angles of [0, 360) never need the clamp, and a device-resident slot may hold anything.
__device__ __forceinline__ int rot_hist_bin(float angle1, float angle2) { return min(max(rot_bin(angle1, angle2), 0), HISTO_LENGTH - 1); }

// ComputeThreeMaxima: the first bin wins a tie (strict >); the second and third are dropped (-1) when they hold less than 10 % of the first
__device__ __forceinline__ void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3) {
    int i1 = -1, i2 = -1, i3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < HISTO_LENGTH; ++i) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { i2 = -1; i3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) i3 = -1;
    ind1 = i1; ind2 = i2; ind3 = i3;
}
__device__ __forceinline__ bool rot_kept(int bin, int ind1, int ind2, int ind3) { return bin == ind1 || bin == ind2 || bin == ind3; }

// The prune of the one-wave matchers, wave-uniform (every lane scans the finished histogram): entry t < count has the bin binOf(t), below 0
// when it never matched; unmatch(t) un-matches an entry outside the kept bins and says whether it still was a match.  Returns the number removed.
template <class BinOf, class Unmatch>
__device__ __forceinline__ int rot_prune_wave(const int* hist, int count, int lane, BinOf binOf, Unmatch unmatch) {
    int ind1, ind2, ind3;
    three_maxima(hist, ind1, ind2, ind3);
    int removed = 0;
    for (int t0 = 0; t0 < count; t0 += 64) {
        const int t = t0 + lane;
        bool rm = false;
        if (t < count) { const int bn = binOf(t); rm = bn >= 0 && !rot_kept(bn, ind1, ind2, ind3) && unmatch(t); }
        removed += __popcll(__ballot(rm));
    }
    return removed;
}

// Histogram, prune and count as a pass of its own over recorded bins, one workgroup of 256 (SearchByBoW behind k_search_bow, SearchForTriangulation
// behind k_tri_search): match[i] >= 0 is a match with the rotation bin qbin[i]; the pruned ones become -1, *nmatches the number left.
__global__ __launch_bounds__(256) void k_rot_finish(int* __restrict__ match, const int* __restrict__ qbin, int n, int checkOri, int* __restrict__ nmatches) {
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int keep[3];
    __shared__ int total;
    const int t = threadIdx.x;
    if (t < HISTO_LENGTH) hist[t] = 0;
    if (t == 0) total = 0;
    __syncthreads();
    if (checkOri) {
        for (int i = t; i < n; i += 256) if (match[i] >= 0) atomicAdd(&hist[qbin[i]], 1);
        __syncthreads();
        if (t == 0) three_maxima(hist, keep[0], keep[1], keep[2]);
        __syncthreads();
    }
    int cnt = 0;
    for (int i = t; i < n; i += 256) {
        if (match[i] < 0) continue;
        if (checkOri && !rot_kept(qbin[i], keep[0], keep[1], keep[2])) { match[i] = -1; continue; }
        ++cnt;
    }
    atomicAdd(&total, cnt);
    __syncthreads();
    if (t == 0) *nmatches = total;
}
