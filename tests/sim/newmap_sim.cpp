// csrc/newmap_math.h on the host: the bit-exact model of k_newmap_points / k_newmap_lines (csrc/newmap.hip) that tests/newmap_sim.py builds with plain g++, once as it is
// and once under the sanitizers.  Stand-alone: reads cases on stdin; floats travel as the decimal value of their 32 bits, doubles as that of their 64.
//   in : 0 n1 n2 nlevels scale_factor | pose1[21] pose2[21] | scale_factors[nlevels] level_sigma2[nlevels] | n1 x (x y octave) | n2 x (x y octave) | n1 x match
//        1 nl1 nl2 nrows nlevels median_depth2 has_free | pose1[21] pose2[21] | scale_factors[nlevels] | nl1 x (sx sy ex ey octave), nl1 x 3 doubles | the same for nl2
//          | nrows x (idx1 idx2) | has_free: nl1 flags, nl2 flags                                                                     (repeated until end of input)
//        pose: Rcw[9] tcw[3] Ow[3] fx fy cx cy invfx invfy (sslam_kf_pose)
//   out: "points" n1 nnew, per row: stage x3d[3] normal[3] max_dist min_dist cos hom[4] err1 err2 ratioDist ratioOctave (the last four: the model's own trace)
//        "lines" nrows nnew, per row: stage s3d[3] e3d[3] normal[3] (doubles) max_dist min_dist cos shom[4] ehom[4] ratio1 .. ratio5 (the model's own trace)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../structure-slam-pointline_amd/csrc/newmap_math.h"

using namespace sslam;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static unsigned long long bits(double f) { unsigned long long u; memcpy(&u, &f, 8); return u; }
static bool read_float(float& f) { unsigned u; if (scanf("%u", &u) != 1) return false; memcpy(&f, &u, 4); return true; }
static bool read_double(double& f) { unsigned long long u; if (scanf("%llu", &u) != 1) return false; memcpy(&f, &u, 8); return true; }
static bool read_pose(sslam_kf_pose& P) {
    float v[21];
    for (float& f : v) if (!read_float(f)) return false;
    memcpy(&P, v, sizeof(P));
    return true;
}
static_assert(sizeof(sslam_kf_pose) == 84, "21 floats");

struct HostWs4 { double m[rc::WS4_DOUBLES]; double& at(int k) { return m[k]; } };

static int points(int n1) {
    int n2, nlevels; float scaleFactor; sslam_kf_pose P1, P2;
    if (scanf("%d %d", &n2, &nlevels) != 2 || !read_float(scaleFactor) || n1 < 0 || n2 < 0 || nlevels < 1 || nlevels > 64 || !read_pose(P1) || !read_pose(P2)) return 2;
    std::vector<float> sf((size_t)nlevels), sigma2((size_t)nlevels);
    for (float& f : sf) if (!read_float(f)) return 2;
    for (float& f : sigma2) if (!read_float(f)) return 2;
    struct Kp { float x, y; int octave; };
    std::vector<Kp> k1((size_t)n1), k2((size_t)n2);
    for (Kp& k : k1) if (!read_float(k.x) || !read_float(k.y) || scanf("%d", &k.octave) != 1) return 2;
    for (Kp& k : k2) if (!read_float(k.x) || !read_float(k.y) || scanf("%d", &k.octave) != 1) return 2;
    std::vector<int> m12((size_t)n1);
    for (int& m : m12) if (scanf("%d", &m) != 1) return 2;
    const float ratioFactor = 1.5f * scaleFactor;
    std::vector<nm::PointOut> out((size_t)n1);
    HostWs4 w;
    int nnew = 0;
    for (int i = 0; i < n1; ++i) {
        nm::PointOut& o = out[(size_t)i];
        memset(&o, 0, sizeof(o));
        const int m = m12[(size_t)i];
        if (m < 0 || m >= n2) { o.stage = nm::PT_NO_MATCH; continue; }
        const Kp &a = k1[(size_t)i], &b = k2[(size_t)m];
        nm::point_row(P1, P2, a.x, a.y, a.octave, b.x, b.y, b.octave, sf.data(), sigma2.data(), nlevels, ratioFactor, w, o);
        nnew += o.stage == nm::PT_CREATED;
    }
    printf("points %d %d", n1, nnew);
    for (const nm::PointOut& o : out) {
        printf(" %d %u %u %u %u %u %u %u %u %u", o.stage, bits(o.x3d[0]), bits(o.x3d[1]), bits(o.x3d[2]), bits(o.normal[0]), bits(o.normal[1]), bits(o.normal[2]), bits(o.max_dist),
               bits(o.min_dist), bits(o.cosv));
        for (float f : o.hom) printf(" %u", bits(f));
        printf(" %u %u %u %u", bits(o.err1), bits(o.err2), bits(o.ratio_dist), bits(o.ratio_octave));
    }
    printf("\n");
    return 0;
}

static int lines(int nl1) {
    int nl2, nrows, nlevels, hasFree; float median; sslam_kf_pose P1, P2;
    if (scanf("%d %d %d", &nl2, &nrows, &nlevels) != 3 || !read_float(median) || scanf("%d", &hasFree) != 1 || nl1 < 0 || nl2 < 0 || nrows < 0 || nlevels < 1 || nlevels > 64 ||
        !read_pose(P1) || !read_pose(P2)) return 2;
    std::vector<float> sf((size_t)nlevels);
    for (float& f : sf) if (!read_float(f)) return 2;
    struct Kl { float e[4]; int octave; double f[3]; };
    std::vector<Kl> l1((size_t)nl1), l2((size_t)nl2);
    for (std::vector<Kl>* v : {&l1, &l2}) {
        for (Kl& k : *v) { for (float& f : k.e) if (!read_float(f)) return 2; if (scanf("%d", &k.octave) != 1) return 2; }
        for (Kl& k : *v) for (double& f : k.f) if (!read_double(f)) return 2;
    }
    std::vector<int> lp((size_t)nrows * 2), free1((size_t)nl1, 1), free2((size_t)nl2, 1);
    for (int& p : lp) if (scanf("%d", &p) != 1) return 2;
    if (hasFree) {
        for (int& f : free1) if (scanf("%d", &f) != 1) return 2;
        for (int& f : free2) if (scanf("%d", &f) != 1) return 2;
    }
    std::vector<nm::LineOut> out((size_t)nrows);
    HostWs4 w;
    int nnew = 0;
    for (int r = 0; r < nrows; ++r) {
        nm::LineOut& o = out[(size_t)r];
        memset(&o, 0, sizeof(o));
        const int a = lp[(size_t)2 * r], b = lp[(size_t)2 * r + 1];
        if (a < 0 || a >= nl1 || b < 0 || b >= nl2) { o.stage = nm::LN_NO_MATCH; continue; }
        if (!free1[(size_t)a] || !free2[(size_t)b]) { o.stage = nm::LN_NOT_FREE; continue; }      // the flags as they stand before the pair creates anything
        const Kl &x = l1[(size_t)a], &y = l2[(size_t)b];
        nm::line_row(P1, P2, x.e, x.f, x.octave, y.e, y.f, median, sf.data(), nlevels, w, o);
        nnew += o.stage == nm::LN_CREATED;
    }
    printf("lines %d %d", nrows, nnew);
    for (const nm::LineOut& o : out) {
        printf(" %d %u %u %u %u %u %u %llu %llu %llu %u %u %u", o.stage, bits(o.s3d[0]), bits(o.s3d[1]), bits(o.s3d[2]), bits(o.e3d[0]), bits(o.e3d[1]), bits(o.e3d[2]),
               bits(o.normal[0]), bits(o.normal[1]), bits(o.normal[2]), bits(o.max_dist), bits(o.min_dist), bits(o.cosv));
        for (float f : o.shom) printf(" %u", bits(f));
        for (float f : o.ehom) printf(" %u", bits(f));
        for (float f : o.ratio) printf(" %u", bits(f));
    }
    printf("\n");
    return 0;
}

int main() {
    int kind, n;
    while (scanf("%d %d", &kind, &n) == 2) {
        const int rc = kind == 0 ? points(n) : kind == 1 ? lines(n) : 2;
        if (rc) return rc;
    }
    return 0;
}
