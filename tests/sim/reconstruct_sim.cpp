// csrc/reconstruct_math.h on the host: the bit-exact model of k_reconstruct (csrc/reconstruct.hip) that tests/reconstruct_sim.py builds with plain g++, once as it is and
// once under the sanitizers.  Stand-alone: reads cases on stdin; floats travel as the decimal value of their 32 bits, doubles as that of their 64.
//   in : n1 n2 model sigma min_parallax min_triangulated fx fy cx cy nl1 nl2 nlp has_lines | n1 x (x y) | n2 x (x y) | n1 x match | n1 x inlier byte | H21[9] F21[9]
//        | has_lines: nl1 x (sx sy ex ey), nl1 x 3 doubles, nl2 x 3 doubles, nlp x (line 1, line 2)                                   (repeated until end of input)
//        a request "-1 count 0" followed by count floats answers one line "acos" with acos_f of each (the header's own function, for the sweep against libm)
//   out: "pose" ok reason model hypothesis n_inliers n_good[8] parallax[8] R21[9] t21[3] n_triangulated n_lines n_lines_triangulated
//        "hyp" h, R[9] t[3] n[3], the selected cosine                         (eight lines; zeros for a hypothesis that was not run)
//        "rows" h nm, per match: stage p3d[3] cos squareError1 squareError2        (eight lines)
//        "p3d" n1 x 3 | "tri" n1 bytes
//        "lines" nlp, per row: s3d[3] e3d[3] flag err1 err2 | "mad" th1 th2    (the two inlier thresholds of :1162-1163; 0 when no line ran)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../structure-slam-pointline_amd/csrc/reconstruct_math.h"

using namespace sslam;
using namespace sslam::rc;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static unsigned long long bits(double f) { unsigned long long u; memcpy(&u, &f, 8); return u; }
static bool read_float(float& f) { unsigned u; if (scanf("%u", &u) != 1) return false; memcpy(&f, &u, 4); return true; }
static bool read_double(double& f) { unsigned long long u; if (scanf("%llu", &u) != 1) return false; memcpy(&f, &u, 8); return true; }

struct HostWs4 { double m[WS4_DOUBLES]; double& at(int k) { return m[k]; } };
struct HostWs3 { double m[WS3_DOUBLES]; double& at(int k) { return m[k - pnp::WS_S]; } };

struct RowRec { int stage; float p3d[3], cosv, err1, err2; };

int main() {
    int n1, n2, model;
    while (scanf("%d %d %d", &n1, &n2, &model) == 3) {
        if (n1 == -1) {      // "-1 count 0" and count floats: acos_f of each
            printf("acos");
            for (int i = 0; i < n2; ++i) { float x; if (!read_float(x)) return 2; printf(" %u", bits(acos_f(x))); }
            printf("\n");
            continue;
        }
        float sigma, minParallax; int minTri, nl1, nl2, nlp, hasLines; Cam K;
        if (!read_float(sigma) || !read_float(minParallax) || scanf("%d", &minTri) != 1 || !read_float(K.fx) || !read_float(K.fy) || !read_float(K.cx) || !read_float(K.cy) ||
            scanf("%d %d %d %d", &nl1, &nl2, &nlp, &hasLines) != 4 || n1 < 0 || n2 < 0 || nl1 < 0 || nl2 < 0 || nlp < 0) return 2;
        std::vector<float> k1((size_t)n1 * 2), k2((size_t)n2 * 2);
        for (float& f : k1) if (!read_float(f)) return 2;
        for (float& f : k2) if (!read_float(f)) return 2;
        std::vector<int> m12((size_t)n1), inl((size_t)n1);
        for (int& m : m12) if (scanf("%d", &m) != 1) return 2;
        for (int& m : inl) if (scanf("%d", &m) != 1) return 2;
        float H21[9], F21[9];
        for (float& f : H21) if (!read_float(f)) return 2;
        for (float& f : F21) if (!read_float(f)) return 2;
        std::vector<float> kl1((size_t)nl1 * 4);
        std::vector<double> fn1((size_t)nl1 * 3), fn2((size_t)nl2 * 3);
        std::vector<int> lp((size_t)nlp * 2);
        if (hasLines) {
            for (float& f : kl1) if (!read_float(f)) return 2;
            for (double& f : fn1) if (!read_double(f)) return 2;
            for (double& f : fn2) if (!read_double(f)) return 2;
            for (int& p : lp) if (scanf("%d", &p) != 1) return 2;
        } else if (nl1 || nl2 || nlp) return 2;

        // the match list (:67-76) and vbMatchesInliers of the model, by match
        struct M { int i; float u1, v1, u2, v2; bool in; };
        std::vector<M> rows;
        const int bit = model == 1 ? 1 : 2;
        int N = 0;
        for (int i = 0; i < n1; ++i) if (m12[(size_t)i] >= 0 && m12[(size_t)i] < n2) {
            const int m = m12[(size_t)i];
            const bool in = model != 0 && (inl[(size_t)i] & bit);
            rows.push_back(M{i, k1[(size_t)2 * i], k1[(size_t)2 * i + 1], k2[(size_t)2 * m], k2[(size_t)2 * m + 1], in});
            if (in) ++N;
        }
        const int nm = (int)rows.size();
        HostWs3 w3; HostWs4 w4;
        Hyp hyp[8]; float nrm[8][3];
        memset(hyp, 0, sizeof(hyp)); memset(nrm, 0, sizeof(nrm));
        int nh = 0, reason = REASON_OK;
        if (model == 0) reason = REASON_SKIPPED;
        else if (model == 1) { if (hypotheses_h(w3, H21, K, hyp, nrm)) nh = 8; else reason = REASON_NOT_SEPARATED; }
        else { hypotheses_f(w3, F21, K, hyp); nh = 4; }
        const float th2 = th2_of(sigma);
        int nGood[8] = {0}; float par[8] = {0}, sel[8] = {0};
        std::vector<std::vector<RowRec>> rec(8, std::vector<RowRec>((size_t)nm, RowRec{0, {0, 0, 0}, 0, 0, 0}));
        for (int h = 0; h < nh; ++h) {
            hyp_setup(K, hyp[h]);
            std::vector<uint32_t> keys;
            for (int r = 0; r < nm; ++r) {
                if (!rows[(size_t)r].in) continue;
                RowOut o;
                check_row(K, hyp[h], rows[(size_t)r].u1, rows[(size_t)r].v1, rows[(size_t)r].u2, rows[(size_t)r].v2, th2, w4, o);
                RowRec& q = rec[(size_t)h][(size_t)r];
                q.stage = o.stage; memcpy(q.p3d, o.p3d, sizeof(q.p3d)); q.cosv = o.cosv; q.err1 = o.err1; q.err2 = o.err2;
                if (o.stage == STAGE_GOOD) keys.push_back(key_of(o.cosv));
            }
            nGood[h] = (int)keys.size();
            if (nGood[h] > 0) {
                const int k = nGood[h] - 1 < 50 ? nGood[h] - 1 : 50;
                sel[h] = value_of(kth_key<uint32_t>(k, [&](uint32_t t) { int c = 0; for (uint32_t x : keys) c += x < t; return c; }));
                par[h] = parallax_of(sel[h]);
            }
        }
        Choice ch{0, reason, -1};
        if (nh == 4) ch = choose_f(nGood, par, N, minParallax, minTri);
        if (nh == 8) ch = choose_h(nGood, par, N, minParallax, minTri);
        float R21[9] = {0}, t21[3] = {0};
        std::vector<float> p3d((size_t)n1 * 3, 0.f); std::vector<int> tri((size_t)n1, 0);
        int nTri = 0;
        if (ch.ok) {
            memcpy(R21, hyp[ch.hypothesis].R, sizeof(R21)); memcpy(t21, hyp[ch.hypothesis].t, sizeof(t21));
            for (int r = 0; r < nm; ++r) {
                const RowRec& q = rec[(size_t)ch.hypothesis][(size_t)r];
                if (q.stage != STAGE_GOOD) continue;
                memcpy(&p3d[(size_t)rows[(size_t)r].i * 3], q.p3d, 12); tri[(size_t)rows[(size_t)r].i] = 1; ++nTri;
            }
        }
        // ReconstructLine with the winner
        std::vector<LineOut> lo((size_t)nlp); std::vector<int> lvalid((size_t)nlp, 0), lflag((size_t)nlp, 0);
        int nLines = 0, nLinesTri = 0; double thr1 = 0.0, thr2 = 0.0;
        for (int r = 0; r < nlp; ++r) {
            memset(&lo[(size_t)r], 0, sizeof(LineOut));
            const int a = lp[(size_t)2 * r], b = lp[(size_t)2 * r + 1];
            lvalid[(size_t)r] = a >= 0 && a < nl1 && b >= 0 && b < nl2;
            nLines += lvalid[(size_t)r];
        }
        if (ch.ok && nLines > 0) {
            std::vector<double> e1, e2;
            for (int r = 0; r < nlp; ++r) if (lvalid[(size_t)r]) {
                const int a = lp[(size_t)2 * r], b = lp[(size_t)2 * r + 1];
                line_row(K, hyp[ch.hypothesis], &kl1[(size_t)a * 4], &fn1[(size_t)a * 3], &fn2[(size_t)b * 3], w4, lo[(size_t)r]);
                e1.push_back(lo[(size_t)r].err1); e2.push_back(lo[(size_t)r].err2);
            }
            auto threshold = [&](const std::vector<double>& e) {
                const int k = (int)e.size() / 2;
                const double med = value_of(kth_key<uint64_t>(k, [&](uint64_t t) { int c = 0; for (double x : e) c += key_of(x) < t; return c; }));
                const double mad = value_of(kth_key<uint64_t>(k, [&](uint64_t t) { int c = 0; for (double x : e) c += key_of(abs_dev(x, med)) < t; return c; }));
                return inlier_threshold(mad);
            };
            thr1 = threshold(e1); thr2 = threshold(e2);
            for (int r = 0; r < nlp; ++r) if (lvalid[(size_t)r]) {
                lflag[(size_t)r] = !(lo[(size_t)r].err1 > thr1 || lo[(size_t)r].err2 > thr2);
                nLinesTri += lflag[(size_t)r];
            }
        }

        printf("pose %d %d %d %d %d", ch.ok, ch.reason, model, ch.hypothesis, N);
        for (int h = 0; h < 8; ++h) printf(" %d", nGood[h]);
        for (int h = 0; h < 8; ++h) printf(" %u", bits(par[h]));
        for (float f : R21) printf(" %u", bits(f));
        for (float f : t21) printf(" %u", bits(f));
        printf(" %d %d %d\n", nTri, nLines, nLinesTri);
        for (int h = 0; h < 8; ++h) {
            printf("hyp %d", h);
            for (float f : hyp[h].R) printf(" %u", bits(f));
            for (float f : hyp[h].t) printf(" %u", bits(f));
            for (float f : nrm[h]) printf(" %u", bits(f));
            printf(" %u\n", bits(sel[h]));
        }
        for (int h = 0; h < 8; ++h) {
            printf("rows %d %d", h, nm);
            for (const RowRec& q : rec[(size_t)h]) printf(" %d %u %u %u %u %u %u", q.stage, bits(q.p3d[0]), bits(q.p3d[1]), bits(q.p3d[2]), bits(q.cosv), bits(q.err1), bits(q.err2));
            printf("\n");
        }
        printf("p3d");
        for (float f : p3d) printf(" %u", bits(f));
        printf("\ntri");
        for (int t : tri) printf(" %d", t);
        printf("\nlines %d", nlp);
        for (int r = 0; r < nlp; ++r) {
            const LineOut& o = lo[(size_t)r];
            printf(" %u %u %u %u %u %u %d %llu %llu", bits(o.s3d[0]), bits(o.s3d[1]), bits(o.s3d[2]), bits(o.e3d[0]), bits(o.e3d[1]), bits(o.e3d[2]), lflag[(size_t)r], bits(o.err1), bits(o.err2));
        }
        printf("\nmad %llu %llu\n", bits(thr1), bits(thr2));
    }
    return 0;
}
