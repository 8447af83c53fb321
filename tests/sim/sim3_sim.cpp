// csrc/sim3_math.h on the host: the bit-exact model of k_sim3_ransac (csrc/sim3.hip) that tests/sim3_sim.py builds with plain g++, once as it is and once under the
// sanitizers.  Stand-alone: reads cases on stdin; floats travel as the decimal value of their 32 bits, doubles of their 64.  The loop is the reference's, one iteration after
// the other (src/Sim3Solver.cc:140-207): the kernel's 64-wide rounds have to reproduce it.
//   in : n1 n2 nlevels fix_scale min_inliers max_iterations seed pair has_sets ncalls probability(64) K1[4] K2[4]
//        | nlevels x sigma2 | n1 x octave | n1 x valid | n1 x 3 floats | n2 x octave | n2 x valid | n2 x 3 floats | n1 x match | has_sets: max_iterations x 3 | ncalls x new_iterations
//   out: "n" N, then N x (row i1, 6 floats: P1im1, P2im2, maxErr1, maxErr2)
//        per call: "hyp" it, 3 set indices, s R[9] t[3], count, the ten N entries, the eigenvector (4 x 64 bits), mvbInliersi as a string of N digits ("-" when N is 0)
//                  (one line per iteration the call ran), then
//                  "state" its_done best_inliers best_it n max_its found_it n_inliers no_more s R[9] t[3]    and    "inl" n1 bytes
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../structure-slam-pointline_amd/csrc/sim3_math.h"

using namespace sslam::s3;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static unsigned long long bits64(double f) { unsigned long long u; memcpy(&u, &f, 8); return u; }
static bool read_float(float& f) { unsigned u; if (scanf("%u", &u) != 1) return false; memcpy(&f, &u, 4); return true; }

struct HostRows { const std::vector<Row>* r; Row operator()(int i) const { return (*r)[(size_t)i]; } };
struct State { int its_done, best_inliers, best_it, n, max_its, found_it, n_inliers, no_more; Sim3 best; };

int main() {
    int n1, n2, nlevels, fixScale, minInliers, maxIterations, hasSets, ncalls; unsigned seed, pair;
    while (scanf("%d %d %d %d %d %d %u %u %d %d", &n1, &n2, &nlevels, &fixScale, &minInliers, &maxIterations, &seed, &pair, &hasSets, &ncalls) == 10) {
        unsigned long long pb; double probability; Cam K1, K2;
        if (scanf("%llu", &pb) != 1 || n1 < 0 || n2 < 0 || nlevels < 1 || minInliers < 1 || maxIterations < 1 || ncalls < 0) return 2;
        memcpy(&probability, &pb, 8);
        if (!read_float(K1.fx) || !read_float(K1.fy) || !read_float(K1.cx) || !read_float(K1.cy) || !read_float(K2.fx) || !read_float(K2.fy) || !read_float(K2.cx) || !read_float(K2.cy)) return 2;
        std::vector<float> sigma2((size_t)nlevels), x1((size_t)n1 * 3), x2((size_t)n2 * 3);
        std::vector<int> oct1((size_t)n1), val1((size_t)n1), oct2((size_t)n2), val2((size_t)n2), m12((size_t)n1), sets, calls((size_t)ncalls);
        for (float& f : sigma2) if (!read_float(f)) return 2;
        for (int& v : oct1) if (scanf("%d", &v) != 1) return 2;
        for (int& v : val1) if (scanf("%d", &v) != 1) return 2;
        for (float& f : x1) if (!read_float(f)) return 2;
        for (int& v : oct2) if (scanf("%d", &v) != 1) return 2;
        for (int& v : val2) if (scanf("%d", &v) != 1) return 2;
        for (float& f : x2) if (!read_float(f)) return 2;
        for (int& v : m12) if (scanf("%d", &v) != 1) return 2;
        if (hasSets) { sets.resize((size_t)maxIterations * 3); for (int& s : sets) if (scanf("%d", &s) != 1) return 2; }
        for (int& v : calls) if (scanf("%d", &v) != 1 || v < 1) return 2;

        // the constructor (:62-109)
        std::vector<Row> rows; std::vector<int> idx1;
        for (int i = 0; i < n1; ++i) {
            const int m = m12[(size_t)i];
            if (m < 0 || m >= n2 || !val1[(size_t)i] || !val2[(size_t)m]) continue;
            const int o1 = oct1[(size_t)i], o2 = oct2[(size_t)m];
            if (o1 < 0 || o1 >= nlevels || o2 < 0 || o2 >= nlevels) continue;
            Row r;
            for (int k = 0; k < 3; ++k) { r.X1[k] = x1[(size_t)i * 3 + k]; r.X2[k] = x2[(size_t)m * 3 + k]; }
            camera_to_image(r.X1, K1, r.p1);
            camera_to_image(r.X2, K2, r.p2);
            r.maxErr1 = max_error(sigma2[(size_t)o1]); r.maxErr2 = max_error(sigma2[(size_t)o2]);
            rows.push_back(r); idx1.push_back(i);
        }
        const int N = (int)rows.size();
        printf("n %d", N);
        for (int i = 0; i < N; ++i) printf(" %d %u %u %u %u %u %u", idx1[(size_t)i], bits(rows[(size_t)i].p1[0]), bits(rows[(size_t)i].p1[1]), bits(rows[(size_t)i].p2[0]),
                                           bits(rows[(size_t)i].p2[1]), bits(rows[(size_t)i].maxErr1), bits(rows[(size_t)i].maxErr2));
        printf("\n");

        HostRows R{&rows};
        State st;
        memset(&st, 0, sizeof(st));      // a new Sim3Solver
        std::string marks((size_t)N, '0');
        for (int call = 0; call < ncalls; ++call) {
            std::vector<int> inl((size_t)n1, 0);
            st.n = N; st.found_it = -1; st.n_inliers = 0; st.no_more = 0;
            if (N < minInliers) {
                st.max_its = 0; st.no_more = 1;
            } else {
                st.max_its = ransac_max_its(probability, minInliers, maxIterations, N);
                if (st.its_done == 0) st.best_it = -1;
                int current = 0;
                while (st.its_done < st.max_its && current < calls[(size_t)call]) {
                    ++current;
                    const int it = st.its_done++;
                    int set[3]; bool valid = true;
                    if (hasSets) for (int j = 0; j < 3; ++j) { set[j] = sets[(size_t)it * 3 + j]; valid = valid && set[j] >= 0 && set[j] < N; }
                    else if (N >= 3) draw_set(seed, pair, (uint32_t)it, N, set);
                    else { set[0] = set[1] = set[2] = -1; valid = false; }
                    Sim3 h;
                    const int count = hypothesis(R, N, K1, K2, set, valid, fixScale != 0, h, [&](int i, bool in) { marks[(size_t)i] = in ? '1' : '0'; });
                    if (!valid) marks.assign((size_t)N, '0');
                    float ne[10] = {0}; double q[4] = {0, 0, 0, 0};
                    if (valid) {
                        float P1[9], P2[9], Pr1[9], Pr2[9], O1[3], O2[3];
                        for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) { P1[i * 3 + j] = rows[(size_t)set[j]].X1[i]; P2[i * 3 + j] = rows[(size_t)set[j]].X2[i]; }
                        centroid(P1, Pr1, O1); centroid(P2, Pr2, O2);
                        n_entries(Pr1, Pr2, ne);
                        jacobi_largest(ne, q);
                    }
                    printf("hyp %d %d %d %d %u", it, set[0], set[1], set[2], bits(h.s));
                    for (float f : h.R) printf(" %u", bits(f));
                    for (float f : h.t) printf(" %u", bits(f));
                    printf(" %d", count);
                    for (float f : ne) printf(" %u", bits(f));
                    for (double d : q) printf(" %llu", bits64(d));
                    printf(" %s\n", N ? marks.c_str() : "-");
                    if (count >= 0 && count >= st.best_inliers) {
                        st.best_inliers = count; st.best_it = it; st.best = h;
                        if (count > minInliers) {
                            st.found_it = it; st.n_inliers = count;
                            for (int i = 0; i < N; ++i) if (marks[(size_t)i] == '1') inl[(size_t)idx1[(size_t)i]] = 1;
                            break;
                        }
                    }
                }
                if (st.found_it < 0 && st.its_done >= st.max_its) st.no_more = 1;
            }
            printf("state %d %d %d %d %d %d %d %d %u", st.its_done, st.best_inliers, st.best_it, st.n, st.max_its, st.found_it, st.n_inliers, st.no_more, bits(st.best.s));
            for (float f : st.best.R) printf(" %u", bits(f));
            for (float f : st.best.t) printf(" %u", bits(f));
            printf("\ninl");
            for (int b : inl) printf(" %d", b);
            printf("\n");
        }
    }
    return 0;
}
