// csrc/pnp_math.h on the host: the bit-exact model of k_pnp_ransac (csrc/pnp.hip) that tests/pnp_sim.py builds with plain g++, once as it is and once under the
// sanitizers.  Stand-alone: reads commands on stdin; floats travel as the decimal value of their 32 bits, doubles of their 64.  The loop is the reference's, one iteration
// after the other with Refine on every qualifying iteration (src/PnPsolver.cc:165-305): the kernel's 64-wide rounds and its remembered Refine have to reproduce it.
//   "case" nf nkf nlevels min_inliers max_iterations seed pair nsets(-1: the library draws) ncalls probability(64) epsilon th2 K[4]
//        | nlevels x sigma2 | nf x octave | nf x 2 floats (pt) | nkf x valid | nkf x 3 floats | nf x assigned | nsets x 4 | ncalls x new_iterations
//     -> "n" N min_inliers max_its, then N x (frame row j, maxErr)
//        per call: "hyp" it, 4 set indices, R[9] t[3] (64 bits), count, N | reach flags << 8 (pnp::REACH_*), rep[3], betas[12] (64 bits), refine ran, refined count, mvbInliersi as N digits ("-" when N is 0)
//                  (one line per iteration the call ran), then "state" with every field of sslam_pnp_state in order and "inl" nf bytes
//   "plan" cap -> "plan" rowBytes ldsBytes ldsOptIn threads maxCap                                  (pnp_plan, csrc/match_plan.h)
//   "table" probability(64) min_inliers max_iterations epsilon cap -> "table" then cap + 1 pairs    (pnp::ransac_params)
//   "params" has_sigma nlevels probability(64) min_inliers max_iterations new_iterations epsilon th2 npairs cap nframes nkeyframes kfcap has_sets nsets
//     -> "params" pnp_params_ok pnp_sizes_ok                                                        (csrc/match_check.h)
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../structure-slam-pointline_amd/csrc/match_check.h"
#include "../../structure-slam-pointline_amd/csrc/pnp_math.h"

namespace sslam { void set_error(const char*, ...) {} }
using namespace sslam::pnp;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static unsigned long long bits64(double f) { unsigned long long u; memcpy(&u, &f, 8); return u; }
static bool read_float(float& f) { unsigned u; if (scanf("%u", &u) != 1) return false; memcpy(&f, &u, 4); return true; }
static bool read_double(double& f) { unsigned long long u; if (scanf("%llu", &u) != 1) return false; memcpy(&f, &u, 8); return true; }

struct HostRows { const std::vector<Row>* r; Row operator()(int i) const { return (*r)[(size_t)i]; } };
struct HostMask { const std::vector<unsigned long long>* m; unsigned long long operator()(int w) const { return (*m)[(size_t)w]; } };
struct HostWs { double d[WS_DOUBLES]; double& at(int k) { return d[k]; } };

static std::vector<unsigned long long> mask_of(const std::string& marks) {
    std::vector<unsigned long long> m((marks.size() + 63) / 64 + 1, 0ull);
    for (size_t i = 0; i < marks.size(); ++i) if (marks[i] == '1') m[i >> 6] |= 1ull << (i & 63);
    return m;
}

static int run_case() {
    int nf, nkf, nlevels, minInliersArg, maxIterations, nsets, ncalls; unsigned seed, pair;
    double probability; float epsilon, th2, Kf[4];
    if (scanf("%d %d %d %d %d %u %u %d %d", &nf, &nkf, &nlevels, &minInliersArg, &maxIterations, &seed, &pair, &nsets, &ncalls) != 9) return 2;
    if (!read_double(probability) || !read_float(epsilon) || !read_float(th2) || nf < 0 || nkf < 0 || nlevels < 1 || minInliersArg < 1 || maxIterations < 1 || ncalls < 0) return 2;
    for (float& f : Kf) if (!read_float(f)) return 2;
    const Cam K{Kf[0], Kf[1], Kf[2], Kf[3]};
    std::vector<float> sigma2((size_t)nlevels), pt((size_t)nf * 2), xw((size_t)nkf * 3);
    std::vector<int> oct((size_t)nf), valid((size_t)nkf), assigned((size_t)nf), sets, calls((size_t)ncalls);
    for (float& f : sigma2) if (!read_float(f)) return 2;
    for (int& v : oct) if (scanf("%d", &v) != 1) return 2;
    for (float& f : pt) if (!read_float(f)) return 2;
    for (int& v : valid) if (scanf("%d", &v) != 1) return 2;
    for (float& f : xw) if (!read_float(f)) return 2;
    for (int& v : assigned) if (scanf("%d", &v) != 1) return 2;
    if (nsets >= 0) { sets.resize((size_t)nsets * 4); for (int& s : sets) if (scanf("%d", &s) != 1) return 2; }
    for (int& v : calls) if (scanf("%d", &v) != 1 || v < 1) return 2;

    // the constructor (:67-110)
    std::vector<Row> rows; std::vector<int> idx;
    for (int j = 0; j < nf; ++j) {
        const int a = assigned[(size_t)j];
        if (a < 0 || a >= nkf || !valid[(size_t)a]) continue;
        const int o = oct[(size_t)j];
        if (o < 0 || o >= nlevels) continue;
        Row r;
        for (int k = 0; k < 3; ++k) r.X[k] = xw[(size_t)a * 3 + k];
        r.u = pt[(size_t)j * 2]; r.v = pt[(size_t)j * 2 + 1];
        r.maxErr = max_error(sigma2[(size_t)o], th2);
        rows.push_back(r); idx.push_back(j);
    }
    const int N = (int)rows.size();
    int32_t minInliers, maxIts;
    ransac_params(probability, minInliersArg, maxIterations, epsilon, N, minInliers, maxIts);
    printf("n %d %d %d", N, minInliers, maxIts);
    for (int i = 0; i < N; ++i) printf(" %d %u", idx[(size_t)i], bits(rows[(size_t)i].maxErr));
    printf("\n");

    HostRows R{&rows};
    HostWs* w = new HostWs;
    memset(w, 0, sizeof(*w));
    sslam_pnp_state st;
    memset(&st, 0, sizeof(st));      // a new PnPsolver
    std::string marks((size_t)N, '0'), bestMarks((size_t)N, '0'), refMarks((size_t)N, '0');
    for (int call = 0; call < ncalls; ++call) {
        std::vector<int> inl((size_t)nf, 0);
        st.n = N; st.min_inliers = minInliers; st.max_its = maxIts; st.found = 0; st.found_it = -1; st.n_inliers = 0; st.no_more = 0;
        for (float& f : st.Tcw) f = 0.f;
        if (N < minInliers) {
            st.no_more = 1;      // :173-177
        } else {
            if (st.its_done == 0) st.best_it = -1;
            int current = 0;
            while (st.its_done < maxIts || current < calls[(size_t)call]) {      // :182
                ++current;
                const int it = st.its_done++;
                int set[4] = {-1, -1, -1, -1}; bool ok = true;
                if (nsets >= 0) {
                    if (it < nsets) for (int j = 0; j < 4; ++j) { set[j] = sets[(size_t)it * 4 + j]; ok = ok && set[j] >= 0 && set[j] < N; }
                    else ok = false;
                } else if (N >= 4) draw_set(seed, pair, (uint32_t)it, N, set);
                else ok = false;
                Pose h; Trace tr;
                const int count = hypothesis(R, N, K, set, ok, *w, h, tr, [&](int i, bool in) { marks[(size_t)i] = in ? '1' : '0'; });
                if (!ok) marks.assign((size_t)N, '0');
                int refRan = 0, refCount = 0;
                if (count >= minInliers) {      // :209
                    if (count > st.best_inliers) {
                        bestMarks = marks; st.best_inliers = count; st.best_it = it;
                        for (int k = 0; k < 9; ++k) st.best_R[k] = h.R[k];
                        for (int k = 0; k < 3; ++k) st.best_t[k] = h.t[k];
                    }
                    // Refine (:260-305)
                    const std::vector<unsigned long long> mask = mask_of(bestMarks);
                    MaskedPts<HostRows, HostMask> P{R, HostMask{&mask}, N, 0};
                    for (char c : bestMarks) if (c == '1') ++P.n;
                    Pose rp; Trace rtr;
                    compute_pose(P, K, *w, rp, rtr);
                    for (int i = 0; i < N; ++i) { const bool in = check_row(rp, K, rows[(size_t)i]); refMarks[(size_t)i] = in ? '1' : '0'; if (in) ++refCount; }
                    refRan = 1;
                    st.refine_ok = refCount > minInliers ? 1 : 0;
                    if (st.refine_ok) {
                        st.found = 1; st.found_it = it; st.n_inliers = refCount;
                        for (int k = 0; k < 3; ++k) { for (int c = 0; c < 3; ++c) st.Tcw[k * 4 + c] = (float)rp.R[k * 3 + c]; st.Tcw[k * 4 + 3] = (float)rp.t[k]; }
                        for (int i = 0; i < N; ++i) if (refMarks[(size_t)i] == '1') inl[(size_t)idx[(size_t)i]] = 1;
                    }
                }
                printf("hyp %d %d %d %d %d", it, set[0], set[1], set[2], set[3]);
                for (double d : h.R) printf(" %llu", bits64(d));
                for (double d : h.t) printf(" %llu", bits64(d));
                printf(" %d %d", count, tr.N | (tr.flags << 8));
                for (double d : tr.rep) printf(" %llu", bits64(d));
                for (int k = 0; k < 3; ++k) for (double d : tr.betas[k]) printf(" %llu", bits64(d));
                printf(" %d %d %s\n", refRan, refCount, N ? marks.c_str() : "-");
                if (st.found) break;
            }
            if (!st.found && st.its_done >= maxIts) {      // :241-255
                st.no_more = 1;
                if (st.best_inliers >= minInliers) {
                    st.found = 2; st.found_it = st.best_it; st.n_inliers = st.best_inliers;
                    for (int k = 0; k < 3; ++k) { for (int c = 0; c < 3; ++c) st.Tcw[k * 4 + c] = (float)st.best_R[k * 3 + c]; st.Tcw[k * 4 + 3] = (float)st.best_t[k]; }
                    for (int i = 0; i < N; ++i) if (bestMarks[(size_t)i] == '1') inl[(size_t)idx[(size_t)i]] = 1;
                }
            }
        }
        printf("state %d %d %d %d %d %d %d %d %d %d %d", st.its_done, st.best_inliers, st.best_it, st.refine_ok, st.n, st.min_inliers, st.max_its, st.found, st.found_it,
               st.n_inliers, st.no_more);
        for (double d : st.best_R) printf(" %llu", bits64(d));
        for (double d : st.best_t) printf(" %llu", bits64(d));
        for (float f : st.Tcw) printf(" %u", bits(f));
        printf("\ninl");
        for (int b : inl) printf(" %d", b);
        printf("\n");
    }
    delete w;
    return 0;
}

int main() {
    static_assert(sizeof(sslam_pnp_state) == 192, "sslam_pnp_state has no padding");
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        const std::string c = cmd;
        if (c == "case") {
            if (int rc = run_case()) return rc;
        } else if (c == "plan") {
            int cap;
            if (scanf("%d", &cap) != 1) return 2;
            const sslam::RansacPlan P = sslam::pnp_plan(cap);
            printf("plan %d %zu %d %u %d\n", P.rowBytes, P.ldsBytes, P.ldsOptIn, P.threads, P.maxCap);
        } else if (c == "table") {
            double probability; int minInliers, maxIterations, cap; float epsilon;
            if (!read_double(probability) || scanf("%d %d", &minInliers, &maxIterations) != 2 || !read_float(epsilon) || scanf("%d", &cap) != 1 || cap < 0) return 2;
            printf("table");
            for (int n = 0; n <= cap; ++n) { int32_t a, b; ransac_params(probability, minInliers, maxIterations, epsilon, n, a, b); printf(" %d %d", a, b); }
            printf("\n");
        } else if (c == "params") {
            int hasSigma, nlevels, minInliers, maxIterations, newIterations, npairs, cap, nframes, nkeyframes, kfcap, hasSets, nsets; double probability; float epsilon, th2;
            if (scanf("%d %d", &hasSigma, &nlevels) != 2 || !read_double(probability) || scanf("%d %d %d", &minInliers, &maxIterations, &newIterations) != 3 ||
                !read_float(epsilon) || !read_float(th2) || scanf("%d %d %d %d %d %d %d", &npairs, &cap, &nframes, &nkeyframes, &kfcap, &hasSets, &nsets) != 7) return 2;
            const float sigma = 1.f;
            printf("params %d %d\n", sslam::pnp_params_ok(hasSigma ? &sigma : nullptr, nlevels, probability, minInliers, maxIterations, newIterations, epsilon, th2) ? 1 : 0,
                   sslam::pnp_sizes_ok(npairs, cap, nframes, nkeyframes, kfcap, hasSets ? (const void*)&sigma : nullptr, nsets) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
