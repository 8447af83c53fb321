// csrc/two_view_math.h on the host: the bit-exact model of k_two_view (csrc/two_view.hip) that tests/two_view_sim.py builds with plain g++, once as it is and once under
// the sanitizers.  Stand-alone: reads cases on stdin, writes every hypothesis and the result; floats travel as the decimal value of their 32 bits.
//   in : n1 n2 iterations sigma seed pair has_sets | n1 x (x y) | n2 x (x y) | n1 x match | has_sets: iterations x 8 indices          (repeated until end of input)
//   out: "norm" 8 floats (meanX sX meanY sY of frame 1, frame 2)
//        "hyp" it, 8 set indices, Hn H21i H12i Fn F21i Fpre (54 floats), scoreH scoreF                                   (one line per iteration; none when nmatches < 8)
//        "res" nmatches model best_it_h best_it_f score_h score_f rh H21[9] F21[9]
//        "inl" n1 bytes
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../structure-slam-pointline_amd/csrc/two_view_math.h"

using namespace sslam::tv;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static bool read_float(float& f) { unsigned u; if (scanf("%u", &u) != 1) return false; f = from_bits(u); return true; }

struct HostWs { double m[WS_DOUBLES]; double& at(int k) { return m[k]; } };
struct HostRows { const std::vector<Row>* r; Row operator()(int i) const { return (*r)[(size_t)i]; } };

int main() {
    int n1, n2, iterations, hasSets; float sigma; unsigned seed, pair;
    while (scanf("%d %d %d", &n1, &n2, &iterations) == 3) {
        if (!read_float(sigma) || scanf("%u %u %d", &seed, &pair, &hasSets) != 3 || n1 < 0 || n2 < 0 || iterations < 1) return 2;
        std::vector<float> k1((size_t)n1 * 2), k2((size_t)n2 * 2);
        for (float& f : k1) if (!read_float(f)) return 2;
        for (float& f : k2) if (!read_float(f)) return 2;
        std::vector<int> m12((size_t)n1), sets;
        for (int& m : m12) if (scanf("%d", &m) != 1) return 2;
        if (hasSets) { sets.resize((size_t)iterations * 8); for (int& s : sets) if (scanf("%d", &s) != 1) return 2; }

        Norm N1, N2;
        normalize_axis(n1, [&](int i) { return k1[(size_t)2 * i]; }, N1.meanX, N1.sX);
        normalize_axis(n1, [&](int i) { return k1[(size_t)2 * i + 1]; }, N1.meanY, N1.sY);
        normalize_axis(n2, [&](int i) { return k2[(size_t)2 * i]; }, N2.meanX, N2.sX);
        normalize_axis(n2, [&](int i) { return k2[(size_t)2 * i + 1]; }, N2.meanY, N2.sY);
        printf("norm %u %u %u %u %u %u %u %u\n", bits(N1.meanX), bits(N1.sX), bits(N1.meanY), bits(N1.sY), bits(N2.meanX), bits(N2.sX), bits(N2.meanY), bits(N2.sY));

        std::vector<Row> rows; std::vector<int> rowOf((size_t)n1, -1);
        for (int i = 0; i < n1; ++i) if (m12[(size_t)i] >= 0 && m12[(size_t)i] < n2) {
            const int m = m12[(size_t)i];
            rowOf[(size_t)i] = (int)rows.size();
            rows.push_back(Row{k1[(size_t)2 * i], k1[(size_t)2 * i + 1], k2[(size_t)2 * m], k2[(size_t)2 * m + 1]});
        }
        const int nm = (int)rows.size();
        HostRows R{&rows};
        HostWs ws;
        float SH = 0.f, SF = 0.f, H21[9] = {0}, F21[9] = {0};
        int bestH = -1, bestF = -1, model = 0;
        float RH = 0.f;
        if (nm >= 8) {
            for (int it = 0; it < iterations; ++it) {
                int set[8]; bool valid = true;
                if (hasSets) for (int j = 0; j < 8; ++j) { set[j] = sets[(size_t)it * 8 + j]; valid = valid && set[j] >= 0 && set[j] < nm; }
                else draw_set(seed, pair, (uint32_t)it, nm, set);
                Hypothesis h;
                hypothesis(R, nm, N1, N2, set, valid, sigma, ws, h);
                printf("hyp %d", it);
                for (int j = 0; j < 8; ++j) printf(" %d", set[j]);
                const float* mats[6] = {h.Hn, h.H21, h.H12, h.Fn, h.F21, h.Fpre};
                for (const float* m : mats) for (int k = 0; k < 9; ++k) printf(" %u", bits(m[k]));
                printf(" %u %u\n", bits(h.scoreH), bits(h.scoreF));
                if (h.scoreH > SH) { SH = h.scoreH; bestH = it; memcpy(H21, h.H21, sizeof(H21)); }
                if (h.scoreF > SF) { SF = h.scoreF; bestF = it; memcpy(F21, h.F21, sizeof(F21)); }
            }
            select_model(SH, SF, RH, model);
        }
        printf("res %d %d %d %d %u %u %u", nm, model, bestH, bestF, bits(SH), bits(SF), bits(RH));
        for (float f : H21) printf(" %u", bits(f));
        for (float f : F21) printf(" %u", bits(f));
        printf("\ninl");
        float H12[9];
        inv3(H21, H12);
        const float iss = inv_sigma_square(sigma);
        for (int i = 0; i < n1; ++i) {
            int b = 0;
            if (nm >= 8 && rowOf[(size_t)i] >= 0) {
                const Row r = rows[(size_t)rowOf[(size_t)i]];
                float s = 0;
                if (bestH >= 0 && check_homography_match(H21, H12, r.u1, r.v1, r.u2, r.v2, iss, s)) b |= 1;
                if (bestF >= 0 && check_fundamental_match(F21, r.u1, r.v1, r.u2, r.v2, iss, s)) b |= 2;
            }
            printf(" %d", b);
        }
        printf("\n");
    }
    return 0;
}
