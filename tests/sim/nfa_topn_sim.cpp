// csrc/nfa_topn.h on the host: the model of the sliced validation of k_nfa_all's top-N form (csrc/lsd_nfa.h) that tests/nfa_topn_sim.py builds with plain g++, once as it
// is and once under the sanitizers.  Stand-alone: reads cases on stdin until the end of input, floats travel as the decimal value of their 32 bits.
//   in : n N rankCap w h | n x (u final accepted uin)    u = upper(r0, margin), final = the response rect_improve's result would get, accepted = 0 / 1,
//                                                        uin = upper(r0, the INNER margin) (= u away from the border; read by mutant 4 alone)
//   out: "flags" n values (0 rejected, 1 accepted, 2 not needed) | "stat" ranked slices validated
// The validation itself is the caller's (u, final, accepted) triple: the model decides only WHICH candidates are looked at, and in what order.
// -DTOPN_MUTANT=k (default 0: the rule) builds a model that is wrong in ONE way a kernel could be; tests/test_nfa_stage_cases_cpu.py shows that the cases of
// tests/nfa_stage_cases.py tell each from the rule by its flags.  1: tau = the (N-1)-th largest accepted response; 2: the (N+1)-th largest; 3: `excluded` with <=;
// 4: the edge margin replaced by the inner one; 5: exclusion allowed with exactly N accepted; 6: ties in the ranking broken by descending index.
#ifndef TOPN_MUTANT
#define TOPN_MUTANT 0
#endif
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../structure-slam-pointline_amd/csrc/nfa_topn.h"

using namespace sslam::topn;

static float from_bits(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static int cand_index(unsigned long long key) { const int i = key_index(key); return TOPN_MUTANT == 6 ? 0x7FFFFFFF - i : i; }

int main() {
    int n, N, rankCap, w, h;
    while (scanf("%d %d %d %d %d", &n, &N, &rankCap, &w, &h) == 5) {
        if (n < 0 || n > (1 << 20)) return 2;
        std::vector<float> u((size_t)n), fin((size_t)n); std::vector<int> acc((size_t)n), flag((size_t)n, FLAG_NOT_NEEDED);
        for (int i = 0; i < n; ++i) {
            unsigned a, b, c; if (scanf("%u %u %d %u", &a, &b, &acc[i], &c) != 4) return 2;
            u[i] = from_bits(TOPN_MUTANT == 4 ? c : a); fin[i] = from_bits(b);
        }
        int slices = 0, validated = 0;
        const bool ranked = ranks(n, N, rankCap, w, h);
        if (!ranked) {
            for (int i = 0; i < n; ++i) flag[i] = acc[i] ? FLAG_ACCEPTED : FLAG_REJECTED;
            slices = 1; validated = n;
        } else {
            std::vector<unsigned long long> keys((size_t)n);
            for (int i = 0; i < n; ++i) keys[i] = rank_key(u[i], TOPN_MUTANT == 6 ? 0x7FFFFFFF - i : i);
            std::sort(keys.begin(), keys.end());
            std::vector<float> accepted;      // final responses of the validated and accepted candidates
            int s0 = 0, s1 = std::min(n, slice_size(N + 1));
            while (s1 > s0) {
                ++slices;
                for (int s = s0; s < s1; ++s) {
                    const int c = cand_index(keys[s]);
                    flag[c] = acc[c] ? FLAG_ACCEPTED : FLAG_REJECTED;
                    if (acc[c]) accepted.push_back(fin[c]);
                }
                validated = s1; s0 = s1;
                if ((int)accepted.size() < N + (TOPN_MUTANT == 5 ? 0 : 1)) { s1 = std::min(n, s0 + slice_size(N + 1 - (int)accepted.size())); continue; }      // not yet more than N accepted: nothing can be excluded
                const int nth = TOPN_MUTANT == 1 ? std::max(N - 2, 0) : TOPN_MUTANT == 2 ? std::min(N, (int)accepted.size() - 1) : N - 1;
                std::nth_element(accepted.begin(), accepted.begin() + nth, accepted.end(), [](float a, float b) { return a > b; });
                const float tau = accepted[nth];
                while (s1 < n && !(TOPN_MUTANT == 3 ? u[cand_index(keys[s1])] <= tau : excluded(u[cand_index(keys[s1])], tau))) ++s1;
            }
        }
        printf("flags");
        for (int i = 0; i < n; ++i) printf(" %d", flag[i]);
        printf("\nstat %d %d %d\n", ranked ? 1 : 0, slices, validated);
    }
    return 0;
}
