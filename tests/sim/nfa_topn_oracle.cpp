// TEST / DESIGN-STUDY INFRASTRUCTURE (not product): walks the CPU oracle's LSD main loop (oracle/lsd_oracle.cpp Lsd::detect, restated as tests/sim/lsd_trace.cpp does) and
// records, for every candidate rectangle, what csrc/nfa_topn.h says of it BEFORE rect_improve and what rect_improve made of it: the data behind profiles/nfa_topn.txt and
// the bound check of tests/test_nfa_topn_cpu.py.  Built by tests/nfa_topn_sim.py with g++ as a shared object; never linked into the library.
#include "../../oracle/lsd_oracle.cpp"
#include "../../structure-slam-pointline_amd/csrc/nfa_topn.h"
namespace orc { int g_gaussVariant = 0; }      // (defined in orb_oracle.cpp, which this single-file build does not link)

// out[cap][12] per candidate in emission order: r0, margin, accepted at the first evaluation, accepted, final response (0 unless accepted), rectangle area (length x width,
// scaled pixels), the final segment's four coordinates (0 unless accepted), max |end point shift| in segment pixels, 0.  Returns the number of candidates.
extern "C" int nfa_topn_frame(const uint8_t* gray, int w, int h, double* out, int cap) {
    using namespace orc;
    namespace tn = sslam::topn;
    Img8 image(w, h); std::memcpy(image.d.data(), gray, (size_t)w * h);
    Lsd L;
    const double prec = M_PI * L.ANG_TH / 180, p = L.ANG_TH / 180;
    L.prologue(image);
    L.LOG_NT = 5 * (std::log10(double(L.w)) + std::log10(double(L.h))) / 2 + std::log10(11.0);
    const size_t min_reg_size = size_t(-L.LOG_NT / std::log10(p));
    L.used.assign((size_t)L.w * L.h, 0);
    std::vector<RegionPoint> reg;
    int cand = 0;
    for (size_t i = 0; i < L.order.size(); ++i) {
        const int idx = L.order[i], px = idx % L.w, py = idx / L.w;
        if (L.used[idx] != 0 || L.angles[idx] == NOTDEF) continue;
        double reg_angle;
        L.region_grow(px, py, reg, reg_angle, prec);
        if (reg.size() < min_reg_size) continue;
        Rect rec;
        L.region2rect(reg, reg_angle, prec, p, rec);
        if (!L.refine(reg, reg_angle, prec, p, rec, L.DENSITY_TH)) continue;
        const Rect first = rec;
        const bool atOnce = L.rect_nfa(first) > L.LOG_EPS;
        const double log_nfa = L.rect_improve(rec);
        const bool ok = log_nfa > L.LOG_EPS;
        if (cand < cap) {
            double* o = out + (size_t)cand * 12;
            o[0] = tn::rect_response(first.x1, first.y1, first.x2, first.y2, w, h);
            o[1] = tn::margin(first.x1, first.y1, first.x2, first.y2, w, h);
            o[2] = atOnce; o[3] = ok;
            // flsd's own conversion (+= 0.5, /= SCALE, float), then the KeyLine fill's response
            double x1 = rec.x1 + 0.5, y1 = rec.y1 + 0.5, x2 = rec.x2 + 0.5, y2 = rec.y2 + 0.5;
            x1 /= L.SCALE; y1 /= L.SCALE; x2 /= L.SCALE; y2 /= L.SCALE;
            const Seg4f s{float(x1), float(y1), float(x2), float(y2)};
            std::vector<KeyLine> kl;
            keylines_from_segments(w, h, std::vector<Seg4f>{s}, kl);
            o[4] = ok ? kl[0].response : 0.0;
            o[5] = dist(first.x1, first.y1, first.x2, first.y2) * first.width;
            o[6] = ok ? s.x1 : 0; o[7] = ok ? s.y1 : 0; o[8] = ok ? s.x2 : 0; o[9] = ok ? s.y2 : 0;
            o[10] = std::max(std::hypot(rec.x1 - first.x1, rec.y1 - first.y1), std::hypot(rec.x2 - first.x2, rec.y2 - first.y2)) / L.SCALE;
            o[11] = 0;
        }
        ++cand;
    }
    return cand;
}
