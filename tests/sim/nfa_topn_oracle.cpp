// TEST / DESIGN-STUDY INFRASTRUCTURE (not product): walks the CPU oracle's LSD main loop (oracle/lsd_oracle.cpp Lsd::detect, restated as tests/sim/lsd_trace.cpp does) and
// records, for every candidate rectangle, what csrc/nfa_topn.h says of it BEFORE rect_improve and what rect_improve made of it: the data behind profiles/nfa_topn.txt and
// the bound check of tests/test_nfa_topn_cpu.py.  nfa_topn_verdicts gives the same row for rectangle records the CALLER supplies over a frame's angle plane: the reference
// side of the injected lists of tests/nfa_stage_cases.py.  Built by tests/nfa_topn_sim.py with g++ as a shared object; never linked into the library.
#include "../../oracle/lsd_oracle.cpp"
#include "../../structure-slam-pointline_amd/csrc/nfa_topn.h"
namespace orc { int g_gaussVariant = 0; }      // (defined in orb_oracle.cpp, which this single-file build does not link)

namespace {

// o[12] for one rectangle record as region2rect / refine left it (`first`): r0, margin, accepted at the first evaluation, accepted, final response (0 unless accepted),
// rectangle area (length x width, scaled pixels), the final segment's four coordinates (0 unless accepted), max |end point shift| in segment pixels, 0.
// The oracle's own rect_nfa and rect_improve decide; L holds the frame's prologue and LOG_NT.
void record_row(const orc::Lsd& L, int w, int h, const orc::Rect& first, double* o) {
    using namespace orc;
    namespace tn = sslam::topn;
    Rect rec = first;
    const bool atOnce = L.rect_nfa(first) > L.LOG_EPS;
    const double log_nfa = L.rect_improve(rec);
    const bool ok = log_nfa > L.LOG_EPS;
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

void prepare(orc::Lsd& L, const uint8_t* gray, int w, int h) {
    orc::Img8 image(w, h); std::memcpy(image.d.data(), gray, (size_t)w * h);
    L.prologue(image);
    L.LOG_NT = 5 * (std::log10(double(L.w)) + std::log10(double(L.h))) / 2 + std::log10(11.0);
}

// the main loop; out[cap][12] = record_row per candidate in emission order, rects (unless null) [cap][12] = the candidate's first record, the twelve Rect fields in order
int walk(const uint8_t* gray, int w, int h, double* out, double* rects, int cap) {
    using namespace orc;
    Lsd L;
    const double prec = M_PI * L.ANG_TH / 180, p = L.ANG_TH / 180;
    prepare(L, gray, w, h);
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
        if (cand < cap) {
            record_row(L, w, h, rec, out + (size_t)cand * 12);
            static_assert(sizeof(Rect) == 12 * sizeof(double), "a record is twelve doubles");
            if (rects) std::memcpy(rects + (size_t)cand * 12, &rec, sizeof(rec));
        }
        ++cand;
    }
    return cand;
}

}  // namespace

// out[cap][12] per candidate in emission order (record_row).  Returns the number of candidates.
extern "C" int nfa_topn_frame(const uint8_t* gray, int w, int h, double* out, int cap) { return walk(gray, w, h, out, nullptr, cap); }

// nfa_topn_frame and, beside it, rects[cap][12] = each candidate's full first record (x1, y1, x2, y2, width, x, y, theta, dx, dy, prec, p) as region2rect / refine left it
extern "C" int nfa_topn_frame_rects(const uint8_t* gray, int w, int h, double* out, double* rects, int cap) { return walk(gray, w, h, out, rects, cap); }

// `n` records the caller supplies over the frame's prologue, each on its own (rect_nfa and rect_improve read the angle plane alone: no verdict depends on another record):
// out[n][12] = record_row.  Duplicated, reordered and foreign rectangles get the oracle's own verdict this way.
extern "C" int nfa_topn_verdicts(const uint8_t* gray, int w, int h, const double* rects, int n, double* out) {
    orc::Lsd L;
    prepare(L, gray, w, h);
    for (int i = 0; i < n; ++i) {
        orc::Rect rec;
        std::memcpy(&rec, rects + (size_t)i * 12, sizeof(rec));
        record_row(L, w, h, rec, out + (size_t)i * 12);
    }
    return n;
}
