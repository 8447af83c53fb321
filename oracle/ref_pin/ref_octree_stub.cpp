// ORACLE — TEST INFRASTRUCTURE ONLY.  Driver of tests/test_orb_tail_cases_cpu.py: the REFERENCE's own DistributeOctTree -- /root/reference/src/ORBextractor.cc compiled
// unmodified against oracle/ref_pin/stub_cv -- on a candidate list read from a file, so that the oracle's quadtree is pinned to it on the edge-case lists of
// tests/orb_tail_cases.py and not only on whole frames.  The function is protected: the driver is a class derived from the extractor.
//   ref_octree_stub <in.bin> <out.bin>
//   in:  int32 W, H, N, n, then n x (x, y, score) relative to minBorder (16): the level's maxBorder - minBorder extents, the features wanted, the list in arrival order
//   out: int32 m, then m x (x, y, score): what DistributeOctTree keeps, in order
// Built with -DPIN_BUMP_ALLOC only (ref_orb_stub.cpp says why): heap addresses increase with creation order, which is decision D1 of the oracle.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <new>
#include <vector>
#include "ORBextractor.h"

#ifdef PIN_BUMP_ALLOC
#include <sys/mman.h>
static char* g_arena = nullptr; static size_t g_off = 0; static const size_t kArena = (size_t)24 << 30;   // lazily committed
static void* bump(size_t n) {
    if (!g_arena) { g_arena = (char*)mmap(nullptr, kArena, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0); if (g_arena == MAP_FAILED) abort(); }
    size_t o = (g_off + 15) & ~(size_t)15; if (o + n > kArena) abort(); g_off = o + n; return g_arena + o;
}
void* operator new(size_t n) { return bump(n); }
void* operator new[](size_t n) { return bump(n); }
void operator delete(void*) noexcept {}
void operator delete[](void*) noexcept {}
void operator delete(void*, size_t) noexcept {}
void operator delete[](void*, size_t) noexcept {}
#endif

struct OctTreeDriver : StructureSLAM::ORBextractor {
    OctTreeDriver(int nfeatures) : StructureSLAM::ORBextractor(nfeatures, 1.2f, 1, 20, 7) {}
    std::vector<cv::KeyPoint> run(const std::vector<cv::KeyPoint>& keys, int W, int H, int N) {
        const int minB = 16;       // EDGE_THRESHOLD - 3, src/ORBextractor.cc:773
        return DistributeOctTree(keys, minB, minB + W, minB, minB + H, N, 0);
    }
};

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[4];
    if (!f.read((char*)hdr, sizeof(hdr)) || hdr[3] < 0) { std::fprintf(stderr, "ref_octree_stub: cannot read %s\n", argv[1]); return 3; }
    std::vector<int> c((size_t)hdr[3] * 3);
    if (!c.empty() && !f.read((char*)c.data(), sizeof(int) * c.size())) return 3;
    std::vector<cv::KeyPoint> keys;
    for (int i = 0; i < hdr[3]; ++i) keys.push_back(cv::KeyPoint((float)c[3 * i], (float)c[3 * i + 1], 7.f, -1, (float)c[3 * i + 2], 0));      // as ComputeKeyPointsOctTree leaves them, :820-825
    OctTreeDriver ext(hdr[2]);
    const std::vector<cv::KeyPoint> kept = ext.run(keys, hdr[0], hdr[1], hdr[2]);
    std::vector<int> out(1, (int)kept.size());
    for (const cv::KeyPoint& k : kept) { out.push_back((int)k.pt.x); out.push_back((int)k.pt.y); out.push_back((int)k.response); }
    std::ofstream o(argv[2], std::ios::binary);
    o.write((const char*)out.data(), sizeof(int) * out.size());
    return o ? 0 : 4;
}
