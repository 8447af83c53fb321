// Host-only checks of the library's host side, built by tests/test_host_checks_cpu.py with a plain host compiler under
// -fsanitize=address,undefined -DSSLAM_TESTING (no GPU, no HIP: tests/sim/hip_stub stands in for the runtime):
//   check_csr (csrc/match_check.h)        which CSR lists a call accepts, and that a refused list is never read past what its offsets promise
//   all_aligned, rows_in_range, fits_31_bits (csrc/match_check.h)   the alignment and size rules of the device-resident batches, on both sides of every bound
//   sim3_params_ok, injected_sets_ok (csrc/match_check.h)   the parameter rules of the RANSAC entry points (two_view.hip, sim3.hip), on both sides of every bound
//   StreamOrderedBuf (csrc/common.h)      which runtime calls acquire / mark / release make, in which order
//   gather_to_root (csrc/group_exchange.h) over the RCCL stand-in (csrc/rccl_standin.h), a thread per rank: the lengths' all-gather and the payload
//                                         exchange of both group forms, for several rank counts, with and without the root's own bytes through the table
// Every array is a heap block of exactly its length, so a read or write past it ends the run.  Prints one line per check group, "ok" at the end.
#include "../../structure-slam-pointline_amd/csrc/common.h"
#include "../../structure-slam-pointline_amd/csrc/match_check.h"
#include "../../structure-slam-pointline_amd/csrc/group_exchange.h"
#include "../../structure-slam-pointline_amd/csrc/rccl_standin.h"
#include <cmath>
#include <cstdarg>
#include <limits>
#include <memory>
#include <thread>

static std::string g_err;
namespace sslam {
void set_error(const char* fmt, ...) {
    char b[512];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof(b), fmt, ap); va_end(ap);
    g_err = b;
}
}  // namespace sslam
using namespace sslam;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

static int csr(std::vector<int32_t> ptr, std::vector<int32_t> idx, int limit, bool with_idx = true) {
    g_err.clear();
    std::vector<int32_t> p(ptr), i(idx);      // exact-size heap copies
    p.shrink_to_fit(); i.shrink_to_fit();
    return check_csr("fn", "node", p.data(), (int)p.size() - 1, with_idx ? i.data() : nullptr, limit);
}
static bool refused(int rc, const char* text) { return rc == SSLAM_ERR_INVALID && g_err.rfind("fn: node ", 0) == 0 && g_err.find(text) != std::string::npos; }

static int check_csr_cases() {
    CHECK(csr({0, 2, 2, 5}, {4, 0, 1, 2, 3}, 5) == SSLAM_OK);                 // an empty list in the middle, the largest index allowed
    CHECK(csr({0}, {}, 5) == SSLAM_OK);                                       // nnodes = 0: nothing to read
    CHECK(csr({0, 0, 0}, {}, 0) == SSLAM_OK);
    CHECK(csr({0, 3}, {7, 8, 9}, 0, false) == SSLAM_OK);                      // offsets alone
    CHECK(refused(csr({0, 100, 5}, {0, 1, 2, 3, 4}, 5), "non-decreasing"));   // the total says 5, the first list 100: refused before an index is read
    CHECK(refused(csr({0, -3}, {}, 5), "non-decreasing"));                    // a negative total
    CHECK(refused(csr({0, 2, -1}, {0, 1}, 5), "non-decreasing"));
    CHECK(refused(csr({1, 2}, {0, 1}, 5), "start at 0"));
    CHECK(refused(csr({0, 2, 100, 5}, {0, 1, 2, 3, 4}, 5, false), "non-decreasing"));
    CHECK(refused(csr({0, 2, 3}, {0, 1, 5}, 5), "out of range"));             // index == limit
    CHECK(refused(csr({0, 2, 3}, {0, -1, 2}, 5), "out of range"));
    CHECK(refused(csr({0, 1}, {0}, 0), "out of range"));                      // no row at all to point at
    printf("check_csr ok\n");
    return 0;
}

static int check_argument_rules() {
    alignas(16) static unsigned char block[64];
    const uint8_t* a = block + 16; const float* f = (const float*)(block + 32); const int32_t* none = nullptr;
    CHECK(all_aligned<16>(a) && all_aligned<16>(a, f) && all_aligned<4>(a, f, block + 4) && all_aligned<8>(block + 8, f));
    for (int off : {1, 2, 4, 8}) {                                             // the largest power of two that divides the address decides
        const uint8_t* m = block + 16 + off;
        for (int al : {2, 4, 8, 16}) {
            const bool want = off % al == 0;
            const bool got = al == 2 ? all_aligned<2>(a, m, f) : al == 4 ? all_aligned<4>(a, m, f) : al == 8 ? all_aligned<8>(a, m, f) : all_aligned<16>(a, m, f);
            CHECK(got == want);
        }
        CHECK(!all_aligned<16>(m) && !all_aligned<16>(f, a, m) && all_aligned<1>(m));      // wherever it stands in the list
    }
    CHECK(all_aligned<16>(a, none, f) && all_aligned<4>(none) && all_aligned<16>((const void*)nullptr, a));      // a null pointer is aligned
    CHECK(!all_aligned<4>(none, block + 17));
    CHECK(!rows_in_range(-1) && rows_in_range(0) && rows_in_range(MAX_ROWS - 1) && !rows_in_range(MAX_ROWS) && MAX_ROWS == 1 << 19);
    CHECK(!rows_in_range(INT32_MIN) && !rows_in_range(INT32_MAX));
    CHECK(fits_31_bits(1, INT32_MAX) && fits_31_bits(INT32_MAX, 1) && !fits_31_bits(1 << 16, 1 << 15) && !fits_31_bits(2, 1 << 30));      // 2^31 - 1 and 2^31
    CHECK(fits_31_bits((1 << 16) - 1, 1 << 15) && fits_31_bits(0, INT32_MAX) && fits_31_bits(INT32_MAX, 0) && !fits_31_bits(INT32_MAX, INT32_MAX));      // no wrap in 64 bits
    printf("argument rules ok\n");
    return 0;
}

static int check_ransac_rules() {
    std::unique_ptr<float[]> table(new float[1]{1.f});      // the rule looks at the pointer, never at a level
    const float* t = table.get();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(sim3_params_ok(t, 1, 0.99, 1, 1, 1) && sim3_params_ok(t, 64, 0.99, 20, 300, 5));
    CHECK(!sim3_params_ok(t, 0, 0.99, 1, 1, 1) && !sim3_params_ok(t, 65, 0.99, 1, 1, 1) && !sim3_params_ok(t, -1, 0.99, 1, 1, 1));      // nlevels in 1 .. 64
    CHECK(!sim3_params_ok(nullptr, 1, 0.99, 1, 1, 1) && !sim3_params_ok(nullptr, 64, 0.99, 1, 1, 1));
    CHECK(!sim3_params_ok(t, 8, 0.0, 1, 1, 1) && !sim3_params_ok(t, 8, 1.0, 1, 1, 1) && !sim3_params_ok(t, 8, nan, 1, 1, 1) && !sim3_params_ok(t, 8, -0.0, 1, 1, 1));
    CHECK(sim3_params_ok(t, 8, std::nextafter(0.0, 1.0), 1, 1, 1) && sim3_params_ok(t, 8, std::nextafter(1.0, 0.0), 1, 1, 1));      // the nearest doubles inside (0, 1)
    CHECK(!sim3_params_ok(t, 8, std::nextafter(1.0, 2.0), 1, 1, 1) && !sim3_params_ok(t, 8, -std::nextafter(0.0, 1.0), 1, 1, 1));
    CHECK(!sim3_params_ok(t, 8, 0.99, 0, 1, 1) && !sim3_params_ok(t, 8, 0.99, 1, 0, 1) && !sim3_params_ok(t, 8, 0.99, 1, 1, 0));      // each count at 0 beside the 1s above
    CHECK(!sim3_params_ok(t, 8, 0.99, -1, 1, 1) && !sim3_params_ok(t, 8, 0.99, 1, INT32_MIN, 1) && sim3_params_ok(t, 8, 0.99, INT32_MAX, INT32_MAX, INT32_MAX));
    // injected sets: npairs * iterations stays below 2^28, asked only where sets are given
    const int32_t sets[1] = {0};
    CHECK(injected_sets_ok(sets, 1, (1 << 28) - 1) && !injected_sets_ok(sets, 1, 1 << 28) && injected_sets_ok(sets, (1 << 28) - 1, 1) && !injected_sets_ok(sets, 1 << 28, 1));
    CHECK(injected_sets_ok(sets, 1 << 14, (1 << 14) - 1) && !injected_sets_ok(sets, 1 << 14, 1 << 14) && injected_sets_ok(sets, (1 << 14) + 1, (1 << 14) - 1));      // 2^28 - 2^14, 2^28, 2^28 - 1
    CHECK(injected_sets_ok(nullptr, 1, 1 << 28) && injected_sets_ok(nullptr, 1 << 28, 1) && injected_sets_ok(nullptr, INT32_MAX, INT32_MAX) && injected_sets_ok(nullptr, 1, (1 << 28) - 1));
    CHECK(!injected_sets_ok(sets, INT32_MAX, INT32_MAX) && injected_sets_ok(sets, 0, INT32_MAX));      // no wrap in 64 bits
    printf("ransac rules ok\n");
    return 0;
}

static bool took(size_t from, std::initializer_list<const char*> names) {
    const std::vector<std::string>& L = hip_stub::log();
    if (L.size() - from != names.size()) return false;
    size_t k = from;
    for (const char* n : names) if (L[k++].rfind(n, 0) != 0) return false;
    return true;
}

static int check_stream_ordered_buf() {
    std::vector<std::string>& L = hip_stub::log();
    hipStream_t s1 = (hipStream_t)0x100, s2 = (hipStream_t)0x200;
    StreamOrderedBuf b;
    size_t at = L.size();
    CHECK(b.acquire(s1, 1000) == SSLAM_OK && took(at, {"hipEventCreate", "hipMalloc"}) && b.buf.cap >= 1000);      // first use: nothing to wait for
    memset(b.as<uint8_t>(), 1, 1000);
    at = L.size(); CHECK(b.mark(s1) == SSLAM_OK && took(at, {"hipEventRecord"}) && b.lastStream == (void*)s1);
    at = L.size(); CHECK(b.acquire(s1, 500) == SSLAM_OK && took(at, {}));                                           // same stream, fits: stream order is enough
    void* before = b.buf.p;
    at = L.size(); CHECK(b.acquire(s2, b.buf.cap) == SSLAM_OK && took(at, {"hipStreamWaitEvent"}) && b.buf.p == before);      // another stream: wait on the device
    CHECK(L.back().find("0x200") != std::string::npos);
    at = L.size(); CHECK(b.mark(s2) == SSLAM_OK && b.lastStream == (void*)s2);
    const size_t big = b.buf.cap + 1;
    at = L.size(); CHECK(b.acquire(s2, big) == SSLAM_OK && took(at, {"hipEventSynchronize", "hipFree", "hipMalloc"}) && b.buf.cap >= big);      // growing frees: host wait first, same stream or not
    memset(b.as<uint8_t>(), 2, big);
    at = L.size(); CHECK(b.acquire(s1, 2 * big) == SSLAM_OK && took(at, {"hipEventSynchronize", "hipFree", "hipMalloc"}));
    CHECK(b.mark(s1) == SSLAM_OK);
    hip_stub::malloc_limit() = 1 << 20;
    at = L.size(); CHECK(b.acquire(s1, (size_t)2 << 20) == SSLAM_ERR_HIP && took(at, {"hipEventSynchronize", "hipFree", "hipMalloc"}) && b.buf.p == nullptr && b.buf.cap == 0);
    CHECK(b.acquire(s1, 100) == SSLAM_OK);                                                                           // usable again after a failed growth
    at = L.size(); b.release(); CHECK(took(at, {"hipEventSynchronize", "hipEventDestroy", "hipFree"}) && !b.done && !b.buf.p && !b.lastStream);
    at = L.size(); b.release(); CHECK(took(at, {}));                                                                 // idempotent
    StreamOrderedBuf never;                                                                                         // a context that never made the call
    at = L.size(); never.release(); CHECK(took(at, {}));
    printf("StreamOrderedBuf ok\n");
    return 0;
}

// what rank r sends in a round: lengths that differ and are no multiple of anything; the last rank of several never has bytes, the root has none in round 2
static uint64_t exchange_len(int G, int r, int round) { return (G > 1 && r == G - 1) || (r == 0 && round == 2) ? 0 : 13 + 37 * (uint64_t)r + 101 * (uint64_t)round + (r == 1 ? 4099 : 0); }

// one rank's side of three rounds: the two-word all-gather of (length, root's capacity) as sslam_group_gather_dev makes it, then gather_to_root.  Returns the line that failed, 0 when none did.
static int exchange_rank(Rccl* R, ncclComm_t comm, int G, int r, bool selfRccl) {
    hipStream_t st = (hipStream_t)(uintptr_t)(0x1000 + r);
    for (int round = 0; round < 3; ++round) {
        const uint64_t mine = exchange_len(G, r, round);
        uint64_t total = 0;
        for (int q = 0; q < G; ++q) total += exchange_len(G, q, round);
        std::unique_ptr<uint64_t[]> pair(new uint64_t[2]{mine, r == 0 ? total : 0}), all(new uint64_t[2 * (size_t)G]);
        if (R->AllGather(pair.get(), all.get(), 2, kNcclUint64, comm, st) != 0) return __LINE__;
        std::unique_ptr<uint64_t[]> bytes(new uint64_t[G]);
        for (int q = 0; q < G; ++q) { bytes[q] = all[2 * q]; if (bytes[q] != exchange_len(G, q, round) || all[2 * q + 1] != (q == 0 ? total : 0)) return __LINE__; }
        std::unique_ptr<uint8_t[]> send(new uint8_t[mine]), recv(r == 0 ? new uint8_t[total] : nullptr);
        memset(send.get(), r + 1, mine);
        if (r == 0) memset(recv.get(), 0xEE, total);
        const GatherStatus x = gather_to_root(R, comm, r, G, bytes.get(), send.get(), recv.get(), selfRccl, st);
        if (x.rccl != 0 || !x.started || x.hip != hipSuccess) return __LINE__;
        if (r == 0) {                                   // the streams back to back in rank order (a write past the total ends the run: the block is exactly that long)
            uint64_t at = 0;
            for (int q = 0; q < G; ++q) for (uint64_t i = 0; i < bytes[q]; ++i) if (recv[at++] != q + 1) return __LINE__;
            if (at != total) return __LINE__;
        }
    }
    return 0;
}

static int check_exchange() {
    Rccl* R = rccl_fake();
    for (int G : {1, 2, 3, 5, 8}) for (int selfRccl = 0; selfRccl < 2; ++selfRccl) for (int form = 0; form < 2; ++form) {
        std::vector<ncclComm_t> comms(G, nullptr);
        std::vector<int> failed(G, 0);
        NcclUid id;
        if (form == 0) CHECK(R->CommInitAll(comms.data(), G, nullptr) == 0);      // one process driving G devices
        else CHECK(R->GetUniqueId(&id) == 0);                                     // one process per GPU: every rank joins with the shared id, from its own thread
        std::vector<std::thread> th;
        for (int r = 0; r < G; ++r) th.emplace_back([&, r] {
            if (form == 1 && R->CommInitRank(&comms[r], G, id, r) != 0) { failed[r] = __LINE__; return; }
            failed[r] = exchange_rank(R, comms[r], G, r, selfRccl != 0);
        });
        for (auto& t : th) t.join();
        for (int r = 0; r < G; ++r) {
            if (failed[r]) printf("exchange: G %d, own bytes through the table %d, form %d: rank %d failed at line %d\n", G, selfRccl, form, r, failed[r]);
            CHECK(failed[r] == 0);
        }
        for (ncclComm_t c : comms) CHECK(R->CommDestroy(c) == 0);
        CHECK(gFakeWorlds.empty());                                                // (a world that is not freed is a leak, which ends the run as well)
    }
    CHECK(gStandinRequested.load() == 0 && tFakeDepth == 0 && tFakeOps.empty());
    printf("exchange ok\n");
    return 0;
}

int main() {
    if (check_csr_cases() || check_argument_rules() || check_ransac_rules() || check_stream_ordered_buf() || check_exchange()) return 1;
    printf("ok\n");
    return 0;
}
