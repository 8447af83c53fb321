// Host-only checks of two pieces of the matchers' host side, built by tests/test_host_checks_cpu.py with a plain host compiler under
// -fsanitize=address,undefined (no GPU, no HIP: tests/sim/hip_stub stands in for the runtime):
//   check_csr (csrc/match_check.h)        which CSR lists a call accepts, and that a refused list is never read past what its offsets promise
//   StreamOrderedBuf (csrc/common.h)      which runtime calls acquire / mark / release make, in which order
// Every array is a heap block of exactly its length, so a read past it ends the run.  Prints one line per check group, "ok" at the end.
#include "../../structure-slam-pointline_amd/csrc/common.h"
#include "../../structure-slam-pointline_amd/csrc/match_check.h"
#include <cstdarg>

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

int main() {
    if (check_csr_cases() || check_stream_ordered_buf()) return 1;
    printf("ok\n");
    return 0;
}
