// Host only; included by ONE translation unit per binary: group.hip under SSLAM_TESTING (libsslam_frontend_testing.so), tests/sim/host_checks.cpp
#pragma once
#include "group_exchange.h"
#include <atomic>
#include <chrono>
#include <condition_variable>
namespace sslam { namespace {
// ------------------------------------------------------------------ sslam_testing_use_rccl_standin(1) (include/sslam_testing.h): an in-process stand-in for the RCCL entry points
// N > 1 has never run on hardware here (one GPU per box), so the group code's multi-member paths -- a host thread per device, uneven tails,
// the collective error agreement, grouped send / receive to the root -- had no execution at all.  With this table selected at group creation
// the "devices" of a group are contexts (streams) of whatever GPUs are visible, dealt round-robin, and the collectives are host-mediated
// device-to-device copies with NCCL's matching rules: a send to p pairs with p's receive from the sender in posting order, calls between
// GroupStart / GroupEnd are issued together, an all-gather is a rendezvous of all ranks.  Same process only (ranks are threads).  It moves
// real bytes between real device buffers through the same code paths; it says nothing about xGMI -- the scaling run stays the driver's.
struct FakeWorld {
    int nranks = 0, refs = 0;
    std::mutex mu; std::condition_variable cv;
    struct Msg { unsigned long id; int src, dst; const void* ptr; size_t bytes; bool taken; };
    std::vector<Msg> box;                           // posted sends, in posting order (entries are named by id: the vector shifts when a sender clears its own)
    unsigned long nextId = 1;
    std::vector<const void*> agPtr; int agArrived = 0, agLeft = 0, agGen = 0;
};
struct FakeComm { FakeWorld* w; int rank; };
struct FakeOp { int kind; const void* sptr; void* rptr; size_t bytes; int peer; FakeComm* c; hipStream_t st; unsigned long id; };      // 0 send, 1 recv
// every wait of the stand-in is bounded: a protocol error of the group code must fail a test, not hang the suite
constexpr std::chrono::seconds kFakeWait(60);
thread_local int tFakeDepth = 0;
thread_local std::vector<FakeOp> tFakeOps;
std::mutex gFakeMu;
std::vector<std::pair<NcclUid, FakeWorld*>> gFakeWorlds;      // worlds being assembled by ncclCommInitRank, keyed by unique id
int gFakeIdCounter = 0;

size_t fake_dtype_bytes(int dt) { return dt == kNcclUint64 ? 8 : 1; }
int fake_flush_ops(std::vector<FakeOp>& ops);
int fake_flush() {
    std::vector<FakeOp> ops; ops.swap(tFakeOps);
    const int rc = fake_flush_ops(ops);
    if (rc != 0)      // an error leaves nothing behind: the rank's own posted sends (device pointers that may die with the caller's buffers) are withdrawn, or a later receive could match them
        for (FakeOp& o : ops) if (o.kind == 0 && o.id) {
            std::lock_guard<std::mutex> lk(o.c->w->mu);
            for (size_t i = 0; i < o.c->w->box.size(); ++i) if (o.c->w->box[i].id == o.id) { o.c->w->box.erase(o.c->w->box.begin() + i); break; }
            o.c->w->cv.notify_all();
        }
    return rc;
}
int fake_flush_ops(std::vector<FakeOp>& ops) {
    // sends first: publish (the data must be final: drain the sender's stream), then receives (wait for the partner's publication, copy,
    // acknowledge), then wait until every own send was taken -- a rank that posts both directions in one group cannot block itself
    for (FakeOp& o : ops) if (o.kind == 0) {
        if (hipStreamSynchronize(o.st) != hipSuccess) return 1;
        std::lock_guard<std::mutex> lk(o.c->w->mu);
        o.id = o.c->w->nextId++;
        o.c->w->box.push_back({o.id, o.c->rank, o.peer, o.sptr, o.bytes, false});
        o.c->w->cv.notify_all();
    }
    auto find = [](FakeWorld* w, unsigned long id) -> FakeWorld::Msg* { for (auto& m : w->box) if (m.id == id) return &m; return nullptr; };
    for (FakeOp& o : ops) if (o.kind == 1) {
        FakeWorld* w = o.c->w; const void* src = nullptr; unsigned long id = 0; size_t bytes = 0;
        {
            std::unique_lock<std::mutex> lk(w->mu);
            // the oldest untaken send of that peer to this rank (receives of one rank are issued by one thread, one after the other)
            if (!w->cv.wait_for(lk, kFakeWait, [&] { for (auto& m : w->box) if (!m.taken && m.src == o.peer && m.dst == o.c->rank) { id = m.id; return true; } return false; })) return 4;
            FakeWorld::Msg* m = find(w, id);
            src = m->ptr; bytes = m->bytes;
        }
        if (bytes != o.bytes) return 2;               // NCCL would hang or corrupt on mismatched sizes: here it is an error
        // stream-ordered on the receiver's stream like the real receive, then drained: the sender may reuse its buffer once this returns
        if (o.bytes && hipMemcpyAsync(o.rptr, src, o.bytes, hipMemcpyDeviceToDevice, o.st) != hipSuccess) return 1;
        if (hipStreamSynchronize(o.st) != hipSuccess) return 1;
        std::lock_guard<std::mutex> lk(w->mu);
        if (FakeWorld::Msg* m = find(w, id)) m->taken = true;
        w->cv.notify_all();
    }
    for (FakeOp& o : ops) if (o.kind == 0) {
        FakeWorld* w = o.c->w;
        std::unique_lock<std::mutex> lk(w->mu);
        if (!w->cv.wait_for(lk, kFakeWait, [&] { FakeWorld::Msg* m = find(w, o.id); return !m || m->taken; })) return 4;
        for (size_t i = 0; i < w->box.size(); ++i) if (w->box[i].id == o.id) { w->box.erase(w->box.begin() + i); break; }
    }
    return 0;
}
int fakeGetUniqueId(NcclUid* u) { std::lock_guard<std::mutex> lk(gFakeMu); memset(u, 0, sizeof(*u)); snprintf(u->internal, sizeof(u->internal), "sslam-fake-rccl-%d", ++gFakeIdCounter); return 0; }
int fakeCommInitAll(ncclComm_t* comms, int n, const int*) {
    FakeWorld* w = new FakeWorld(); w->nranks = n; w->refs = n; w->agPtr.assign(n, nullptr);
    for (int r = 0; r < n; ++r) comms[r] = (ncclComm_t) new FakeComm{w, r};
    return 0;
}
int fakeCommInitRank(ncclComm_t* comm, int n, NcclUid id, int rank) {
    std::lock_guard<std::mutex> lk(gFakeMu);
    FakeWorld* w = nullptr;
    for (auto& e : gFakeWorlds) if (memcmp(e.first.internal, id.internal, sizeof(id.internal)) == 0) w = e.second;
    if (!w) { w = new FakeWorld(); w->nranks = n; w->agPtr.assign(n, nullptr); gFakeWorlds.push_back({id, w}); }
    if (w->nranks != n || rank < 0 || rank >= n) return 3;
    ++w->refs;
    *comm = (ncclComm_t) new FakeComm{w, rank};
    return 0;
}
int fakeCommDestroy(ncclComm_t c_) {
    FakeComm* c = (FakeComm*)c_; if (!c) return 0;
    std::lock_guard<std::mutex> lk(gFakeMu);
    if (--c->w->refs == 0) {
        for (size_t i = 0; i < gFakeWorlds.size(); ++i) if (gFakeWorlds[i].second == c->w) { gFakeWorlds.erase(gFakeWorlds.begin() + i); break; }
        delete c->w;
    }
    delete c; return 0;
}
int fakeGroupStart() { ++tFakeDepth; return 0; }
int fakeGroupEnd() { if (--tFakeDepth > 0) return 0; tFakeDepth = 0; return fake_flush(); }
int fakeSend(const void* p, size_t count, int dt, int peer, ncclComm_t c, hipStream_t st) {
    tFakeOps.push_back({0, p, nullptr, count * fake_dtype_bytes(dt), peer, (FakeComm*)c, st, 0});
    return tFakeDepth ? 0 : fake_flush();
}
int fakeRecv(void* p, size_t count, int dt, int peer, ncclComm_t c, hipStream_t st) {
    tFakeOps.push_back({1, nullptr, p, count * fake_dtype_bytes(dt), peer, (FakeComm*)c, st, 0});
    return tFakeDepth ? 0 : fake_flush();
}
int fakeAllGather(const void* sp, void* rp, size_t count, int dt, ncclComm_t c_, hipStream_t st) {
    FakeComm* c = (FakeComm*)c_; FakeWorld* w = c->w; const size_t bytes = count * fake_dtype_bytes(dt);
    if (hipStreamSynchronize(st) != hipSuccess) return 1;
    std::vector<const void*> ptrs;
    {
        std::unique_lock<std::mutex> lk(w->mu);
        if (!w->cv.wait_for(lk, kFakeWait, [&] { return w->agLeft == 0; })) return 4;              // the previous round has been left by everybody
        const int gen = w->agGen;
        w->agPtr[c->rank] = sp;
        if (++w->agArrived == w->nranks) { w->agLeft = w->nranks; w->agArrived = 0; ++w->agGen; w->cv.notify_all(); }
        else if (!w->cv.wait_for(lk, kFakeWait, [&] { return w->agGen != gen; })) return 4;
        ptrs = w->agPtr;
    }
    int rc = 0;
    for (int r = 0; r < w->nranks && !rc; ++r) if (bytes && hipMemcpyAsync((char*)rp + (size_t)r * bytes, ptrs[r], bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = 1;
    if (hipStreamSynchronize(st) != hipSuccess) rc = 1;
    std::unique_lock<std::mutex> lk(w->mu);
    if (--w->agLeft == 0) w->cv.notify_all();
    if (!w->cv.wait_for(lk, kFakeWait, [&] { return w->agLeft == 0; })) return 4;                  // nobody's send buffer is reused before everybody has copied it
    return rc;
}
const char* fakeGetErrorString(int e) { return e == 4 ? "fake rccl: a peer did not show up within 60 s" : e == 2 ? "fake rccl: send / receive sizes differ" : e == 3 ? "fake rccl: inconsistent communicator arguments" : "fake rccl: HIP error"; }
Rccl* rccl_fake() {
    static Rccl F;
    static std::once_flag once;
    std::call_once(once, [] {
        F.h = (void*)&F; F.GetUniqueId = fakeGetUniqueId; F.CommInitRank = fakeCommInitRank; F.CommInitAll = fakeCommInitAll; F.CommDestroy = fakeCommDestroy;
        F.GroupStart = fakeGroupStart; F.GroupEnd = fakeGroupEnd; F.Send = fakeSend; F.Recv = fakeRecv; F.AllGather = fakeAllGather; F.GetErrorString = fakeGetErrorString;
    });
    return &F;
}
// selected by a TEST entry point only (sslam_testing_use_rccl_standin, include/sslam_testing.h) -- no environment variable changes which library a product group binds
std::atomic<int> gStandinRequested{0};
} }  // namespace sslam::
