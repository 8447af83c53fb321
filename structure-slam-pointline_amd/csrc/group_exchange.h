// The payload exchange of the multi-GPU path, host only: the RCCL entry points as a table (bound at run time by group.hip, or the in-process
// stand-in of rccl_standin.h) and the one grouped send / receive that takes every rank's record stream to the root.  Both group forms call it
// (sslam_group_gather_dev, the workers of sslam_frontend_batch_sharded); tests/sim/host_checks.cpp runs it without a GPU.
#pragma once
#include "common.h"
namespace sslam {

typedef struct ncclComm* ncclComm_t;
struct NcclUid { char internal[128]; };
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(NcclUid*) = nullptr;
    int (*CommInitRank)(ncclComm_t*, int, NcclUid, int) = nullptr;
    int (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclUint8 = 1, kNcclUint64 = 5;      // ncclDataType_t (rccl.h)

static inline const char* rccl_error_text(const Rccl* R, int status) { return R && R->GetErrorString ? R->GetErrorString(status) : "rccl error"; }
// the root's own stream through ncclSend / ncclRecv instead of a device-to-device copy (RCCL moves bytes on a one-GPU box); set and cleared between calls
static inline bool root_sends_to_itself() { return getenv("SSLAM_GROUP_SELF_SENDRECV") != nullptr; }
// the first nonzero RCCL status, whether GroupStart succeeded (the status is then a send's, a receive's or GroupEnd's), the root's own copy
struct GatherStatus { int rccl = 0; bool started = false; hipError_t hip = hipSuccess; };

// Rank r's bytes[r] bytes at d_send go to the root's d_recv (root only) at the sum of the lengths before r: one grouped receive per rank that has
// bytes and the root's own send (with selfRccl; a copy behind the group otherwise), elsewhere one send.  Once GroupStart has succeeded GroupEnd is
// reached whatever a send or receive returned (nothing more is posted after the first failure): a rank that left in between would leave its peers
// blocked in their half.  Enqueues on `st` and returns: no synchronisation, no error text -- the callers do both.
static inline GatherStatus gather_to_root(const Rccl* R, ncclComm_t comm, int rank, int nranks, const uint64_t* bytes, const void* d_send, void* d_recv,
                                          bool selfRccl, hipStream_t st) {
    GatherStatus s;
    if ((s.started = (s.rccl = R->GroupStart()) == 0)) {
        if (rank == 0) {
            uint64_t off = 0;
            for (int r = 0; r < nranks; ++r) {
                if (bytes[r] && (r != 0 || selfRccl) && !s.rccl) s.rccl = R->Recv((uint8_t*)d_recv + off, (size_t)bytes[r], kNcclUint8, r, comm, st);
                off += bytes[r];
            }
            if (selfRccl && bytes[0] && !s.rccl) s.rccl = R->Send(d_send, (size_t)bytes[0], kNcclUint8, 0, comm, st);
        } else if (bytes[rank]) s.rccl = R->Send(d_send, (size_t)bytes[rank], kNcclUint8, 0, comm, st);
        const int end = R->GroupEnd();
        if (!s.rccl) s.rccl = end;
    }
    if (rank == 0 && !selfRccl && bytes[0]) s.hip = hipMemcpyAsync(d_recv, d_send, (size_t)bytes[0], hipMemcpyDeviceToDevice, st);
    return s;
}
}  // namespace sslam
