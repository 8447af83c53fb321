// The argument check of the CSR lists that matcher entry points take (match.hip): vocabulary nodes, observation sets, children.  Host code and no
// HIP in here: tests/sim/host_checks.cpp compiles it with a plain host compiler under the sanitizers and supplies its own set_error.
#pragma once
#include <cstdint>
#include "../../include/sslam_frontend.h"

namespace sslam {

// List r owns idx[ptr[r] .. ptr[r + 1]).  Well formed: ptr[0] == 0 and non-decreasing offsets -- so the total ptr[nnodes] is >= 0 and no list
// reaches past it: a call sizes its arena by the total -- and 0 <= idx[i] < limit (idx == nullptr: the offsets alone).  Anything else is
// SSLAM_ERR_INVALID with the error text "<fn>: <what> ...", before the call stages or launches anything.
void set_error(const char* fmt, ...);      // ctx.hip
inline int check_csr(const char* fn, const char* what, const int32_t* ptr, int nnodes, const int32_t* idx, int limit) {
    bool ok = ptr[0] == 0;
    for (int r = 0; r < nnodes && ok; ++r) ok = ptr[r + 1] >= ptr[r];
    if (!ok) { set_error("%s: %s offsets must start at 0 and be non-decreasing", fn, what); return SSLAM_ERR_INVALID; }
    if (idx) for (int i = 0; i < ptr[nnodes]; ++i) if (idx[i] < 0 || idx[i] >= limit) { set_error("%s: %s index out of range", fn, what); return SSLAM_ERR_INVALID; }
    return SSLAM_OK;
}

}  // namespace sslam
