// ORACLE — TEST INFRASTRUCTURE ONLY.  C API of the CPU restatement, loaded via
// ctypes by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg only.
// The product (structure-slam-pointline_amd/) never includes or links this.
#pragma once
#include <cstdint>
#include <cstddef>

// The LSD prologue as the detector leaves it for region growing, and its per-gradient expressions over the whole gradient range (lsd_oracle.cpp says what each array holds)
extern "C" int orc_lsd_prologue(const uint8_t* gray, int w, int h, size_t stride, int32_t* size_out, float* deg_out, int32_t* s_out, float* cs_out, int32_t* order_out,
                                int32_t* stat_out);
extern "C" int orc_lsd_grad_table(float* tab_out, int32_t* smin_out);
