// metasnv_amd/csrc/hiptry.h -- HIP_TRY, once: a failed runtime call ends the calling function with MSNV_EHIP and the call's own text.
// For the files hipcc compiles (it brings the runtime's header in); the g++-compiled host files never see the runtime.
#pragma once

#include <hip/hip_runtime_api.h>

#include "msnv_internal.h"

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return ::msnv::fail(MSNV_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
