// lbm_hip_try.h — the error check of every HIP call that lbm_kernels.hip (lbm_p2p_impl.h with it), lbm_f64.hip, lbm_rows64.hip and
// lbm_rccl.cpp make.  Host side only; not part of the ABI.
//
// A failed HIP call leaves "<the call as written>: <HIP's words>" in lbm_last_error() and takes the exit `on_fail` (HIP_TRY: return 1).
// (Both stringify their own argument: passed on through another macro, constants that are macros themselves would be spelled out.)
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "lbm_internal.h"

// (A failed call stays the thread's last HIP error until it is read.  It is read here: otherwise the next hipGetLastError() after a
// launch — of another object of this thread, perhaps much later — would report this failure as its own.)
inline bool hip_failed(hipError_t e, const char* call)
{
  if (e != hipSuccess) {
    lbm_internal::set_error(std::string(call) + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
  }
  return e != hipSuccess;
}
#define HIP_TRY_OR(expr, on_fail) do { if (hip_failed((expr), #expr)) { on_fail; } } while (0)
#define HIP_TRY(expr) do { if (hip_failed((expr), #expr)) return 1; } while (0)
