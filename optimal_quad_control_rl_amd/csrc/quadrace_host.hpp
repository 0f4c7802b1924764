// quadrace_host.hpp -- the host support every entry point of the C ABI shares: the error string behind qr_last_error(), the check of a
// HIP call, the test for a stream under capture.  Host code only and nothing with device code behind it (quadrace_ppo_f32.hip includes it
// without quadrace_device.hpp); quadrace_launch.hpp includes it for everyone else.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/quadrace.h"

namespace qr {

// records `msg` for qr_last_error() of the calling thread and returns `code` (defined in quadrace_abi.hip)
int set_last_error(int code, const std::string& msg);

// is the caller capturing `st` into a graph?  (the NULL stream cannot be captured; a failed query counts as "no")
inline bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return st != nullptr && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

}  // namespace qr

// a HIP call that must succeed: on failure the enclosing entry point returns QR_E_HIP with "<the call's text>: <hipGetErrorString>"
#define QR_HIP(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            return qr::set_last_error(QR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
    } while (0)
