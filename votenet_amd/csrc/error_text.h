// error_text.h -- the error text behind a library's *_last_error() (host only).  Every library of this project keeps its own: it holds
// one `static thread_local ErrorText` object, so a failure in one library never changes what another's *_last_error() returns.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include "../../include/votenet_hip.h" // the status codes VOTENET_OK, VOTENET_E_*

namespace votenet {

struct ErrorText {
    char text[512];

    int vset(int code, const char *fmt, va_list ap)
    {
        vsnprintf(text, sizeof(text), fmt, ap);
        return code;
    }
    int set(int code, const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vset(code, fmt, ap);
        va_end(ap);
        return code;
    }
    int check(hipError_t e, const char *what)
    {
        if (e != hipSuccess) return set(VOTENET_E_HIP, "%s: %s", what, hipGetErrorString(e));
        return VOTENET_OK;
    }
    int check_launch(const char *what) { return check(hipGetLastError(), what); }
};

// `return` the library's status 1 with a text when an argument check fails
#define VN_REQUIRE_IN(err, cond, ...)                                             \
    do {                                                                          \
        if (!(cond)) return (err).set(VOTENET_E_INVALID_ARGUMENT, __VA_ARGS__);   \
    } while (0)

} // namespace votenet
