// host_rt.h — error plumbing of the host-side runtimes (engine*.hip, f32_*.hip).  `e` is a handle with a std::string `err`; each
// macro returns from the enclosing int function: 1 after writing the message, or the failing callee's code.
#pragma once
#include <cstdio>
#include <hip/hip_runtime.h>

#define DM_FAIL(e, ...) do { char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__); (e)->err = _b; return 1; } while (0)
#define DM_HIP(e, call) do { hipError_t _r = (call); if (_r != hipSuccess) { \
    char _b[512]; snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #call, hipGetErrorString(_r), __FILE__, __LINE__); \
    (e)->err = _b; return 1; } } while (0)
#define DM_TRY(x) do { int _rc = (x); if (_rc) return _rc; } while (0)
