// What every t2s_api*.hip file needs at the extern "C" boundary: the HIP error hand-off and the small argument-check helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" int t2s_internal_fail_hip(int e);   // defined in t2s_api.hip: records the HIP error text, returns T2S_EHIP

#define T2S_CHECK_HIP(expr)                                          \
    do {                                                             \
        hipError_t _e = (expr);                                      \
        if (_e != hipSuccess) return t2s_internal_fail_hip((int)_e); \
    } while (0)

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// aligned to m bytes, m a power of two (NULL is)
static inline bool aligned_to(const void* p, unsigned m) { return ((uintptr_t)p & (m - 1)) == 0; }
// a push over the frames [n0, n) of a stream whose buffers hold N_cap frames
static inline bool window_ok(int N_cap, int n0, int n) { return N_cap > 0 && N_cap <= (1 << 30) && n0 >= 0 && n >= n0 && n <= N_cap; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// a hi/lo plane pair: both present, both 16-byte aligned
static inline bool planes_ok(const void* a, const void* b) { return a && b && al16(a) && al16(b); }
