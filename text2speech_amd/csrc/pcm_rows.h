// What the table-addressed PCM kernels (resample.hip, trim.hip, loudness.hip, limiter.hip) share: the clamps that keep a row's
// (src_start, src_count, dst_start, dst_cap) inside the buffers whatever the table holds, all in 64-bit, and the rounding to int16.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

// the samples of a row that lie inside [0, src_len), at most max_count of them
static __device__ __forceinline__ long pcm_src_count(long s0, long n, long src_len, long max_count = LONG_MAX) {
    if (n < 0 || s0 < 0 || s0 >= src_len) return 0;
    if (n > src_len - s0) n = src_len - s0;
    return n > max_count ? max_count : n;
}

// the outputs of a row that may be written: at most max_out, inside [d0, d0 + cap) and inside [0, dst_len)
static __device__ __forceinline__ long pcm_dst_cap(long cap, long max_out, long d0, long dst_len) {
    if (cap > max_out) cap = max_out;
    if (cap < 0 || d0 < 0 || d0 >= dst_len) return 0;
    return cap > dst_len - d0 ? dst_len - d0 : cap;
}

static __device__ __forceinline__ short pcm_round16(double v) {
    const double q = rint(v);                                   // ties to even
    if (q >= 32767.0) return 32767;
    if (q <= -32768.0) return -32768;
    return q == q ? (short)(int)q : (short)0;                   // NaN: 0
}
