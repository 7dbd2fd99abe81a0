// extern "C" boundary of the time warp: warp.hip's kernels, for whole rows and for the pushes of a stream (include/t2s_hip.h states
// what they compute).
#include "../../include/t2s_hip.h"
#include "t2s_api_common.h"
#include "warp_ops.h"

#include <string.h>

// B entries of F frames (and T_in symbols where there is a path): positive, B a grid dimension, B T_in numbered in an int
static bool warp_shape_ok(int B, int F, int T_in) {
    return B > 0 && B <= 65535 && F > 0 && F <= (1 << 30) && T_in >= 0 && (long)B * T_in <= 0x7fffffffL;
}
static bool rate_ok(double r) { return r >= 0.125 && r <= 8.0; }     // (false for a NaN)

extern "C" {

int t2s_warp_block(void) { return T2S_WARP_BLOCK; }

int t2s_warp_map(const int* lengths, int B, int F, long stretch, const long* stretches, const int* path, long ld_path,
                 const float* rates, long ld_rates, const int* in_len, int T_in, double min_rate, double max_rate, int cap, long* cum,
                 int* out_len, int* first_last, void* stream) {
    if ((!cum && !out_len && !first_last) || !aligned_to(lengths, 4) || !aligned_to(stretches, 8) || !aligned_to(path, 4) ||
        !aligned_to(rates, 4) || !aligned_to(in_len, 4) || !aligned_to(cum, 8) || !aligned_to(out_len, 4) || !aligned_to(first_last, 4) ||
        !warp_shape_ok(B, F, T_in) || cap < 1 || !rate_ok(min_rate) || !rate_ok(max_rate) || min_rate > max_rate)
        return T2S_EINVAL;
    if ((rates || first_last) && !path) return T2S_EINVAL;
    if (path && (T_in < 1 || ld_path < F)) return T2S_EINVAL;
    if (rates && (ld_rates < T_in || stretches || stretch != T2S_WARP_Q)) return T2S_EINVAL;
    if (!rates && !stretches && (stretch < (T2S_WARP_Q >> 3) || stretch > (T2S_WARP_Q << 3))) return T2S_EINVAL;
    WarpMapArgs a;
    memset(&a, 0, sizeof(a));
    a.lengths = lengths; a.B = B; a.F = F; a.T_in = T_in; a.cap = cap; a.stretch = stretch; a.stretches = stretches; a.path = path;
    a.ld_path = ld_path; a.rates = rates; a.ld_rates = ld_rates; a.in_len = in_len; a.min_rate = min_rate; a.max_rate = max_rate;
    a.cum = cum; a.out_len = out_len; a.first_last = first_last;
    T2S_CHECK_HIP(t2s_launch_warp_map(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_warp_gather(const void* x, int src_kind, int B, int C, int F, long ld_row, long ld_entry, const int* lengths, const long* cum,
                    const int* out_len, void* out, int cap, void* stream) {
    if (!x || !cum || !out_len || !out || (src_kind != 1 && src_kind != 2) || !aligned_to(lengths, 4) || !aligned_to(cum, 8) ||
        !aligned_to(out_len, 4) || !warp_shape_ok(B, F, 0) || C < 1 || C > 65535 * T2S_WARP_CH || cap < 1 || ld_row < F ||
        ld_entry / C < ld_row)
        return T2S_EINVAL;
    const size_t el = src_kind == 1 ? 4 : 2;
    if (((uintptr_t)x | (uintptr_t)out) & (el - 1)) return T2S_EINVAL;
    const uintptr_t s0 = (uintptr_t)x, s1 = s0 + ((size_t)(B - 1) * ld_entry + (size_t)(C - 1) * ld_row + F) * el;
    const uintptr_t d0 = (uintptr_t)out, d1 = d0 + (size_t)B * C * cap * el;
    if (s0 < d1 && d0 < s1) return T2S_EINVAL;                  // never in place
    WarpGatherArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.ld_row = ld_row; a.ld_entry = ld_entry; a.B = B; a.C = C; a.F = F; a.cap = cap; a.lengths = lengths; a.cum = cum;
    a.out_len = out_len; a.out = out;
    T2S_CHECK_HIP(t2s_launch_warp_gather(a, src_kind, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_warp_spans(const long* cum, const int* first_last, int B, int F, int T_in, const int* in_len, const int* lengths, int hop,
                   const long* trim_start, const long* trim_end, const long* offsets, long up, long down, long total,
                   const long* total_dev, long* spans, void* stream) {
    if (!cum || !first_last || !spans || !aligned_to(cum, 8) || !aligned_to(first_last, 4) || !aligned_to(spans, 8) ||
        !aligned_to(in_len, 4) || !aligned_to(lengths, 4) || !aligned_to(trim_start, 8) || !aligned_to(trim_end, 8) ||
        !aligned_to(offsets, 8) || !aligned_to(total_dev, 8) || !warp_shape_ok(B, F, T_in) || T_in < 1 || hop < 1 || hop > (1 << 20) ||
        (long)F * hop > (1L << 39) || !trim_start != !trim_end || up < 1 || up > (1 << 20) || down < 1 || down > (1 << 20) || total < 0)
        return T2S_EINVAL;
    WarpSpansArgs a;
    memset(&a, 0, sizeof(a));
    a.cum = cum; a.first_last = first_last; a.B = B; a.F = F; a.T_in = T_in; a.in_len = in_len; a.lengths = lengths; a.hop = hop;
    a.trim_start = trim_start; a.trim_end = trim_end; a.offsets = offsets; a.up = up; a.down = down; a.total = total;
    a.total_dev = total_dev; a.spans = spans;
    T2S_CHECK_HIP(t2s_launch_warp_spans(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_warp_window_map(int B, int N_cap, int n0, int n, long stretch, const long* stretches, const int* path, long ld_path,
                        const int* in_len, int T_in, long* cum, int* first_last, void* stream) {
    if (!cum || !aligned_to(cum, 8) || !aligned_to(stretches, 8) || !aligned_to(path, 4) || !aligned_to(in_len, 4) ||
        !aligned_to(first_last, 4) || B < 1 || B > 65535 || T_in < 0 || (long)B * T_in > 0x7fffffffL || !window_ok(N_cap, n0, n))
        return T2S_EINVAL;
    if (first_last && !path) return T2S_EINVAL;
    if (path && (T_in < 1 || ld_path < n)) return T2S_EINVAL;
    if (!stretches && (stretch < (T2S_WARP_Q >> 3) || stretch > (T2S_WARP_Q << 3))) return T2S_EINVAL;
    WarpWindowMapArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.N_cap = N_cap; a.T_in = T_in; a.n0 = n0; a.n = n; a.stretch = stretch; a.stretches = stretches; a.path = path;
    a.ld_path = ld_path; a.in_len = in_len; a.cum = cum; a.first_last = first_last;
    T2S_CHECK_HIP(t2s_launch_warp_window_map(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_warp_window_gather(const void* x, int src_kind, int B, int C, int N_cap, int n, long ld_row, long ld_entry, const long* cum,
                           long j0, long j1, void* out, void* stream) {
    if (!cum || !aligned_to(cum, 8) || (src_kind != 1 && src_kind != 2) || B < 1 || B > 65535 || C < 1 || C > 65535 * T2S_WARP_CH ||
        !window_ok(N_cap, 0, n) || j0 < 0 || j1 < j0 || j1 > 0x7fffffffL)
        return T2S_EINVAL;
    if (j1 == j0) return T2S_OK;                                // nothing asked for: nothing launched
    if (!x || !out || n < 1 || ld_row < n || ld_entry / C < ld_row) return T2S_EINVAL;
    const size_t el = src_kind == 1 ? 4 : 2;
    if (((uintptr_t)x | (uintptr_t)out) & (el - 1)) return T2S_EINVAL;
    const uintptr_t s0 = (uintptr_t)x, s1 = s0 + ((size_t)(B - 1) * ld_entry + (size_t)(C - 1) * ld_row + n) * el;
    const uintptr_t d0 = (uintptr_t)out, d1 = d0 + (size_t)B * C * (size_t)(j1 - j0) * el;
    if (s0 < d1 && d0 < s1) return T2S_EINVAL;                  // never in place
    WarpWindowGatherArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.ld_row = ld_row; a.ld_entry = ld_entry; a.B = B; a.C = C; a.N_cap = N_cap; a.n = n; a.j0 = j0; a.j1 = j1; a.cum = cum;
    a.out = out;
    T2S_CHECK_HIP(t2s_launch_warp_window_gather(a, src_kind, (hipStream_t)stream));
    return T2S_OK;
}

}  // extern "C"
