// extern "C" boundary of the alignment check: align.hip's kernels, for whole rows and for the pushes of a stream (include/t2s_hip.h
// states what they compute).
#include "../../include/t2s_hip.h"
#include "t2s_api_common.h"
#include "align_ops.h"

#include <string.h>

// B entries of N frames of T_in symbols: all positive, and B N rows are numbered in an int
static bool align_shape_ok(int B, int N, int T_in) { return B > 0 && N > 0 && T_in > 0 && (long)B * N <= 0x7fffffffL; }

extern "C" {

int t2s_align_rows(const void* A, int src_kind, int B, int N, int T_in, long ld_row, long ld_entry, const int* in_len,
                   const int* out_len, int* pos, float* peak, unsigned char* bad, void* stream) {
    if (!A || !pos || !peak || !bad || (src_kind != 1 && src_kind != 2) || ((uintptr_t)A & (src_kind == 1 ? 3 : 1)) ||
        !aligned_to(in_len, 4) || !aligned_to(out_len, 4) || !aligned_to(pos, 4) || !aligned_to(peak, 4) || !align_shape_ok(B, N, T_in) ||
        ld_row < T_in || ld_entry / N < ld_row)
        return T2S_EINVAL;
    AlignRowsArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.ld_row = ld_row; a.ld_entry = ld_entry; a.B = B; a.N = N; a.T_in = T_in; a.in_len = in_len; a.out_len = out_len;
    a.pos = pos; a.peak = peak; a.bad = bad;
    T2S_CHECK_HIP(t2s_launch_align_rows(a, src_kind, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_align_stats(const int* pos, const float* peak, const unsigned char* bad, int B, int N, int T_in, const int* in_len,
                    const int* out_len, int max_frames, int skip_max, int back_max, int stall_max, int end_slack, double min_focus,
                    int* stats, double* focus, int* dur, int* flags, void* stream) {
    if (!pos || !peak || !bad || !stats || !focus || !dur || !flags || !aligned_to(pos, 4) || !aligned_to(peak, 4) ||
        !aligned_to(in_len, 4) || !aligned_to(out_len, 4) || !aligned_to(stats, 4) || !aligned_to(focus, 8) || !aligned_to(dur, 4) ||
        !aligned_to(flags, 4) || !align_shape_ok(B, N, T_in))
        return T2S_EINVAL;
    AlignStatsArgs a;
    memset(&a, 0, sizeof(a));
    a.pos = pos; a.peak = peak; a.bad = bad; a.B = B; a.N = N; a.T_in = T_in; a.in_len = in_len; a.out_len = out_len;
    a.thr.max_frames = max_frames; a.thr.skip_max = skip_max; a.thr.back_max = back_max; a.thr.stall_max = stall_max;
    a.thr.end_slack = end_slack; a.thr.min_focus = min_focus;
    a.stats = stats; a.focus = focus; a.dur = dur; a.flags = flags;
    T2S_CHECK_HIP(t2s_launch_align_stats(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_align_window_state(void) { return (int)sizeof(AlignWindowState); }

int t2s_align_window(const void* A, int src_kind, int B, int N_cap, int T_in, int n0, int n, int last, long ld_row, long ld_entry,
                     const int* in_len, int max_frames, int skip_max, int back_max, int stall_max, int end_slack, double min_focus,
                     int* pos, float* peak, unsigned char* bad, void* state, int* stats, double* focus, int* dur, int* flags,
                     void* stream) {
    if (!pos || !peak || !bad || !state || !stats || !focus || !dur || !flags || (src_kind != 1 && src_kind != 2) ||
        !aligned_to(in_len, 4) || !aligned_to(pos, 4) || !aligned_to(peak, 4) || !aligned_to(state, 8) || !aligned_to(stats, 4) ||
        !aligned_to(focus, 8) || !aligned_to(dur, 4) || !aligned_to(flags, 4) || B < 1 || T_in < 1 || !window_ok(N_cap, n0, n) ||
        (long)B * N_cap > 0x7fffffffL || (last != 0 && last != 1))
        return T2S_EINVAL;
    const int m = n - n0;
    if (m > 0 && (!A || ((uintptr_t)A & (src_kind == 1 ? 3 : 1)) || ld_row < T_in || ld_entry / m < ld_row)) return T2S_EINVAL;
    AlignWindowArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.ld_row = ld_row; a.ld_entry = ld_entry; a.B = B; a.N_cap = N_cap; a.T_in = T_in; a.n0 = n0; a.n = n; a.last = last;
    a.in_len = in_len;
    a.thr.max_frames = max_frames; a.thr.skip_max = skip_max; a.thr.back_max = back_max; a.thr.stall_max = stall_max;
    a.thr.end_slack = end_slack; a.thr.min_focus = min_focus;
    a.pos = pos; a.peak = peak; a.bad = bad; a.state = (AlignWindowState*)state; a.stats = stats; a.focus = focus; a.dur = dur;
    a.flags = flags;
    T2S_CHECK_HIP(t2s_launch_align_window(a, src_kind, (hipStream_t)stream));
    return T2S_OK;
}

}  // extern "C"
