// extern "C" boundary of the control inside a stream: stream_ctl.hip's four kernels (include/t2s_hip.h states what they compute).
#include "../../include/t2s_hip.h"
#include "t2s_api_common.h"
#include "stream_ctl_ops.h"

#include <string.h>

#define SC_Q (1L << T2S_WARP_Q_BITS)

static bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }
static bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }
// a push over the frames [n0, n) of buffers that hold N_cap frames
static bool window_ok(int N_cap, int n0, int n) { return N_cap > 0 && N_cap <= (1 << 30) && n0 >= 0 && n >= n0 && n <= N_cap; }

extern "C" {

int t2s_align_window_state(void) { return (int)sizeof(AlignWindowState); }

int t2s_align_window(const void* A, int src_kind, int B, int N_cap, int T_in, int n0, int n, int last, long ld_row, long ld_entry,
                     const int* in_len, int max_frames, int skip_max, int back_max, int stall_max, int end_slack, double min_focus,
                     int* pos, float* peak, unsigned char* bad, void* state, int* stats, double* focus, int* dur, int* flags,
                     void* stream) {
    if (!pos || !peak || !bad || !state || !stats || !focus || !dur || !flags || (src_kind != 1 && src_kind != 2) || !al4(in_len) ||
        !al4(pos) || !al4(peak) || !al8(state) || !al4(stats) || !al8(focus) || !al4(dur) || !al4(flags) || B < 1 || T_in < 1 ||
        !window_ok(N_cap, n0, n) || (long)B * N_cap > 0x7fffffffL || (last != 0 && last != 1))
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

int t2s_warp_window_map(int B, int N_cap, int n0, int n, long stretch, const long* stretches, const int* path, long ld_path,
                        const int* in_len, int T_in, long* cum, int* first_last, void* stream) {
    if (!cum || !al8(cum) || !al8(stretches) || !al4(path) || !al4(in_len) || !al4(first_last) || B < 1 || B > 65535 || T_in < 0 ||
        (long)B * T_in > 0x7fffffffL || !window_ok(N_cap, n0, n))
        return T2S_EINVAL;
    if (first_last && !path) return T2S_EINVAL;
    if (path && (T_in < 1 || ld_path < n)) return T2S_EINVAL;
    if (!stretches && (stretch < (SC_Q >> 3) || stretch > (SC_Q << 3))) return T2S_EINVAL;
    WarpWindowMapArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.N_cap = N_cap; a.T_in = T_in; a.n0 = n0; a.n = n; a.stretch = stretch; a.stretches = stretches; a.path = path;
    a.ld_path = ld_path; a.in_len = in_len; a.cum = cum; a.first_last = first_last;
    T2S_CHECK_HIP(t2s_launch_warp_window_map(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_warp_window_gather(const void* x, int src_kind, int B, int C, int N_cap, int n, long ld_row, long ld_entry, const long* cum,
                           long j0, long j1, void* out, void* stream) {
    if (!cum || !al8(cum) || (src_kind != 1 && src_kind != 2) || B < 1 || B > 65535 || C < 1 || C > 65535 * T2S_WARP_CH ||
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
