// extern "C" boundary of the biquad-cascade filter (sosfilt.hip): rows by table and the windows of a stream.
#include "../../include/t2s_hip.h"
#include "t2s_api_common.h"
#include "sosfilt.h"

#include <string.h>

static inline bool sos_al8(const void* p) { return aligned_to(p, 8); }
static inline bool sos_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

int t2s_sos_tile(void) { return T2S_SOS_TILE; }
int t2s_sos_segment(void) { return T2S_SOS_SEGMENT; }
int t2s_sos_max_sections(void) { return T2S_SOS_MAX_SECTIONS; }
int t2s_sos_table_doubles(void) { return T2S_SOS_TAB_DOUBLES; }

long t2s_sos_scratch(int n_rows, long max_count, int n_sections) {
    if (n_rows <= 0 || n_rows > 65535 || max_count <= 0 || max_count > 0x7fffffffL || n_sections < 1 || n_sections > T2S_SOS_MAX_SECTIONS)
        return -1;
    return (long)n_rows * ((max_count + T2S_SOS_TILE - 1) / T2S_SOS_TILE) * 2 * n_sections;
}

int t2s_sos_filter(const void* src, int src_kind, long src_len, const long* table, int n_rows, long max_count, const double* gains,
                   const double* tab, int n_sections, double* scratch, long scratch_len, void* dst, int dst_kind, long dst_len,
                   long max_out, int* counts, void* stream) {
    if (!src || !table || !tab || !scratch || !dst || !counts || !sos_al8(table) || !sos_al8(gains) || !sos_al8(tab) || !sos_al8(scratch) ||
        !aligned_to(counts, 4) || src_kind < 0 || src_kind > 2 || dst_kind < 0 || dst_kind > 1 || (src_kind != 0 && dst_kind != 1) ||
        src_len <= 0 || dst_len <= 0 || n_rows <= 0 || n_rows > 65535 || max_count <= 0 || max_count > 0x7fffffffL || max_out <= 0 ||
        max_out > (1L << 40) || n_sections < 1 || n_sections > T2S_SOS_MAX_SECTIONS ||
        scratch_len < t2s_sos_scratch(n_rows, max_count, n_sections))
        return T2S_EINVAL;
    const size_t src_el = src_kind == 1 ? 4 : 2, dst_el = dst_kind == 1 ? 4 : 2;
    if (!aligned_to(src, (unsigned)src_el) || !aligned_to(dst, (unsigned)dst_el) ||
        sos_overlap(src, (size_t)src_len * src_el, dst, (size_t)dst_len * dst_el))            // never in place
        return T2S_EINVAL;
    SosArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.n_rows = n_rows; a.n_sections = n_sections; a.max_count = max_count;
    a.tiles = (max_count + T2S_SOS_TILE - 1) / T2S_SOS_TILE; a.gains = gains; a.tab = tab; a.scratch = scratch;
    a.dst = dst; a.dst_len = dst_len; a.max_out = max_out; a.counts = counts;
    T2S_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * 2 * (size_t)n_rows, (hipStream_t)stream));
    T2S_CHECK_HIP(t2s_launch_sos_filter(a, src_kind, dst_kind, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_sos_window_carry(int n_sections) {
    if (n_sections < 1 || n_sections > T2S_SOS_MAX_SECTIONS) return -1;
    return 16 * n_sections + 4 * T2S_SOS_TILE;
}

int t2s_sos_window(const void* carry_in, void* carry_out, const void* piece, int is_half, int B, long n, long ldp, long N0,
                   const double* gains, const double* tab, int n_sections, double* scratch, long scratch_len, float* out, long ldo,
                   int* counts, void* stream) {
    if (!carry_in || !carry_out || !tab || !scratch || !counts || !sos_al8(carry_in) || !sos_al8(carry_out) || !sos_al8(gains) ||
        !sos_al8(tab) || !sos_al8(scratch) || !aligned_to(counts, 4) || (is_half != 0 && is_half != 1) || B <= 0 || B > 65535 || n < 0 ||
        n > 0x7fffffffL - T2S_SOS_TILE || N0 < 0 || N0 > (1L << 40) || n_sections < 1 || n_sections > T2S_SOS_MAX_SECTIONS ||
        (n > 0 && (!piece || !out || ldp < n || ldo < n || !aligned_to(piece, is_half ? 2 : 4) || !aligned_to(out, 4))))
        return T2S_EINVAL;
    const long head = N0 % T2S_SOS_TILE, L = head + n;
    const size_t bytes = (size_t)t2s_sos_window_carry(n_sections);
    if (sos_overlap(carry_in, bytes * B, carry_out, bytes * B)) return T2S_EINVAL;            // ping-pong
    if (n == 0) {                                               // nothing arrives: the carry passes on as it is
        T2S_CHECK_HIP(hipMemcpyAsync(carry_out, carry_in, bytes * B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return T2S_OK;
    }
    if (scratch_len < t2s_sos_scratch(B, L, n_sections)) return T2S_EINVAL;
    SosArgs a;
    memset(&a, 0, sizeof(a));
    a.src = piece; a.n_rows = B; a.n_sections = n_sections; a.max_count = L; a.tiles = (L + T2S_SOS_TILE - 1) / T2S_SOS_TILE;
    a.gains = gains; a.tab = tab; a.scratch = scratch; a.dst = out; a.counts = counts;
    a.carry_in = (const char*)carry_in; a.carry_out = (char*)carry_out; a.carry_bytes = (long)bytes; a.head = head; a.ldp = ldp; a.ldo = ldo;
    T2S_CHECK_HIP(t2s_launch_sos_window(a, is_half, (hipStream_t)stream));
    return T2S_OK;
}
