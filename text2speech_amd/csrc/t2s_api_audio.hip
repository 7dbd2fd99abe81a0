// extern "C" boundary of the audio front-end / back-end (STFT, mel, inverse STFT, denoiser glue).
#include "../../include/t2s_hip.h"
#include "t2s_kernels.h"
#include "t2s_api_common.h"
#include "audio_ops.h"
#include "tacotron_ops.h"

#include <math.h>
#include <string.h>

// y[item][row] = sum_k W[row][k] x[item * sx + k]  per batch element, through the GEMV / matrix-core dispatcher
static hipError_t frames_gemm(const float* W, int rows, int K, const float* x, long sx, int items, float* y, long sy_item,
                              long sy_row, hipStream_t s) {
    GemvArgs g;
    memset(&g, 0, sizeof(g));
    g.W1 = W; g.ld1 = K; g.k1 = K; g.x1 = x; g.n1 = K; g.sx1 = sx;
    g.y = y; g.sy_item = sy_item; g.sy_row = sy_row; g.rows = rows; g.items = items; g.mask_scale = 1.f;
    return t2s_launch_gemv(g, s);
}

// ---- one body per stage: the plain entry point passes no lengths, its _ragged partner a padded batch's (include/t2s_hip.h) --------
// `lengths` / `frames` ([B] int32 on the device, for the kernels) and their host copy (for the checks and the item counts here) are
// both given or both NULL.  Each contraction is launched per entry with the entry's own item count: the dispatcher behind
// frames_gemm chooses GEMV or matrix cores by item count, so this is what makes an entry's bits those of its solo call.
// B is a grid y / z dimension of the glue kernels, hence B <= 65535 where one is launched over the batch.
static int stft_transform(const float* audio, int B, int T, const int* lengths, const int* lengths_host, const float* fwd_basis,
                          int n_fft, int hop, float* xp, long ldp, float* ft, float* mag, float* phase, float* magT, long ld_mt,
                          void* stream) {
    const int c = n_fft / 2 + 1;
    if (!audio || !fwd_basis || !xp || !ft || B <= 0 || B > 65535 || T <= n_fft / 2 || n_fft <= 0 || (n_fft & 15) || hop <= 0 ||
        (hop & 3) || (ldp & 3) || ldp < T + n_fft || n_fft > 4096 || (magT && (ld_mt < c || (ld_mt & 15))))
        return T2S_EINVAL;
    const int F = T / hop + 1;
    if (lengths_host)
        for (int b = 0; b < B; ++b)
            if (lengths_host[b] <= n_fft / 2 || lengths_host[b] > T) return T2S_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    T2S_CHECK_HIP(t2s_launch_reflect_pad(audio, B, T, lengths, n_fft / 2, xp, ldp, s));
    for (int b = 0; b < B; ++b)
        T2S_CHECK_HIP(frames_gemm(fwd_basis, 2 * c, n_fft, xp + (size_t)b * ldp, hop, lengths_host ? lengths_host[b] / hop + 1 : F,
                                  ft + (size_t)b * F * 2 * c, 2 * c, 1, s));
    if (mag || phase || magT)
        T2S_CHECK_HIP(t2s_launch_stft_mag_phase(ft, B, F, c, 2 * c, lengths, hop, T, n_fft / 2, mag, phase, magT, ld_mt, s));
    return T2S_OK;
}

static int mel_from_mag(const float* magT, long ld_mt, int B, int F, const int* frames, const int* frames_host,
                        const float* mel_basis_p, int n_mel, float clip, float* mel, void* stream) {
    if (!magT || !mel_basis_p || !mel || B <= 0 || F <= 0 || n_mel <= 0 || ld_mt <= 0 || (ld_mt & 15)) return T2S_EINVAL;
    if (frames_host)
        for (int b = 0; b < B; ++b)
            if (frames_host[b] < 1 || frames_host[b] > F) return T2S_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    for (int b = 0; b < B; ++b)
        T2S_CHECK_HIP(frames_gemm(mel_basis_p, n_mel, (int)ld_mt, magT + (size_t)b * F * ld_mt, ld_mt, frames_host ? frames_host[b] : F,
                                  mel + (size_t)b * n_mel * F, 1, F, s));
    // with frames the kernel also stores the zeros behind every end, so it runs whatever the clip
    if (frames || clip > 0.f) T2S_CHECK_HIP(t2s_launch_log_clamp(mel, B, n_mel, F, frames, clip, s));
    return T2S_OK;
}

static int stft_inverse(const float* mag, const float* phase, int B, int F, const int* frames, const int* frames_host, int n_fft,
                        int hop, const float* inv_basis_t, long ld_rc, const float* bias, float strength, const float* win_sq,
                        float tiny, float* rc, float* frames_buf, float* out, void* stream) {
    const int c = n_fft / 2 + 1;
    if (!mag || !phase || !inv_basis_t || !rc || !frames_buf || !out || B <= 0 || B > 65535 || F <= 1 || n_fft <= 0 || hop <= 0 ||
        ld_rc < 2 * c || (ld_rc & 15))
        return T2S_EINVAL;
    if (frames_host)
        for (int b = 0; b < B; ++b)
            if (frames_host[b] < 2 || frames_host[b] > F) return T2S_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    T2S_CHECK_HIP(t2s_launch_stft_recombine(mag, phase, B, F, c, frames, bias, strength, rc, ld_rc, s));
    for (int b = 0; b < B; ++b)
        T2S_CHECK_HIP(frames_gemm(inv_basis_t, n_fft, (int)ld_rc, rc + (size_t)b * F * ld_rc, ld_rc, frames_host ? frames_host[b] : F,
                                  frames_buf + (size_t)b * F * n_fft, n_fft, 1, s));
    T2S_CHECK_HIP(t2s_launch_stft_overlap_add(frames_buf, win_sq, B, F, frames, n_fft, hop, (float)n_fft / (float)hop, tiny, out,
                                              hop * (F - 1), s));
    return T2S_OK;
}

extern "C" {

int t2s_stft_transform(const float* audio, int B, int T, const float* fwd_basis, int n_fft, int hop, float* xp, long ldp,
                       float* ft, float* mag, float* phase, float* magT, long ld_mt, void* stream) {
    return stft_transform(audio, B, T, nullptr, nullptr, fwd_basis, n_fft, hop, xp, ldp, ft, mag, phase, magT, ld_mt, stream);
}

int t2s_stft_transform_ragged(const float* audio, int B, int T, const int* lengths, const int* lengths_host, const float* fwd_basis,
                              int n_fft, int hop, float* xp, long ldp, float* ft, float* mag, float* phase, float* magT, long ld_mt,
                              void* stream) {
    if (!lengths || !lengths_host) return T2S_EINVAL;
    return stft_transform(audio, B, T, lengths, lengths_host, fwd_basis, n_fft, hop, xp, ldp, ft, mag, phase, magT, ld_mt, stream);
}

int t2s_mel_from_mag(const float* magT, long ld_mt, int B, int F, const float* mel_basis_p, int n_mel, float clip, float* mel,
                     void* stream) {
    return mel_from_mag(magT, ld_mt, B, F, nullptr, nullptr, mel_basis_p, n_mel, clip, mel, stream);
}

int t2s_mel_from_mag_ragged(const float* magT, long ld_mt, int B, int F, const int* frames, const int* frames_host,
                            const float* mel_basis_p, int n_mel, float clip, float* mel, void* stream) {
    if (!frames || !frames_host) return T2S_EINVAL;
    return mel_from_mag(magT, ld_mt, B, F, frames, frames_host, mel_basis_p, n_mel, clip, mel, stream);
}

int t2s_stft_inverse(const float* mag, const float* phase, int B, int F, int n_fft, int hop, const float* inv_basis_t, long ld_rc,
                     const float* bias, float strength, const float* win_sq, float tiny, float* rc, float* frames, float* out,
                     void* stream) {
    return stft_inverse(mag, phase, B, F, nullptr, nullptr, n_fft, hop, inv_basis_t, ld_rc, bias, strength, win_sq, tiny, rc, frames,
                        out, stream);
}

int t2s_stft_inverse_ragged(const float* mag, const float* phase, int B, int F, const int* frames, const int* frames_host, int n_fft,
                            int hop, const float* inv_basis_t, long ld_rc, const float* bias, float strength, const float* win_sq,
                            float tiny, float* rc, float* frames_buf, float* out, void* stream) {
    if (!frames || !frames_host) return T2S_EINVAL;
    return stft_inverse(mag, phase, B, F, frames, frames_host, n_fft, hop, inv_basis_t, ld_rc, bias, strength, win_sq, tiny, rc,
                        frames_buf, out, stream);
}

int t2s_pcm16(const void* x, int is_half, int B, int N, long ldx, const int* lengths, short* out, void* stream) {
    if (!x || !out || B <= 0 || B > 65535 || N <= 0 || ldx < N) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_pcm16(x, is_half, B, N, ldx, lengths, out, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_pcm16_gather(const short* pool, long pool_len, const long* table, int B, int N, float max_wav_value, float* out, long ldo,
                     void* stream) {
    // (the comparison is false for NaN, the subtraction is NaN for an infinity)
    if (!pool || !table || !out || pool_len <= 0 || B <= 0 || B > 65535 || N <= 0 || ldo < N || !(max_wav_value > 0.f) ||
        max_wav_value - max_wav_value != 0.f)
        return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_pcm16_gather(pool, pool_len, table, B, N, max_wav_value, out, ldo, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_gate_targets(const int* frames, int B, int T, float* gate, void* stream) {
    if (!frames || !gate || B <= 0 || B > 65535 || T <= 0) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_gate_targets(frames, B, T, gate, (hipStream_t)stream));
    return T2S_OK;
}

// ---- sample-rate conversion: both entry points launch resample.hip's one kernel --------------------------------------------------------
static bool resample_filter_ok(const double* h, int n_taps, int up, int down) {
    if (!h || ((uintptr_t)h & 7) || n_taps < 3 || !(n_taps & 1) || up < 1 || down < 1 || up > 512 || down > 512) return false;
    int a = up, b = down;
    while (b) { const int t = a % b; a = b; b = t; }
    return a == 1 && t2s_resample_lds_bytes(n_taps, up) <= T2S_RESAMPLE_LDS_MAX;
}

int t2s_resample_tile(void) { return T2S_RESAMPLE_TILE; }

int t2s_resample_table(const void* src, int src_kind, long src_len, const long* table, int n_rows, const double* h, int n_taps, int up,
                       int down, void* dst, int dst_kind, long dst_len, long max_out, int* out_lengths, void* stream) {
    if (!src || !table || !dst || src_kind < 0 || src_kind > 2 || dst_kind < 0 || dst_kind > 1 || src_len <= 0 || dst_len <= 0 ||
        n_rows <= 0 || n_rows > 65535 || max_out <= 0 || max_out > (1L << 40) || !resample_filter_ok(h, n_taps, up, down))
        return T2S_EINVAL;
    ResampleArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.h = h; a.n_taps = n_taps; a.up = up; a.down = down;
    a.dst = dst; a.dst_len = dst_len; a.max_out = max_out; a.out_lengths = out_lengths;
    T2S_CHECK_HIP(t2s_launch_resample(a, src_kind, dst_kind, n_rows, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_resample_batch(const void* x, int is_half, int B, int N, long ldx, const int* lengths, const double* h, int n_taps, int up,
                       int down, float* out, int N_out, long ldo, int* out_lengths, void* stream) {
    if (!x || !out || B <= 0 || B > 65535 || N <= 0 || N_out <= 0 || ldx < N || ldo < N_out || !resample_filter_ok(h, n_taps, up, down))
        return T2S_EINVAL;
    ResampleArgs a;
    memset(&a, 0, sizeof(a));
    a.src = x; a.src_len = (long)(B - 1) * ldx + N; a.lengths = lengths; a.N = N; a.ldx = ldx; a.N_out = N_out; a.ldo = ldo;
    a.h = h; a.n_taps = n_taps; a.up = up; a.down = down;
    a.dst = out; a.dst_len = (long)(B - 1) * ldo + N_out; a.max_out = N_out; a.out_lengths = out_lengths;
    T2S_CHECK_HIP(t2s_launch_resample(a, is_half ? 2 : 1, 1, B, (hipStream_t)stream));
    return T2S_OK;
}

// ---- peak rescaling and silence trimming: trim.hip's three kernels ------------------------------------------------------------------
// (a comparison with NaN is false, the subtraction is NaN for an infinity)
static bool finite_nonneg(double v) { return v >= 0.0 && v - v == 0.0; }
static bool trim_frames_ok(int frame_length, int hop, int pad_mode, long max_frames) {
    return frame_length >= 2 && frame_length <= T2S_TRIM_MAX_FRAME && hop >= 1 && hop <= frame_length && (pad_mode == 0 || pad_mode == 1) &&
           max_frames > 0 && max_frames <= (1L << 40);
}

int t2s_trim_tile(void) { return T2S_TRIM_TILE; }

int t2s_trim_energy(const void* src, int src_kind, long src_len, const long* table, int n_rows, int frame_length, int hop, int pad_mode,
                    long max_frames, double* energy, long energy_len, double* stats, void* stream) {
    if (!src || !table || !stats || !aligned_to(table, 8) || !aligned_to(stats, 8) || !aligned_to(energy, 8) || src_kind < 0 ||
        src_kind > 2 || src_len <= 0 || n_rows <= 0 || n_rows > 65535 || (energy && energy_len <= 0) ||
        !trim_frames_ok(frame_length, hop, pad_mode, max_frames))
        return T2S_EINVAL;
    TrimEnergyArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.frame_length = frame_length; a.hop = hop; a.reflect = pad_mode == 0;
    a.max_frames = max_frames; a.energy = energy; a.energy_len = energy ? energy_len : 0; a.stats = stats;
    T2S_CHECK_HIP(t2s_launch_trim_energy(a, src_kind, n_rows, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_trim_bounds(const long* table, int n_rows, int src_kind, long src_len, int frame_length, int hop, int pad_mode, long max_frames,
                    const double* energy, long energy_len, const double* stats, double top_db, int rescale, double rescaling_max,
                    double peak_floor, long* bounds, void* stream) {
    if (!table || !energy || !stats || !bounds || !aligned_to(table, 8) || !aligned_to(energy, 8) || !aligned_to(stats, 8) ||
        !aligned_to(bounds, 8) || src_kind < 0 || src_kind > 2 || src_len <= 0 || n_rows <= 0 || n_rows > 65535 || energy_len <= 0 ||
        !trim_frames_ok(frame_length, hop, pad_mode, max_frames) || !finite_nonneg(top_db) || !finite_nonneg(rescaling_max) ||
        !finite_nonneg(peak_floor) || (rescale != 0 && rescale != 1) || (rescale && !(rescaling_max > 0.0)))
        return T2S_EINVAL;
    TrimBoundsArgs a;
    memset(&a, 0, sizeof(a));
    a.table = table; a.src_len = src_len; a.frame_length = frame_length; a.hop = hop; a.reflect = pad_mode == 0; a.rescale = rescale;
    a.max_frames = max_frames; a.energy = energy; a.energy_len = energy_len; a.stats = stats; a.rho = pow(10.0, -top_db / 10.0);
    a.rescaling_max = rescaling_max; a.peak_floor = peak_floor; a.unit_gain = src_kind == 0 ? 1.0 / 32768.0 : 1.0; a.bounds = bounds;
    T2S_CHECK_HIP(t2s_launch_trim_bounds(a, n_rows, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_trim_gather(const void* src, int src_kind, long src_len, const long* table, int n_rows, const long* bounds, const double* stats,
                    double rescaling_max, double peak_floor, void* dst, int dst_kind, long dst_len, long max_out, int* out_lengths,
                    void* stream) {
    if (!src || !table || !dst || !aligned_to(table, 8) || !aligned_to(bounds, 8) || !aligned_to(stats, 8) || src_kind < 0 ||
        src_kind > 2 || dst_kind != (src_kind == 0 ? 0 : 1) || src_len <= 0 || dst_len <= 0 || n_rows <= 0 || n_rows > 65535 ||
        max_out <= 0 || max_out > (1L << 40) || !finite_nonneg(rescaling_max) || !finite_nonneg(peak_floor) ||
        (stats && !(rescaling_max > 0.0)))
        return T2S_EINVAL;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)src_len * (src_kind == 1 ? 4 : 2);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)dst_len * (dst_kind == 1 ? 4 : 2);
    if (s0 < d1 && d0 < s1) return T2S_EINVAL;                  // never in place
    TrimGatherArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.bounds = bounds; a.stats = stats;
    a.scale_num = src_kind == 0 ? rescaling_max * 32768.0 : rescaling_max; a.peak_floor = peak_floor;
    a.dst = dst; a.dst_len = dst_len; a.max_out = max_out; a.out_lengths = out_lengths;
    T2S_CHECK_HIP(t2s_launch_trim_gather(a, src_kind, dst_kind, n_rows, (hipStream_t)stream));
    return T2S_OK;
}

// ---- programme loudness: loudness.hip's measure (four launches) and apply -----------------------------------------------------------
int t2s_loud_tile(void) { return T2S_LOUD_TILE; }
int t2s_loud_segment(void) { return T2S_LOUD_SEGMENT; }

long t2s_loud_scratch(int n_rows, long max_count) {
    if (n_rows <= 0 || n_rows > 65535 || max_count <= 0 || max_count > 0x7fffffffL) return -1;
    const long tiles = (max_count + T2S_LOUD_TILE - 1) / T2S_LOUD_TILE, hops = max_count / T2S_LOUD_MIN_HOP + 1;
    return (long)n_rows * (tiles * T2S_LOUD_TILE_DOUBLES + hops);
}

int t2s_loud_measure(const void* src, int src_kind, long src_len, const long* table, int n_rows, long max_count, int fs_hop,
                     const double* coef, double* scratch, long scratch_len, double gate_abs, double target_T, double peak_limit,
                     double* stats, int* counts, void* stream) {
    // (a comparison with NaN is false, the subtraction is NaN for an infinity)
    if (!src || !table || !coef || !scratch || !stats || !counts || !aligned_to(table, 8) || !aligned_to(coef, 8) ||
        !aligned_to(scratch, 8) || !aligned_to(stats, 8) || ((uintptr_t)counts & 3) || src_kind < 0 || src_kind > 2 || src_len <= 0 ||
        n_rows <= 0 || n_rows > 65535 || max_count <= 0 || max_count > 0x7fffffffL || fs_hop < T2S_LOUD_MIN_HOP ||
        fs_hop > T2S_LOUD_MAX_HOP || T2S_LOUD_SEGMENT > fs_hop || !finite_nonneg(gate_abs) || !(target_T > 0.0) ||
        target_T - target_T != 0.0 || peak_limit != peak_limit || scratch_len < t2s_loud_scratch(n_rows, max_count))
        return T2S_EINVAL;
    LoudMeasureArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.n_rows = n_rows; a.h = fs_hop; a.max_count = max_count;
    a.tiles_max = (max_count + T2S_LOUD_TILE - 1) / T2S_LOUD_TILE; a.hops_max = max_count / T2S_LOUD_MIN_HOP + 1;
    a.row_doubles = a.tiles_max * T2S_LOUD_TILE_DOUBLES + a.hops_max;
    a.coef = coef; a.scratch = scratch; a.unit = src_kind == 0 ? 1.0 / 32768.0 : 1.0;
    a.gate_abs = gate_abs; a.target_T = target_T; a.peak_limit = peak_limit > 0.0 ? peak_limit : 0.0; a.stats = stats; a.counts = counts;
    T2S_CHECK_HIP(t2s_launch_loud_measure(a, src_kind, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_loud_apply(const void* src, int src_kind, long src_len, const long* table, int n_rows, const double* stats, void* dst,
                   int dst_kind, long dst_len, long max_out, int* out_lengths, void* stream) {
    if (!src || !table || !stats || !dst || !aligned_to(table, 8) || !aligned_to(stats, 8) || src_kind < 0 || src_kind > 2 ||
        dst_kind != (src_kind == 0 ? 0 : 1) || src_len <= 0 || dst_len <= 0 || n_rows <= 0 || n_rows > 65535 || max_out <= 0 ||
        max_out > (1L << 40))
        return T2S_EINVAL;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)src_len * (src_kind == 1 ? 4 : 2);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)dst_len * (dst_kind == 1 ? 4 : 2);
    if (s0 < d1 && d0 < s1) return T2S_EINVAL;                  // never in place
    LoudApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.stats = stats; a.dst = dst; a.dst_len = dst_len; a.max_out = max_out;
    a.out_lengths = out_lengths;
    T2S_CHECK_HIP(t2s_launch_loud_apply(a, src_kind, dst_kind, n_rows, (hipStream_t)stream));
    return T2S_OK;
}

// ---- joining the rows of padded batches into one utterance: join.hip's two kernels --------------------------------------------------
int t2s_join_tile(void) { return T2S_JOIN_TILE; }

int t2s_join_offsets(const int* lengths, const int* row_caps, const int* order, const int* gaps, int gap, int n, float* dst,
                     long dst_cap, long* offsets, int* length, void* stream) {
    if (!lengths || !row_caps || !dst || !offsets || !length || !aligned_to(offsets, 8) || n <= 0 || n > 65535 || dst_cap <= 0 ||
        dst_cap > 0x7fffffffL || gap < 0)
        return T2S_EINVAL;
    JoinOffsetsArgs a;
    memset(&a, 0, sizeof(a));
    a.lengths = lengths; a.row_caps = row_caps; a.order = order; a.gaps = gaps; a.gap = gap; a.n = n; a.dst_cap = dst_cap;
    a.offsets = offsets; a.length = length;
    T2S_CHECK_HIP(t2s_launch_join_offsets(a, dst, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_join_gather(const void* src, int src_kind, int B, int N, long ldx, const int* lengths, const int* pos, const long* offsets,
                    int n, int fade, int fade_ends, float* dst, long dst_cap, void* stream) {
    if (!src || !lengths || !pos || !offsets || !dst || !aligned_to(offsets, 8) || (src_kind != 1 && src_kind != 2) || B <= 0 ||
        B > 65535 || N <= 0 || ldx < N || n <= 0 || n > 65535 || fade < 0 || fade > 65536 || dst_cap <= 0 || dst_cap > 0x7fffffffL)
        return T2S_EINVAL;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + ((size_t)(B - 1) * ldx + N) * (src_kind == 1 ? 4 : 2);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)dst_cap * 4;
    if (s0 < d1 && d0 < s1) return T2S_EINVAL;                  // never in place
    JoinGatherArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.N = N; a.ldx = ldx; a.lengths = lengths; a.pos = pos; a.offsets = offsets; a.n = n; a.fade = fade;
    a.fade_ends = fade_ends != 0; a.dst = dst; a.dst_cap = dst_cap;
    T2S_CHECK_HIP(t2s_launch_join_gather(a, src_kind, B, (hipStream_t)stream));
    return T2S_OK;
}

}  // extern "C"
