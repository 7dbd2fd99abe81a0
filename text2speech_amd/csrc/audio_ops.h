// Launchers of the audio front-end / back-end kernels (audio_ops.hip).  `lengths` / `frames` ([B] int32, device) may be NULL: every
// entry then has the batch's extent.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

hipError_t t2s_launch_reflect_pad(const float* x, int B, int T, const int* lengths, int pad, float* xp, long ldp, hipStream_t s);
hipError_t t2s_launch_stft_mag_phase(const float* ft, int B, int F, int c, long ld_ft, const int* lengths, int hop, int T, int pad,
                                     float* mag, float* phase, float* magT, long ld_mt, hipStream_t s);
hipError_t t2s_launch_stft_recombine(const float* mag, const float* phase, int B, int F, int c, const int* frames, const float* bias,
                                     float strength, float* rc, long ld_rc, hipStream_t s);
hipError_t t2s_launch_stft_overlap_add(const float* frames_buf, const float* win_sq, int B, int F, const int* frames, int n_fft,
                                       int hop, float scale, float tiny, float* out, int n_out, hipStream_t s);
hipError_t t2s_launch_log_clamp(float* x, int B, int n_mel, int F, const int* frames, float clip, hipStream_t s);
hipError_t t2s_launch_pcm16(const void* x, int is_half, int B, int N, long ldx, const int* lengths, short* out, hipStream_t s);
// training batches from a pool of int16 clips: `table` [B][2] int64 (start, count) on the device, any value safe
hipError_t t2s_launch_pcm16_gather(const short* pool, long pool_len, const long* table, int B, int N, float max_wav, float* out,
                                   long ldo, hipStream_t s);
hipError_t t2s_launch_gate_targets(const int* frames, int B, int T, float* gate, hipStream_t s);

// sample-rate conversion (resample.hip): one kernel for a pool addressed through a table and for a padded batch
#define T2S_RESAMPLE_TILE 1024                  // consecutive outputs of one row per workgroup
#define T2S_RESAMPLE_LDS_MAX (96 * 1024)        // the filter's polyphase table must fit: 84 KB at max(up, down) = 512, half_width 10
struct ResampleArgs {
    const void* src;            // int16 / f32 / f16 [src_len]
    long src_len;
    const long* table;          // [n_rows][4] int64 on the device: src_start, src_count, dst_start, dst_cap; NULL: the batch form below
    const int* lengths;         // batch form: [n_rows] int32 on the device or NULL (every row holds N)
    long N, ldx, N_out, ldo;    // batch form: row b reads src + b ldx, writes dst + b ldo, dst_cap = N_out
    const double* h;            // [n_taps], n_taps odd
    int n_taps, up, down;
    int lp;                     // (filled in by the launcher) doubles between two phases of the table in LDS
    void* dst;                  // int16 / f32 [dst_len]
    long dst_len;
    long max_out;               // outputs the grid covers per row
    int* out_lengths;           // [n_rows] int32 or NULL
};
int t2s_resample_lds_bytes(int n_taps, int up);
// src_kind 0 int16, 1 f32, 2 f16; dst_kind 0 int16, 1 f32
hipError_t t2s_launch_resample(const ResampleArgs& a, int src_kind, int dst_kind, int n_rows, hipStream_t s);

// peak rescaling and silence trimming (trim.hip): frame energies and per-row maxima, the kept range per row, the gather
#define T2S_TRIM_TILE 64                        // consecutive frames of one row per workgroup of the energy pass
#define T2S_TRIM_MAX_FRAME 8192                 // the longest frame_length
struct TrimEnergyArgs {
    const void* src;            // int16 / f32 / f16 [src_len]
    long src_len;
    const long* table;          // [n_rows][3] int64 on the device: src_start, src_count, energy_start
    int frame_length, hop, reflect;
    long max_frames;            // frames the grid covers per row
    double* energy;             // [energy_len] or NULL: the peaks only
    long energy_len;
    double* stats;              // [n_rows][2]: max |x|, max E_f (-1: a reflect row of at most frame_length / 2 samples); zeroed by the launcher
};
struct TrimBoundsArgs {
    const long* table;          // the energy pass's
    long src_len;
    int frame_length, hop, reflect, rescale;
    long max_frames;
    const double* energy;
    long energy_len;
    const double* stats;
    double rho;                 // 10^(-top_db / 10)
    double rescaling_max, peak_floor;
    double unit_gain;           // the view gain without rescaling: 1 / 32768 for int16 sources, 1 for floats
    long* bounds;               // [n_rows][2]: start, end
};
struct TrimGatherArgs {
    const void* src;
    long src_len;
    const long* table;          // [n_rows][4] int64 on the device: src_start, src_count, dst_start, dst_cap
    const long* bounds;         // [n_rows][2] or NULL: the whole row
    const double* stats;        // [n_rows][2] or NULL: no rescaling
    double scale_num;           // a sample is multiplied by scale_num / max(peak, peak_floor): rescaling_max (x 32768 for int16)
    double peak_floor;
    void* dst;                  // int16 / f32 [dst_len]
    long dst_len;
    long max_out;               // outputs the grid covers per row
    int* out_lengths;           // [n_rows] int32 or NULL
};
hipError_t t2s_launch_trim_energy(const TrimEnergyArgs& a, int src_kind, int n_rows, hipStream_t s);
hipError_t t2s_launch_trim_bounds(const TrimBoundsArgs& a, int n_rows, hipStream_t s);
// (src_kind, dst_kind): int16 -> int16, f32 -> f32, f16 -> f32
hipError_t t2s_launch_trim_gather(const TrimGatherArgs& a, int src_kind, int dst_kind, int n_rows, hipStream_t s);

// programme loudness (loudness.hip): K-weighting by tiles and segments, hop energies, both gates, the gain; then the gain applied
#define T2S_LOUD_SEGMENT 32                     // consecutive samples one lane filters
#define T2S_LOUD_TILE (256 * T2S_LOUD_SEGMENT)  // consecutive samples of one row per workgroup
#define T2S_LOUD_MIN_HOP 400                    // 100 ms at 4 kHz
#define T2S_LOUD_MAX_HOP 38400                  // ... at 384 kHz
#define T2S_LOUD_HOPS (T2S_LOUD_TILE / T2S_LOUD_MIN_HOP + 2)    // the most hops that touch one tile
#define T2S_LOUD_TILE_DOUBLES (5 + T2S_LOUD_HOPS)               // scratch per tile: state [4], peak, the hops' parts
#define T2S_LOUD_COEF_POW 16                    // coef: [0, 10) the biquads, [16, 144) P_S^(2^k) k = 0 .. 7, [144, 160) P_tile
#define T2S_LOUD_COEF_TILE (T2S_LOUD_COEF_POW + 8 * 16)
#define T2S_LOUD_COEF_DOUBLES (T2S_LOUD_COEF_TILE + 16)
struct LoudMeasureArgs {
    const void* src;            // int16 / f32 / f16 [src_len]
    long src_len;
    const long* table;          // [n_rows][2] int64 on the device: src_start, src_count
    int n_rows, h;
    long max_count;             // samples the grid and the scratch cover per row; a longer row is cut there
    long tiles_max, hops_max;   // ceil(max_count / tile), max_count / T2S_LOUD_MIN_HOP + 1
    long row_doubles;           // tiles_max T2S_LOUD_TILE_DOUBLES + hops_max: the scratch of one row
    const double* coef;         // [T2S_LOUD_COEF_DOUBLES]
    double* scratch;            // [n_rows][row_doubles]
    double unit;                // 1 / 32768 for int16 sources, 1 for floats
    double gate_abs, target_T, peak_limit;
    double* stats;              // [n_rows][4]: ms, lufs, peak, g
    int* counts;                // [n_rows][4]: J, |A|, |R|, flags
};
struct LoudApplyArgs {
    const void* src;
    long src_len;
    const long* table;          // [n_rows][4] int64 on the device: src_start, src_count, dst_start, dst_cap
    const double* stats;        // the measure's
    void* dst;                  // int16 / f32 [dst_len]
    long dst_len;
    long max_out;               // outputs the grid covers per row
    int* out_lengths;           // [n_rows] int32 or NULL
};
hipError_t t2s_launch_loud_measure(const LoudMeasureArgs& a, int src_kind, hipStream_t s);
// (src_kind, dst_kind): int16 -> int16, f32 -> f32, f16 -> f32
hipError_t t2s_launch_loud_apply(const LoudApplyArgs& a, int src_kind, int dst_kind, int n_rows, hipStream_t s);

// joining the rows of padded batches into one utterance (join.hip): the scan of the lengths, then one gather per source batch
#define T2S_JOIN_TILE 2048                      // samples of one row per workgroup of the gather
struct JoinOffsetsArgs {
    const int* lengths;         // [n] int32 on the device, by row; any value safe
    const int* row_caps;        // [n] int32: the N of each row's batch
    const int* order;           // [n] int32: position -> row, or NULL (the identity)
    const int* gaps;            // [n - 1] int32 by position, or NULL: `gap` everywhere
    int gap, n;
    long dst_cap;
    long* offsets;              // [n + 1] int64, unclipped; offsets[n] = total
    int* length;                // [1] int32: min(total, dst_cap)
};
struct JoinGatherArgs {
    const void* src;            // f32 / f16, B rows of N samples, ldx apart
    long N, ldx;
    const int* lengths;         // [B] int32
    const int* pos;             // [B] int32: the row's position; outside [0, n): not part of the join
    const long* offsets;        // the scan's
    int n, fade, fade_ends;
    float* dst;
    long dst_cap;
};
// zeroes dst[0 : dst_cap) on the stream, then scans
hipError_t t2s_launch_join_offsets(const JoinOffsetsArgs& a, float* dst, hipStream_t s);
// src_kind 1 f32, 2 f16
hipError_t t2s_launch_join_gather(const JoinGatherArgs& a, int src_kind, int B, hipStream_t s);
