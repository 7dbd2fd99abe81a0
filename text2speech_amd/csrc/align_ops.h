// Kernel arguments and launchers of align.hip: the row pass and the entry pass over a batch of attention alignments, and over the
// frames of one push of a stream (text2speech_amd/alignment.py alignment_report / AlignmentStream; include/t2s_hip.h states the
// definition).
#pragma once
#include <hip/hip_runtime.h>

#define T2S_ALIGN_ROWS 4                        // rows per workgroup of the row pass: one wave each
#define T2S_ALIGN_BLOCK 256                     // frames per step of the entry pass: one per thread

struct AlignRowsArgs {
    const void* A;              // f32 / f16, B entries of N rows of T_in columns
    long ld_row, ld_entry;      // elements between rows (>= T_in) and between entries (>= N ld_row)
    int B, N, T_in;
    const int* in_len;          // [B] int32 or NULL (T_in); any value safe
    const int* out_len;         // [B] int32 or NULL (N); any value safe
    int* pos;                   // [B, N]
    float* peak;                // [B, N]
    unsigned char* bad;         // [B, N]
};
struct AlignThresholds {        // a negative integer threshold, or min_focus <= 0, switches its bit off
    int max_frames, skip_max, back_max, stall_max, end_slack;
    double min_focus;
};
struct AlignStatsArgs {
    const int* pos;             // the row pass's three outputs, [B, N]
    const float* peak;
    const unsigned char* bad;
    int B, N, T_in;
    const int* in_len;
    const int* out_len;
    AlignThresholds thr;
    int* stats;                 // [B, 8]
    double* focus;              // [B]
    int* dur;                   // [B, T_in], zeroed by the launcher
    int* flags;                 // [B]
};
struct AlignWindowState {       // one per entry: what the entry pass carries from push to push
    int carry;                  // the frame the run of frame n0 - 1 started at
    int red[5];                 // max_skip, max_back, longest_stall, covered, bad_rows
    int pad[2];
    double part[T2S_ALIGN_BLOCK];       // partial i: the sum of peak[t], t % 256 == i, in ascending t
};
struct AlignWindowArgs {        // both passes over the frames [n0, n) of a stream whose buffers persist in HBM
    const void* A;              // f32 / f16, B entries of n - n0 rows of T_in columns: the frames [n0, n)
    long ld_row, ld_entry;      // elements between rows (>= T_in) and between entries (>= (n - n0) ld_row)
    int B, N_cap, T_in, n0, n, last;
    const int* in_len;          // [B] int32 or NULL (T_in); any value safe
    AlignThresholds thr;
    int* pos;                   // [B, N_cap], columns [n0, n) written
    float* peak;                // [B, N_cap]
    unsigned char* bad;         // [B, N_cap]
    AlignWindowState* state;    // [B]
    int* stats;                 // [B, 8]
    double* focus;              // [B]
    int* dur;                   // [B, T_in], zeroed by the launcher where n0 == 0
    int* flags;                 // [B]
};
// src_kind 1 f32, 2 f16
hipError_t t2s_launch_align_rows(const AlignRowsArgs& a, int src_kind, hipStream_t s);
// zeroes dur on the stream, then runs the entry pass
hipError_t t2s_launch_align_stats(const AlignStatsArgs& a, hipStream_t s);
// src_kind 1 f32, 2 f16.  The memset of dur where n0 == 0, the row pass over [n0, n) where it is not empty, the entry pass.
hipError_t t2s_launch_align_window(const AlignWindowArgs& a, int src_kind, hipStream_t s);
