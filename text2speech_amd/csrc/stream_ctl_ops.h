// Kernel arguments and launchers of stream_ctl.hip: the alignment check and the time warp of a stream, pushed piece by piece over
// buffers that persist in HBM (text2speech_amd/alignment.py AlignmentStream, text2speech_amd/rate.py WarpStream;
// include/t2s_hip.h states the definition).
#pragma once
#include <hip/hip_runtime.h>

#include "align_ops.h"
#include "warp_ops.h"

struct AlignWindowState {       // one per entry: what the entry pass carries from push to push
    int carry;                  // the frame the run of frame n0 - 1 started at
    int red[5];                 // max_skip, max_back, longest_stall, covered, bad_rows
    int pad[2];
    double part[T2S_ALIGN_BLOCK];       // partial i: the sum of peak[t], t % 256 == i, in ascending t
};

struct AlignWindowArgs {
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
struct WarpWindowMapArgs {
    int B, N_cap, T_in, n0, n;
    long stretch;               // this push's, where stretches is not given
    const long* stretches;      // [B] int64 or NULL: one per entry; clamped to [2^17, 2^23] on the device
    const int* path;            // [B] rows of >= n values, ld_path apart, or NULL
    long ld_path;
    const int* in_len;          // [B] int32 or NULL (T_in); any value safe
    long* cum;                  // [B, N_cap + 1]: cum[b, n0] is the carry
    int* first_last;            // [B, T_in, 2] or NULL (needs path); set to -1 by the launcher where n0 == 0
};
struct WarpWindowGatherArgs {
    const void* x;              // f32 / f16, B entries of C rows of >= n frames: the mel known so far
    long ld_row, ld_entry;
    int B, C, N_cap, n;
    long j0, j1;                // the output columns asked for
    const long* cum;            // [B, N_cap + 1]
    void* out;                  // [B, C, j1 - j0] of x's type, dense
};
// src_kind 1 f32, 2 f16.  The row pass over [n0, n) where it is not empty, the memset of dur where n0 == 0, the entry pass.
hipError_t t2s_launch_align_window(const AlignWindowArgs& a, int src_kind, hipStream_t s);
hipError_t t2s_launch_warp_window_map(const WarpWindowMapArgs& a, hipStream_t s);
hipError_t t2s_launch_warp_window_gather(const WarpWindowGatherArgs& a, int src_kind, hipStream_t s);
