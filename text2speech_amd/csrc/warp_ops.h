// Kernel arguments and launchers of warp.hip: the cumulative map of a time warp, the gather that warps a mel along it and the
// symbol spans read from it, and the map and the gather over the frames of one push of a stream (text2speech_amd/rate.py warp_mel /
// symbol_spans / WarpStream; include/t2s_hip.h states the definition).
#pragma once
#include <hip/hip_runtime.h>

#define T2S_WARP_Q_BITS 20                      // stretches count output frames in units of 1 / 2^20
#define T2S_WARP_Q (1L << T2S_WARP_Q_BITS)      // a stretch of 1: rate 1
#define T2S_WARP_BLOCK 256                      // frames per step of the map's walk, and output frames per tile of the gather
#define T2S_WARP_CH 16                          // channels one workgroup of the gather walks

struct WarpMapArgs {
    const int* lengths;         // [B] int32 or NULL (F); any value safe
    int B, F, T_in, cap;
    long stretch;               // every frame's, where neither stretches nor rates is given
    const long* stretches;      // [B] int64 or NULL: one per entry; clamped to [2^17, 2^23] on the device
    const int* path;            // [B] rows of F values, ld_path apart, or NULL
    long ld_path;
    const float* rates;         // [B] rows of T_in values, ld_rates apart, or NULL (needs path)
    long ld_rates;
    const int* in_len;          // [B] int32 or NULL (T_in); any value safe
    double min_rate, max_rate;
    long* cum;                  // [B, F + 1] or NULL
    int* out_len;               // [B] or NULL
    int* first_last;            // [B, T_in, 2] or NULL (needs path); set to -1 by the launcher
};
struct WarpGatherArgs {
    const void* x;              // f32 / f16, B entries of C rows of F frames
    long ld_row, ld_entry;
    int B, C, F, cap;
    const int* lengths;         // as the map's
    const long* cum;            // [B, F + 1]
    const int* out_len;         // [B]: the map's
    void* out;                  // [B, C, cap] of x's type, dense
};
struct WarpSpansArgs {
    const long* cum;            // [B, F + 1]
    const int* first_last;      // [B, T_in, 2]
    int B, F, T_in;
    const int* in_len;
    const int* lengths;
    long hop;
    const long* trim_start;     // [B] or NULL; with trim_end
    const long* trim_end;       // trim_len = trim_end - trim_start
    const long* offsets;        // [B] or NULL
    long up, down, total;
    const long* total_dev;      // [1] or NULL: in the place of `total`
    long* spans;                // [B, T_in, 2]
};
struct WarpWindowMapArgs {      // the map over the frames [n0, n) of a stream whose table persists in HBM
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
// sets first_last to -1 on the stream where it is given, then walks the entries
hipError_t t2s_launch_warp_map(const WarpMapArgs& a, hipStream_t s);
// src_kind 1 f32, 2 f16
hipError_t t2s_launch_warp_gather(const WarpGatherArgs& a, int src_kind, hipStream_t s);
hipError_t t2s_launch_warp_spans(const WarpSpansArgs& a, hipStream_t s);
// sets first_last to -1 where it is given and n0 == 0, then extends the map
hipError_t t2s_launch_warp_window_map(const WarpWindowMapArgs& a, hipStream_t s);
// src_kind 1 f32, 2 f16; launches nothing where j1 <= j0
hipError_t t2s_launch_warp_window_gather(const WarpWindowGatherArgs& a, int src_kind, hipStream_t s);
