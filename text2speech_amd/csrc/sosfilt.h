// Biquad cascades on PCM rows in device memory (sosfilt.hip, t2s_api_sosfilt.hip): the geometry, the layout of the host-built
// table and the launch arguments.  include/t2s_hip.h states the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#define T2S_SOS_SEGMENT 16                      // samples a lane filters in sequence
#define T2S_SOS_LANES 256                       // lanes (segments) of a tile
#define T2S_SOS_TILE (T2S_SOS_SEGMENT * T2S_SOS_LANES)
#define T2S_SOS_MAX_SECTIONS 8
#define T2S_SOS_STEPS 8                         // log2(T2S_SOS_LANES)

// the table (doubles): [5 j, 5 j + 5) b0 b1 b2 a1 a2 of section j; [40 + 32 j + 4 k, ... + 4) the 2 x 2 row-major zero-input map of
// section j over SEGMENT 2^k samples, k = 0 .. 7; [296, 296 + (2 n)^2) the 2 n x 2 n row-major zero-input map of the cascade over a tile
#define T2S_SOS_TAB_POW 40
#define T2S_SOS_TAB_TILE (T2S_SOS_TAB_POW + 4 * T2S_SOS_STEPS * T2S_SOS_MAX_SECTIONS)
#define T2S_SOS_TAB_DOUBLES (T2S_SOS_TAB_TILE + 4 * T2S_SOS_MAX_SECTIONS * T2S_SOS_MAX_SECTIONS)

// One row r is L_r samples counted from the start of a tile of the row.
//  rows by table (carry_in == NULL): table [n_rows][4] = (src_start, src_count, dst_start, dst_cap); L_r = the clamped src_count, the
//    start state is zero, outputs i < min(L_r, cap) go to dst + dst_start + i and +0 behind them up to cap.
//  a stream's window (carry_in != NULL): L = head + n for every row; sample i < head is carry_in's, the others the piece's; the start
//    state is carry_in's; outputs i >= head go to out + r ldo + (i - head); carry_out receives the state at the start of tile L / TILE
//    and the L % TILE samples behind it.
struct SosArgs {
    const void* src;        // table rows: the pool / batch;  window: the piece
    long src_len;
    const long* table;
    int n_rows;
    int n_sections;
    long max_count;         // table rows: a longer row is cut here;  window: L
    long tiles;             // tiles of scratch a row owns: ceil(max_count / TILE), at least 1
    const double* gains;    // [n_rows] or NULL
    const double* tab;
    double* scratch;        // [n_rows][tiles][2 n]
    void* dst;
    long dst_len;
    long max_out;
    int* counts;            // [n_rows][2]: nonfinite, clipped
    // window
    const char* carry_in;
    char* carry_out;
    long carry_bytes;       // per row: 2 n doubles, then TILE floats
    long head;              // samples of the current tile that carry_in holds, < TILE
    long ldp, ldo;
};

hipError_t t2s_launch_sos_filter(const SosArgs& a, int src_kind, int dst_kind, hipStream_t s);
hipError_t t2s_launch_sos_window(const SosArgs& a, int is_half, hipStream_t s);
