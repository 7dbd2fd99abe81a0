// The resampler's tile, stated once for the whole-row kernel (resample.hip) and the stream's window kernel (delivery.hip): the
// filter phase by phase in LDS and the loop that makes one output.  Both kernels run this loop - k ascending, one double fma a
// tap from +0 - so a stream's windows are the whole-row result bit for bit by construction.  What differs stays in the kernels:
// where a sample comes from (`at(k)` of the source handed in) and where the output goes.
#pragma once
#include "audio_ops.h"

#define RS_THREADS 256

// hp[p][i] = h[p + i up], rows lp doubles apart: every thread of the workgroup calls it; a barrier ends it
static __device__ __forceinline__ void rs_stage_phases(double* hp, const double* h, int n_taps, int up, int lp, int tid) {
    for (int j = tid; j < n_taps; j += RS_THREADS) hp[(j % up) * lp + j / up] = h[j];
    __syncthreads();
}

// the tile of T2S_RESAMPLE_TILE outputs from m0 on
struct RsTile {
    int n_taps, up, down, lp;
    int L;                      // taps of the longest phase
    long q0;                    // c0 / up, c0 = n_taps / 2 + m0 down: h's index under source sample 0, for output m0
    unsigned r0;                // c0 % up
    __device__ __forceinline__ RsTile(long m0, int n_taps_, int up_, int down_, int lp_) : n_taps(n_taps_), up(up_), down(down_), lp(lp_) {
        L = (n_taps + up - 1) / up;
        const long c0 = (long)(n_taps / 2) + m0 * (long)down;
        q0 = c0 / (long)up;
        r0 = (unsigned)(c0 % (long)up);
    }
    // output m0 + o of a row of src.end() samples: the float64 sum over the taps inside the row, whose samples src.at(k) gives.
    // (The source states its own end: handed in beside it, the compiler no longer sees that k_hi keeps k below the end the
    // window's at() tests, and that test stays in the loop - measured, 8 % of resample_window_kernel.)
    template <typename Src>
    __device__ __forceinline__ double output(int o, const Src& src, const double* hp) const {
        const unsigned e = r0 + (unsigned)o * (unsigned)down;   // < 512 + 1023 * 512
        const unsigned p = e % (unsigned)up;
        const long kc = q0 + e / (unsigned)up;                  // the sample under tap p; tap p + i up is under kc - i
        const int cnt = L - ((long)p + (long)(L - 1) * (long)up >= n_taps ? 1 : 0);
        const long k_lo = kc - (cnt - 1) > 0 ? kc - (cnt - 1) : 0;
        const long n_in = src.end();
        const long k_hi = kc < n_in - 1 ? kc : n_in - 1;
        const double* hrow = hp + (size_t)p * lp;
        double acc = 0.0;
        for (long k = k_lo; k <= k_hi; ++k) acc = fma((double)src.at(k), hrow[kc - k], acc);
        return acc;
    }
};

// a whole row in memory; k_lo and k_hi keep k inside it
template <typename T>
struct RsRow {
    const T* x;
    long n;
    __device__ __forceinline__ long end() const { return n; }
    __device__ __forceinline__ T at(long k) const { return x[k]; }
};
