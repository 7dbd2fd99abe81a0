// The limiter's tile, stated once for the whole-row kernel (limiter.hip) and the stream's window kernel (delivery.hip): the
// geometry, the LDS layout, the envelope at one sample, the sliding minimum with the window sum, and the workgroup's reduction of
// a tile's statistics.  include/t2s_hip.h states the arithmetic.  Both kernels run these loops - the same order of every fma, the
// same barriers - so a stream's windows are the whole-row result bit for bit by construction.  What differs stays in the kernels:
// where a sample comes from, where the outputs and the statistics go.
#pragma once
#include "t2s_api_common.h"

#include <math.h>

#define LM_THREADS 256
#define LM_TILE 1024                            // outputs of one row per workgroup: t2s_limit_tile()
#define LM_MAX_L 1024
#define LM_MAX_HW 32
#define LM_OUT (LM_TILE / LM_THREADS)           // outputs a thread makes
#define LM_EPT ((LM_TILE + 4 * LM_MAX_L) / LM_THREADS)          // elements of r a thread holds at most
#define LM_RED (4 * (LM_THREADS / 64))          // doubles in front of the staging: the partial results of the reductions,
#define LM_HEAD (LM_RED + 2)                    // ... and the workgroup's "some r is below 1" word

static_assert(LM_TILE % LM_THREADS == 0 && (4 * LM_MAX_L) % LM_THREADS == 0, "whole elements per thread");
static_assert(8 * LM_HEAD + 8 * (LM_TILE + 4 * LM_MAX_L) + 4 * (LM_TILE + 4 * LM_MAX_L + 2 * LM_MAX_HW) <= 65536, "the staging fits 64 KB of LDS");
static_assert(LM_HEAD % 2 == 0, "the staging starts 16-byte aligned");

// The tile's LDS, all dynamic and 16-byte aligned (a static in front of it would shift the base of the doubles):
// 144 + 8 E + 4 (E + 2 half_width) bytes, E = LM_TILE + 4 L.
struct LmTileLds {
    double (*red)[LM_THREADS / 64];             // [4][waves]: the workgroup's reductions
    int* any;                                   // some r in the tile's reach is below 1
    double* A;                                  // [E]: r over base - 2 L .., then the minima in place
    float* xs;                                  // [E + 2 half_width]: x over base - 2 L - half_width ..
};
static __device__ __forceinline__ LmTileLds lm_tile_lds(double* smem, int E) {
    LmTileLds l;
    l.red = (double (*)[LM_THREADS / 64])smem;
    l.any = (int*)(smem + LM_RED);
    l.A = smem + LM_HEAD;
    l.xs = (float*)(l.A + E);
    return l;
}
static inline size_t lm_tile_lds_bytes(int L, int hw) {
    const size_t E = LM_TILE + 4 * (size_t)L;
    return 8 * LM_HEAD + 8 * E + 4 * ((E + 2 * (size_t)hw + 3) & ~(size_t)3);
}

// what every entry point refuses about the gains, the filter, the window and the ceiling
static inline bool lm_params_ok(const double* gains, const double* h, int n_taps, int os, int half_width, const double* w, int lookahead,
                                double ceiling) {
    if (!h || !w || !aligned_to(h, 8) || !aligned_to(w, 8) || !aligned_to(gains, 8)) return false;
    if (os != 1 && os != 2 && os != 4) return false;
    if (half_width < 1 || half_width > LM_MAX_HW || n_taps != 2 * half_width * os + 1) return false;
    if (lookahead < 0 || lookahead > LM_MAX_L) return false;
    // (a comparison with NaN is false, the subtraction is NaN for an infinity)
    return ceiling > 0.0 && ceiling - ceiling == 0.0 && (double)(float)ceiling == ceiling;
}

// The envelope p at the sample staged in xq[hw]: the largest of |u| and the OS phase sums of 2 hw + 1 taps over xq[0 .. 2 hw],
// u = x gu formed in double at each use.  MUTE: p is +inf where the sample or an interpolated value is not finite (the window
// kernel, which has no measure pass in front of it to flag the row).
template <int OS, bool MUTE>
static __device__ __forceinline__ double lm_envelope(const float* xq, int hw, double gu, const double* h) {
    double p = fabs((double)xq[hw] * gu);
    int nf = !(p < (double)INFINITY);
    if (OS > 1) {
        double acc[OS];
#pragma unroll
        for (int ph = 0; ph < OS; ++ph) acc[ph] = 0.0;
        const double* hh = h + OS * 2 * hw;                     // tap ph + os (2 hw - d) meets sample i - hw + d
        for (int d = 0; d <= 2 * hw; ++d) {
            const double uv = (double)xq[d] * gu;
#pragma unroll
            for (int ph = 0; ph < OS; ++ph)
                if (ph == 0 || d > 0) acc[ph] = fma(uv, hh[ph - OS * d], acc[ph]);
        }
#pragma unroll
        for (int ph = 0; ph < OS; ++ph) {
            p = fmax(p, fabs(acc[ph]));
            nf |= !(fabs(acc[ph]) < (double)INFINITY);
        }
    }
    return MUTE && nf ? (double)INFINITY : p;
}

// s of the thread's LM_OUT outputs (tid + e LM_THREADS) from r in A[E]: the minimum of r over 2 L + 1 by doubling in place
// (windows of 1, 2, 4 .. and one last overlapping step: read, barrier, write, barrier), its sum under the window w in ascending
// k, and the smaller of that and r.  It holds barriers: every thread of the workgroup calls it, or none.
static __device__ __forceinline__ void lm_min_window_sum(double* A, int E, int L, const double* w, int tid, double s[LM_OUT]) {
    double rs[LM_OUT];
#pragma unroll
    for (int e = 0; e < LM_OUT; ++e) rs[e] = A[2 * L + tid + e * LM_THREADS];
    const int W = 2 * L + 1;
    double v[LM_EPT];
    int win = 1;
    while (win < W) {
        const int sh = 2 * win <= W ? win : W - win;            // the last step overlaps
#pragma unroll
        for (int e = 0; e < LM_EPT; ++e) {
            const int q = tid + e * LM_THREADS;
            if (q + sh < E) v[e] = fmin(A[q], A[q + sh]);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < LM_EPT; ++e) {
            const int q = tid + e * LM_THREADS;
            if (q + sh < E) A[q] = v[e];
        }
        __syncthreads();
        win += sh;
    }
    // ---- A[b] is now m at base - L + b: the window sum of the thread's outputs, in ascending k ----
    double acc[LM_OUT];
#pragma unroll
    for (int e = 0; e < LM_OUT; ++e) acc[e] = 0.0;
    const double* m = A + tid;
    for (int k = 0; k < W; ++k) {
        const double wk = w[k];
#pragma unroll
        for (int e = 0; e < LM_OUT; ++e) acc[e] = fma(wk, m[k + e * LM_THREADS], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < LM_OUT; ++e) s[e] = fmin(rs[e], acc[e]);
}

// The workgroup's largest tp and sp, smallest smin, the sum of cnt (integers below 2^53: exact in any order) and the or of bad,
// all order-free; thread 0 holds them afterwards.  A wave's bad rides on the sign of its count through LDS.  It holds a barrier.
static __device__ __forceinline__ void lm_reduce(double (*red)[LM_THREADS / 64], int tid, double& tp, double& sp, double& smin, double& cnt,
                                                 int& bad) {
    for (int off = 32; off; off >>= 1) {
        tp = fmax(tp, __shfl_xor(tp, off));
        sp = fmax(sp, __shfl_xor(sp, off));
        smin = fmin(smin, __shfl_xor(smin, off));
        cnt += __shfl_xor(cnt, off);
        bad |= __shfl_xor(bad, off);
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = tp; red[1][tid >> 6] = sp; red[2][tid >> 6] = smin; red[3][tid >> 6] = bad ? -1.0 - cnt : cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < LM_THREADS / 64; ++wv) {
            tp = fmax(tp, red[0][wv]); sp = fmax(sp, red[1][wv]); smin = fmin(smin, red[2][wv]);
            const double cw = red[3][wv];
            if (cw < 0.0) { bad = 1; cnt += -1.0 - cw; }
            else cnt += cw;
        }
    }
}
