// True-peak metering and a look-ahead limiter on PCM in device memory (text2speech_amd/audio.py Limiter, data.py PcmPool.true_peak /
// limit, longform.py limit_long).  include/t2s_hip.h states the arithmetic: the envelope p of the row oversampled by the caller's
// polyphase filter, the gain r = c / p that each sample needs, its minimum m over +-L samples, m smoothed by a normalised Hann
// window of 2 L + 1 taps, and the row times the smaller of that and r.  Three kernels:
//
//   limit_tile_kernel<.., APPLY = false>  grid tiles x rows.  A workgroup makes LM_TILE outputs of one row.  It stages the row's
//                        samples over the tile and 2 L + half_width to either side in LDS (floats: every source format is exact in
//                        one; u = x g is formed in double at each use, the same bits every time), forms r over the tile and 2 L to
//                        either side (os phase sums of 2 half_width + 1 taps a sample), the sliding minimum over 2 L + 1 by
//                        doubling in place (windows of 1, 2, 4 .. and one last overlapping step; every thread reads its elements
//                        into registers, a barrier, then writes), and the window sum from LDS for its four outputs.  A tile with
//                        no r below 1 in reach skips the minimum and the sum: s is exactly 1 there (the window's sum is not below
//                        1).  The tile's peaks, its smallest s and its count go to the scratch.
//   limit_reduce_kernel  one wave per row: max, min and the integer sum over the row's tiles - all order-free - and the flags.
//   limit_tile_kernel<.., APPLY = true>   the same tile again (the envelope is recomputed, not stored in between), then u s stored
//                        coalesced, +0 up to dst_cap.  A row that the measure found not limited, or not finite, takes the short
//                        way: one multiply (or a bit copy) a sample, nothing staged.
//
// Nothing waits across workgroups and no atomic is used.  Tiles are counted from the row's own first sample and every sum has one
// order: a row's statistics and samples are the same bits alone and at any place of any batch or pool.
//
// Memory safety: src_count is cut to what lies inside [0, src_len) (and, measuring, to max_count, which sizes the grid and the
// scratch); the destination to [dst_start, dst_start + dst_cap) inside [0, dst_len) and to max_out; all in 64-bit, whatever the
// tables hold (csrc/pcm_rows.h).  LDS, all dynamic (csrc/limit_tile.h): 61.8 KB at L = 1024 and half_width = 32, two workgroups to a
// CU; 15.7 KB at L = 67.
//
// The tile's geometry, its LDS layout, the envelope, the minimum with the window sum and the workgroup's reduction are
// csrc/limit_tile.h's, which the stream's window kernel (csrc/delivery.hip) runs too.
#include "../../include/t2s_hip.h"
#include "t2s_common.h"
#include "t2s_api_common.h"
#include "limit_tile.h"
#include "pcm_rows.h"

#include <limits.h>
#include <math.h>
#include <string.h>

struct LimitArgs {
    const void* src;            // int16 / f32 / f16 [src_len]
    long src_len;
    const long* table;          // int64 on the device: [n_rows][2] src_start, src_count (measure); [n_rows][4] + dst_start, dst_cap
    int n_rows, os, hw, L;
    long max_count;             // measure: samples the grid and the scratch cover per row
    long tiles_max;             // ceil(max_count / LM_TILE)
    const double* gains;        // [n_rows] or NULL
    const double* h;            // [2 hw os + 1]
    const double* w;            // [2 L + 1]
    double c, unit;             // the ceiling; 1 / 32768 for int16 sources, 1 for floats
    double* scratch;            // measure: [n_rows][tiles_max][4] = true peak, sample peak, s_min, count (-1: not finite)
    double* stats;              // measure: [n_rows][4]
    int* counts;                // measure: [n_rows][2]
    const int* counts_in;       // apply: the measure's
    void* dst;                  // apply: int16 / f32 [dst_len]
    long dst_len, max_out;
    int* out_lengths;           // apply: [n_rows] int32 or NULL
};

static __device__ __forceinline__ void lm_store(short* p, double o) { *p = pcm_round16(32768.0 * o); }
static __device__ __forceinline__ void lm_store(float* p, double o) { *p = (float)o; }

template <typename TSrc, typename TDst, int OS, bool APPLY>
__global__ __launch_bounds__(LM_THREADS) void limit_tile_kernel(const LimitArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lm_smem[];
    const int tid = threadIdx.x, r = blockIdx.y;
    const long base = (long)blockIdx.x * LM_TILE;
    const int L = a.L, hw = a.hw;
    const int E = LM_TILE + 4 * L, X = E + 2 * hw;
    const LmTileLds lds = lm_tile_lds(lm_smem, E);
    double* A = lds.A;
    float* xs = lds.xs;
    const long* t = a.table + (APPLY ? 4 : 2) * (size_t)r;
    const long s0 = t[0];
    const long n = pcm_src_count(s0, t[1], a.src_len, APPLY ? LONG_MAX : a.max_count);
    const TSrc* x = (const TSrc*)a.src + (n > 0 ? s0 : 0);
    double gu = (a.gains ? a.gains[r] : 1.0) * a.unit;          // (g / 32768 is exact: u = (x / 32768) g bit for bit)
    const double c = a.c;

    long cap = 0, valid = 0;
    TDst* out = nullptr;
    if (APPLY) {
        const long d0 = t[2];
        cap = pcm_dst_cap(t[3], a.max_out, d0, a.dst_len);
        valid = n < cap ? n : cap;
        if (blockIdx.x == 0 && tid == 0 && a.out_lengths) a.out_lengths[r] = valid > INT_MAX ? INT_MAX : (int)valid;
        if (base >= cap) return;                                // (the whole workgroup)
        out = (TDst*)a.dst + d0;
        const int flags = a.counts_in[2 * (size_t)r + 1];
        if ((flags & 8) || !(flags & 1) || base >= valid) {
            // ---- not limited (s = 1), not finite (copied without its gain), or behind the row: nothing staged ----
            const bool copy = (flags & 8) || gu == a.unit;
            for (int o = tid; o < LM_TILE; o += LM_THREADS) {
                const long i = base + o;
                if (i >= cap) break;
                if (i >= valid) out[i] = (TDst)0;
                else if (copy) out[i] = (TDst)x[i];
                else lm_store(out + i, (double)(float)x[i] * gu);
            }
            return;
        }
    } else if (base >= n) return;

    // ---- stage the samples: every one once, coalesced; zeros outside the row ----
    const long x0 = base - 2 * L - hw;
    for (int q = tid; q < X; q += LM_THREADS) {
        const long i = x0 + q;
        xs[q] = (i >= 0 && i < n) ? (float)x[i] : 0.f;
    }
    if (tid == 0) *lds.any = 0;
    __syncthreads();

    // ---- r over the tile and 2 L to either side; the tile's own peaks and count ----
    double tp = 0.0, sp = 0.0, cnt = 0.0;
    int bad = 0, any = 0;
#pragma unroll 1
    for (int q = tid; q < E; q += LM_THREADS) {
        const long i = base - 2 * L + q;
        double rv = 1.0;
        if (i >= 0 && i < n) {
            // (the sample alone decides "not finite" here: the measure flags the whole row, and the apply then copies it)
            const double p = lm_envelope<OS, false>(xs + q, hw, gu, a.h);
            if (p > c) rv = c / p;
            if (!APPLY && q >= 2 * L && q < 2 * L + LM_TILE) {
                const double au = fabs((double)xs[q + hw] * gu);
                tp = fmax(tp, p);
                sp = fmax(sp, au);
                cnt += p > c ? 1.0 : 0.0;
                bad |= !(au < (double)INFINITY);
            }
        }
        A[q] = rv;
        any |= rv < 1.0;
    }
    if (any) *lds.any = 1;
    __syncthreads();                                            // (A is whole)
    any = *lds.any;

    double s[LM_OUT];
#pragma unroll
    for (int e = 0; e < LM_OUT; ++e) s[e] = 1.0;
    if (any) lm_min_window_sum(A, E, L, a.w, tid, s);

    if (APPLY) {
#pragma unroll
        for (int e = 0; e < LM_OUT; ++e) {
            const int o = tid + e * LM_THREADS;
            const long i = base + o;
            if (i < valid) lm_store(out + i, ((double)xs[2 * L + hw + o] * gu) * s[e]);
            else if (i < cap) out[i] = (TDst)0;
        }
        return;
    }

    // ---- the tile's statistics: order-free reductions over the workgroup ----
    double smin = 1.0;
#pragma unroll
    for (int e = 0; e < LM_OUT; ++e)
        if (base + tid + e * LM_THREADS < n) smin = fmin(smin, s[e]);
    lm_reduce(lds.red, tid, tp, sp, smin, cnt, bad);
    if (tid == 0) {
        double* o = a.scratch + ((size_t)r * a.tiles_max + blockIdx.x) * 4;
        o[0] = tp; o[1] = sp; o[2] = smin; o[3] = bad ? -1.0 : cnt;
    }
}

__global__ __launch_bounds__(64) void limit_reduce_kernel(const LimitArgs a) {
    const int tid = threadIdx.x, r = blockIdx.x;
    const long* t = a.table + 2 * (size_t)r;
    const long n = pcm_src_count(t[0], t[1], a.src_len, a.max_count);
    const long nt = (n + LM_TILE - 1) / LM_TILE;                // <= tiles_max, since n <= max_count
    const double* tiles = a.scratch + (size_t)r * a.tiles_max * 4;
    double tp = 0.0, sp = 0.0, smin = 1.0, cnt = 0.0;
    int bad = 0;
    for (long q = tid; q < nt; q += 64) {
        const double* o = tiles + 4 * q;
        tp = fmax(tp, o[0]); sp = fmax(sp, o[1]); smin = fmin(smin, o[2]);
        if (o[3] < 0.0) bad = 1;
        else cnt += o[3];
    }
    for (int off = 32; off; off >>= 1) {
        tp = fmax(tp, __shfl_xor(tp, off));
        sp = fmax(sp, __shfl_xor(sp, off));
        smin = fmin(smin, __shfl_xor(smin, off));
        cnt += __shfl_xor(cnt, off);
        bad |= __shfl_xor(bad, off);
    }
    if (tid != 0) return;
    double* st = a.stats + 4 * (size_t)r;
    int* ct = a.counts + 2 * (size_t)r;
    if (bad) {
        st[0] = (double)INFINITY; st[1] = (double)INFINITY; st[2] = 1.0; st[3] = 0.0;
        ct[0] = 0; ct[1] = 8;
    } else {
        st[0] = tp; st[1] = sp; st[2] = smin; st[3] = 0.0;
        ct[0] = (int)cnt; ct[1] = cnt > 0.0 ? 1 : 0;
    }
}

template <typename TSrc, typename TDst, bool APPLY>
static void lm_launch(const LimitArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(LM_THREADS);
    const size_t lds = lm_tile_lds_bytes(a.L, a.hw);
    if (a.os == 1) hipLaunchKernelGGL((limit_tile_kernel<TSrc, TDst, 1, APPLY>), grid, block, lds, s, a);
    else if (a.os == 2) hipLaunchKernelGGL((limit_tile_kernel<TSrc, TDst, 2, APPLY>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((limit_tile_kernel<TSrc, TDst, 4, APPLY>), grid, block, lds, s, a);
}

static hipError_t lm_launch_measure(const LimitArgs& a, int src_kind, hipStream_t s) {
    if (a.tiles_max < 1 || a.tiles_max > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.tiles_max, a.n_rows);
    switch (src_kind) {
        case 0: lm_launch<short, short, false>(a, grid, s); break;
        case 1: lm_launch<float, float, false>(a, grid, s); break;
        case 2: lm_launch<_Float16, float, false>(a, grid, s); break;
        default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(limit_reduce_kernel, dim3(a.n_rows), dim3(64), 0, s, a);
    return hipGetLastError();
}

static hipError_t lm_launch_apply(const LimitArgs& a, int src_kind, hipStream_t s) {
    const long tiles = (a.max_out + LM_TILE - 1) / LM_TILE;
    if (tiles < 1 || tiles > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, a.n_rows);
    switch (src_kind) {
        case 0: lm_launch<short, short, true>(a, grid, s); break;
        case 1: lm_launch<float, float, true>(a, grid, s); break;
        case 2: lm_launch<_Float16, float, true>(a, grid, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- the extern "C" boundary ----------------------------------------------------------------------------------------------------------
extern "C" {

int t2s_limit_tile(void) { return LM_TILE; }
int t2s_limit_max_lookahead(void) { return LM_MAX_L; }
int t2s_limit_max_half_width(void) { return LM_MAX_HW; }

long t2s_limit_scratch(int n_rows, long max_count) {
    if (n_rows <= 0 || n_rows > 65535 || max_count <= 0 || max_count > 0x7fffffffL) return -1;
    return (long)n_rows * ((max_count + LM_TILE - 1) / LM_TILE) * 4;
}

int t2s_limit_measure(const void* src, int src_kind, long src_len, const long* table, int n_rows, long max_count, const double* gains,
                      const double* h, int n_taps, int os, int half_width, const double* w, int lookahead, double ceiling,
                      double* scratch, long scratch_len, double* stats, int* counts, void* stream) {
    if (!src || !table || !scratch || !stats || !counts || !aligned_to(table, 8) || !aligned_to(scratch, 8) || !aligned_to(stats, 8) ||
        ((uintptr_t)counts & 3) || src_kind < 0 || src_kind > 2 || src_len <= 0 || n_rows <= 0 || n_rows > 65535 || max_count <= 0 ||
        max_count > 0x7fffffffL || !lm_params_ok(gains, h, n_taps, os, half_width, w, lookahead, ceiling) ||
        scratch_len < t2s_limit_scratch(n_rows, max_count))
        return T2S_EINVAL;
    LimitArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.n_rows = n_rows; a.os = os; a.hw = half_width; a.L = lookahead;
    a.max_count = max_count; a.tiles_max = (max_count + LM_TILE - 1) / LM_TILE; a.gains = gains; a.h = h; a.w = w; a.c = ceiling;
    a.unit = src_kind == 0 ? 1.0 / 32768.0 : 1.0; a.scratch = scratch; a.stats = stats; a.counts = counts;
    T2S_CHECK_HIP(lm_launch_measure(a, src_kind, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_limit_apply(const void* src, int src_kind, long src_len, const long* table, int n_rows, const double* gains, const double* h,
                    int n_taps, int os, int half_width, const double* w, int lookahead, double ceiling, const int* counts, void* dst,
                    int dst_kind, long dst_len, long max_out, int* out_lengths, void* stream) {
    if (!src || !table || !counts || !dst || !aligned_to(table, 8) || ((uintptr_t)counts & 3) || ((uintptr_t)out_lengths & 3) || src_kind < 0 ||
        src_kind > 2 || dst_kind != (src_kind == 0 ? 0 : 1) || src_len <= 0 || dst_len <= 0 || n_rows <= 0 || n_rows > 65535 ||
        max_out <= 0 || max_out > (1L << 40) || !lm_params_ok(gains, h, n_taps, os, half_width, w, lookahead, ceiling))
        return T2S_EINVAL;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)src_len * (src_kind == 1 ? 4 : 2);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)dst_len * (dst_kind == 1 ? 4 : 2);
    if (s0 < d1 && d0 < s1) return T2S_EINVAL;                  // never in place
    LimitArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_len = src_len; a.table = table; a.n_rows = n_rows; a.os = os; a.hw = half_width; a.L = lookahead;
    a.gains = gains; a.h = h; a.w = w; a.c = ceiling; a.unit = src_kind == 0 ? 1.0 / 32768.0 : 1.0; a.counts_in = counts;
    a.dst = dst; a.dst_len = dst_len; a.max_out = max_out; a.out_lengths = out_lengths;
    T2S_CHECK_HIP(lm_launch_apply(a, src_kind, (hipStream_t)stream));
    return T2S_OK;
}

}  // extern "C"
