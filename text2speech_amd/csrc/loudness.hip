// Programme loudness of PCM in device memory: ITU-R BS.1770-4 / EBU R128 gated loudness (K-weighting, 400 ms blocks on a 100 ms hop,
// the absolute and the relative gate) and the gain that brings a row to a target, on a pool of clips or a padded batch
// (text2speech_amd/audio.py Loudness, text2speech_amd/data.py PcmPool.loudness / normalize_loudness).  include/t2s_hip.h states the
// arithmetic.  The K-weighting is two biquads in cascade - a recursive filter, so a sample's output depends on every sample before
// it.  It runs in parallel along a row because the filter is linear: the state (4 doubles) at the end of a stretch of samples is
//     s_end = P s_start + e        P: the zero-input map over the stretch, e: the end state from a zero start,
// so stretches are filtered from zero independently and their states chained afterwards.  Four launches measure, one applies:
//
//   loud_tile_kernel<false>  grid tiles x rows.  A workgroup stages a tile of 256 x S consecutive samples of one row in LDS (floats;
//                        segment l at stride S + 1, so that the lanes of a wave walking their segments fall on different banks),
//                        lane l runs segment l through both biquads from zero, and the 256 end states are combined by a
//                        Hillis-Steele scan over the lanes: x_l += P_S^(2^k) x_(l - 2^k), k = 0 .. 7.  Lane 255's is the tile's
//                        end state from a zero start; it goes to the scratch.
//   loud_chain_kernel    one thread per row walks its tiles: c_(t+1) = P_tile c_t + e_t, and leaves every tile's START state
//                        in the place of e_t.
//   loud_tile_kernel<true>   the same staging and scan, lane 0 starting from the tile's start state; then every lane runs its
//                        segment again from the state in front of it and sums the squares of the output in ascending sample
//                        order, in two parts where a hop boundary falls inside the segment (S <= hop: never more than one).
//                        One thread per hop of the tile adds the lanes' parts in ascending lane order; the tile's hop sums, its
//                        peak (a non-finite sample counts as +inf) go to the scratch.
//   loud_gate_kernel     one workgroup per row: hop energies z_k (the tiles' parts in ascending tile order), block mean squares,
//                        both gates, ms, lufs, peak, gain, counts and flags.
//   loud_apply_kernel    rows (src_start, src_count, dst_start, dst_cap): every sample times the row's gain, +0 up to dst_cap.
//
// A carry passes from tile to tile only through a kernel boundary on the one stream: no workgroup waits for another.  Tiles,
// segments and hops are counted from the row's own first sample, every sum has one order that depends on the row's length and the
// hop alone, and no atomic is used: a row's hop energies, statistics and samples are the same bits alone and at any place of any
// batch or pool, at any alignment, whatever lies behind its length.
//
// Memory safety: src_count is cut to what lies inside [0, src_len) and to max_count, which sizes the grid and the scratch; the
// destination to [dst_start, dst_start + dst_cap) inside [0, dst_len); all of it in 64-bit, whatever the tables hold
// (csrc/pcm_rows.h).
#include "t2s_common.h"
#include "audio_ops.h"
#include "pcm_rows.h"

#include <limits.h>
#include <math.h>

#define LD_THREADS 256
#define LD_S T2S_LOUD_SEGMENT
#define LD_STRIDE (LD_S + 1)
#define LD_UNROLL 8                             // samples a thread has in flight while it stages
#define LD_APPLY_TILE 2048                      // outputs of one row per workgroup of the apply
#define LD_STEPS 8                              // log2(LD_THREADS): steps of the scan over the lanes

static_assert(LD_THREADS * LD_S == T2S_LOUD_TILE, "a tile is one segment per lane");
static_assert((1 << LD_STEPS) == LD_THREADS, "the scan covers the workgroup");
static_assert(T2S_LOUD_TILE % (LD_THREADS * LD_UNROLL) == 0, "staging loop");
static_assert(T2S_LOUD_HOPS <= LD_THREADS, "one thread per hop of a tile");

static __device__ __forceinline__ double ld_abs(float v) {
    const double a = fabs((double)v);
    return a < (double)INFINITY ? a : (double)INFINITY;          // NaN too
}

// one sample through both biquads (transposed direct form II); c: b0 b1 b2 a1 a2 of the shelf, then of the high-pass
static __device__ __forceinline__ double ld_step(double s[4], const double* __restrict__ c, double x) {
    const double y1 = fma(c[0], x, s[0]);
    s[0] = fma(-c[3], y1, fma(c[1], x, s[1]));
    s[1] = fma(-c[4], y1, c[2] * x);
    const double y2 = fma(c[5], y1, s[2]);
    s[2] = fma(-c[8], y2, fma(c[6], y1, s[3]));
    s[3] = fma(-c[9], y2, c[7] * y1);
    return y2;
}

// s += P t, P 4 x 4 row-major
static __device__ __forceinline__ void ld_madd(double s[4], const double* __restrict__ P, const double t[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = fma(P[4 * i + 3], t[3], fma(P[4 * i + 2], t[2], fma(P[4 * i + 1], t[1], fma(P[4 * i], t[0], s[i]))));
}

template <typename TSrc, bool ENERGY>
__global__ __launch_bounds__(LD_THREADS) void loud_tile_kernel(const LoudMeasureArgs a) {
    __shared__ float xs[LD_THREADS * LD_STRIDE];
    __shared__ double sc[2][LD_THREADS][4];
    __shared__ double s_peak[LD_THREADS / 64];
    const int tid = threadIdx.x, r = blockIdx.y;
    const long* t = a.table + 2 * (size_t)r;
    const long s0 = t[0];
    const long n = pcm_src_count(s0, t[1], a.src_len, a.max_count);
    const long base = (long)blockIdx.x * T2S_LOUD_TILE;
    if (base >= n) return;                                      // (the whole workgroup)
    const int m = n - base < T2S_LOUD_TILE ? (int)(n - base) : T2S_LOUD_TILE;
    const TSrc* x = (const TSrc*)a.src + s0 + base;
    double* tile = a.scratch + (size_t)r * a.row_doubles + (size_t)blockIdx.x * T2S_LOUD_TILE_DOUBLES;
    const double unit = a.unit;

    // ---- stage the tile: every sample once, coalesced; zeros behind the row's end ----
    double peak = 0.0;
    for (int i0 = tid; i0 < T2S_LOUD_TILE; i0 += LD_THREADS * LD_UNROLL) {
        float v[LD_UNROLL];
#pragma unroll
        for (int u = 0; u < LD_UNROLL; ++u) {
            const int i = i0 + u * LD_THREADS;
            const float w = (float)x[i < m ? i : 0];            // (m > 0: x[0] is the row's own)
            v[u] = i < m ? w : 0.f;
        }
#pragma unroll
        for (int u = 0; u < LD_UNROLL; ++u) {
            const int i = i0 + u * LD_THREADS;
            xs[(i / LD_S) * LD_STRIDE + (i % LD_S)] = v[u];
            if (ENERGY) peak = fmax(peak, ld_abs(v[u]));
        }
    }
    if (ENERGY) {
        for (int off = 32; off; off >>= 1) peak = fmax(peak, __shfl_xor(peak, off));
        if ((tid & 63) == 0) s_peak[tid >> 6] = peak;
    }
    __syncthreads();

    double c[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) c[i] = a.coef[i];

    // ---- every segment from zero (lane 0 of the energy pass: from the tile's start state) ----
    const float* p = xs + tid * LD_STRIDE;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, start[4] = {0.0, 0.0, 0.0, 0.0};
    if (ENERGY && tid == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = start[i] = tile[i];
    }
    for (int i = 0; i < LD_S; ++i) ld_step(s, c, (double)p[i] * unit);

    // ---- the scan over the lanes: afterwards s is lane tid's end state as the row's filter leaves it ----
    int cur = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) sc[0][tid][i] = s[i];
    __syncthreads();
    for (int k = 0; k < LD_STEPS; ++k) {
        const int d = 1 << k;
        if (tid >= d) {
            double tt[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) tt[i] = sc[cur][tid - d][i];
            ld_madd(s, a.coef + T2S_LOUD_COEF_POW + 16 * k, tt);
        }
        cur ^= 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[cur][tid][i] = s[i];
        __syncthreads();
    }
    if (!ENERGY) {
        if (tid == LD_THREADS - 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) tile[i] = s[i];
        }
        return;
    }

    // ---- again, from the state in front of the segment: the squares of the output, split at a hop boundary ----
    if (tid > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) start[i] = sc[cur][tid - 1][i];
    }
    const long h = a.h;
    const long seg0 = base + (long)tid * LD_S;                  // the segment's first sample, counted from the row's
    const long to_edge = (seg0 / h + 1) * h - seg0;             // samples up to the next hop boundary: 1 .. h
    int lim = m - tid * LD_S;                                   // the row's samples in this segment
    lim = lim < 0 ? 0 : (lim > LD_S ? LD_S : lim);
    const int cut = to_edge < lim ? (int)to_edge : lim;
    double acc0 = 0.0, acc1 = 0.0;
    for (int i = 0; i < cut; ++i) {
        const double y = ld_step(start, c, (double)p[i] * unit);
        acc0 = fma(y, y, acc0);
    }
    for (int i = cut; i < lim; ++i) {
        const double y = ld_step(start, c, (double)p[i] * unit);
        acc1 = fma(y, y, acc1);
    }
    __syncthreads();                                            // every lane has read its neighbour's state
    double* part = &sc[0][0][0];                                // [LD_THREADS][2]
    part[2 * tid] = acc0;
    part[2 * tid + 1] = acc1;
    __syncthreads();

    // ---- one thread per hop of the tile: the lanes' parts in ascending lane order ----
    const long k_first = base / h, k_last = (base + m - 1) / h;
    if (tid <= k_last - k_first && tid < T2S_LOUD_HOPS) {
        const long k = k_first + tid;
        const long lo_row = k * h > base ? k * h : base;
        const long hi_row = (k + 1) * h < base + m ? (k + 1) * h : base + m;
        const int lo = (int)(lo_row - base), hi = (int)(hi_row - base);         // 0 <= lo < hi <= m
        const int l0 = lo / LD_S, l1 = (hi - 1) / LD_S;
        // lane l0's segment starts in front of the hop iff the hop starts inside it: then its second part counts
        double z = part[2 * l0 + ((lo % LD_S) != 0 ? 1 : 0)];
        for (int l = l0 + 1; l <= l1; ++l) z += part[2 * l];
        tile[5 + tid] = z;
    }
    if (tid == 0) {
        double pk = s_peak[0];
        for (int w = 1; w < LD_THREADS / 64; ++w) pk = fmax(pk, s_peak[w]);
        tile[4] = pk * unit;
    }
}

__global__ __launch_bounds__(64) void loud_chain_kernel(const LoudMeasureArgs a) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n_rows) return;
    const long* t = a.table + 2 * (size_t)r;
    const long n = pcm_src_count(t[0], t[1], a.src_len, a.max_count);
    const long nt = (n + T2S_LOUD_TILE - 1) / T2S_LOUD_TILE;    // <= tiles_max, since n <= max_count
    double* tile = a.scratch + (size_t)r * a.row_doubles;
    const double* P = a.coef + T2S_LOUD_COEF_TILE;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (long q = 0; q < nt; ++q, tile += T2S_LOUD_TILE_DOUBLES) {
        double e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            e[i] = tile[i];
            tile[i] = c[i];
        }
        ld_madd(e, P, c);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = e[i];
    }
}

static __device__ __forceinline__ double ld_block_ms(const double* z, long j, double four_h) {
    return (((z[j] + z[j + 1]) + z[j + 2]) + z[j + 3]) / four_h;
}

__global__ __launch_bounds__(LD_THREADS) void loud_gate_kernel(const LoudMeasureArgs a) {
    __shared__ double s_sum[LD_THREADS];
    __shared__ long s_cnt[LD_THREADS];
    __shared__ double s_b[2];
    const int tid = threadIdx.x, r = blockIdx.x;
    const long* t = a.table + 2 * (size_t)r;
    const long n = pcm_src_count(t[0], t[1], a.src_len, a.max_count);
    const long h = a.h;
    const long nt = (n + T2S_LOUD_TILE - 1) / T2S_LOUD_TILE;
    long nh = n / h;
    if (nh > a.hops_max) nh = a.hops_max;                       // (never: hops_max covers max_count at the shortest hop)
    const double* tiles = a.scratch + (size_t)r * a.row_doubles;
    double* z = a.scratch + (size_t)r * a.row_doubles + (size_t)a.tiles_max * T2S_LOUD_TILE_DOUBLES;

    // ---- the peak, and every hop's energy: its tiles' parts in ascending tile order ----
    double peak = 0.0;
    for (long q = tid; q < nt; q += LD_THREADS) peak = fmax(peak, tiles[q * T2S_LOUD_TILE_DOUBLES + 4]);
    s_sum[tid] = peak;
    for (long k = tid; k < nh; k += LD_THREADS) {
        const long q0 = (k * h) / T2S_LOUD_TILE, q1 = ((k + 1) * h - 1) / T2S_LOUD_TILE;
        double e = tiles[q0 * T2S_LOUD_TILE_DOUBLES + 5 + (k - (q0 * T2S_LOUD_TILE) / h)];
        for (long q = q0 + 1; q <= q1; ++q) e += tiles[q * T2S_LOUD_TILE_DOUBLES + 5 + (k - (q * T2S_LOUD_TILE) / h)];
        z[k] = e;
    }
    __syncthreads();
    for (int w = LD_THREADS / 2; w; w >>= 1) {
        if (tid < w) s_sum[tid] = fmax(s_sum[tid], s_sum[tid + w]);
        __syncthreads();
    }
    peak = s_sum[0];
    __syncthreads();
    const bool finite = peak < (double)INFINITY;

    // ---- the gates: every thread a run of consecutive blocks, the runs added in ascending order ----
    const long J = nh > 3 ? nh - 3 : 0;
    const long per = (J + LD_THREADS - 1) / LD_THREADS;
    const long j0 = tid * per < J ? tid * per : J, j1 = j0 + per < J ? j0 + per : J;
    const double four_h = 4.0 * (double)h;
    double sum = 0.0, ms = 0.0;
    long cnt = 0, nA = 0, nR = 0;
    if (finite)
        for (long j = j0; j < j1; ++j) {
            const double v = ld_block_ms(z, j, four_h);
            if (v > a.gate_abs) {
                sum += v;
                ++cnt;
            }
        }
    s_sum[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        double sA = 0.0;
        long cA = 0;
        for (int q = 0; q < LD_THREADS; ++q) {
            sA += s_sum[q];
            cA += s_cnt[q];
        }
        s_b[0] = cA > 0 ? 0.1 * (sA / (double)cA) : 0.0;
        s_cnt[0] = cA;
    }
    __syncthreads();
    const double thr = s_b[0];
    nA = s_cnt[0];
    __syncthreads();
    sum = 0.0;
    cnt = 0;
    if (nA > 0)
        for (long j = j0; j < j1; ++j) {
            const double v = ld_block_ms(z, j, four_h);
            if (v > a.gate_abs && v > thr) {
                sum += v;
                ++cnt;
            }
        }
    s_sum[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    if (tid != 0) return;
    double sR = 0.0;
    for (int q = 0; q < LD_THREADS; ++q) {
        sR += s_sum[q];
        nR += s_cnt[q];
    }
    int flags = 0;
    if (J == 0) flags |= 1;
    if (!finite) flags |= 8;
    else if (J > 0 && nA == 0) flags |= 2;
    double g = 1.0, lufs = -(double)INFINITY;
    if (flags) {
        ms = 0.0;
        if (!finite) lufs = (double)NAN;
    } else {
        ms = sR / (double)nR;                                   // (nR >= 1: the loudest block of A passes the relative gate)
        lufs = -0.691 + 10.0 * log10(ms);
        g = sqrt(a.target_T / ms);
        if (a.peak_limit > 0.0 && peak * g > a.peak_limit) {
            g = a.peak_limit / peak;
            flags |= 4;
        }
    }
    double* st = a.stats + 4 * (size_t)r;
    st[0] = ms; st[1] = lufs; st[2] = peak; st[3] = g;
    int* ct = a.counts + 4 * (size_t)r;
    ct[0] = (int)J; ct[1] = (int)nA; ct[2] = (int)nR; ct[3] = flags;
}

static __device__ __forceinline__ void ld_put(short* p, short x, bool scaled, double g) { *p = scaled ? pcm_round16((double)x * g) : x; }
static __device__ __forceinline__ void ld_put(float* p, float x, bool scaled, double g) { *p = scaled ? (float)((double)x * g) : x; }
static __device__ __forceinline__ void ld_put(float* p, _Float16 x, bool scaled, double g) { ld_put(p, (float)x, scaled, g); }

template <typename TSrc, typename TDst>
__global__ __launch_bounds__(LD_THREADS) void loud_apply_kernel(const LoudApplyArgs a) {
    const int tid = threadIdx.x, r = blockIdx.y;
    const long m0 = (long)blockIdx.x * LD_APPLY_TILE;
    const long* t = a.table + 4 * (size_t)r;
    const long s0 = t[0], d0 = t[2];
    const long cap = pcm_dst_cap(t[3], a.max_out, d0, a.dst_len);
    const long n = pcm_src_count(s0, t[1], a.src_len);
    const long valid = n < cap ? n : cap;
    if (blockIdx.x == 0 && tid == 0 && a.out_lengths) a.out_lengths[r] = valid > INT_MAX ? INT_MAX : (int)valid;
    if (m0 >= cap) return;
    const double g = a.stats[4 * (size_t)r + 3];
    const bool scaled = g != 1.0;                               // a gain of one copies bit for bit
    const TSrc* x = (const TSrc*)a.src + (n > 0 ? s0 : 0);
    TDst* out = (TDst*)a.dst + d0;
    for (int o = tid; o < LD_APPLY_TILE; o += LD_THREADS) {
        const long m = m0 + o;
        if (m >= cap) break;
        if (m < valid) ld_put(out + m, x[m], scaled, g);
        else out[m] = (TDst)0;
    }
}

hipError_t t2s_launch_loud_measure(const LoudMeasureArgs& a, int src_kind, hipStream_t s) {
    if (a.tiles_max < 1 || a.tiles_max > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.tiles_max, a.n_rows), block(LD_THREADS);
    switch (src_kind) {
        case 0: hipLaunchKernelGGL((loud_tile_kernel<short, false>), grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL((loud_tile_kernel<float, false>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((loud_tile_kernel<_Float16, false>), grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(loud_chain_kernel, dim3((a.n_rows + 63) / 64), dim3(64), 0, s, a);
    switch (src_kind) {
        case 0: hipLaunchKernelGGL((loud_tile_kernel<short, true>), grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL((loud_tile_kernel<float, true>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((loud_tile_kernel<_Float16, true>), grid, block, 0, s, a); break;
    }
    hipLaunchKernelGGL(loud_gate_kernel, dim3(a.n_rows), dim3(LD_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t t2s_launch_loud_apply(const LoudApplyArgs& a, int src_kind, int dst_kind, int n_rows, hipStream_t s) {
    const long tiles = (a.max_out + LD_APPLY_TILE - 1) / LD_APPLY_TILE;
    if (tiles < 1 || tiles > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, n_rows), block(LD_THREADS);
    switch (src_kind * 2 + dst_kind) {
        case 0: hipLaunchKernelGGL((loud_apply_kernel<short, short>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((loud_apply_kernel<float, float>), grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL((loud_apply_kernel<_Float16, float>), grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
