// Delivery inside a stream (text2speech_amd/audio.py DeliveryStream, streaming.py synthesize_stream(delivery=)): the resampler and the
// limiter window by window, and G.711 bytes.  include/t2s_hip.h states the arithmetic.  Both stages are local - an output of the
// resampler reads ceil(n_taps / up) source samples, an output of the limiter 2 L + half_width samples to either side - so a stream
// keeps a short tail of its row, the carry, from window to window and every output is computed from carry | piece by the loop the
// whole-row kernel runs - one statement of each, csrc/resample_tap.h for csrc/resample.hip and this file, csrc/limit_tile.h for
// csrc/limiter.hip and this file: the concatenation of a stream's windows is the whole-row result bit for bit.
//
//   resample_window_kernel  grid (tiles + 1) x rows.  A workgroup makes T2S_RESAMPLE_TILE outputs counted from the window's first:
//                           the filter phase by phase in LDS, then per output one loop over k ascending, one double fma a tap
//                           from +0, over the carry and then the piece.  The last workgroup of a row writes the next carry.
//   limit_window_kernel     grid (tiles + 1) x rows.  A workgroup makes LM_TILE outputs: samples staged in LDS as floats, r over
//                           the tile and 2 L to either side, the sliding minimum by doubling, the window sum; a tile with no r below
//                           1 in reach skips both.  Its peaks, smallest s, count and flags go into the row's running state by
//                           integer atomics (max / min of the bit patterns of non-negative doubles, add, or): order-free, so the
//                           state does not depend on the order the workgroups arrive in.  The last workgroup writes the next carry.
//   g711_kernel             one int16 code -> one byte, by the integer algorithm of the header.
//
// Nothing waits across workgroups and there is no floating-point atomic.  carry_in is only read and carry_out only written
// (ping-pong: the entry points refuse the two overlapping).
//
// Memory safety: a sample at global index i is read from the piece when K0 <= i < K0 + n, from the carry when K0 - C <= i < K0 and
// i >= 0, and is 0 otherwise - whatever K0, M0 / O0 hold; an output index lies in [0, M1 - M0), which the entry point has checked
// against out_cap; the state index is the row.  The LDS of both kernels is laid out and sized by the shared headers.
#include "../../include/t2s_hip.h"
#include "t2s_common.h"
#include "t2s_api_common.h"
#include "audio_ops.h"
#include "limit_tile.h"
#include "resample_tap.h"

#include <limits.h>
#include <math.h>
#include <string.h>

#define DV_THREADS 256
#define DV_MAX_POS (1L << 40)                   // the largest sample index of a stream's row

static_assert(DV_THREADS == RS_THREADS && DV_THREADS == LM_THREADS, "one workgroup size: the carry's roll serves both kernels");

// the two-segment source of a window: carry [C] holds the samples K0 - C .. K0 - 1, piece [n] the samples K0 .. K0 + n - 1
template <typename TPiece>
struct DvSource {
    const float* carry;
    const TPiece* piece;
    long K0, K1;
    int C;
    __device__ __forceinline__ long end() const { return K1; }
    __device__ __forceinline__ float at(long i) const {
        if (i < 0 || i >= K1) return 0.f;
        if (i >= K0) return (float)piece[i - K0];
        const long d = K0 - i;
        return d <= C ? carry[C - d] : 0.f;
    }
    // the next carry: the last C samples of carry | piece, widened exactly
    __device__ __forceinline__ void roll(float* carry_out, int tid) const {
        const long n = K1 - K0;
        for (int j = tid; j < C; j += DV_THREADS) {
            const long e = (long)j + n;                         // position in carry | piece
            carry_out[j] = e < C ? carry[e] : (float)piece[e - C];
        }
    }
};

// floor(a / b) and ceil(a / b) for b > 0 and any a
static inline long dv_floor_div(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static inline long dv_ceil_div(long a, long b) { return -dv_floor_div(-a, b); }

// ---- the resampler ----------------------------------------------------------------------------------------------------------------------
struct RsWindowArgs {
    const float* carry_in;      // [B][C]
    float* carry_out;           // [B][C]
    const void* piece;          // f32 / f16 [B] rows of n, ldp apart
    long n, ldp, K0, M0, M1;
    const double* h;
    int n_taps, up, down, lp, C;
    float* out;                 // [B] rows of M1 - M0, ldo apart
    long ldo;
    unsigned tiles;
};

template <typename TPiece>
__global__ __launch_bounds__(DV_THREADS) void resample_window_kernel(const RsWindowArgs a) {
    extern __shared__ double dv_hp[];
    const int tid = threadIdx.x, r = blockIdx.y;
    DvSource<TPiece> src;
    src.carry = a.carry_in + (size_t)r * a.C;
    src.piece = (const TPiece*)a.piece + (size_t)r * a.ldp;
    src.K0 = a.K0; src.K1 = a.K0 + a.n; src.C = a.C;
    if (blockIdx.x == a.tiles) {
        src.roll(a.carry_out + (size_t)r * a.C, tid);
        return;
    }
    const long m0 = a.M0 + (long)blockIdx.x * T2S_RESAMPLE_TILE;
    rs_stage_phases(dv_hp, a.h, a.n_taps, a.up, a.lp, tid);

    const RsTile tile(m0, a.n_taps, a.up, a.down, a.lp);
    float* out = a.out + (size_t)r * a.ldo;
    for (int o = tid; o < T2S_RESAMPLE_TILE; o += DV_THREADS) {
        const long m = m0 + o;
        if (m >= a.M1) break;
        out[m - a.M0] = (float)tile.output(o, src, dv_hp);         // one rounding
    }
}

template <typename TPiece>
static hipError_t dv_launch_resample(const RsWindowArgs& a, int B, hipStream_t s) {
    static std::atomic<unsigned long long> attr_mask{0};
    const hipError_t e = t2s_raise_lds_limit((const void*)resample_window_kernel<TPiece>, T2S_RESAMPLE_LDS_MAX, attr_mask);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((resample_window_kernel<TPiece>), dim3(a.tiles + 1, B), dim3(DV_THREADS),
                       (size_t)t2s_resample_lds_bytes(a.n_taps, a.up), s, a);
    return hipGetLastError();
}

// ---- the limiter ------------------------------------------------------------------------------------------------------------------------
struct LmWindowArgs {
    const float* carry_in;
    float* carry_out;
    const void* piece;
    long n, ldp, N0, O0, O1;
    const double* gains;        // [B] or NULL
    const double* h;            // [2 hw os + 1]
    const double* w;            // [2 L + 1]
    double c;
    int hw, L, C;
    float* out;                 // [B] rows of O1 - O0, ldo apart
    long ldo;
    unsigned long long* state;  // [B][5]: the bits of max p, max |u|, min s, 0, then (int32 count, int32 flags)
    unsigned tiles;
};

template <typename TPiece, int OS>
__global__ __launch_bounds__(DV_THREADS) void limit_window_kernel(const LmWindowArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dv_smem[];
    const int tid = threadIdx.x, r = blockIdx.y;
    DvSource<TPiece> src;
    src.carry = a.carry_in + (size_t)r * a.C;
    src.piece = (const TPiece*)a.piece + (size_t)r * a.ldp;
    src.K0 = a.N0; src.K1 = a.N0 + a.n; src.C = a.C;
    if (blockIdx.x == a.tiles) {
        src.roll(a.carry_out + (size_t)r * a.C, tid);
        return;
    }
    const long base = a.O0 + (long)blockIdx.x * LM_TILE;
    const long N1 = src.K1;
    const int L = a.L, hw = a.hw;
    const int E = LM_TILE + 4 * L, X = E + 2 * hw;
    const LmTileLds lds = lm_tile_lds(dv_smem, E);
    double* A = lds.A;
    float* xs = lds.xs;
    const double gu = a.gains ? a.gains[r] : 1.0;
    const double c = a.c;

    // ---- stage the samples: every one once; zeros outside the row (and behind what the stream has seen) ----
    const long x0 = base - 2 * L - hw;
    for (int q = tid; q < X; q += DV_THREADS) xs[q] = src.at(x0 + q);
    if (tid == 0) *lds.any = 0;
    __syncthreads();

    // ---- r over the tile and 2 L to either side; the peaks and the count of what this tile delivers ----
    double tp = 0.0, sp = 0.0;
    int cnt = 0, bad = 0, any = 0;
#pragma unroll 1
    for (int q = tid; q < E; q += DV_THREADS) {
        const long i = base - 2 * L + q;
        double rv = 1.0;
        if (i >= 0 && i < N1) {
            // (a sample or an interpolated value that is not finite mutes: p is +inf there)
            const double p = lm_envelope<OS, true>(xs + q, hw, gu, a.h);
            if (p > c) rv = c / p;
            if (q >= 2 * L && q < 2 * L + LM_TILE && i < a.O1) {
                const double au = fabs((double)xs[q + hw] * gu);
                tp = fmax(tp, p);
                sp = fmax(sp, au < (double)INFINITY ? au : (double)INFINITY);
                cnt += p > c ? 1 : 0;
                bad |= !(p < (double)INFINITY);
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

    float* out = a.out + (size_t)r * a.ldo;
    double smin = 1.0;
#pragma unroll
    for (int e = 0; e < LM_OUT; ++e) {
        const int o = tid + e * DV_THREADS;
        const long i = base + o;
        if (i < a.O1) {
            const double u = (double)xs[2 * L + hw + o] * gu;
            out[i - a.O0] = fabs(u) < (double)INFINITY ? (float)(u * s[e]) : 0.f;
            smin = fmin(smin, s[e]);
        }
    }

    // ---- the tile's statistics into the row's state: order-free, whatever order the workgroups arrive in ----
    double total = (double)cnt;
    lm_reduce(lds.red, tid, tp, sp, smin, total, bad);
    if (tid == 0) {
        unsigned long long* st = a.state + 5 * (size_t)r;
        int* ct = (int*)(st + 4);
        // (non-negative doubles order as their bit patterns; a tile that changes nothing issues no atomic)
        if (tp > 0.0) atomicMax(st + 0, (unsigned long long)__double_as_longlong(tp));
        if (sp > 0.0) atomicMax(st + 1, (unsigned long long)__double_as_longlong(sp));
        if (smin < 1.0) atomicMin(st + 2, (unsigned long long)__double_as_longlong(smin));
        const int flags = (total > 0.0 ? 1 : 0) | (bad ? 8 : 0);
        if (total > 0.0) atomicAdd(ct + 0, (int)total);
        if (flags) atomicOr(ct + 1, flags);
    }
}

template <typename TPiece>
static hipError_t dv_launch_limit(const LmWindowArgs& a, int os, int B, hipStream_t s) {
    const dim3 grid(a.tiles + 1, B), block(DV_THREADS);
    const size_t lds = lm_tile_lds_bytes(a.L, a.hw);
    if (os == 1) hipLaunchKernelGGL((limit_window_kernel<TPiece, 1>), grid, block, lds, s, a);
    else if (os == 2) hipLaunchKernelGGL((limit_window_kernel<TPiece, 2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((limit_window_kernel<TPiece, 4>), grid, block, lds, s, a);
    return hipGetLastError();
}

// ---- G.711 ------------------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ unsigned char dv_ulaw(int x) {
    int v = x >> 2, mask = 0xFF;                                // 14 bits
    if (v < 0) { v = -v; mask = 0x7F; }
    if (v > 8159) v = 8159;
    v += 33;
    int seg = 0;
    while (seg < 8 && v > (0x3F << seg) + ((1 << seg) - 1)) ++seg;          // ends 0x3F, 0x7F .. 0x1FFF
    const int code = seg >= 8 ? 0x7F : ((seg << 4) | ((v >> (seg + 1)) & 0xF));
    return (unsigned char)(code ^ mask);
}
static __device__ __forceinline__ unsigned char dv_alaw(int x) {
    int v = x >> 3, mask = 0xD5;                                // 13 bits
    if (v < 0) { v = -v - 1; mask = 0x55; }
    int seg = 0;
    while (seg < 8 && v > (0x1F << seg) + ((1 << seg) - 1)) ++seg;          // ends 0x1F, 0x3F .. 0xFFF
    const int code = seg >= 8 ? 0x7F : ((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 0xF));
    return (unsigned char)(code ^ mask);
}

__global__ __launch_bounds__(DV_THREADS) void g711_kernel(const short* pcm, long n, int law, unsigned char* out) {
    const long i = (long)blockIdx.x * DV_THREADS + threadIdx.x;
    if (i >= n) return;
    const int x = pcm[i];
    out[i] = law ? dv_alaw(x) : dv_ulaw(x);
}

// ---- the extern "C" boundary ----------------------------------------------------------------------------------------------------------
static long dv_gcd(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }

static bool dv_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

// what both window entry points refuse about the rows
static bool dv_rows_ok(const float* carry_in, float* carry_out, const void* piece, int is_half, int B, long n, long ldp, long pos0,
                       long out0, int C, const float* out, long ldo) {
    if (!carry_in || !carry_out || B <= 0 || B > 65535 || n < 0 || n > 0x7fffffffL || (n > 0 && (!piece || ldp < n)) ||
        pos0 < 0 || out0 < 0 || pos0 > DV_MAX_POS - n || out0 > DV_MAX_POS || C < 1 || ldo < 0)
        return false;
    if (!aligned_to(carry_in, 4) || !aligned_to(carry_out, 4) || !aligned_to(out, 4) || !aligned_to(piece, is_half ? 2 : 4)) return false;
    return !dv_overlap(carry_in, carry_out, (size_t)B * C * sizeof(float));
}

extern "C" {

int t2s_resample_window_carry(int n_taps, int up) {
    if (n_taps < 3 || up < 1) return -1;
    return (int)(((long)n_taps + up - 1) / up);
}

long t2s_resample_window_end(long K1, long M0, int n_taps, int up, int down, int final) {
    if (K1 < 0 || K1 > DV_MAX_POS || M0 < 0 || n_taps < 3 || up < 1 || down < 1 || up > 512 || down > 512) return -1;
    const long M1 = final ? dv_ceil_div(K1 * up, down) : dv_ceil_div(K1 * up - n_taps / 2, down);
    return M1 > M0 ? M1 : M0;
}

int t2s_resample_window(const float* carry_in, float* carry_out, const void* piece, int is_half, int B, long n, long ldp, long K0,
                        long M0, int final, const double* h, int n_taps, int up, int down, float* out, long out_cap, long ldo,
                        void* stream) {
    if (!h || !aligned_to(h, 8) || up < 1 || down < 1 || up > 512 || down > 512 || dv_gcd(up, down) != 1 || n_taps < 3 || !(n_taps & 1) ||
        t2s_resample_lds_bytes(n_taps, up) > T2S_RESAMPLE_LDS_MAX)
        return T2S_EINVAL;
    const int C = t2s_resample_window_carry(n_taps, up);
    if (!dv_rows_ok(carry_in, carry_out, piece, is_half, B, n, ldp, K0, M0, C, out, ldo)) return T2S_EINVAL;
    const long M1 = t2s_resample_window_end(K0 + n, M0, n_taps, up, down, final);
    if (M1 < 0 || (M1 > M0 && !out) || M1 - M0 > out_cap || M1 - M0 > ldo || M1 - M0 > 0x7fffffffL) return T2S_EINVAL;
    RsWindowArgs a;
    memset(&a, 0, sizeof(a));
    a.carry_in = carry_in; a.carry_out = carry_out; a.piece = piece; a.n = n; a.ldp = ldp; a.K0 = K0; a.M0 = M0; a.M1 = M1; a.h = h;
    a.n_taps = n_taps; a.up = up; a.down = down; a.lp = (int)((((long)n_taps + up - 1) / up) | 1); a.C = C; a.out = out; a.ldo = ldo;
    a.tiles = (unsigned)((M1 - M0 + T2S_RESAMPLE_TILE - 1) / T2S_RESAMPLE_TILE);
    T2S_CHECK_HIP(is_half ? dv_launch_resample<_Float16>(a, B, (hipStream_t)stream) : dv_launch_resample<float>(a, B, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_limit_window_carry(int lookahead, int half_width) {
    if (lookahead < 0 || lookahead > LM_MAX_L || half_width < 1 || half_width > LM_MAX_HW) return -1;
    return 2 * (2 * lookahead + half_width);
}

long t2s_limit_window_end(long N1, long O0, int lookahead, int half_width, int final) {
    if (N1 < 0 || N1 > DV_MAX_POS || O0 < 0 || t2s_limit_window_carry(lookahead, half_width) < 0) return -1;
    const long O1 = final ? N1 : N1 - (2 * lookahead + half_width);
    return O1 > O0 ? O1 : O0;
}

int t2s_limit_window(const float* carry_in, float* carry_out, const void* piece, int is_half, int B, long n, long ldp, long N0, long O0,
                     int final, const double* gains, const double* h, int n_taps, int os, int half_width, const double* w,
                     int lookahead, double ceiling, float* out, long out_cap, long ldo, void* state, void* stream) {
    if (!state || !aligned_to(state, 8) || !lm_params_ok(gains, h, n_taps, os, half_width, w, lookahead, ceiling)) return T2S_EINVAL;
    const int C = t2s_limit_window_carry(lookahead, half_width);
    if (!dv_rows_ok(carry_in, carry_out, piece, is_half, B, n, ldp, N0, O0, C, out, ldo)) return T2S_EINVAL;
    const long O1 = t2s_limit_window_end(N0 + n, O0, lookahead, half_width, final);
    if (O1 < 0 || O0 > N0 + n || (O1 > O0 && !out) || O1 - O0 > out_cap || O1 - O0 > ldo || O1 - O0 > 0x7fffffffL) return T2S_EINVAL;
    LmWindowArgs a;
    memset(&a, 0, sizeof(a));
    a.carry_in = carry_in; a.carry_out = carry_out; a.piece = piece; a.n = n; a.ldp = ldp; a.N0 = N0; a.O0 = O0; a.O1 = O1;
    a.gains = gains; a.h = h; a.w = w; a.c = ceiling; a.hw = half_width; a.L = lookahead; a.C = C; a.out = out; a.ldo = ldo;
    a.state = (unsigned long long*)state;
    a.tiles = (unsigned)((O1 - O0 + LM_TILE - 1) / LM_TILE);
    T2S_CHECK_HIP(is_half ? dv_launch_limit<_Float16>(a, os, B, (hipStream_t)stream) : dv_launch_limit<float>(a, os, B, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_g711(const short* pcm, long n, int law, unsigned char* out, void* stream) {
    if (!pcm || !out || !aligned_to(pcm, 2) || n <= 0 || n > DV_MAX_POS || (law != 0 && law != 1)) return T2S_EINVAL;
    hipLaunchKernelGGL(g711_kernel, dim3((unsigned)((n + DV_THREADS - 1) / DV_THREADS)), dim3(DV_THREADS), 0, (hipStream_t)stream, pcm, n,
                       law, out);
    T2S_CHECK_HIP(hipGetLastError());
    return T2S_OK;
}

}  // extern "C"
