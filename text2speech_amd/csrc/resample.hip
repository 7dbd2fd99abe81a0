// Sample-rate conversion by a rational factor up / down: the polyphase FIR of scipy.signal.resample_poly (zero extension, the
// caller's filter h of n_taps = 2 half + 1 doubles), on a pool of clips or a padded batch (text2speech_amd/audio.py Resampler,
// text2speech_amd/data.py PcmPool.resample).
//
//   y[m] = sum_k x[k] h[half + m down - k up]      over 0 <= k < n_in with the tap index inside [0, n_taps)
//
// One kernel for every form, templated on the source (int16 / f32 / f16) and destination (int16 / f32) types.  A workgroup makes
// T2S_RESAMPLE_TILE consecutive outputs of one row.  The tap index of output m walks h with stride up, always in the residue class
// p = (half + m down) mod up, so the workgroup first copies h into LDS phase by phase - hp[p][i] = h[p + i up], rows lp = odd
// doubles apart - and an output then reads one row of it at unit stride while k runs over consecutive input samples.  Inputs are
// read from global memory: neighbouring lanes read neighbouring samples and each sample serves about n_taps / max(up, down)
// outputs of the tile out of the vector L1.
//
// Every output is one loop of its own: k ascending, one double-precision fused multiply-add per tap (the product is not rounded),
// starting from +0.  The loop depends on (m, n_in, the filter) only - not on the tile, the row or the place in the pool - so a
// clip's bits are the same alone and in any batch, and the int16 result is the rounding of the float64 sum.
//
// Memory safety: a row's (src_start, src_count, dst_start, dst_cap) are clamped so that only [0, src_len) is read and only
// [dst_start, dst_start + dst_cap) inside [0, dst_len) is written, whatever the table or lengths hold; all of it in 64-bit.
#include "t2s_common.h"
#include "audio_ops.h"

#include <limits.h>

#define RS_THREADS 256

static __device__ __forceinline__ void rs_put(short* p, double v) {
    const double r = rint(v);                               // ties to even
    short s = 0;                                            // NaN
    if (r >= 32767.0) s = 32767;
    else if (r <= -32768.0) s = -32768;
    else if (r == r) s = (short)(int)r;
    *p = s;
}
static __device__ __forceinline__ void rs_put(float* p, double v) { *p = (float)v; }      // one rounding

template <typename TSrc, typename TDst>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs a) {
    extern __shared__ double rs_hp[];
    const int tid = threadIdx.x, r = blockIdx.y;
    const long m0 = (long)blockIdx.x * T2S_RESAMPLE_TILE;
    long s0, n_in, d0, cap;
    if (a.table) {
        const long* t = a.table + 4 * (size_t)r;
        s0 = t[0]; n_in = t[1]; d0 = t[2]; cap = t[3];
    } else {
        s0 = (long)r * a.ldx;
        n_in = a.lengths ? (long)a.lengths[r] : a.N;
        if (n_in > a.N) n_in = a.N;
        d0 = (long)r * a.ldo;
        cap = a.N_out;
    }
    if (n_in < 0 || s0 < 0 || s0 >= a.src_len) n_in = 0;
    else if (n_in > a.src_len - s0) n_in = a.src_len - s0;
    if (cap > a.max_out) cap = a.max_out;
    if (cap < 0 || d0 < 0 || d0 >= a.dst_len) cap = 0;
    else if (cap > a.dst_len - d0) cap = a.dst_len - d0;
    const long up = a.up, down = a.down;
    const long n_out = n_in > (LONG_MAX - down) / up ? LONG_MAX : (n_in * up + down - 1) / down;
    const long valid = n_out < cap ? n_out : cap;
    if (blockIdx.x == 0 && tid == 0 && a.out_lengths) a.out_lengths[r] = valid > INT_MAX ? INT_MAX : (int)valid;
    if (m0 >= cap) return;

    TDst* out = (TDst*)a.dst + d0;
    if (m0 >= valid) {                                      // a tile behind the row's end: +0 up to dst_cap
        for (int o = tid; o < T2S_RESAMPLE_TILE && m0 + o < cap; o += RS_THREADS) out[m0 + o] = (TDst)0;
        return;
    }
    const int n_taps = a.n_taps, lp = a.lp;
    for (int j = tid; j < n_taps; j += RS_THREADS) rs_hp[(j % a.up) * lp + j / a.up] = a.h[j];
    __syncthreads();

    const int L = (n_taps + a.up - 1) / a.up;               // taps of the longest phase
    const long c0 = (long)(n_taps / 2) + m0 * down;         // h's index under input sample 0, for output m0
    const long q0 = c0 / up;
    const unsigned r0 = (unsigned)(c0 % up);
    const TSrc* x = (const TSrc*)a.src + s0;
    for (int o = tid; o < T2S_RESAMPLE_TILE; o += RS_THREADS) {
        const long m = m0 + o;
        if (m >= cap) break;
        double acc = 0.0;
        if (m < valid) {
            const unsigned e = r0 + (unsigned)o * (unsigned)a.down;          // < 512 + 1023 * 512
            const unsigned p = e % (unsigned)a.up;
            const long kc = q0 + e / (unsigned)a.up;                          // the sample under tap p; tap p + i up is under kc - i
            const int cnt = L - ((long)p + (long)(L - 1) * up >= n_taps ? 1 : 0);
            const long k_lo = kc - (cnt - 1) > 0 ? kc - (cnt - 1) : 0;
            const long k_hi = kc < n_in - 1 ? kc : n_in - 1;
            const double* hrow = rs_hp + (size_t)p * lp;
            for (long k = k_lo; k <= k_hi; ++k) acc = fma((double)x[k], hrow[kc - k], acc);
        }
        rs_put(out + m, acc);
    }
}

int t2s_resample_lds_bytes(int n_taps, int up) {
    const long L = ((long)n_taps + up - 1) / up;
    const long bytes = (long)up * (L | 1) * (long)sizeof(double);
    return bytes > INT_MAX ? INT_MAX : (int)bytes;
}

template <typename TSrc, typename TDst>
static hipError_t rs_launch(const ResampleArgs& a, int n_rows, hipStream_t s) {
    static std::atomic<unsigned long long> attr_mask{0};        // per instantiation; bit d = raised on device d
    const hipError_t e = t2s_raise_lds_limit((const void*)resample_kernel<TSrc, TDst>, T2S_RESAMPLE_LDS_MAX, attr_mask);
    if (e != hipSuccess) return e;
    const long tiles = (a.max_out + T2S_RESAMPLE_TILE - 1) / T2S_RESAMPLE_TILE;
    hipLaunchKernelGGL((resample_kernel<TSrc, TDst>), dim3((unsigned)tiles, n_rows), dim3(RS_THREADS),
                       (size_t)t2s_resample_lds_bytes(a.n_taps, a.up), s, a);
    return hipGetLastError();
}

hipError_t t2s_launch_resample(const ResampleArgs& args, int src_kind, int dst_kind, int n_rows, hipStream_t s) {
    ResampleArgs a = args;
    a.lp = (int)((((long)a.n_taps + a.up - 1) / a.up) | 1);
    const long tiles = (a.max_out + T2S_RESAMPLE_TILE - 1) / T2S_RESAMPLE_TILE;
    if (tiles > 0x7fffffffL || t2s_resample_lds_bytes(a.n_taps, a.up) > T2S_RESAMPLE_LDS_MAX) return hipErrorInvalidValue;
    switch (src_kind * 2 + dst_kind) {
        case 0: return rs_launch<short, short>(a, n_rows, s);
        case 1: return rs_launch<short, float>(a, n_rows, s);
        case 2: return rs_launch<float, short>(a, n_rows, s);
        case 3: return rs_launch<float, float>(a, n_rows, s);
        case 4: return rs_launch<_Float16, short>(a, n_rows, s);
        case 5: return rs_launch<_Float16, float>(a, n_rows, s);
    }
    return hipErrorInvalidValue;
}
