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
// [dst_start, dst_start + dst_cap) inside [0, dst_len) is written, whatever the table or lengths hold; all of it in 64-bit
// (csrc/pcm_rows.h).
//
// The phase table and the loop of one output are csrc/resample_tap.h's, which the stream's window kernel (csrc/delivery.hip) runs
// too.
#include "t2s_common.h"
#include "audio_ops.h"
#include "pcm_rows.h"
#include "resample_tap.h"

#include <limits.h>

static __device__ __forceinline__ void rs_put(short* p, double v) { *p = pcm_round16(v); }
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
    n_in = pcm_src_count(s0, n_in, a.src_len);
    cap = pcm_dst_cap(cap, a.max_out, d0, a.dst_len);
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
    rs_stage_phases(rs_hp, a.h, a.n_taps, a.up, a.lp, tid);

    const RsTile tile(m0, a.n_taps, a.up, a.down, a.lp);
    const RsRow<TSrc> row{(const TSrc*)a.src + s0, n_in};
    for (int o = tid; o < T2S_RESAMPLE_TILE; o += RS_THREADS) {
        const long m = m0 + o;
        if (m >= cap) break;
        rs_put(out + m, m < valid ? tile.output(o, row, rs_hp) : 0.0);
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
