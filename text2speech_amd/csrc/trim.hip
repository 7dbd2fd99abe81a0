// Peak rescaling and silence trimming of PCM in device memory: librosa.effects.trim's decision (frame RMS in dB below the clip's
// loudest frame) and the reference's `wav / abs(wav).max() * rescaling_max`, on a pool of clips or a padded batch
// (text2speech_amd/audio.py Trimmer, text2speech_amd/data.py PcmPool.rescale_trim).  Three kernels, one launch each:
//
//   trim_energy_kernel   rows (src_start, src_count, energy_start): every frame's energy E_f = sum of the squares of the fl padded
//                        samples from f h on (reflect or zero padding by fl / 2 at both ends) as a double into a scratch, and per
//                        row max |x| and max_f E_f into a [n_rows][2] double table
//   trim_bounds_kernel   (start, end) per row: the first and last frame with max(E_f, F) > rho max(E_max, F), times the hop
//   trim_gather_kernel   rows (src_start, src_count, dst_start, dst_cap): the kept range, rescaled, +0 behind it up to dst_cap
//
// Energy pass: a workgroup makes T2S_TRIM_TILE consecutive frames of one row.  It stages the samples under as many of them as fit
// (TR_LDS_FLOATS, always at least one frame) in LDS as floats - the padding is applied there, every sample comes from global memory
// once per chunk, coalesced - and then each wave sums one frame at a time: lane l adds the squares of samples l, l + 64, ... in
// ascending order in double, and the 64 partial sums are combined by an xor butterfly (32, 16, ..., 1).  The order depends on the
// frame length alone - not on the chunk, the tile, the row or the place in the pool - so a clip's energies are the same bits alone
// and in any batch; int16 sums are integers below 2^53 and therefore exact.  The peak is taken over each workgroup's own stretch
// of the row, T2S_TRIM_TILE hop samples (the row's last workgroup takes what is left), so that samples under no frame count too.
// Both maxima go to the table with one 64-bit integer atomic max per wave on the doubles' bits (non-negative doubles order as
// integers; a non-finite sample counts as +inf, a NaN energy's bits lie above +inf's): order independent, no waits.
//
// Memory safety: src_count is cut to what lies inside [0, src_len), the frame count to max_frames and to what the scratch holds
// behind energy_start, the destination to [dst_start, dst_start + dst_cap) inside [0, dst_len), bounds to [0, src_count]; all of it
// in 64-bit, whatever the tables hold (csrc/pcm_rows.h).
#include "t2s_common.h"
#include "audio_ops.h"
#include "pcm_rows.h"

#include <limits.h>
#include <math.h>

#define TR_THREADS 256
#define TR_WAVES (TR_THREADS / 64)
#define TR_UNROLL 8                             // samples a thread has in flight while it stages or scans
#define TR_LDS_FLOATS 10240                     // 40 KB: four workgroups per CU; >= the longest frame (T2S_TRIM_MAX_FRAME)
#define TR_GATHER_TILE 2048                     // outputs of one row per workgroup of the gather

static_assert(TR_LDS_FLOATS >= T2S_TRIM_MAX_FRAME, "one frame must fit");

// frames of a row of n samples that the scratch holds: 1 + (n + 2 pad - fl) / h, none for a reflect row of at most pad samples
static __device__ __forceinline__ long tr_frames(long n, int fl, int h, int reflect, long e0, long energy_len, long max_frames) {
    const int pad = fl / 2;
    if (n <= 0 || (reflect && n <= pad) || e0 < 0 || e0 >= energy_len) return 0;
    long nf = 1 + (n + 2 * pad - fl) / h;
    if (nf > max_frames) nf = max_frames;
    if (nf > energy_len - e0) nf = energy_len - e0;
    return nf;
}

static __device__ __forceinline__ double tr_wave_max(double v) {
    for (int off = 32; off; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

static __device__ __forceinline__ double tr_abs(float v) {
    const double a = fabs((double)v);
    return a < (double)INFINITY ? a : (double)INFINITY;          // NaN too
}

template <typename TSrc>
__global__ __launch_bounds__(TR_THREADS) void trim_energy_kernel(const TrimEnergyArgs a) {
    __shared__ float lds[TR_LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.y;
    const long* t = a.table + 3 * (size_t)r;
    const long s0 = t[0], e0 = t[2];
    const long n = pcm_src_count(s0, t[1], a.src_len);
    const int fl = a.frame_length, h = a.hop, pad = fl / 2, reflect = a.reflect;
    const long nf = a.energy ? tr_frames(n, fl, h, reflect, e0, a.energy_len, a.max_frames) : 0;
    const TSrc* x = (const TSrc*)a.src + (n > 0 ? s0 : 0);
    unsigned long long* stats = (unsigned long long*)a.stats + 2 * (size_t)r;

    if (blockIdx.x == 0 && tid == 0 && reflect && n > 0 && n <= pad) ((double*)stats)[1] = -1.0;      // the flag: no frames

    // ---- the peak over this workgroup's own stretch of the row ----
    const long span = (long)T2S_TRIM_TILE * h;
    const long p_lo = (long)blockIdx.x * span;
    const long p_hi = (blockIdx.x + 1 == gridDim.x || n - p_lo <= span) ? n : p_lo + span;
    double peak = 0.0;
    for (long s = p_lo + tid; s < p_hi; s += TR_THREADS * TR_UNROLL) {       // TR_UNROLL independent loads in flight per thread
        float v[TR_UNROLL];
#pragma unroll
        for (int u = 0; u < TR_UNROLL; ++u) {
            const long su = s + (long)u * TR_THREADS;
            v[u] = (float)x[su < p_hi ? su : s];                // (a repeat of x[s] changes no maximum)
        }
#pragma unroll
        for (int u = 0; u < TR_UNROLL; ++u) peak = fmax(peak, tr_abs(v[u]));
    }
    peak = tr_wave_max(peak);
    if (lane == 0 && peak > 0.0) atomicMax(stats, (unsigned long long)__double_as_longlong(peak));

    // ---- the energies of frames f_lo .. f_hi ----
    const long f_lo = (long)blockIdx.x * T2S_TRIM_TILE;
    const long f_hi = nf - f_lo < T2S_TRIM_TILE ? nf : f_lo + T2S_TRIM_TILE;
    if (f_lo >= f_hi) return;
    int c = (TR_LDS_FLOATS - fl) / h + 1;                        // frames whose samples fit in LDS together
    if (c > T2S_TRIM_TILE) c = T2S_TRIM_TILE;
    unsigned long long e_max = 0;                                // (the same in every lane of a wave)
    for (long f0 = f_lo; f0 < f_hi; f0 += c) {
        const int fc = f_hi - f0 < c ? (int)(f_hi - f0) : c;
        const int cnt = (fc - 1) * h + fl;                       // <= TR_LDS_FLOATS
        const long j0 = f0 * h - pad;                            // the source index under lds[0]
        for (int i0 = tid; i0 < cnt; i0 += TR_THREADS * TR_UNROLL) {             // branch-free, so that the loads go out together
            float v[TR_UNROLL];
#pragma unroll
            for (int u = 0; u < TR_UNROLL; ++u) {
                long s = j0 + i0 + u * TR_THREADS;
                if (s < 0) s = reflect ? -s : -1;
                else if (s >= n) s = reflect ? 2 * (n - 1) - s : -1;
                const bool in = s >= 0 && s < n && i0 + u * TR_THREADS < cnt;
                const float t = (float)x[in ? s : 0];           // (n > 0 here: x[0] is the row's own)
                v[u] = in ? t : 0.f;
            }
#pragma unroll
            for (int u = 0; u < TR_UNROLL; ++u)
                if (i0 + u * TR_THREADS < cnt) lds[i0 + u * TR_THREADS] = v[u];
        }
        __syncthreads();
        for (int f = wave; f < fc; f += TR_WAVES) {
            const float* p = lds + f * h;
            double acc = 0.0;
            for (int j = lane; j < fl; j += 64) {
                const double v = (double)p[j];
                acc = fma(v, v, acc);
            }
            for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
            const unsigned long long bits = (unsigned long long)__double_as_longlong(acc);
            if (bits > e_max) e_max = bits;
            if (lane == 0) a.energy[e0 + f0 + f] = acc;
        }
        __syncthreads();
    }
    if (lane == 0 && e_max) atomicMax(stats + 1, e_max);
}

// The decision in double, without logarithms: frame f is loud iff max(E_f, F) > rho max(E_max, F), F = 1e-10 fl / g^2.
static __device__ __forceinline__ double tr_gain(double peak, int rescale, double rescaling_max, double peak_floor, double unit) {
    const double peak_eff = peak > peak_floor ? peak : peak_floor;
    return (rescale && peak_eff > 0.0) ? rescaling_max / peak_eff : unit;
}

__global__ __launch_bounds__(TR_THREADS) void trim_bounds_kernel(const TrimBoundsArgs a) {
    __shared__ long s_first[TR_THREADS], s_last[TR_THREADS];
    const int tid = threadIdx.x, r = blockIdx.x;
    const long* t = a.table + 3 * (size_t)r;
    const long e0 = t[2];
    const long n = pcm_src_count(t[0], t[1], a.src_len);
    const long nf = tr_frames(n, a.frame_length, a.hop, a.reflect, e0, a.energy_len, a.max_frames);
    const double peak = a.stats[2 * (size_t)r], e_max = a.stats[2 * (size_t)r + 1];
    long first = LONG_MAX, last = -1;
    if (e_max > 0.0 && e_max < (double)INFINITY && peak < (double)INFINITY) {           // no flag, not all zeros, no non-finite sample
        const double g = tr_gain(peak, a.rescale, a.rescaling_max, a.peak_floor, a.unit_gain);
        const double F = 1e-10 * (double)a.frame_length / (g * g);
        const double thr = a.rho * (e_max > F ? e_max : F);
        for (long f = tid; f < nf; f += TR_THREADS) {
            const double E = a.energy[e0 + f];
            if ((E > F ? E : F) > thr) {
                if (f < first) first = f;
                last = f;
            }
        }
    }
    s_first[tid] = first;
    s_last[tid] = last;
    __syncthreads();
    for (int w = TR_THREADS / 2; w; w >>= 1) {
        if (tid < w) {
            if (s_first[tid + w] < s_first[tid]) s_first[tid] = s_first[tid + w];
            if (s_last[tid + w] > s_last[tid]) s_last[tid] = s_last[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        long start = 0, end = 0;
        if (s_last[0] >= 0) {
            start = s_first[0] * a.hop;
            end = (s_last[0] + 1) * a.hop;
            if (end > n) end = n;
        }
        a.bounds[2 * (size_t)r] = start;
        a.bounds[2 * (size_t)r + 1] = end;
    }
}

static __device__ __forceinline__ void tr_put(short* p, short x, int scaled, double s) { *p = scaled ? pcm_round16((double)x * s) : x; }
static __device__ __forceinline__ void tr_put(float* p, float x, int scaled, double s) { *p = scaled ? (float)((double)x * s) : x; }
static __device__ __forceinline__ void tr_put(float* p, _Float16 x, int scaled, double s) { tr_put(p, (float)x, scaled, s); }

template <typename TSrc, typename TDst>
__global__ __launch_bounds__(TR_THREADS) void trim_gather_kernel(const TrimGatherArgs a) {
    const int tid = threadIdx.x, r = blockIdx.y;
    const long m0 = (long)blockIdx.x * TR_GATHER_TILE;
    const long* t = a.table + 4 * (size_t)r;
    long s0 = t[0];
    const long d0 = t[2], cap = pcm_dst_cap(t[3], a.max_out, d0, a.dst_len);
    long n = pcm_src_count(s0, t[1], a.src_len);
    if (a.bounds) {                                             // the kept range of the row, cut to the row
        long b0 = a.bounds[2 * (size_t)r], b1 = a.bounds[2 * (size_t)r + 1];
        if (b0 < 0) b0 = 0;
        if (b0 > n) b0 = n;
        if (b1 > n) b1 = n;
        if (b1 < b0) b1 = b0;
        s0 += b0;
        n = b1 - b0;
    }
    const long valid = n < cap ? n : cap;
    if (blockIdx.x == 0 && tid == 0 && a.out_lengths) a.out_lengths[r] = valid > INT_MAX ? INT_MAX : (int)valid;
    if (m0 >= cap) return;
    int scaled = 0;
    double s = 1.0;
    if (a.stats) {
        const double peak = a.stats[2 * (size_t)r];
        const double peak_eff = peak > a.peak_floor ? peak : a.peak_floor;
        if (peak_eff > 0.0) {
            scaled = 1;
            s = a.scale_num / peak_eff;                         // one division; then one product and one rounding per sample
        }
    }
    const TSrc* x = (const TSrc*)a.src + (n > 0 ? s0 : 0);
    TDst* out = (TDst*)a.dst + d0;
    for (int o = tid; o < TR_GATHER_TILE; o += TR_THREADS) {
        const long m = m0 + o;
        if (m >= cap) break;
        if (m < valid) tr_put(out + m, x[m], scaled, s);
        else out[m] = (TDst)0;
    }
}

hipError_t t2s_launch_trim_energy(const TrimEnergyArgs& a, int src_kind, int n_rows, hipStream_t s) {
    const long tiles = (a.max_frames + T2S_TRIM_TILE - 1) / T2S_TRIM_TILE;
    if (tiles < 1 || tiles > 0x7fffffffL) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.stats, 0, (size_t)n_rows * 2 * sizeof(double), s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)tiles, n_rows), block(TR_THREADS);
    switch (src_kind) {
        case 0: hipLaunchKernelGGL(trim_energy_kernel<short>, grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL(trim_energy_kernel<float>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(trim_energy_kernel<_Float16>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t t2s_launch_trim_bounds(const TrimBoundsArgs& a, int n_rows, hipStream_t s) {
    hipLaunchKernelGGL(trim_bounds_kernel, dim3(n_rows), dim3(TR_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t t2s_launch_trim_gather(const TrimGatherArgs& a, int src_kind, int dst_kind, int n_rows, hipStream_t s) {
    const long tiles = (a.max_out + TR_GATHER_TILE - 1) / TR_GATHER_TILE;
    if (tiles < 1 || tiles > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, n_rows), block(TR_THREADS);
    switch (src_kind * 2 + dst_kind) {
        case 0: hipLaunchKernelGGL((trim_gather_kernel<short, short>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((trim_gather_kernel<float, float>), grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL((trim_gather_kernel<_Float16, float>), grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
