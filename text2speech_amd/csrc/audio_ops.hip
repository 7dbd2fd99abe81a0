// Audio front-end / back-end on device: the reference's STFT-as-conv1d (utils/stft.py:72-129),
// TacotronSTFT.mel_spectrogram (utils/layers.py:63-79) and the Denoiser's spectral subtraction (waveglow/denoiser.py:34-40).
//
// The two contractions (frames x windowed Fourier basis, mel basis x magnitudes, and the inverse basis) go through
// t2s_gemv: overlapping frames are just "items" whose stride is the hop, so no frame matrix is ever materialised, and at
// 9+ frames the products run on the f32 matrix cores (sbgemm.hip) - exact f32, which log-mel of quiet bands needs.
// What is left here is the bandwidth-bound glue: reflect padding, magnitude / phase, recombination (with the optional
// bias subtraction of the denoiser fused), overlap-add with the window-sum-square normalisation, log-clamp.
#include "t2s_common.h"
#include "t2s_kernels.h"
#include "audio_ops.h"

// ---- a padded batch whose entry b holds lengths[b] samples / frames[b] frames (device int32 [B]) ---------------------------------
// Every stage below is one kernel whose `lengths` / `frames` may be NULL: then each entry's extent is the batch's (T samples,
// F frames).  With a pointer, an element below the entry's end gets the same expression evaluated on the entry's own extent;
// behind the end the kernel stores +0 (outputs) or nothing (scratch) and loads nothing.  The device values are clamped to the range
// the entry point has validated on the host copy, so an array that disagrees with its host copy cannot move an address out of a
// buffer.
static __device__ __forceinline__ int clamp_len(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// xp[b][i] = x[b][reflect(i - pad)] about sample len - 1, i in [0, len + 2 pad), len = lengths ? lengths[b] : T; the rest of the row
// is left alone   (F.pad(..., mode='reflect'), utils/stft.py:79-83)
__global__ void reflect_pad_kernel(const float* __restrict__ x, int T, const int* __restrict__ lengths, int pad,
                                   float* __restrict__ xp, long ldp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    const int len = lengths ? clamp_len(lengths[b], pad + 1, T) : T;
    if (i >= len + 2 * pad) return;
    int j = i - pad;
    if (j < 0) j = -j;
    if (j >= len) j = 2 * (len - 1) - j;
    xp[(size_t)b * ldp + i] = x[(size_t)b * T + j];
}

// ft [B][F][ld_ft] (real rows 0..c-1, imaginary rows c..2c-1)  ->  mag, phase [B][c][F]  and  magT [B*F][ld_mt] (zero padded);
// with lengths, for f < lengths[b] / hop + 1, and +0 in mag, phase and magT behind (ft is not read there)
__global__ void stft_mag_phase_kernel(const float* __restrict__ ft, int F, int c, long ld_ft, const int* __restrict__ lengths,
                                      int hop, int T, int pad, float* __restrict__ mag, float* __restrict__ phase,
                                      float* __restrict__ magT, long ld_mt) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;       // bin (or padding column of magT)
    const int f = blockIdx.y, b = blockIdx.z;
    if (k >= ld_mt && k >= c) return;
    const bool live = !lengths || f < clamp_len(lengths[b], pad + 1, T) / hop + 1;
    float m = 0.f;
    if (k < c) {
        float ph = 0.f;
        if (live) {
            const float* row = ft + ((size_t)b * F + f) * ld_ft;
            const float re = row[k], im = row[c + k];
            // the pinned rounding of the magnitude: im * im rounded, then one fused multiply-add.  Written `re * re + im * im` the
            // compiler is free to round both squares (a packed multiply), which moves the last bit of one magnitude in fifty
            m = sqrtf(__builtin_fmaf(re, re, im * im));
            if (phase) ph = atan2f(im, re);
        }
        if (mag) mag[((size_t)b * c + k) * F + f] = m;
        if (phase) phase[((size_t)b * c + k) * F + f] = ph;
    }
    if (magT && k < ld_mt) magT[((size_t)b * F + f) * ld_mt + k] = m;
}

// rc[b*F + f][k] = k < c ? m cos(ph) : k < 2c ? m sin(ph) : 0,  m = max(mag - strength * bias[k], 0) when bias is given
// (utils/stft.py:102-103; waveglow/denoiser.py:36-38); with frames, for f < frames[b]: behind, mag and phase are not read and rc
// (scratch) is not written
__global__ void stft_recombine_kernel(const float* __restrict__ mag, const float* __restrict__ phase, int F, int c,
                                      const int* __restrict__ frames, const float* __restrict__ bias, float strength,
                                      float* __restrict__ rc, long ld_rc) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y, b = blockIdx.z;
    if (k >= ld_rc || (frames && f >= clamp_len(frames[b], 2, F))) return;
    float v = 0.f;
    if (k < 2 * c) {
        const int bin = k < c ? k : k - c;
        const size_t i = ((size_t)b * c + bin) * F + f;
        float m = mag[i];
        if (bias) m = fmaxf(m - bias[bin] * strength, 0.f);
        const float ph = phase[i];
        v = k < c ? m * cosf(ph) : m * sinf(ph);
    }
    rc[((size_t)b * F + f) * ld_rc + k] = v;
}

// out[b][n] = scale / wss[p] * sum_f frames_buf[b][f][p - f hop],  p = n + n_fft/2,  wss[p] = sum_f win_sq[p - f hop]
// (conv_transpose1d overlap-add, window-sum-square normalisation where it exceeds tiny, trim: utils/stft.py:105-127), f below
// Fb = frames ? frames[b] : F (so in the window-sum-square too); +0 from sample hop (Fb - 1), which without frames is n_out
__global__ void stft_overlap_add_kernel(const float* __restrict__ frames_buf, const float* __restrict__ win_sq, int F,
                                        const int* __restrict__ frames, int n_fft, int hop, float scale, float tiny,
                                        float* __restrict__ out, int n_out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= n_out) return;
    const int Fb = frames ? clamp_len(frames[b], 2, F) : F;
    if (n >= hop * (Fb - 1)) {
        out[(size_t)b * n_out + n] = 0.f;
        return;
    }
    const int p = n + n_fft / 2;
    int f_lo = (p - n_fft + hop) / hop;            // ceil((p - n_fft + 1) / hop) for p - n_fft + 1 > 0
    if (p - n_fft + 1 <= 0) f_lo = 0;
    int f_hi = p / hop;
    if (f_hi > Fb - 1) f_hi = Fb - 1;
    float acc = 0.f, wss = 0.f;
    for (int f = f_lo; f <= f_hi; ++f) {
        const int j = p - f * hop;
        acc += frames_buf[((size_t)b * F + f) * n_fft + j];
        if (win_sq) wss += win_sq[j];
    }
    if (win_sq) {
        if (wss > tiny) acc /= wss;
        acc *= scale;
    }
    out[(size_t)b * n_out + n] = acc;
}

// x [B][n_mel][F] <- log(max(x, clip)) where clip > 0 (dynamic_range_compression, utils/audio_processing.py:78-84 with C = 1;
// clip <= 0: the product stays); with frames, for f < frames[b], and +0 behind (not read there).
// The logarithm in double, rounded once - a precision choice, not a repair: the device's logf is 1.6 units in the last place
// off at the clamp floor 1e-5 that every silent frame takes (-11.5129271 for -11.5129255; profiles/tail_kernel_tests.md);
// this form gives the nearest f32, which a test can pin bit for bit, and a mel spectrogram is a few thousand elements.
__global__ void log_clamp_kernel(float* x, int n_mel, int F, const int* __restrict__ frames, size_t n, float clip) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (frames) {
        const int f = (int)(i % (size_t)F), b = (int)(i / ((size_t)n_mel * F));
        if (f >= clamp_len(frames[b], 1, F)) {
            x[i] = 0.f;
            return;
        }
    }
    if (clip > 0.f) x[i] = (float)log((double)fmaxf(x[i], clip));
}

// out[b][n] = (int16) trunc(x[b][n] * 32768), saturated to [-32768, 32767], NaN -> 0; 0 at and behind lengths[b] (x is not read there).
// One element per thread and 2-byte stores: rows of odd N or odd ldx need no alignment beyond the element.
template <typename TIn>
__global__ void pcm16_kernel(const TIn* __restrict__ x, int N, long ldx, const int* __restrict__ lengths, short* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= N) return;
    short v = 0;
    if (!lengths || n < lengths[b]) {
        const float s = (float)x[(size_t)b * ldx + n] * 32768.f;          // exact: a power of two
        if (s >= 32767.f) v = 32767;
        else if (s <= -32768.f) v = -32768;
        else if (s == s) v = (short)(int)s;                                // (int) truncates toward zero
    }
    out[(size_t)b * N + n] = v;
}

// ---- training batches from a pool of int16 clips (text2speech_amd/data.py) ------------------------------------------------------------
// out[b][t] = (float)pool[start_b + t] / max_wav for t < c_b, +0 for c_b <= t < N: t2s_pcm16's inverse, row b's samples taken at
// table[b] = (start, count).  c_b is count clamped to [0, N] and to what the pool holds behind start; a start outside the pool
// gives 0, so no table value moves a load out of [pool, pool + pool_len).
// A lane makes 8 consecutive outputs.  Their 16 source bytes begin at any 2-byte phase of a 16-byte granule, so the lane loads the
// two aligned granules that straddle them and shifts: whole words first (two conditional stages, no register indexing), then the odd
// half-word.  Where either granule crosses one of the pool's two ends the lane loads its valid samples one by one instead.  The
// stores are two float4 where the lane's 8 outputs are all inside the row and 16-byte aligned, single floats otherwise.
#define GATHER_PER_LANE 8
__global__ __launch_bounds__(256) void pcm16_gather_kernel(const short* __restrict__ pool, long pool_len, const long* __restrict__ table,
                                                            int N, float max_wav, float* __restrict__ out, long ldo) {
    const long first = ((long)blockIdx.x * 256 + threadIdx.x) * GATHER_PER_LANE;
    const int b = blockIdx.y;
    if (first >= N) return;
    const int t0 = (int)first;
    const long start = table[2 * (size_t)b], count = table[2 * (size_t)b + 1];
    long c = count < 0 ? 0 : (count > N ? (long)N : count);
    if (start < 0 || start >= pool_len) c = 0;
    else if (c > pool_len - start) c = pool_len - start;
    const int live = c - t0 >= GATHER_PER_LANE ? GATHER_PER_LANE : (c > t0 ? (int)(c - t0) : 0);      // samples this lane converts
    const int room = N - t0 >= GATHER_PER_LANE ? GATHER_PER_LANE : N - t0;                            // outputs this lane stores

    short v[GATHER_PER_LANE];
#pragma unroll
    for (int i = 0; i < GATHER_PER_LANE; ++i) v[i] = 0;
    if (live > 0) {
        const short* src = pool + start + t0;
        const uintptr_t a = (uintptr_t)src, a0 = a & ~(uintptr_t)15;
        const uintptr_t lo = (uintptr_t)pool, hi = lo + 2 * (uintptr_t)pool_len;
        if (a0 >= lo && a0 + 32 <= hi) {
            const uint4 g0 = *(const uint4*)a0, g1 = *(const uint4*)(a0 + 16);
            unsigned w[9] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, 0u};
            const unsigned phase = (unsigned)(a - a0) >> 1;                   // 0 .. 7 half-words into the first granule
            if (phase & 4) {
#pragma unroll
                for (int k = 0; k < 7; ++k) w[k] = w[k + 2];
            }
            if (phase & 2) {
#pragma unroll
                for (int k = 0; k < 5; ++k) w[k] = w[k + 1];
            }
            if (phase & 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] = (w[k] >> 16) | (w[k + 1] << 16);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[2 * k] = (short)(w[k] & 0xffffu);
                v[2 * k + 1] = (short)(w[k] >> 16);
            }
        } else {
#pragma unroll
            for (int i = 0; i < GATHER_PER_LANE; ++i)
                if (i < live) v[i] = src[i];
        }
    }
    float f[GATHER_PER_LANE];
#pragma unroll
    for (int i = 0; i < GATHER_PER_LANE; ++i) f[i] = i < live ? (float)v[i] / max_wav : 0.f;
    float* dst = out + (size_t)b * ldo + t0;
    if (room == GATHER_PER_LANE && ((uintptr_t)dst & 15) == 0) {
        ((float4*)dst)[0] = make_float4(f[0], f[1], f[2], f[3]);
        ((float4*)dst)[1] = make_float4(f[4], f[5], f[6], f[7]);
    } else {
#pragma unroll
        for (int i = 0; i < GATHER_PER_LANE; ++i)
            if (i < room) dst[i] = f[i];
    }
}

// gate[b][t] = 1 from frame frames[b] - 1 on, 0 in front (the reference's gate_padded[i, mel.size(1) - 1:] = 1, utils/data_utils.py:146):
// frames[b] <= 0 makes the row 1, frames[b] > T makes it 0
__global__ void gate_targets_kernel(const int* __restrict__ frames, int T, float* __restrict__ gate) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (t >= T) return;
    gate[(size_t)b * T + t] = t + 1 >= frames[b] ? 1.f : 0.f;
}

hipError_t t2s_launch_pcm16_gather(const short* pool, long pool_len, const long* table, int B, int N, float max_wav, float* out,
                                   long ldo, hipStream_t s) {
    const int per_block = 256 * GATHER_PER_LANE;
    hipLaunchKernelGGL(pcm16_gather_kernel, dim3((N + per_block - 1) / per_block, B), dim3(256), 0, s, pool, pool_len, table, N,
                       max_wav, out, ldo);
    return hipGetLastError();
}
hipError_t t2s_launch_gate_targets(const int* frames, int B, int T, float* gate, hipStream_t s) {
    hipLaunchKernelGGL(gate_targets_kernel, dim3((T + 255) / 256, B), dim3(256), 0, s, frames, T, gate);
    return hipGetLastError();
}

hipError_t t2s_launch_reflect_pad(const float* x, int B, int T, const int* lengths, int pad, float* xp, long ldp, hipStream_t s) {
    hipLaunchKernelGGL(reflect_pad_kernel, dim3((T + 2 * pad + 255) / 256, B), dim3(256), 0, s, x, T, lengths, pad, xp, ldp);
    return hipGetLastError();
}
hipError_t t2s_launch_stft_mag_phase(const float* ft, int B, int F, int c, long ld_ft, const int* lengths, int hop, int T, int pad,
                                     float* mag, float* phase, float* magT, long ld_mt, hipStream_t s) {
    const int cols = (int)(ld_mt > c ? ld_mt : c);
    hipLaunchKernelGGL(stft_mag_phase_kernel, dim3((cols + 255) / 256, F, B), dim3(256), 0, s, ft, F, c, ld_ft, lengths, hop, T, pad,
                       mag, phase, magT, magT ? ld_mt : 0);
    return hipGetLastError();
}
hipError_t t2s_launch_stft_recombine(const float* mag, const float* phase, int B, int F, int c, const int* frames, const float* bias,
                                     float strength, float* rc, long ld_rc, hipStream_t s) {
    hipLaunchKernelGGL(stft_recombine_kernel, dim3((unsigned)((ld_rc + 255) / 256), F, B), dim3(256), 0, s, mag, phase, F, c, frames,
                       bias, strength, rc, ld_rc);
    return hipGetLastError();
}
hipError_t t2s_launch_stft_overlap_add(const float* frames_buf, const float* win_sq, int B, int F, const int* frames, int n_fft,
                                       int hop, float scale, float tiny, float* out, int n_out, hipStream_t s) {
    hipLaunchKernelGGL(stft_overlap_add_kernel, dim3((n_out + 255) / 256, B), dim3(256), 0, s, frames_buf, win_sq, F, frames, n_fft,
                       hop, scale, tiny, out, n_out);
    return hipGetLastError();
}
hipError_t t2s_launch_log_clamp(float* x, int B, int n_mel, int F, const int* frames, float clip, hipStream_t s) {
    const size_t n = (size_t)B * n_mel * F;
    hipLaunchKernelGGL(log_clamp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n_mel, F, frames, n, clip);
    return hipGetLastError();
}
hipError_t t2s_launch_pcm16(const void* x, int is_half, int B, int N, long ldx, const int* lengths, short* out, hipStream_t s) {
    const dim3 grid((N + 255) / 256, B);
    if (is_half) hipLaunchKernelGGL(pcm16_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)x, N, ldx, lengths, out);
    else hipLaunchKernelGGL(pcm16_kernel<float>, grid, dim3(256), 0, s, (const float*)x, N, ldx, lengths, out);
    return hipGetLastError();
}
