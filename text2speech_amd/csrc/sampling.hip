// Counter-based random draws keyed by a per-entry seed (include/t2s_hip.h, "keyed sampling"): the prenet dropout masks of a batch of
// texts and the Gaussian noise of a batch of mels, each value a function of (the entry's seed, the element's index inside the entry)
// and of nothing else - not of the batch size, the entry's place in the batch, the padded length or any generator state.  So an
// entry draws the same bits alone and in any batch.  Three kernels, one launch each, and their extern "C" entry points:
//
//   bernoulli_mask_keyed_kernel   mask[t][b][j] = what bernoulli_mask_kernel (tacotron_ops.hip) stores at index t row + j under the
//                                 seed seeds[b]: the same hash, the same 24 bits against the same threshold
//   wg_noise_keyed_kernel         z[b][c][t] = sigma_b * (float)n, n a unit Gaussian by Box-Muller in double precision from two
//                                 hashed 53-bit uniforms per column pair (2 q, 2 q + 1): the cosine branch on the even column, the
//                                 sine branch on the odd one.  One thread makes both members of a pair and stores them together.
//   wg_noise_keyed_at_kernel      the same values for a window of the utterance's columns: z[b][c][j] = what the kernel above stores
//                                 at column c0_b + j (streaming.py: a window of a mel vocoded alone).  Both call wg_noise_pair.
//
// Both are elementwise and launch bound at the sizes they serve (2 M floats for 1000 mel frames): a workgroup of the noise kernel
// makes T2S_NOISE_TILE columns of one (entry, channel) row, two pairs per thread 256 pairs apart, so that a wave's stores are
// contiguous - 8 bytes per lane where the row starts on an 8-byte boundary (L even, or an even row), two 4-byte stores otherwise.
//
// Memory safety: the mask kernel writes index (t B + b) row + j for t row + j < n_steps row only; the noise kernel columns t < L of
// row b G + c only (the window form: j < L of that row, and j >= 0 - the member of a pair that lies outside the window is dropped);
// all read seeds[b] (and sigmas[b], col0s[b]) for b < B = gridDim.  All of it in 64-bit.
#include "../../include/t2s_hip.h"
#include "t2s_api_common.h"

#include <math.h>

typedef unsigned long long u64;

#define SM_THREADS 256
#define NZ_PAIRS 2                                          // column pairs per thread
#define T2S_NOISE_TILE (SM_THREADS * NZ_PAIRS * 2)          // columns of one row per workgroup: 1024

#define SM_GOLD 0x9E3779B97F4A7C15ull
#define SM_NOISE_DOMAIN 0x5741564547ull                     // keeps the noise keys apart from the mask hash under one user seed

// splitmix64's finaliser, as in bernoulli_mask_kernel
static __device__ __forceinline__ u64 sm_mix(u64 x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(SM_THREADS) void bernoulli_mask_keyed_kernel(unsigned char* mask, size_t n, int B, int row, const u64* seeds,
                                                                          unsigned int keep_thr) {
    const size_t i = (size_t)blockIdx.x * SM_THREADS + threadIdx.x;       // t row + j: the entry's own flat index
    if (i >= n) return;
    const int b = blockIdx.y;
    const u64 x = sm_mix(i * SM_GOLD + seeds[b]);
    const size_t t = i / (size_t)row, j = i - t * (size_t)row;
    mask[(t * (size_t)B + b) * (size_t)row + j] = (unsigned char)(((unsigned int)(x >> 40)) < keep_thr);
}

// One Box-Muller pair: the draws of columns (2 q, 2 q + 1) of channel c under the entry's key, scaled.  Both noise kernels call it,
// so a column's value cannot depend on which of them made it.
static __device__ __forceinline__ void wg_noise_pair(int c, long q, u64 key, float sg, float& n0, float& n1) {
    const u64 p = ((u64)c << 40) | (u64)q;
    const u64 ha = sm_mix((2 * p) * SM_GOLD + key), hb = sm_mix((2 * p + 1) * SM_GOLD + key);
    const double u1 = (double)((ha >> 11) + 1) * 0x1p-53;             // (0, 1]
    const double u2 = (double)(hb >> 11) * 0x1p-53;                   // [0, 1)
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    n0 = sg * (float)(r * cs);
    n1 = sg * (float)(r * sn);
}

__global__ __launch_bounds__(SM_THREADS) void wg_noise_keyed_kernel(float* z, int G, long L, const u64* seeds, float sigma,
                                                                    const float* sigmas) {
    const int c = blockIdx.y, b = blockIdx.z;
    const u64 key = sm_mix(seeds[b] * SM_GOLD + SM_NOISE_DOMAIN);
    const float sg = sigmas ? sigmas[b] : sigma;
    float* out = z + ((size_t)b * G + c) * (size_t)L;
    const bool pair_store = ((uintptr_t)out & 7) == 0;
    const long q0 = (long)blockIdx.x * (T2S_NOISE_TILE / 2) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < NZ_PAIRS; ++u) {
        const long q = q0 + u * SM_THREADS, t = 2 * q;
        if (t >= L) return;
        float n0, n1;
        wg_noise_pair(c, q, key, sg, n0, n1);
        if (t + 1 < L) {
            if (pair_store) *reinterpret_cast<float2*>(out + t) = make_float2(n0, n1);
            else { out[t] = n0; out[t + 1] = n1; }
        } else {
            out[t] = n0;
        }
    }
}

// The window form: z[b][c][j] is column c0 + j of the utterance, c0 = col0s[b] where given, else col0.  Pairs are those of the
// utterance's columns, so an odd c0 puts the cosine member of the first pair in front of the window and an even last column the sine
// member of the last pair behind it: each member is stored only where 0 <= j < L.  A workgroup makes the T2S_NOISE_TILE / 2 pairs
// from floor(c0 / 2) + blockIdx.x * (T2S_NOISE_TILE / 2) on; the grid covers floor(L / 2) + 1 pairs, the most a window of L columns
// can touch.
__global__ __launch_bounds__(SM_THREADS) void wg_noise_keyed_at_kernel(float* z, int G, long L, long col0, const long long* col0s,
                                                                       const u64* seeds, float sigma, const float* sigmas) {
    const int c = blockIdx.y, b = blockIdx.z;
    const u64 key = sm_mix(seeds[b] * SM_GOLD + SM_NOISE_DOMAIN);
    const float sg = sigmas ? sigmas[b] : sigma;
    const long c0 = col0s ? (long)col0s[b] : col0;
    float* out = z + ((size_t)b * G + c) * (size_t)L;
    const long q0 = (c0 >> 1) + (long)blockIdx.x * (T2S_NOISE_TILE / 2) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < NZ_PAIRS; ++u) {
        const long q = q0 + u * SM_THREADS, j = 2 * q - c0;          // j >= -1
        if (j >= L) return;
        float n0, n1;
        wg_noise_pair(c, q, key, sg, n0, n1);
        if (j >= 0 && j + 1 < L && (((uintptr_t)(out + j)) & 7) == 0) {
            *reinterpret_cast<float2*>(out + j) = make_float2(n0, n1);
        } else {
            if (j >= 0) out[j] = n0;
            if (j + 1 < L) out[j + 1] = n1;
        }
    }
}

extern "C" {

int t2s_bernoulli_mask_keyed(unsigned char* mask, int n_steps, int B, int row, const unsigned long long* seeds, float keep_prob,
                             void* stream) {
    if (!mask || !seeds || n_steps <= 0 || B <= 0 || row <= 0 || B > 65535 || !(keep_prob > 0.f && keep_prob <= 1.f)) return T2S_EINVAL;
    const size_t n = (size_t)n_steps * (size_t)row;
    const size_t tiles = (n + SM_THREADS - 1) / SM_THREADS;
    if (tiles > 0x7fffffffull) return T2S_EINVAL;
    const unsigned int thr = (unsigned int)(keep_prob * 16777216.0f);     // as t2s_bernoulli_mask's
    hipLaunchKernelGGL(bernoulli_mask_keyed_kernel, dim3((unsigned)tiles, B), dim3(SM_THREADS), 0, (hipStream_t)stream, mask, n, B, row,
                       seeds, thr);
    T2S_CHECK_HIP(hipGetLastError());
    return T2S_OK;
}

int t2s_noise_tile(void) { return T2S_NOISE_TILE; }

int t2s_wg_noise_keyed(float* z, int B, int G, long L, const unsigned long long* seeds, float sigma, const float* sigmas, void* stream) {
    if (!z || !seeds || B <= 0 || G <= 0 || L <= 0 || B > 65535 || G > 65535 || L >= (1L << 40)) return T2S_EINVAL;
    if (!(sigma >= 0.f) || isinf(sigma)) return T2S_EINVAL;               // NaN too
    if ((size_t)B * (size_t)G > ((size_t)1 << 60) / (size_t)L) return T2S_EINVAL;       // B G L elements: no such buffer
    const long tiles = (L + T2S_NOISE_TILE - 1) / T2S_NOISE_TILE;         // < 2^30
    hipLaunchKernelGGL(wg_noise_keyed_kernel, dim3((unsigned)tiles, G, B), dim3(SM_THREADS), 0, (hipStream_t)stream, z, G, L, seeds, sigma,
                       sigmas);
    T2S_CHECK_HIP(hipGetLastError());
    return T2S_OK;
}

int t2s_wg_noise_keyed_at(float* z, int B, int G, long L, long col0, const long long* col0s, const unsigned long long* seeds, float sigma,
                          const float* sigmas, void* stream) {
    if (!z || !seeds || B <= 0 || G <= 0 || L <= 0 || B > 65535 || G > 65535 || L >= (1L << 40)) return T2S_EINVAL;
    if (!(sigma >= 0.f) || isinf(sigma)) return T2S_EINVAL;               // NaN too
    if ((size_t)B * (size_t)G > ((size_t)1 << 60) / (size_t)L) return T2S_EINVAL;
    if (col0 < 0 || col0 >= (1L << 40) - L) return T2S_EINVAL;            // col0 + L >= 2^40: the pair index has 39 bits
    const long tiles = (L / 2 + 1 + T2S_NOISE_TILE / 2 - 1) / (T2S_NOISE_TILE / 2);     // < 2^30
    hipLaunchKernelGGL(wg_noise_keyed_at_kernel, dim3((unsigned)tiles, G, B), dim3(SM_THREADS), 0, (hipStream_t)stream, z, G, L, col0,
                       col0s, seeds, sigma, sigmas);
    T2S_CHECK_HIP(hipGetLastError());
    return T2S_OK;
}

}  // extern "C"
