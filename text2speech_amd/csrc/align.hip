// Looking at the attention alignments of a batch on the device: where every decoder frame attends, and per entry whether that path
// is the text - skips, backward jumps, stalls, an end that was never reached, a diffuse attention (text2speech_amd/alignment.py
// alignment_report, text2speech_amd/longform.py synthesize_long(check=)).  include/t2s_hip.h carries the definition; in short:
//
//   S_b = clamp(in_len[b], 1, T_in), F_b = clamp(out_len[b], 0, N).  Row pass, t < F_b: pos[b,t] the smallest j < S_b at which
//   A[b,t,j] is largest (scan from best = -inf, update on v > best: a NaN is never chosen), peak[b,t] that value as f32, bad[b,t]
//   whether any of the S_b values is not finite; t >= F_b: -1, 0, 0 and the row is not loaded.  Entry pass: the largest forward
//   and backward step of pos, the longest run of equal pos, the last pos, the frames per symbol (dur) and how many symbols have
//   any, the rows with a non-finite value, the mean peak in double, and the flag bits the thresholds make of those.
//
// Two kernels:
//
//   align_rows_kernel   one wave per row, T2S_ALIGN_ROWS rows per workgroup, the grid covers B N rows.  Lane l scans columns
//                       l, l + 64, ... (a coalesced load per step; every lane keeps the smallest column of its own maximum),
//                       then six exchanges reduce (value, column) across the wave, ties to the smaller column.  No LDS, no barrier.
//   align_stats_kernel  one workgroup per entry, T2S_ALIGN_BLOCK frames per step, one frame per thread.  A run's length needs the
//                       frame its run started at: the start frames (t where pos[t] != pos[t-1]) are scanned with a running maximum
//                       in LDS, and the last value is carried into the next step.  The peaks are summed in double, thread i over
//                       frames i, i + 256, ... in that order, then by a fixed tree over the 256 partial sums: the order depends on
//                       F_b alone.  dur is counted with integer atomics on the entry's own row, which the launcher zeroed on the
//                       same stream; the thread that finds a count at 0 counts the symbol as covered.  Integer maxima and sums
//                       meet in LDS atomics: exact in any order.
//
// Memory safety: both lengths are clamped; a row at or behind F_b and a column at or behind S_b are never read; the entry pass
// trusts no pos it reads (one outside [0, S_b) is counted in no dur) and differences of pos are formed in 64 bits.
#include "t2s_common.h"
#include "align_ops.h"

#include <limits.h>
#include <math.h>

static __device__ __forceinline__ int al_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static __device__ __forceinline__ bool al_not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

template <typename TSrc>
__global__ __launch_bounds__(64 * T2S_ALIGN_ROWS) void align_rows_kernel(const AlignRowsArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * T2S_ALIGN_ROWS + wave;
    if (r >= (long)a.B * a.N) return;                           // (wave-uniform; the kernel has no barrier)
    const int b = (int)(r / a.N), t = (int)(r % a.N);
    const int S = al_clamp(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const int F = al_clamp(a.out_len ? a.out_len[b] : a.N, 0, a.N);
    if (t >= F) {
        if (lane == 0) {
            a.pos[r] = -1;
            a.peak[r] = 0.f;
            a.bad[r] = 0;
        }
        return;
    }
    const TSrc* row = (const TSrc*)a.A + (size_t)b * a.ld_entry + (size_t)t * a.ld_row;
    float best = -INFINITY;
    int idx = INT_MAX;                                          // no column yet
    bool nf = false;
    for (long j = lane; j < S; j += 64) {
        const float v = (float)row[j];
        nf |= al_not_finite(v);
        if (v > best) {
            best = v;
            idx = (int)j;
        }
    }
    for (int m = 32; m; m >>= 1) {
        const float ov = __shfl_xor(best, m);
        const int oi = __shfl_xor(idx, m);
        if (ov > best || (ov == best && oi < idx)) {
            best = ov;
            idx = oi;
        }
    }
    const bool any_nf = __ballot(nf) != 0;
    if (lane == 0) {
        a.pos[r] = idx == INT_MAX ? 0 : idx;                    // nothing above -inf: the scan's starting column
        a.peak[r] = best;
        a.bad[r] = any_nf ? 1 : 0;
    }
}

__global__ __launch_bounds__(T2S_ALIGN_BLOCK) void align_stats_kernel(const AlignStatsArgs a) {
    __shared__ int s_scan[T2S_ALIGN_BLOCK];
    __shared__ double s_sum[T2S_ALIGN_BLOCK];
    __shared__ int s_carry;
    __shared__ int s_red[5];                                    // max_skip, max_back, longest_stall, covered, bad_rows
    const int tid = threadIdx.x, b = blockIdx.x;
    const int S = al_clamp(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const int F = al_clamp(a.out_len ? a.out_len[b] : a.N, 0, a.N);
    const int* pos = a.pos + (size_t)b * a.N;
    const float* peak = a.peak + (size_t)b * a.N;
    const unsigned char* bad = a.bad + (size_t)b * a.N;
    int* dur = a.dur + (size_t)b * a.T_in;
    if (tid == 0) s_carry = -1;
    if (tid < 5) s_red[tid] = 0;
    __syncthreads();
    int skip = 0, back = 0, stall = 0, covered = 0, bad_rows = 0;
    double sum = 0.0;
    for (int t0 = 0; t0 < F; t0 += T2S_ALIGN_BLOCK) {           // (F is the same for every thread: the barriers below are uniform)
        const int t = t0 + tid;
        const bool valid = t < F;
        int p = 0, start = -1;
        bool end = false;
        if (valid) {
            p = pos[t];
            sum += (double)peak[t];
            bad_rows += bad[t] != 0;
            if (p >= 0 && p < S && atomicAdd(&dur[p], 1) == 0) ++covered;
            if (t > 0) {
                const long d = (long)p - (long)pos[t - 1];
                if (d != 0) start = t;
                if (d > skip) skip = d > INT_MAX ? INT_MAX : (int)d;
                if (-d > back) back = -d > INT_MAX ? INT_MAX : (int)-d;
            } else {
                start = 0;
            }
            end = t == F - 1 || pos[t + 1] != p;
        }
        s_scan[tid] = start;
        __syncthreads();
        for (int w = 1; w < T2S_ALIGN_BLOCK; w <<= 1) {         // inclusive running maximum of the start frames
            const int v = tid >= w ? s_scan[tid - w] : -1;
            __syncthreads();
            if (v > s_scan[tid]) s_scan[tid] = v;
            __syncthreads();
        }
        const int carry = s_carry;
        const int first = s_scan[tid] > carry ? s_scan[tid] : carry;        // the frame this thread's run started at
        if (end && t - first + 1 > stall) stall = t - first + 1;
        __syncthreads();
        if (tid == T2S_ALIGN_BLOCK - 1) s_carry = first;
        __syncthreads();
    }
    atomicMax(&s_red[0], skip);
    atomicMax(&s_red[1], back);
    atomicMax(&s_red[2], stall);
    atomicAdd(&s_red[3], covered);
    atomicAdd(&s_red[4], bad_rows);
    s_sum[tid] = sum;
    __syncthreads();
    for (int w = T2S_ALIGN_BLOCK / 2; w; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const int last = F > 0 ? pos[F - 1] : -1;
        const double focus = F > 0 ? s_sum[0] / (double)F : 0.0;
        const AlignThresholds& th = a.thr;
        int* st = a.stats + (size_t)b * 8;
        st[0] = F;
        st[1] = S;
        st[2] = s_red[0];
        st[3] = s_red[1];
        st[4] = s_red[2];
        st[5] = last;
        st[6] = s_red[3];
        st[7] = s_red[4];
        a.focus[b] = focus;
        int f = 0;
        if (th.max_frames > 0 && F >= th.max_frames) f |= 1;
        if (th.skip_max >= 0 && s_red[0] > th.skip_max) f |= 2;
        if (th.back_max >= 0 && s_red[1] > th.back_max) f |= 4;
        if (th.stall_max >= 0 && s_red[2] > th.stall_max) f |= 8;
        if (th.end_slack >= 0 && (long)last < (long)S - 1 - (long)th.end_slack) f |= 16;
        if (th.min_focus > 0.0 && !(focus >= th.min_focus)) f |= 32;
        if (s_red[4] > 0) f |= 64;
        if (F == 0) f |= 128;
        a.flags[b] = f;
    }
}

hipError_t t2s_launch_align_rows(const AlignRowsArgs& a, int src_kind, hipStream_t s) {
    const long rows = (long)a.B * a.N;
    const dim3 grid((unsigned)((rows + T2S_ALIGN_ROWS - 1) / T2S_ALIGN_ROWS)), block(64 * T2S_ALIGN_ROWS);
    switch (src_kind) {
        case 1: hipLaunchKernelGGL(align_rows_kernel<float>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(align_rows_kernel<_Float16>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t t2s_launch_align_stats(const AlignStatsArgs& a, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(a.dur, 0, (size_t)a.B * a.T_in * sizeof(int), s);       // the counts start at 0
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(align_stats_kernel, dim3(a.B), dim3(T2S_ALIGN_BLOCK), 0, s, a);
    return hipGetLastError();
}
