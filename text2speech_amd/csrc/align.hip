// Looking at the attention alignments of a batch on the device: where every decoder frame attends, and per entry whether that path
// is the text - skips, backward jumps, stalls, an end that was never reached, a diffuse attention (text2speech_amd/alignment.py
// alignment_report, text2speech_amd/longform.py synthesize_long(check=)) - for whole rows, and pushed piece by piece while the
// utterance is still decoded (text2speech_amd/alignment.py AlignmentStream, text2speech_amd/streaming.py synthesize_stream(control=)).
// include/t2s_hip.h carries the definition; in short:
//
//   S_b = clamp(in_len[b], 1, T_in), F_b = clamp(out_len[b], 0, N).  Row pass, t < F_b: pos[b,t] the smallest j < S_b at which
//   A[b,t,j] is largest (scan from best = -inf, update on v > best: a NaN is never chosen), peak[b,t] that value as f32, bad[b,t]
//   whether any of the S_b values is not finite; t >= F_b: -1, 0, 0 and the row is not loaded.  Entry pass: the largest forward
//   and backward step of pos, the longest run of equal pos, the last pos, the frames per symbol (dur) and how many symbols have
//   any, the rows with a non-finite value, the mean peak in double, and the flag bits the thresholds make of those.
//
// Two loops, each stated once, and two kernels around each - one for whole rows, one for the frames [n0, n) of a push:
//
//   align_scan_row     one wave per row.  Lane l scans columns l, l + 64, ... (a coalesced load per step; every lane keeps the
//                      smallest column of its own maximum), then six exchanges reduce (value, column) across the wave, ties to the
//                      smaller column.  No LDS, no barrier.  align_rows_kernel runs it over the B N rows of a batch, T2S_ALIGN_ROWS
//                      rows per workgroup, and writes the padding behind F_b; align_window_rows_kernel runs it over the B (n - n0)
//                      new rows and writes columns [n0, n) of pos / peak / bad [B, N_cap].
//   align_entry_pass   one workgroup per entry, T2S_ALIGN_BLOCK frames per step, one frame per thread.  A run's length needs the
//                      frame its run started at: the start frames (t where pos[t] != pos[t-1]) are scanned with a running maximum
//                      in LDS, and the last value is carried into the next step.  The peaks are summed in double, frame t into
//                      partial t % 256 in ascending t, then by a fixed tree over the 256 partial sums: the order depends on the
//                      number of frames alone.  dur is counted with integer atomics on the entry's own row, which the launcher
//                      zeroed on the same stream; the thread that finds a count at 0 counts the symbol as covered.  Integer maxima
//                      and sums meet in LDS atomics: exact in any order.  align_stats_kernel runs it from frame 0 and from zeros
//                      over [0, F_b); align_window_stats_kernel runs it over [n0, n) from the entry's state block.
//
// The stream's contract is that after every push its outputs are what the whole-row kernels give for the prefix [0, n), bit for bit,
// whatever the cuts.  The entry pass is a prefix computation - running maxima, integer counts and a sum in a fixed lane order - so
// what it carries fits a per-entry state block (AlignWindowState): the maxima, the counts, the run-start carry and the 256 double
// partial sums.  The window form walks steps of 256 that start at a multiple of 256, so thread i owns partial i as in the whole-row
// form, and the tree is formed from the current partials on every push.  A run still open at frame n - 1 counts with its current
// length: that is what the whole-row form does for its last run, and what lets a stall be seen while it happens.  The four flag bits
// that only an utterance's end decides (1, 16, 32, 128) are set on the push that says it is the last.  dur is zeroed by the launcher
// where n0 == 0.
//
// Memory safety: every length is clamped, n0 and n to [0, N_cap]; a row at or behind F_b and a column at or behind S_b are never
// read; the entry pass trusts no pos it reads (one outside [0, S_b) is counted in no dur) and differences of pos are formed in 64
// bits.
#include "t2s_common.h"
#include "align_ops.h"

#include <limits.h>
#include <math.h>

static __device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// One wave over the S columns of one row: the column of the maximum (0 where nothing lies above -inf: the scan's starting column),
// the maximum, and whether any value is not finite - the same in every lane.
template <typename TSrc>
static __device__ __forceinline__ void align_scan_row(const TSrc* row, int S, int lane, int& idx, float& best, bool& any_nf) {
    best = -INFINITY;
    idx = INT_MAX;                                              // no column yet
    bool nf = false;
    for (long j = lane; j < S; j += 64) {
        const float v = (float)row[j];
        nf |= not_finite(v);
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
    any_nf = __ballot(nf) != 0;
    if (idx == INT_MAX) idx = 0;
}

template <typename TSrc>
__global__ __launch_bounds__(64 * T2S_ALIGN_ROWS) void align_rows_kernel(const AlignRowsArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * T2S_ALIGN_ROWS + wave;
    if (r >= (long)a.B * a.N) return;                           // (wave-uniform; the kernel has no barrier)
    const int b = (int)(r / a.N), t = (int)(r % a.N);
    const int S = clamp_int(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const int F = clamp_int(a.out_len ? a.out_len[b] : a.N, 0, a.N);
    if (t >= F) {
        if (lane == 0) {
            a.pos[r] = -1;
            a.peak[r] = 0.f;
            a.bad[r] = 0;
        }
        return;
    }
    int idx;
    float best;
    bool any_nf;
    align_scan_row((const TSrc*)a.A + (size_t)b * a.ld_entry + (size_t)t * a.ld_row, S, lane, idx, best, any_nf);
    if (lane == 0) {
        a.pos[r] = idx;
        a.peak[r] = best;
        a.bad[r] = any_nf ? 1 : 0;
    }
}

template <typename TSrc>
__global__ __launch_bounds__(64 * T2S_ALIGN_ROWS) void align_window_rows_kernel(const AlignWindowArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = clamp_int(a.n0, 0, a.N_cap), n = clamp_int(a.n, n0, a.N_cap), m = n - n0;
    const long r = (long)blockIdx.x * T2S_ALIGN_ROWS + wave;
    if (m == 0 || r >= (long)a.B * m) return;                   // (wave-uniform; the kernel has no barrier)
    const int b = (int)(r / m), i = (int)(r % m);
    const int S = clamp_int(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    int idx;
    float best;
    bool any_nf;
    align_scan_row((const TSrc*)a.A + (size_t)b * a.ld_entry + (size_t)i * a.ld_row, S, lane, idx, best, any_nf);
    if (lane == 0) {
        const size_t o = (size_t)b * a.N_cap + n0 + i;
        a.pos[o] = idx;
        a.peak[o] = best;
        a.bad[o] = any_nf ? 1 : 0;
    }
}

// One workgroup over the frames [n0, n) of one entry, whose rows of pos / peak / bad / dur it is given.  CARRY: the running values
// come from *st where n0 > 0 and are saved there; without it n0 is 0, they start from zeros and st is not touched.  `last` opens the
// flag bits that only an utterance's end decides.
template <bool CARRY>
static __device__ __forceinline__ void align_entry_pass(const int* pos, const float* peak, const unsigned char* bad, int* dur, int S, int n0,
                                                        int n, AlignWindowState* st, const AlignThresholds& th, int last, int* stats,
                                                        double* focus_out, int* flags) {
    __shared__ int s_scan[T2S_ALIGN_BLOCK];
    __shared__ double s_sum[T2S_ALIGN_BLOCK];
    __shared__ int s_carry;
    __shared__ int s_red[5];                                    // max_skip, max_back, longest_stall, covered, bad_rows
    const int tid = threadIdx.x;
    const bool resume = CARRY && n0 > 0;
    if (tid == 0) s_carry = resume ? st->carry : -1;
    if (tid < 5) s_red[tid] = resume ? st->red[tid] : 0;
    double sum = resume ? st->part[tid] : 0.0;
    __syncthreads();
    int skip = 0, back = 0, stall = 0, covered = 0, bad_rows = 0;
    for (int t0 = n0 - n0 % T2S_ALIGN_BLOCK; t0 < n; t0 += T2S_ALIGN_BLOCK) {      // (the same for every thread: the barriers are uniform)
        const int t = t0 + tid;
        const bool valid = t >= n0 && t < n;
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
            end = t == n - 1 || pos[t + 1] != p;                // a run open at the prefix's last frame counts as it stands
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
    if (CARRY) st->part[tid] = sum;
    s_sum[tid] = sum;
    __syncthreads();
    for (int w = T2S_ALIGN_BLOCK / 2; w; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    if (CARRY && tid < 5) st->red[tid] = s_red[tid];
    if (tid == 0) {
        if (CARRY) st->carry = s_carry;
        const int last_pos = n > 0 ? pos[n - 1] : -1;
        const double focus = n > 0 ? s_sum[0] / (double)n : 0.0;
        stats[0] = n;
        stats[1] = S;
        stats[2] = s_red[0];
        stats[3] = s_red[1];
        stats[4] = s_red[2];
        stats[5] = last_pos;
        stats[6] = s_red[3];
        stats[7] = s_red[4];
        *focus_out = focus;
        int f = 0;
        if (th.skip_max >= 0 && s_red[0] > th.skip_max) f |= 2;
        if (th.back_max >= 0 && s_red[1] > th.back_max) f |= 4;
        if (th.stall_max >= 0 && s_red[2] > th.stall_max) f |= 8;
        if (s_red[4] > 0) f |= 64;
        if (last) {                                             // the bits that only an utterance's end decides
            if (th.max_frames > 0 && n >= th.max_frames) f |= 1;
            if (th.end_slack >= 0 && (long)last_pos < (long)S - 1 - (long)th.end_slack) f |= 16;
            if (th.min_focus > 0.0 && !(focus >= th.min_focus)) f |= 32;
            if (n == 0) f |= 128;
        }
        *flags = f;
    }
}

__global__ __launch_bounds__(T2S_ALIGN_BLOCK) void align_stats_kernel(const AlignStatsArgs a) {
    const int b = blockIdx.x;
    const int S = clamp_int(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const int F = clamp_int(a.out_len ? a.out_len[b] : a.N, 0, a.N);
    const size_t o = (size_t)b * a.N;
    align_entry_pass<false>(a.pos + o, a.peak + o, a.bad + o, a.dur + (size_t)b * a.T_in, S, 0, F, nullptr, a.thr, 1,
                            a.stats + (size_t)b * 8, a.focus + b, a.flags + b);
}

__global__ __launch_bounds__(T2S_ALIGN_BLOCK) void align_window_stats_kernel(const AlignWindowArgs a) {
    const int b = blockIdx.x;
    const int S = clamp_int(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const int n0 = clamp_int(a.n0, 0, a.N_cap), n = clamp_int(a.n, n0, a.N_cap);
    const size_t o = (size_t)b * a.N_cap;
    align_entry_pass<true>(a.pos + o, a.peak + o, a.bad + o, a.dur + (size_t)b * a.T_in, S, n0, n, a.state + b, a.thr, a.last,
                           a.stats + (size_t)b * 8, a.focus + b, a.flags + b);
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

hipError_t t2s_launch_align_window(const AlignWindowArgs& a, int src_kind, hipStream_t s) {
    if (src_kind != 1 && src_kind != 2) return hipErrorInvalidValue;
    if (a.n0 == 0) {
        const hipError_t e = hipMemsetAsync(a.dur, 0, (size_t)a.B * a.T_in * sizeof(int), s);   // the counts start at 0
        if (e != hipSuccess) return e;
    }
    const long rows = (long)a.B * (a.n - a.n0);
    if (rows > 0) {
        const dim3 grid((unsigned)((rows + T2S_ALIGN_ROWS - 1) / T2S_ALIGN_ROWS)), block(64 * T2S_ALIGN_ROWS);
        if (src_kind == 1) hipLaunchKernelGGL(align_window_rows_kernel<float>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(align_window_rows_kernel<_Float16>, grid, block, 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(align_window_stats_kernel, dim3(a.B), dim3(T2S_ALIGN_BLOCK), 0, s, a);
    return hipGetLastError();
}
