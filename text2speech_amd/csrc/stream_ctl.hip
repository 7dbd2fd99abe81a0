// The alignment check and the time warp inside a stream: align.hip's two passes and warp.hip's map and gather, restated over the
// frames [n0, n) of one push with their running values kept in HBM, so that after every push the outputs are what the whole-row
// kernels give for the prefix [0, n) - bit for bit, whatever the cuts (text2speech_amd/alignment.py AlignmentStream,
// text2speech_amd/rate.py WarpStream, text2speech_amd/streaming.py synthesize_stream(control=)).  include/t2s_hip.h carries the
// definition.  Both are prefix computations:
//
//   the alignment statistics are running maxima, integer counts and a sum in a fixed lane order: the maxima, the counts and the
//   run-start carry sit in a per-entry state block, and so do the 256 double partial sums of the peaks - frame t is added into
//   partial t % 256 in ascending t, and the 256-way tree is formed from the current partials on every push;
//   the time warp is a cumulative integer map: the table persists, so cum[b, n0] is the carry.
//
// Four kernels:
//
//   align_window_rows_kernel   align_rows_kernel's scan over the B (n - n0) new rows: one wave per row, ties to the smaller column,
//                              a NaN is never chosen.  Writes columns [n0, n) of pos / peak / bad [B, N_cap].
//   align_window_stats_kernel  one workgroup per entry walking the new frames in steps of 256 that start at a multiple of 256, so
//                              thread i owns partial i.  A run still open at frame n - 1 counts with its current length - what the
//                              whole-row kernel does for its last run, and what lets a stall be seen while it happens.  dur is
//                              counted with integer atomics on the entry's own row, which the launcher zeroed where n0 == 0.
//   warp_window_map_kernel     warp_map_kernel's step over [n0, n) with one stretch per entry: extends cum[b, n0 + 1 .. n] from the
//                              stored cum[b, n0].  first / last meet in integer atomics (first as an unsigned minimum) on rows the
//                              launcher set to -1 where n0 == 0: path[f - 1] is read from the persistent path, nothing is carried,
//                              first only ever decreases and last only ever increases.
//   warp_window_gather_kernel  warp_gather_kernel's expression for the output columns [j0, j1) with F_b = n: bisection in cum, a
//                              formed once, one rounding to the mel's type; 16 channels per workgroup, coalesced along time.
//
// Memory safety: n0 and n are clamped to [0, N_cap] and every length is clamped; a column at or behind S_b is never read; the
// entry pass trusts no pos it reads (one outside [0, S_b) is counted in no dur) and forms differences of pos in 64 bits; a path value
// indexes the first / last row only inside [0, S_b); the gather's f lies in [0, n) whatever cum holds.
#include "t2s_common.h"
#include "stream_ctl_ops.h"

#include <limits.h>
#include <math.h>

#define SC_Q (1L << T2S_WARP_Q_BITS)

static __device__ __forceinline__ int sc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static __device__ __forceinline__ long sc_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }
static __device__ __forceinline__ bool sc_not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

template <typename TSrc>
__global__ __launch_bounds__(64 * T2S_ALIGN_ROWS) void align_window_rows_kernel(const AlignWindowArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = sc_clamp(a.n0, 0, a.N_cap), n = sc_clamp(a.n, n0, a.N_cap), m = n - n0;
    const long r = (long)blockIdx.x * T2S_ALIGN_ROWS + wave;
    if (m == 0 || r >= (long)a.B * m) return;                   // (wave-uniform; the kernel has no barrier)
    const int b = (int)(r / m), i = (int)(r % m);
    const int S = sc_clamp(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const TSrc* row = (const TSrc*)a.A + (size_t)b * a.ld_entry + (size_t)i * a.ld_row;
    float best = -INFINITY;
    int idx = INT_MAX;                                          // no column yet
    bool nf = false;
    for (long j = lane; j < S; j += 64) {
        const float v = (float)row[j];
        nf |= sc_not_finite(v);
        if (v > best) {
            best = v;
            idx = (int)j;
        }
    }
    for (int w = 32; w; w >>= 1) {
        const float ov = __shfl_xor(best, w);
        const int oi = __shfl_xor(idx, w);
        if (ov > best || (ov == best && oi < idx)) {
            best = ov;
            idx = oi;
        }
    }
    const bool any_nf = __ballot(nf) != 0;
    if (lane == 0) {
        const size_t o = (size_t)b * a.N_cap + n0 + i;
        a.pos[o] = idx == INT_MAX ? 0 : idx;                    // nothing above -inf: the scan's starting column
        a.peak[o] = best;
        a.bad[o] = any_nf ? 1 : 0;
    }
}

__global__ __launch_bounds__(T2S_ALIGN_BLOCK) void align_window_stats_kernel(const AlignWindowArgs a) {
    __shared__ int s_scan[T2S_ALIGN_BLOCK];
    __shared__ double s_sum[T2S_ALIGN_BLOCK];
    __shared__ int s_carry;
    __shared__ int s_red[5];                                    // max_skip, max_back, longest_stall, covered, bad_rows
    const int tid = threadIdx.x, b = blockIdx.x;
    const int S = sc_clamp(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const int n0 = sc_clamp(a.n0, 0, a.N_cap), n = sc_clamp(a.n, n0, a.N_cap);
    const int* pos = a.pos + (size_t)b * a.N_cap;
    const float* peak = a.peak + (size_t)b * a.N_cap;
    const unsigned char* bad = a.bad + (size_t)b * a.N_cap;
    int* dur = a.dur + (size_t)b * a.T_in;
    AlignWindowState* st = a.state + b;
    if (tid == 0) s_carry = n0 > 0 ? st->carry : -1;
    if (tid < 5) s_red[tid] = n0 > 0 ? st->red[tid] : 0;
    double sum = n0 > 0 ? st->part[tid] : 0.0;
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
    st->part[tid] = sum;
    s_sum[tid] = sum;
    __syncthreads();
    for (int w = T2S_ALIGN_BLOCK / 2; w; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    if (tid < 5) st->red[tid] = s_red[tid];
    if (tid == 0) {
        st->carry = s_carry;
        const int last = n > 0 ? pos[n - 1] : -1;
        const double focus = n > 0 ? s_sum[0] / (double)n : 0.0;
        const AlignThresholds& th = a.thr;
        int* out = a.stats + (size_t)b * 8;
        out[0] = n;
        out[1] = S;
        out[2] = s_red[0];
        out[3] = s_red[1];
        out[4] = s_red[2];
        out[5] = last;
        out[6] = s_red[3];
        out[7] = s_red[4];
        a.focus[b] = focus;
        int f = 0;
        if (th.skip_max >= 0 && s_red[0] > th.skip_max) f |= 2;
        if (th.back_max >= 0 && s_red[1] > th.back_max) f |= 4;
        if (th.stall_max >= 0 && s_red[2] > th.stall_max) f |= 8;
        if (s_red[4] > 0) f |= 64;
        if (a.last) {                                           // the bits that only an utterance's end decides
            if (th.max_frames > 0 && n >= th.max_frames) f |= 1;
            if (th.end_slack >= 0 && (long)last < (long)S - 1 - (long)th.end_slack) f |= 16;
            if (th.min_focus > 0.0 && !(focus >= th.min_focus)) f |= 32;
            if (n == 0) f |= 128;
        }
        a.flags[b] = f;
    }
}

__global__ __launch_bounds__(T2S_WARP_BLOCK) void warp_window_map_kernel(const WarpWindowMapArgs a) {
    __shared__ long s_scan[T2S_WARP_BLOCK];
    __shared__ long s_carry;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n0 = sc_clamp(a.n0, 0, a.N_cap), n = sc_clamp(a.n, n0, a.N_cap);
    const int S = sc_clamp(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in > 0 ? a.T_in : 1);
    const int* path = a.path ? a.path + (size_t)b * a.ld_path : nullptr;
    int* fl = a.first_last && path ? a.first_last + (size_t)b * a.T_in * 2 : nullptr;
    long* cum = a.cum + (size_t)b * ((size_t)a.N_cap + 1);
    const long s_entry = a.stretches ? sc_clampl(a.stretches[b], SC_Q >> 3, SC_Q << 3) : a.stretch;
    if (tid == 0) {
        if (n0 == 0) cum[0] = 0;
        s_carry = n0 == 0 ? 0 : cum[n0];
    }
    __syncthreads();
    for (int f0 = n0; f0 < n; f0 += T2S_WARP_BLOCK) {           // (the same for every thread: the barriers below are uniform)
        const int f = f0 + tid;
        long s = 0;
        if (f < n) {
            s = s_entry;
            if (fl) {
                const int k = path[f];
                if (k >= 0 && k < S) {
                    if (f == 0 || path[f - 1] != k) atomicMin((unsigned*)&fl[2 * k], (unsigned)f);
                    if (f == n - 1 || path[f + 1] != k) atomicMax(&fl[2 * k + 1], f);
                }
            }
        }
        s_scan[tid] = s;
        __syncthreads();
        for (int w = 1; w < T2S_WARP_BLOCK; w <<= 1) {          // inclusive scan of the step's stretches
            const long v = tid >= w ? s_scan[tid - w] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const long c = s_carry + s_scan[tid];
        if (f < n) cum[(size_t)f + 1] = c;
        __syncthreads();
        if (tid == T2S_WARP_BLOCK - 1) s_carry = c;
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(T2S_WARP_BLOCK) void warp_window_gather_kernel(const WarpWindowGatherArgs a) {
    const int b = blockIdx.y;
    const long width = a.j1 - a.j0;
    const long i = (long)blockIdx.x * T2S_WARP_BLOCK + threadIdx.x;
    const int Fb = sc_clamp(a.n, 0, a.N_cap);
    if (i >= width || Fb == 0) return;                          // (no barrier in this kernel)
    const long j = a.j0 + i;
    const int c0 = blockIdx.z * T2S_WARP_CH, c1 = c0 + T2S_WARP_CH < a.C ? c0 + T2S_WARP_CH : a.C;
    T* out = (T*)a.out + ((size_t)b * a.C + c0) * (size_t)width + i;
    const long* cum = a.cum + (size_t)b * ((size_t)a.N_cap + 1);
    const long p = (2 * j + 1) << T2S_WARP_Q_BITS;
    int lo = 0, hi = Fb;                                        // m[f] <= p for every f < lo, m[f] > p for every f >= hi
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] + cum[mid + 1] <= p) lo = mid + 1; else hi = mid;
    }
    int f = lo - 1;
    double w = 0.0;
    if (f < 0) {
        f = 0;
    } else if (f >= Fb - 1) {
        f = Fb - 1;
    } else {
        const long m0 = cum[f] + cum[f + 1], m1 = cum[f + 1] + cum[f + 2];
        w = (double)(p - m0) / (double)(m1 - m0);
    }
    const T* x = (const T*)a.x + (size_t)b * a.ld_entry + (size_t)c0 * a.ld_row + f;
    if (w == 0.0) {
        for (int c = c0; c < c1; ++c, x += a.ld_row, out += width) *out = *x;
    } else {
        for (int c = c0; c < c1; ++c, x += a.ld_row, out += width) *out = (T)((1.0 - w) * (double)x[0] + w * (double)x[1]);
    }
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

hipError_t t2s_launch_warp_window_map(const WarpWindowMapArgs& a, hipStream_t s) {
    if (a.first_last && a.n0 == 0) {
        const hipError_t e = hipMemsetAsync(a.first_last, 0xff, (size_t)a.B * a.T_in * 2 * sizeof(int), s);     // -1: no frame yet
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(warp_window_map_kernel, dim3(a.B), dim3(T2S_WARP_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t t2s_launch_warp_window_gather(const WarpWindowGatherArgs& a, int src_kind, hipStream_t s) {
    const long width = a.j1 - a.j0;
    if (width <= 0) return hipSuccess;                          // nothing asked for: nothing launched
    const dim3 grid((unsigned)((width + T2S_WARP_BLOCK - 1) / T2S_WARP_BLOCK), a.B, (unsigned)((a.C + T2S_WARP_CH - 1) / T2S_WARP_CH));
    const dim3 block(T2S_WARP_BLOCK);
    switch (src_kind) {
        case 1: hipLaunchKernelGGL(warp_window_gather_kernel<float>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(warp_window_gather_kernel<_Float16>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
