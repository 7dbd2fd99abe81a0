// Warping a batch of mels in time on the device, and reading the symbols' timestamps from the same map: speaking rate without a
// change of pitch, and [start, end) of every symbol in samples (text2speech_amd/rate.py warp_mel / symbol_spans,
// text2speech_amd/longform.py synthesize_long_timed(speed=, timestamps=)).  include/t2s_hip.h carries the definition; in short, with
// Q = 2^20 and exact int64 arithmetic for everything discrete:
//
//   F_b = clamp(lengths[b], 0, F), S_b = clamp(in_len[b], 1, T_in).  Source frame f < F_b has a stretch s[b,f] > 0, its output frames
//   in units of 1 / Q: one value for all, one per entry, or rint(Q / clamp((double)rates[b, path[b,f]], min_rate, max_rate)) - with
//   Q (rate 1) where the path value lies outside [0, S_b) or the table holds a NaN.  c[b,0] = 0, c[b,f+1] = c[b,f] + s[b,f], entries
//   behind F_b repeat c[b,F_b].  F'_b = 0 for F_b = 0, else clamp((c[b,F_b] + Q / 2) >> 20, 1, cap).
//   Output frame j < F'_b: p = (2j + 1) Q, m[f] = c[f] + c[f+1], f the largest index with m[f] <= p.  None: x[0].  f >= F_b - 1:
//   x[F_b - 1].  Else a = (double)(p - m[f]) / (double)(m[f+1] - m[f]); a == 0: x[f] (x[f+1] is not read), else
//   (T)((1 - a) (double)x[f] + a (double)x[f+1]): one rounding to the mel's type.  Columns F'_b .. cap - 1 are +0.
//   Symbol k < S_b: first / last the smallest / largest f < F_b with path[b,f] == k; its span is c[first] .. c[last + 1], in samples
//   u = (t hop) >> 20, then clamp(u - trim_start, 0, trim_len), + offset, min(u up / down, total), each step where given.
//
// The map's step and the gather's column are stated once each, with a whole-row kernel and a window kernel around each; the window
// kernels are the same warp pushed piece by piece while the mel is still decoded (text2speech_amd/rate.py WarpStream,
// text2speech_amd/streaming.py synthesize_stream(control=)):
//
//   warp_scan_step, warp_mark_first_last
//                       one workgroup per entry, T2S_WARP_BLOCK frames per step, one frame per thread: the stretches are scanned in
//                       LDS in int64 and the last sum is carried into the next step, so any F works.  first / last meet in integer
//                       atomics on the entry's own row, which the launcher set to -1 on the same stream (first as an unsigned
//                       minimum: -1 is its largest value) - only a run's first and last frame issue one.  Exact in any order.
//                       warp_map_kernel walks [0, F) from 0, looks the stretch up in the rates table, repeats c[F_b] behind F_b and
//                       writes F'_b; warp_window_map_kernel walks [n0, n) with one stretch per entry.
//   warp_column         a thread owns one output column, finds its f by bisection in the entry's row of c (at most 32 steps, in the
//                       cache after the first), forms a once and walks 16 channels.  Neighbouring threads read neighbouring frames
//                       and store neighbouring columns: coalesced along time.  warp_gather_kernel, grid ceil(cap / 256) x B x
//                       ceil(C / 16), runs it for the columns below F'_b and fills the rest with +0; warp_window_gather_kernel runs
//                       it for the output columns [j0, j1) with F_b = n.
//   warp_spans_kernel   one thread per (entry, symbol).
//
// The stream's contract is that after every push its outputs are what the whole-row kernels give for the prefix [0, n), bit for bit,
// whatever the cuts.  The map is a cumulative integer table that persists in HBM [B, N_cap + 1], so it is its own carry: a push
// extends c[b, n0 + 1 .. n] from the stored c[b, n0].  Nothing is carried for first / last either: path[f - 1] is read from the
// persistent path, the launcher sets the rows to -1 where n0 == 0, and over the pushes first only ever decreases and last only ever
// increases - a run cut by a push marks frame n - 1 as its last, and the next push raises it.
//
// Memory safety: every length is clamped, n0 and n to [0, N_cap]; a path value indexes the table and the first / last row only inside
// [0, S_b); the gather's f lies in [0, F_b) whatever c holds and its column inside [0, cap); the span pass uses first / last only
// inside [0, F_b).
#include "t2s_common.h"
#include "warp_ops.h"

#include <limits.h>
#include <math.h>

static __device__ __forceinline__ long clamp_long(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One step of the map's walk: the inclusive scan of the workgroup's stretches on top of the carry.  Returns c behind this thread's
// frame and leaves the last thread's in the carry.  Every thread of the workgroup calls it: the barriers are inside.
static __device__ __forceinline__ long warp_scan_step(long s, long* s_scan, long& s_carry) {
    const int tid = threadIdx.x;
    s_scan[tid] = s;
    __syncthreads();
    for (int w = 1; w < T2S_WARP_BLOCK; w <<= 1) {
        const long v = tid >= w ? s_scan[tid - w] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    const long c = s_carry + s_scan[tid];
    __syncthreads();
    if (tid == T2S_WARP_BLOCK - 1) s_carry = c;
    __syncthreads();
    return c;
}

// Frame f attends to symbol k: where it opens or closes a run of k, it meets the symbol's first / last frame.
static __device__ __forceinline__ void warp_mark_first_last(int* fl, const int* path, int f, int k, int last_frame) {
    if (f == 0 || path[f - 1] != k) atomicMin((unsigned*)&fl[2 * k], (unsigned)f);
    if (f == last_frame || path[f + 1] != k) atomicMax(&fl[2 * k + 1], f);
}

__global__ __launch_bounds__(T2S_WARP_BLOCK) void warp_map_kernel(const WarpMapArgs a) {
    __shared__ long s_scan[T2S_WARP_BLOCK];
    __shared__ long s_carry;
    const int tid = threadIdx.x, b = blockIdx.x, F = a.F;
    const int S = clamp_int(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in > 0 ? a.T_in : 1);
    const int Fb = clamp_int(a.lengths ? a.lengths[b] : F, 0, F);
    const int* path = a.path ? a.path + (size_t)b * a.ld_path : nullptr;
    const float* rates = a.rates && path ? a.rates + (size_t)b * a.ld_rates : nullptr;
    int* fl = a.first_last && path ? a.first_last + (size_t)b * a.T_in * 2 : nullptr;
    long* cum = a.cum ? a.cum + (size_t)b * ((size_t)F + 1) : nullptr;
    const long s_entry = rates ? T2S_WARP_Q : (a.stretches ? clamp_long(a.stretches[b], T2S_WARP_Q >> 3, T2S_WARP_Q << 3) : a.stretch);
    if (tid == 0) {
        s_carry = 0;
        if (cum) cum[0] = 0;
    }
    __syncthreads();
    for (int f0 = 0; f0 < F; f0 += T2S_WARP_BLOCK) {            // (F is the same for every thread: the barriers are uniform)
        const int f = f0 + tid;
        long s = 0;                                             // behind F_b: c[F_b] is repeated
        if (f < Fb) {
            s = s_entry;
            if (path) {
                const int k = path[f];
                if (k >= 0 && k < S) {
                    if (rates) {
                        const double v = (double)rates[k];
                        if (v == v) s = (long)rint((double)T2S_WARP_Q / (v < a.min_rate ? a.min_rate : (v > a.max_rate ? a.max_rate : v)));
                    }
                    if (fl) warp_mark_first_last(fl, path, f, k, Fb - 1);
                }
            }
        }
        const long c = warp_scan_step(s, s_scan, s_carry);
        if (cum && f < F) cum[(size_t)f + 1] = c;
    }
    if (tid == 0 && a.out_len)
        a.out_len[b] = Fb == 0 ? 0 : (int)clamp_long((s_carry + (T2S_WARP_Q >> 1)) >> T2S_WARP_Q_BITS, 1, a.cap);
}

__global__ __launch_bounds__(T2S_WARP_BLOCK) void warp_window_map_kernel(const WarpWindowMapArgs a) {
    __shared__ long s_scan[T2S_WARP_BLOCK];
    __shared__ long s_carry;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n0 = clamp_int(a.n0, 0, a.N_cap), n = clamp_int(a.n, n0, a.N_cap);
    const int S = clamp_int(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in > 0 ? a.T_in : 1);
    const int* path = a.path ? a.path + (size_t)b * a.ld_path : nullptr;
    int* fl = a.first_last && path ? a.first_last + (size_t)b * a.T_in * 2 : nullptr;
    long* cum = a.cum + (size_t)b * ((size_t)a.N_cap + 1);
    const long s_entry = a.stretches ? clamp_long(a.stretches[b], T2S_WARP_Q >> 3, T2S_WARP_Q << 3) : a.stretch;
    if (tid == 0) {
        if (n0 == 0) cum[0] = 0;
        s_carry = n0 == 0 ? 0 : cum[n0];
    }
    __syncthreads();
    for (int f0 = n0; f0 < n; f0 += T2S_WARP_BLOCK) {           // (the same for every thread: the barriers are uniform)
        const int f = f0 + tid;
        long s = 0;
        if (f < n) {
            s = s_entry;
            if (fl) {
                const int k = path[f];
                if (k >= 0 && k < S) warp_mark_first_last(fl, path, f, k, n - 1);
            }
        }
        const long c = warp_scan_step(s, s_scan, s_carry);
        if (f < n) cum[(size_t)f + 1] = c;
    }
}

// Output column j of one entry for the channels [c0, c1): x points at frame 0 of channel c0 (rows ld_row apart), out at the
// column's element of channel c0 (rows out_stride apart).  Fb >= 1.
template <typename T>
static __device__ __forceinline__ void warp_column(const long* cum, int Fb, long j, const T* x, long ld_row, T* out, size_t out_stride,
                                                   int c0, int c1) {
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
    x += f;
    if (w == 0.0) {                                             // x[1] is not read
        for (int c = c0; c < c1; ++c, x += ld_row, out += out_stride) *out = *x;
    } else {
        for (int c = c0; c < c1; ++c, x += ld_row, out += out_stride) *out = (T)((1.0 - w) * (double)x[0] + w * (double)x[1]);
    }
}

template <typename T>
__global__ __launch_bounds__(T2S_WARP_BLOCK) void warp_gather_kernel(const WarpGatherArgs a) {
    const int b = blockIdx.y, cap = a.cap, F = a.F;
    const long j = (long)blockIdx.x * T2S_WARP_BLOCK + threadIdx.x;
    if (j >= cap) return;                                       // (no barrier in this kernel)
    const int c0 = blockIdx.z * T2S_WARP_CH, c1 = c0 + T2S_WARP_CH < a.C ? c0 + T2S_WARP_CH : a.C;
    const int Fb = clamp_int(a.lengths ? a.lengths[b] : F, 0, F);
    const int n_out = Fb == 0 ? 0 : clamp_int(a.out_len[b], 0, cap);
    T* out = (T*)a.out + ((size_t)b * a.C + c0) * (size_t)cap + j;
    if (j >= n_out) {
        for (int c = c0; c < c1; ++c, out += cap) *out = (T)0;
        return;
    }
    warp_column(a.cum + (size_t)b * ((size_t)F + 1), Fb, j, (const T*)a.x + (size_t)b * a.ld_entry + (size_t)c0 * a.ld_row, a.ld_row, out,
                (size_t)cap, c0, c1);
}

template <typename T>
__global__ __launch_bounds__(T2S_WARP_BLOCK) void warp_window_gather_kernel(const WarpWindowGatherArgs a) {
    const int b = blockIdx.y;
    const long width = a.j1 - a.j0;
    const long i = (long)blockIdx.x * T2S_WARP_BLOCK + threadIdx.x;
    const int Fb = clamp_int(a.n, 0, a.N_cap);
    if (i >= width || Fb == 0) return;                          // (no barrier in this kernel)
    const int c0 = blockIdx.z * T2S_WARP_CH, c1 = c0 + T2S_WARP_CH < a.C ? c0 + T2S_WARP_CH : a.C;
    warp_column(a.cum + (size_t)b * ((size_t)a.N_cap + 1), Fb, a.j0 + i, (const T*)a.x + (size_t)b * a.ld_entry + (size_t)c0 * a.ld_row,
                a.ld_row, (T*)a.out + ((size_t)b * a.C + c0) * (size_t)width + i, (size_t)width, c0, c1);
}

__global__ __launch_bounds__(T2S_WARP_BLOCK) void warp_spans_kernel(const WarpSpansArgs a) {
    const long i = (long)blockIdx.x * T2S_WARP_BLOCK + threadIdx.x;
    if (i >= (long)a.B * a.T_in) return;
    const int b = (int)(i / a.T_in), k = (int)(i % a.T_in);
    const int S = clamp_int(a.in_len ? a.in_len[b] : a.T_in, 1, a.T_in);
    const int Fb = clamp_int(a.lengths ? a.lengths[b] : a.F, 0, a.F);
    long u0 = -1, u1 = -1;
    if (k < S) {
        const int first = a.first_last[2 * i], last = a.first_last[2 * i + 1];
        if (first >= 0 && last >= first && last < Fb) {
            const long* cum = a.cum + (size_t)b * ((size_t)a.F + 1);
            const long total = a.total_dev ? *a.total_dev : a.total;
            long u[2] = {cum[first], cum[last + 1]};
            for (int e = 0; e < 2; ++e) {
                long v = (u[e] * a.hop) >> T2S_WARP_Q_BITS;
                if (a.trim_start) {
                    v -= a.trim_start[b];
                    const long len = a.trim_end[b] - a.trim_start[b];
                    v = v < 0 ? 0 : v;
                    v = v > len ? len : v;
                }
                if (a.offsets) v += a.offsets[b];
                v = v * a.up / a.down;
                u[e] = v < total ? v : total;
            }
            u0 = u[0];
            u1 = u[1];
        }
    }
    a.spans[2 * i] = u0;
    a.spans[2 * i + 1] = u1;
}

hipError_t t2s_launch_warp_map(const WarpMapArgs& a, hipStream_t s) {
    if (a.first_last) {
        const hipError_t e = hipMemsetAsync(a.first_last, 0xff, (size_t)a.B * a.T_in * 2 * sizeof(int), s);     // -1: no frame yet
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(warp_map_kernel, dim3(a.B), dim3(T2S_WARP_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t t2s_launch_warp_gather(const WarpGatherArgs& a, int src_kind, hipStream_t s) {
    const dim3 grid((unsigned)((a.cap + T2S_WARP_BLOCK - 1) / T2S_WARP_BLOCK), a.B, (unsigned)((a.C + T2S_WARP_CH - 1) / T2S_WARP_CH));
    const dim3 block(T2S_WARP_BLOCK);
    switch (src_kind) {
        case 1: hipLaunchKernelGGL(warp_gather_kernel<float>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(warp_gather_kernel<_Float16>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t t2s_launch_warp_spans(const WarpSpansArgs& a, hipStream_t s) {
    const long n = (long)a.B * a.T_in;
    hipLaunchKernelGGL(warp_spans_kernel, dim3((unsigned)((n + T2S_WARP_BLOCK - 1) / T2S_WARP_BLOCK)), dim3(T2S_WARP_BLOCK), 0, s, a);
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
