// extern "C" boundary of the training kernels.
#include "../../include/t2s_hip.h"
#include "t2s_kernels.h"
#include "train_ops.h"
#include "t2s_api_common.h"
#include "conv_gemm_args.h"

#include <math.h>
#include <string.h>

// Can the backward GEMM with `rows` output rows over B x L columns take PERM_PAIR8-packed operands (16-byte epilogue pieces)?  Only
// the 256-row ping-pong kernels have that epilogue: the grid rule of bwd_pp256 (conv_gemm_args.h), whole 32-row groups.
extern "C" int t2s_wg_bwd_pair8_ok(int B, int rows, int L) {
    if (B <= 0 || rows <= 0 || L <= 0 || rows % 32) return 0;
    return (long)cdiv(rows, 256) * cdiv(L, 256) * B >= 100 ? 1 : 0;
}

// rows [row0, row0+1) scale kernel lives in waveglow_ops.hip's weightnorm_small (scale-only form below)
__global__ void weightnorm_scale_kernel(const float* v, const float* g, int O, int K, float* scale) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= O) return;
    if (!g) { scale[o] = 1.f; return; }
    float ss = 0.f;
    for (int k = 0; k < K; ++k) ss += v[(size_t)o * K + k] * v[(size_t)o * K + k];
    scale[o] = g[o] / sqrtf(ss);
}

extern "C" {

int t2s_wg_in_cond_gate_train(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                              const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, void* T_hi, void* T_lo,
                              void* G_hi, void* G_lo, int B, int C, int n_cond, int taps, int dilation, int L, int Lp,
                              int halo, int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(X_hi, X_lo) || !planes_ok(acts_hi, acts_lo) || !bias || !al16(bias)) return T2S_EINVAL;
    if (!planes_ok(G_hi, G_lo) || ((T_hi || T_lo) && !planes_ok(T_hi, T_lo))) return T2S_EINVAL;      // tanh planes are optional
    if ((n_cond > 0 && !planes_ok(S_hi, S_lo)) || !gate_shape_ok(B, C, taps, dilation, L, Lp, halo, Mpad)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(X_hi, X_lo, cdiv(C, 32), taps, dilation, S_hi, S_lo, cdiv(n_cond, 32));
    g.output(acts_hi, acts_lo, cdiv(C, 32));
    g.a.T_hi = (u16*)T_hi; g.a.T_lo = (u16*)T_lo; g.a.G_hi = (u16*)G_hi; g.a.G_lo = (u16*)G_lo; g.a.tc = g.a.oc;
    g.a.C = C;
    T2S_CHECK_HIP(g.launch(EPI_GATE, 2 * C, 256, stream));
    return T2S_OK;
}

int t2s_wg_in_cond_gate_fold_train(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                                   const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, void* G_hi, void* G_lo,
                                   int act_bchunks, const void* fold_A, float* fold_acc, int fold_init, int B, int C, int n_cond,
                                   int taps, int dilation, int L, int Lp, int halo, int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(X_hi, X_lo) || !planes_ok(acts_hi, acts_lo) || !planes_ok(G_hi, G_lo) || !bias ||
        !al16(bias))
        return T2S_EINVAL;
    if ((n_cond > 0 && !planes_ok(S_hi, S_lo)) || !fold_ok(fold_A, fold_acc, C)) return T2S_EINVAL;
    if (!gate_shape_ok(B, C, taps, dilation, L, Lp, halo, Mpad) || (act_bchunks != 0 && act_bchunks < cdiv(C, 32))) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(X_hi, X_lo, cdiv(C, 32), taps, dilation, S_hi, S_lo, cdiv(n_cond, 32));
    g.output(acts_hi, acts_lo, act_bchunks ? act_bchunks : cdiv(C, 32));      // oc = batch stride of the acts / sigmoid planes
    g.fold(fold_A, fold_acc, fold_init);
    g.a.G_hi = (u16*)G_hi; g.a.G_lo = (u16*)G_lo; g.a.tc = g.a.oc;
    g.a.C = C;
    T2S_CHECK_HIP(g.launch(EPI_GATE, 2 * C, gate_tile_rows(B, C, L), stream));
    return T2S_OK;
}

int t2s_wg_res_only_train(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                          int act_bchunks, const void* R_hi, const void* R_lo, void* X_hi, void* X_lo, int B, int C, int L, int Lp,
                          int halo, int Mpad, int pair8, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(acts_hi, acts_lo) || !planes_ok(X_hi, X_lo) || !planes_ok(R_hi, R_lo) || !bias ||
        !al16(bias))
        return T2S_EINVAL;
    if (C <= 0 || C % 4 || (pair8 && C % 32) || !geometry_ok(B, L, Lp, halo, Mpad, C)) return T2S_EINVAL;
    if (act_bchunks != 0 && act_bchunks < cdiv(C, 32)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(acts_hi, acts_lo, cdiv(C, 32), 1, 1, nullptr, nullptr, 0, act_bchunks);
    g.output(X_hi, X_lo, cdiv(C, 32));
    g.a.R_hi = (const u16*)R_hi; g.a.R_lo = (const u16*)R_lo;
    g.a.C = 0; g.a.n_res = C; g.a.pair8 = pair8 ? 1 : 0;
    T2S_CHECK_HIP(g.launch(EPI_RESSKIP, C, 128, stream));
    return T2S_OK;
}

int t2s_wg_skip_sum(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                    int n_k_chunks, int act_bchunks, float* skip, int B, int C, int L, int Lp, int halo, int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(acts_hi, acts_lo) || !bias || !al16(bias) || !skip || !al16(skip)) return T2S_EINVAL;
    if (C <= 0 || C % 4 || n_k_chunks <= 0 || !geometry_ok(B, L, Lp, halo, Mpad, C)) return T2S_EINVAL;
    if (act_bchunks != 0 && act_bchunks < n_k_chunks) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(acts_hi, acts_lo, n_k_chunks, 1, 1, nullptr, nullptr, 0, act_bchunks);
    g.output(nullptr, nullptr, cdiv(C, 32));
    g.a.skip = skip; g.a.C = C; g.a.n_res = 0; g.a.skip_init = 1;
    T2S_CHECK_HIP(g.launch(EPI_RESSKIP, C, lockstep_tile_rows(B, C, L), stream));
    return T2S_OK;
}

int t2s_wg_res_skip_train(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi,
                          const void* acts_lo, const void* R_hi, const void* R_lo, void* X_hi, void* X_lo, float* skip,
                          int B, int C, int n_res, int skip_init, int L, int Lp, int halo, int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(acts_hi, acts_lo) || !bias || !al16(bias) || !skip || !al16(skip)) return T2S_EINVAL;
    if (n_res > 0 && (!planes_ok(X_hi, X_lo) || !planes_ok(R_hi, R_lo))) return T2S_EINVAL;
    if (C <= 0 || C % 4 || (n_res != 0 && n_res != C) || !geometry_ok(B, L, Lp, halo, Mpad, n_res + C)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(acts_hi, acts_lo, cdiv(C, 32), 1, 1);
    g.output(X_hi, X_lo, cdiv(C, 32));
    g.a.R_hi = (const u16*)R_hi; g.a.R_lo = (const u16*)R_lo;
    g.a.skip = skip; g.a.C = C; g.a.n_res = n_res; g.a.skip_init = skip_init;
    T2S_CHECK_HIP(g.launch(EPI_RESSKIP, n_res + C, 256, stream));
    return T2S_OK;
}

int t2s_wg_bwd_gate_dgrad(const void* A_hi, const void* A_lo, const float* zero_bias, const void* DX_hi,
                          const void* DX_lo, const void* DS_hi, const void* DS_lo, const void* T_hi, const void* T_lo,
                          const void* G_hi, const void* G_lo, int tg_bchunks, void* DP_hi, void* DP_lo, int dp_bchunks, int B, int C,
                          int L, int Lp, int halo, int Mpad, int pair8, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(DS_hi, DS_lo) || !planes_ok(T_hi, T_lo) || !planes_ok(G_hi, G_lo) ||
        !planes_ok(DP_hi, DP_lo) || !zero_bias)
        return T2S_EINVAL;
    if (DX_hi && !planes_ok(DX_hi, DX_lo)) return T2S_EINVAL;
    if (C <= 0 || C % 32 || !geometry_ok(B, L, Lp, halo, Mpad, C)) return T2S_EINVAL;
    if ((dp_bchunks != 0 && dp_bchunks < 2 * (C / 32)) || (tg_bchunks != 0 && tg_bchunks < C / 32)) return T2S_EINVAL;
    const int cc = C / 32;
    ConvGemm g(A_hi, A_lo, zero_bias);
    g.geometry(B, L, Lp, halo, Mpad);
    if (DX_hi) g.k_side(DX_hi, DX_lo, cc, 1, 1, DS_hi, DS_lo, cc);      // K = [d_x channels | d_skip channels]
    else g.k_side(DS_hi, DS_lo, cc, 1, 1);                              // last layer: only skip rows exist
    g.output(DP_hi, DP_lo, dp_bchunks ? dp_bchunks : 2 * cc);           // oc = batch stride of the output planes (a slice of a wider set)
    g.a.T_hi = (u16*)T_hi; g.a.T_lo = (u16*)T_lo; g.a.G_hi = (u16*)G_hi; g.a.G_lo = (u16*)G_lo;
    g.a.tc = tg_bchunks ? tg_bchunks : cc;                              // the same for the saved gate output / sigmoid planes
    g.a.C = C; g.a.pair8 = pair8 ? 1 : 0;
    const bool pp = bwd_pp256(g.a, C);
    if (pair8 && !pp) return T2S_EINVAL;        // PERM_PAIR8 operands need the 256-row ping-pong kernel (t2s_wg_bwd_pair8_ok)
    T2S_CHECK_HIP(g.launch(EPI_GATE_BWD, C, pp ? 256 : lockstep_tile_rows(B, C, L), stream, pp));
    return T2S_OK;
}

int t2s_conv_accumulate(const void* A_hi, const void* A_lo, const float* zero_bias, const void* X_hi, const void* X_lo,
                        int x_bchunks, void* O_hi, void* O_lo, int B, int Cin, int Cout, int taps, int dilation, int init, int L, int Lp,
                        int halo, int Mpad, int pair8, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(X_hi, X_lo) || !planes_ok(O_hi, O_lo) || !zero_bias) return T2S_EINVAL;
    if (Cin <= 0 || Cout <= 0 || Cout % 4 || !taps_ok(taps, dilation, halo) || !geometry_ok(B, L, Lp, halo, Mpad, Cout)) return T2S_EINVAL;
    if ((x_bchunks != 0 && x_bchunks < cdiv(Cin, 32)) || (pair8 && Cout % 32)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, zero_bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(X_hi, X_lo, cdiv(Cin, 32), taps, dilation, nullptr, nullptr, 0, x_bchunks);
    g.output(O_hi, O_lo, cdiv(Cout, 32));
    g.a.C = 0; g.a.n_res = Cout; g.a.res_init = init;      // every row takes the residual branch
    g.a.pair8 = pair8 ? 1 : 0;
    const bool pp = bwd_pp256(g.a, Cout);
    if (pair8 && !pp) return T2S_EINVAL;        // PERM_PAIR8 operands need the 256-row ping-pong kernel (t2s_wg_bwd_pair8_ok)
    T2S_CHECK_HIP(g.launch(EPI_RESSKIP, Cout, pp ? 256 : accumulate_tile_rows(B, Cout, L), stream, pp));
    return T2S_OK;
}

// The two weight-gradient GEMMs: M x N outputs over K = B x time chunks [k0, k1) of time-major planes, one f32 slab per K split.
static bool wgrad_shape_ok(const void* A_hi, const void* A_lo, const void* X_hi, const void* X_lo, const float* zero_bias, float* out,
                           int B, int M, int N, int Mpad, int Npad, int n_tchunks, int k0, int k1) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(X_hi, X_lo) || !zero_bias || !out) return false;
    return M > 0 && M % 4 == 0 && geometry_ok(B, N, Npad, 0, Mpad, M) && n_tchunks > 0 && k0 >= 0 && k1 <= n_tchunks && k0 < k1;
}
// `slabs` grid batch entries, each a K range of kchunk steps
static void wgrad_fill(ConvGemm& g, const void* X_hi, const void* X_lo, float* out, int slabs, int M, int N, int Mpad, int Npad,
                       int n_tchunks, int k0, int k1, int kchunk) {
    g.geometry(slabs, N, Npad, 0, Mpad);
    g.k_side(X_hi, X_lo, n_tchunks, 1, 1);
    g.output(nullptr, nullptr, cdiv(M, 32));
    g.a.a_bstride = (long)n_tchunks * Mpad * 32;
    g.a.out_f32 = out; g.a.C = M; g.a.act = ACT_NONE;
    g.a.k0 = k0; g.a.kend = k1; g.a.kchunk = kchunk;
}

int t2s_wgrad_gemm(const void* A_hi, const void* A_lo, const void* X_hi, const void* X_lo, const float* zero_bias,
                   float* out, int B, int M, int N, int Mpad, int Npad, int n_tchunks, int k0, int k1, int ksplit,
                   void* stream) {
    if (!wgrad_shape_ok(A_hi, A_lo, X_hi, X_lo, zero_bias, out, B, M, N, Mpad, Npad, n_tchunks, k0, k1)) return T2S_EINVAL;
    if (ksplit < 1 || ksplit > 16) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, zero_bias);
    wgrad_fill(g, X_hi, X_lo, out, B * ksplit, M, N, Mpad, Npad, n_tchunks, k0, k1, cdiv(k1 - k0, ksplit));
    g.a.ksplit = ksplit;
    // unsplit from chunk 0: the kernel takes its plain path and walks a.nk K-steps from chunk 0, so a.nk is where [0, k1) ends (the
    // A / X addressing goes by n_tchunks through a_bstride and xc, not by nk); every other form clips to kend in the kernel
    if (ksplit == 1 && k0 == 0) g.a.nk = k1;
    T2S_CHECK_HIP(g.launch(EPI_BIAS_ACT, M, 256, stream));
    return T2S_OK;
}

int t2s_wgrad_gemm_flat(const void* A_hi, const void* A_lo, const void* X_hi, const void* X_lo, const float* zero_bias,
                        float* out, int B, int M, int N, int Mpad, int Npad, int n_tchunks, int k0, int k1, int nsplit,
                        void* stream) {
    if (!wgrad_shape_ok(A_hi, A_lo, X_hi, X_lo, zero_bias, out, B, M, N, Mpad, Npad, n_tchunks, k0, k1)) return T2S_EINVAL;
    if (nsplit < 1 || nsplit > B * (k1 - k0)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, zero_bias);
    wgrad_fill(g, X_hi, X_lo, out, nsplit, M, N, Mpad, Npad, n_tchunks, k0, k1, cdiv(B * (k1 - k0), nsplit));
    g.a.ksplit = 1; g.a.kflat = B;
    if ((long)g.a.kchunk * (nsplit - 1) >= (long)B * (k1 - k0)) return T2S_EINVAL;      // every slab must own >= 1 K-step
    T2S_CHECK_HIP(g.launch(EPI_BIAS_ACT, M, 256, stream));
    return T2S_OK;
}

int t2s_wgrad_cl(const t2s_wgrad_chunk* a_chunks, int n_a_chunks, const t2s_wgrad_chunk* b_chunks, int n_b_chunks, float* out,
                 int B, int M, int N, int ldp, int k0, int k1, int nsplit, int bias_cols, void* stream) {
    static_assert(sizeof(t2s_wgrad_chunk) == sizeof(WgradChunk), "t2s_wgrad_chunk layout");
    if (!a_chunks || !b_chunks || !out || B <= 0 || M <= 0 || N <= 0 || k0 < 0 || k0 >= k1 || nsplit < 1) return T2S_EINVAL;
    // (bias_cols on whole N tiles only: t2s_launch_wgrad_cl, which holds the same three conditions, says why)
    if (ldp < N || (ldp % 4 == 0 && !al16(out)) || (bias_cols && (ldp % 4 || ldp < N + 4 || N % 256))) return T2S_EINVAL;
    const int n_mtiles = cdiv(M, 256), n_ntiles = cdiv(N, 256);
    if (n_a_chunks != n_mtiles * 8 || n_b_chunks != n_ntiles * 8 || nsplit > B * (k1 - k0)) return T2S_EINVAL;
    WgradClArgs a;
    a.a_chunks = (const WgradChunk*)a_chunks; a.b_chunks = (const WgradChunk*)b_chunks; a.P = out;
    a.M = M; a.N = N; a.ldp = ldp; a.n_mtiles = n_mtiles; a.n_ntiles = n_ntiles; a.B = B; a.k0 = k0; a.k1 = k1;
    a.nslab = nsplit; a.kchunk = cdiv(B * (k1 - k0), nsplit);
    a.bias_cols = bias_cols ? 1 : 0;
    if ((long)a.kchunk * (nsplit - 1) >= (long)B * (k1 - k0)) return T2S_EINVAL;      // every slab must own >= 1 K-block
    T2S_CHECK_HIP(t2s_launch_wgrad_cl(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_plane_transpose(const void* src_hi, const void* src_lo, int B, int src_chunks, int n_chunks, int Lp, int shift,
                        void* dst_hi, void* dst_lo, int Npad, int n_off, void* stream) {
    if (!planes_ok(src_hi, src_lo) || !planes_ok(dst_hi, dst_lo) || B <= 0 || n_chunks <= 0 || n_chunks > src_chunks ||
        Lp <= 0 || n_off % 32 || n_off + n_chunks * 32 > Npad)
        return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_plane_transpose((const u16*)src_hi, (const u16*)src_lo, B, src_chunks, n_chunks, Lp, shift,
                                             (u16*)dst_hi, (u16*)dst_lo, Npad, n_off, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_tm_ones_row(void* dst_hi, void* dst_lo, int B, int Lp, int halo, int L, int Npad, int n_row, void* stream) {
    if (!dst_hi || !dst_lo || B <= 0 || Lp <= 0 || n_row < 0 || n_row >= Npad) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_tm_ones_row((u16*)dst_hi, (u16*)dst_lo, B, Lp, halo, L, Npad, n_row, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_pack_transposed(const float* v, const float* scale, int O, int Cin, int Kt, int flip, int O_pad, int Mpad,
                        int koff, void* A_hi, void* A_lo, int pair8, void* stream) {
    if (!v || !planes_ok(A_hi, A_lo) || O <= 0 || Cin <= 0 || Kt <= 0 || O_pad % 32 || O_pad < O || Mpad % 256 ||
        Mpad < Cin || koff % 32 || (pair8 && Cin % 32))
        return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_pack_transposed(v, scale, O, Cin, Kt, flip, O_pad, Mpad, koff, (u16*)A_hi, (u16*)A_lo, pair8 ? 1 : 0,
                                             (hipStream_t)stream));
    return T2S_OK;
}

int t2s_weightnorm_scale(const float* v, const float* g, int O, int K, float* scale, void* stream) {
    if (!v || !scale || O <= 0 || K <= 0) return T2S_EINVAL;
    hipLaunchKernelGGL(weightnorm_scale_kernel, dim3((O + 255) / 256), dim3(256), 0, (hipStream_t)stream, v, g, O, K, scale);
    T2S_CHECK_HIP(hipGetLastError());
    return T2S_OK;
}

int t2s_wn_backward(const float* P, int nsplit, int Prows, int Pcols, int row_off, int col_off, int tap_stride,
                    int col_bias, int n_bias_cols, const float* v, const float* g, int O, int Cin, int Kt, float* dv, float* dg,
                    float* db, int db_accum, void* stream) {
    if (!P || !v || !dv || (g && !dg) || nsplit <= 0 || O <= 0 || Cin <= 0 || Kt <= 0) return T2S_EINVAL;
    if (n_bias_cols < 1) n_bias_cols = 1;
    if (row_off + O > Prows || col_off + (Kt - 1) * tap_stride + Cin > Pcols || (db && col_bias + n_bias_cols > Pcols)) return T2S_EINVAL;
    if ((size_t)Cin * Kt * sizeof(float) > 48 * 1024) return T2S_EINVAL;
    WnBwdArgs a;
    a.P = P; a.v = v; a.g = g; a.dv = dv; a.dg = dg; a.db = db;
    a.nsplit = nsplit; a.Prows = Prows; a.Pcols = Pcols; a.row_off = row_off; a.col_off = col_off;
    a.tap_stride = tap_stride; a.col_bias = col_bias; a.n_bias_cols = n_bias_cols; a.O = O; a.Cin = Cin; a.Kt = Kt; a.db_accum = db_accum;
    T2S_CHECK_HIP(t2s_launch_wn_backward(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_affine_backward(float* z, float* dz, const float* wn_out, const float* g_log_s, int g_log_s_scalar, float* d_out, int B,
                           int n_group, int c_off, int n_half, int L, void* stream) {
    if (!z || !dz || !wn_out || !d_out || B <= 0 || L <= 0 || n_half <= 0 || c_off < 0 || c_off + 2 * n_half > n_group)
        return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_affine_backward(z, dz, wn_out, g_log_s, g_log_s_scalar, d_out, B, n_group, c_off, n_half, L,
                                             (hipStream_t)stream));
    return T2S_OK;
}

long t2s_small_wgrad_scratch(int B, int chunks) { return (long)t2s_small_wgrad_scratch_floats(B, chunks); }

int t2s_small_wgrad(const void* P_hi, const void* P_lo, const float* P_f32, const float* Q, float* out, float* rowsum,
                    float* scratch, int B, int chunks, int Lp, int halo, int L, int R, int J, int Jtot, int q_off, int out_transposed,
                    void* stream) {
    if ((!P_f32 && (!P_hi || !P_lo)) || !Q || !out || !scratch || B <= 0 || chunks <= 0 || L <= 0 || R <= 0 || R > chunks * 32 ||
        J <= 0 || J > 16 || q_off < 0 || q_off + J > Jtot)
        return T2S_EINVAL;
    SmallWgradArgs a;
    a.P_hi = (const u16*)P_hi; a.P_lo = (const u16*)P_lo; a.P_f32 = P_f32; a.Q = Q; a.out = out; a.rowsum = rowsum; a.scratch = scratch;
    a.B = B; a.chunks = chunks; a.Lp = Lp; a.halo = halo; a.L = L; a.R = R; a.J = J; a.Jtot = Jtot; a.q_off = q_off;
    a.out_transposed = out_transposed;
    T2S_CHECK_HIP(t2s_launch_small_wgrad(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_rows_sum(const float* Q, int B, int Jtot, int q_off, int J, int L, float* out, void* stream) {
    if (!Q || !out || B <= 0 || J <= 0 || q_off < 0 || q_off + J > Jtot || L <= 0) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_rows_sum(Q, B, Jtot, q_off, J, L, out, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_start_dgrad(const void* X_hi, const void* X_lo, const float* w, float* dz, int B, int n_group, int c_off,
                       int n_half, int C, int L, int Lp, int halo, void* stream) {
    if (!X_hi || !X_lo || !w || !dz || B <= 0 || L <= 0 || n_half <= 0 || n_half > 8 || c_off < 0 ||
        c_off + n_half > n_group || C <= 0)
        return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_start_dgrad((const u16*)X_hi, (const u16*)X_lo, w, dz, B, n_group, c_off, n_half, C, L, Lp,
                                         halo, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_convinv_wgrad(const float* dz, const float* zin, const float* Winv, const float* gscale_ptr, float gmul,
                         int B, int n_group, int c_off, int n, int L, float* dW, void* stream) {
    if (!dz || !zin || !Winv || !dW || B <= 0 || L <= 0 || n <= 0 || n > 16 || c_off < 0 || c_off + n > n_group) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_convinv_wgrad(dz, zin, Winv, gscale_ptr, gmul, B, n_group, c_off, n, L, dW, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_upsample_wgrad(const void* D_hi, const void* D_lo, const float* mel, int B, int n_mel, int frames, int ksize,
                          int stride, int n_group, int L, int Lp, int halo, float* dW, float* db, void* stream) {
    if (!D_hi || !D_lo || !mel || !dW || !db || B <= 0 || n_mel <= 0 || n_mel > 80 || frames <= 0 || L <= 0) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_upsample_wgrad((const u16*)D_hi, (const u16*)D_lo, mel, B, n_mel, frames, ksize, stride,
                                            n_group, L, Lp, halo, dW, (hipStream_t)stream));
    T2S_CHECK_HIP(t2s_launch_upsample_bgrad((const u16*)D_hi, (const u16*)D_lo, B, n_mel, n_group, L, Lp, halo, db,
                                            (hipStream_t)stream));
    return T2S_OK;
}

int t2s_adam_table(const t2s_adam_job* jobs, int n_jobs, long total_blocks, float lr, float beta1, float beta2,
                   float eps, int step, float gscale, float weight_decay, void* stream) {
    if (!jobs || n_jobs <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffL || step <= 0) return T2S_EINVAL;
    static_assert(sizeof(t2s_adam_job) == sizeof(AdamJob), "t2s_adam_job layout");
    // the bias corrections in double, rounded once: 1 - powf(0.999f, step) cancels to a relative error of 3e-6 that every element's step
    // would carry (profiles/tail_kernel_tests.md)
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    T2S_CHECK_HIP(t2s_launch_adam_table((const AdamJob*)jobs, n_jobs, total_blocks, lr, beta1, beta2, eps, bc1, bc2s, gscale,
                                        weight_decay, (hipStream_t)stream));
    return T2S_OK;
}

static bool table_ok(const t2s_adam_job* jobs, int n_jobs, long total_blocks) {
    return jobs && n_jobs > 0 && total_blocks > 0 && total_blocks <= 0x7fffffffL;
}

int t2s_grad_norm_partials(void) { return T2S_GRAD_NORM_BLOCKS; }

int t2s_grad_norm_table(const t2s_adam_job* jobs, int n_jobs, long total_blocks, float gscale, float max_norm, double* partial,
                        float* out, void* stream) {
    if (!table_ok(jobs, n_jobs, total_blocks) || !partial || !out || !(max_norm >= 0.f)) return T2S_EINVAL;      // (a NaN fails >=)
    T2S_CHECK_HIP(t2s_launch_grad_norm_table((const AdamJob*)jobs, n_jobs, total_blocks, gscale, max_norm, partial, out,
                                             (hipStream_t)stream));
    return T2S_OK;
}

int t2s_grad_scale_table(const t2s_adam_job* jobs, int n_jobs, long total_blocks, const float* clip, void* stream) {
    if (!table_ok(jobs, n_jobs, total_blocks) || !clip) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_grad_scale_table((const AdamJob*)jobs, n_jobs, total_blocks, clip, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_adam_table_clip(const t2s_adam_job* jobs, int n_jobs, long total_blocks, float lr, float beta1, float beta2, float eps,
                        int step, float gscale, float weight_decay, const float* clip, int skip_nonfinite, void* stream) {
    if (!table_ok(jobs, n_jobs, total_blocks) || step <= 0 || !clip) return T2S_EINVAL;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));      // as t2s_adam_table
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    T2S_CHECK_HIP(t2s_launch_adam_table_clip((const AdamJob*)jobs, n_jobs, total_blocks, lr, beta1, beta2, eps, bc1, bc2s, gscale,
                                             weight_decay, clip, skip_nonfinite, (hipStream_t)stream));
    return T2S_OK;
}

}  // extern "C"
