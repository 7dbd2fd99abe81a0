// extern "C" boundary: argument validation + launch.  No torch types, no allocation, no sync.
#include "../../include/t2s_hip.h"
#include "t2s_kernels.h"
#include "t2s_api_common.h"
#include "conv_gemm_args.h"

#include <stdlib.h>
#include <string.h>

static thread_local char g_hip_err[256] = "";

extern "C" int t2s_internal_fail_hip(int ei) {
    hipError_t e = (hipError_t)ei;
    strncpy(g_hip_err, hipGetErrorString(e), sizeof(g_hip_err) - 1);
    g_hip_err[sizeof(g_hip_err) - 1] = 0;
    return T2S_EHIP;
}

// ---- entry points that exist in two operand formats: the build's default planes, and (`h16`, the _h16 symbols) fp16 planes with
// a one-plane A operand whose lo pointer is never read.  One body each, so that the checks cannot drift apart.

// the A operand: a (hi, lo) pair, or with h16 the hi plane alone
static inline bool a_operand_ok(const void* A_hi, const void* A_lo, bool h16) { return h16 ? (A_hi && al16(A_hi)) : planes_ok(A_hi, A_lo); }

static int pack_table(const t2s_pack_job* jobs, int n_jobs, long total_rows, void* stream, bool h16) {
    if (!jobs || n_jobs <= 0 || total_rows <= 0 || total_rows > 0x7fffffffL) return T2S_EINVAL;
    static_assert(sizeof(t2s_pack_job) == sizeof(PackJob), "t2s_pack_job layout");
    T2S_CHECK_HIP(t2s_launch_pack_table((const PackJob*)jobs, n_jobs, total_rows, (hipStream_t)stream, h16));
    return T2S_OK;
}

static int upsample_squeeze(const float* mel, const float* W, const float* bias, int B, int n_mel, int frames, int ksize, int stride,
                            int n_group, int L, int Lp, int halo, void* S_hi, void* S_lo, void* stream, bool h16) {
    if (!mel || !W || !bias || !S_hi || !S_lo) return T2S_EINVAL;
    if (B <= 0 || n_mel <= 0 || frames <= 0 || L <= 0 || n_group <= 0 || stride <= 0 || ksize % stride) return T2S_EINVAL;
    if (!al16(W) || !al16(S_hi) || !al16(S_lo)) return T2S_EINVAL;
    if (Lp < t2s_plane_rows(L, halo)) return T2S_EINVAL;
    // every squeezed sample must exist in the transposed-conv output (reference glow.py:216 assert)
    if ((long)L * n_group > (long)(frames - 1) * stride + ksize) return T2S_EINVAL;
    if (n_group == 8 && (stride % 8 || ksize % 8)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_upsample_squeeze(mel, W, bias, B, n_mel, frames, ksize, stride, n_group, L, Lp, halo,
                                              (u16*)S_hi, (u16*)S_lo, (hipStream_t)stream, h16));
    return T2S_OK;
}

// `lengths` (h16 only): t2s_wg_start_h16_ragged
static int wg_start(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C, int L, int Lp,
                    int halo, void* X_hi, void* X_lo, void* stream, bool h16, const int* lengths = nullptr) {
    if (!z || !w || !bias || !X_hi || !X_lo) return T2S_EINVAL;
    if (B <= 0 || L <= 0 || C <= 0 || n_half <= 0 || n_half > 8 || c_off < 0 || c_off + n_half > n_group) return T2S_EINVAL;
    if (!al16(X_hi) || !al16(X_lo) || Lp < t2s_plane_rows(L, halo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_start(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, (u16*)X_hi, (u16*)X_lo,
                                   (hipStream_t)stream, 0, 0, nullptr, nullptr, lengths, h16));
    return T2S_OK;
}

static int endfold_weights(const t2s_endfold_job* jobs, int n_jobs, int C, void* stream, bool h16) {
    if (!jobs || n_jobs <= 0 || C <= 0 || (size_t)8 * C * sizeof(float) > 60 * 1024) return T2S_EINVAL;
    static_assert(sizeof(t2s_endfold_job) == sizeof(EndFoldJob), "t2s_endfold_job layout");
    T2S_CHECK_HIP(t2s_launch_endfold_weights((const EndFoldJob*)jobs, n_jobs, C, (hipStream_t)stream, h16));
    return T2S_OK;
}

static int in_cond_gate_fold(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                             const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A, float* fold_acc,
                             int fold_init, int B, int C, int n_cond, int taps, int dilation, int L, int Lp, int halo, int Mpad,
                             void* stream, bool h16, const int* lengths = nullptr) {
    if (!a_operand_ok(A_hi, A_lo, h16) || !planes_ok(X_hi, X_lo) || !planes_ok(acts_hi, acts_lo) || !bias || !al16(bias)) return T2S_EINVAL;
    if ((n_cond > 0 && !planes_ok(S_hi, S_lo)) || !fold_ok(fold_A, fold_acc, C)) return T2S_EINVAL;
    if (!gate_shape_ok(B, C, taps, dilation, L, Lp, halo, Mpad)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(X_hi, X_lo, cdiv(C, 32), taps, dilation, S_hi, S_lo, cdiv(n_cond, 32));
    g.output(acts_hi, acts_lo, cdiv(C, 32));
    g.fold(fold_A, fold_acc, fold_init);
    g.a.C = C;
    g.a.lengths = lengths;      // (h16 only: t2s_wg_in_cond_gate_fold_h16_ragged)
    T2S_CHECK_HIP(g.launch(EPI_GATE, 2 * C, gate_tile_rows(B, C, L), stream, false, h16));
    return T2S_OK;
}

extern "C" {

int t2s_abi_version(void) { return 4; }

int t2s_sizeof_taco_decoder(void) { return (int)sizeof(t2s_taco_decoder); }
int t2s_sizeof_taco_bptt(void) { return (int)sizeof(t2s_taco_bptt); }

int t2s_operand_format(void) {
#ifdef T2S_SPLIT_F16
    return 1;
#else
    return 0;
#endif
}

const char* t2s_error_string(int code) {
    switch (code) {
        case T2S_OK: return "ok";
        case T2S_EINVAL: return "invalid argument";
        case T2S_EHIP: return "HIP runtime error";
        default: return "unknown error";
    }
}
const char* t2s_last_hip_error(void) { return g_hip_err; }

int t2s_plane_rows(int L, int halo) { return cdiv(L, 256) * 256 + 2 * halo; }
int t2s_padded_rows(int rows) { return cdiv(rows, 256) * 256; }

int t2s_pack_conv_weight(const float* v, const float* g, int g_is_scale, const float* bias_in, int O, int Cin, int Kt,
                         int perm, int C_gate, int row_off, int Mpad, int koff, int Cin_pad, void* A_hi, void* A_lo,
                         float* bias_out, int bias_accumulate, void* stream) {
    if (!v || !A_hi || !A_lo || O <= 0 || Cin <= 0 || Kt <= 0) return T2S_EINVAL;
    if (Mpad % 256 || koff % 32 || Cin_pad % 32 || Cin_pad < Cin) return T2S_EINVAL;
    if (perm == T2S_PERM_GATE) {
        if (O != 2 * C_gate || cdiv(C_gate, 128) * 256 > Mpad) return T2S_EINVAL;
    } else if (perm == T2S_PERM_NONE) {
        if (row_off < 0 || row_off + O > Mpad) return T2S_EINVAL;
    } else {
        return T2S_EINVAL;
    }
    PackArgs a;
    a.v = v; a.g = g; a.bias_in = bias_in;
    a.A_hi = (u16*)A_hi; a.A_lo = (u16*)A_lo; a.bias_out = bias_out;
    a.O = O; a.Cin = Cin; a.Kt = Kt; a.perm = perm; a.C_gate = C_gate; a.Mpad = Mpad; a.koff = koff;
    a.Cin_pad = Cin_pad; a.bias_accumulate = bias_accumulate; a.row_off = row_off; a.g_is_scale = g_is_scale;
    T2S_CHECK_HIP(t2s_launch_pack(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_pack_conv_weight_table(const t2s_pack_job* jobs, int n_jobs, long total_rows, void* stream) {
    return pack_table(jobs, n_jobs, total_rows, stream, false);
}
int t2s_pack_conv_weight_table_h16(const t2s_pack_job* jobs, int n_jobs, long total_rows, void* stream) {
    return pack_table(jobs, n_jobs, total_rows, stream, true);
}

int t2s_weightnorm_small(const float* v, const float* g, int O, int K, float* w, void* stream) {
    if (!v || !w || O <= 0 || K <= 0) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_weightnorm_small(v, g, O, K, w, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_upsample_squeeze(const float* mel, const float* W, const float* bias, int B, int n_mel, int frames,
                            int ksize, int stride, int n_group, int L, int Lp, int halo, void* S_hi, void* S_lo,
                            void* stream) {
    return upsample_squeeze(mel, W, bias, B, n_mel, frames, ksize, stride, n_group, L, Lp, halo, S_hi, S_lo, stream, false);
}
int t2s_wg_upsample_squeeze_h16(const float* mel, const float* W, const float* bias, int B, int n_mel, int frames,
                                int ksize, int stride, int n_group, int L, int Lp, int halo, void* S_hi, void* S_lo,
                                void* stream) {
    return upsample_squeeze(mel, W, bias, B, n_mel, frames, ksize, stride, n_group, L, Lp, halo, S_hi, S_lo, stream, true);
}

int t2s_wg_audio_squeeze(float* audio, float* z, int B, int T, int n_group, int L, int unsqueeze, void* stream) {
    if (!audio || !z || B <= 0 || L <= 0 || n_group <= 0 || (long)L * n_group > T) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_audio_squeeze(audio, z, B, T, n_group, L, unsqueeze, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_audio_window(const float* z, int B, int G, int L, int k0, int k1, float* dst, long ld_dst, long dst_off, void* stream) {
    if (!z || !dst || B <= 0 || B > 65535 || G <= 0 || L <= 0 || k0 < 0 || k0 >= k1 || k1 > L || dst_off < 0 || ld_dst <= 0) return T2S_EINVAL;
    if ((long)(k1 - k0) * G > ld_dst - dst_off) return T2S_EINVAL;      // the kept samples must fit the row behind dst_off
    T2S_CHECK_HIP(t2s_launch_audio_window(z, B, G, L, k0, k1, dst, ld_dst, dst_off, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_convinv(float* z, const float* W, int B, int n_group, int c_off, int n_rem, int L, void* stream) {
    if (!z || !W || B <= 0 || L <= 0 || n_rem <= 0 || n_rem > 16 || c_off < 0 || c_off + n_rem > n_group) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_convinv(z, W, B, n_group, c_off, n_rem, L, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_small_logdet_inv(const float* W, int n, float scale, float* logdet_out, float* inv_out, void* stream) {
    if (!W || n <= 0 || n > 16 || (!logdet_out && !inv_out)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_small_logdet_inv(W, n, scale, logdet_out, inv_out, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_small_logdet_inv_batch(const t2s_small_mat_job* jobs, int n_jobs, float scale, void* stream) {
    if (!jobs || n_jobs <= 0) return T2S_EINVAL;
    static_assert(sizeof(t2s_small_mat_job) == sizeof(SmallMatJob), "t2s_small_mat_job layout");
    T2S_CHECK_HIP(t2s_launch_small_logdet_batch((const SmallMatJob*)jobs, n_jobs, scale, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_small_logdet_inv_batch_host(const t2s_small_mat_job* host_jobs, int n_jobs, float scale, void* stream) {
    if (!host_jobs || n_jobs <= 0 || n_jobs > 16) return T2S_EINVAL;
    for (int i = 0; i < n_jobs; ++i)
        if (!host_jobs[i].W || host_jobs[i].n <= 0 || host_jobs[i].n > 16) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_small_logdet_batch_host((const SmallMatJob*)host_jobs, n_jobs, scale, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_start(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                 int L, int Lp, int halo, void* X_hi, void* X_lo, void* stream) {
    return wg_start(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, X_hi, X_lo, stream, false);
}
int t2s_wg_start_h16(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                     int L, int Lp, int halo, void* X_hi, void* X_lo, void* stream) {
    return wg_start(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, X_hi, X_lo, stream, true);
}
int t2s_wg_start_h16_ragged(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                            int L, int Lp, int halo, void* X_hi, void* X_lo, const int* lengths, void* stream) {
    if (!lengths) return T2S_EINVAL;
    return wg_start(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, X_hi, X_lo, stream, true, lengths);
}

// window chunks of the folded WN.start: 2 (two column sets per chunk) or 4 (one), each set taps * (n_half + 1) columns wide
static bool win_chunks_ok(int taps, int n_half, int win_chunks) {
    if (taps <= 0 || !(taps & 1) || n_half <= 0 || (win_chunks != 2 && win_chunks != 4)) return false;
    return (4 / win_chunks) * taps * (n_half + 1) <= 32;
}

// t2s_wg_start_window and, with `lengths`, the window form of t2s_wg_start_ragged
static int start_window(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C, int L,
                        int Lp, int halo, void* X_hi, void* X_lo, int taps, int win_chunks, void* W_hi, void* W_lo,
                        const int* lengths, void* stream) {
    if (!z || !w || !bias || !planes_ok(X_hi, X_lo) || !planes_ok(W_hi, W_lo)) return T2S_EINVAL;
    if (B <= 0 || L <= 0 || C <= 0 || n_half <= 0 || n_half > 8 || c_off < 0 || c_off + n_half > n_group) return T2S_EINVAL;
    if (!win_chunks_ok(taps, n_half, win_chunks) || cdiv(C, 32) < win_chunks || Lp < t2s_plane_rows(L, halo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_start(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, (u16*)X_hi, (u16*)X_lo,
                                   (hipStream_t)stream, taps, win_chunks, (u16*)W_hi, (u16*)W_lo, lengths));
    return T2S_OK;
}

int t2s_wg_start_window(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                        int L, int Lp, int halo, void* X_hi, void* X_lo, int taps, int win_chunks, void* W_hi, void* W_lo,
                        void* stream) {
    return start_window(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, X_hi, X_lo, taps, win_chunks, W_hi, W_lo, nullptr, stream);
}

int t2s_wg_start_ragged(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                        int L, int Lp, int halo, void* X_hi, void* X_lo, int taps, int win_chunks, void* W_hi, void* W_lo,
                        const int* lengths, void* stream) {
    if (!lengths) return T2S_EINVAL;
    if (W_hi || W_lo)
        return start_window(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, X_hi, X_lo, taps, win_chunks, W_hi, W_lo, lengths, stream);
    // no window planes: t2s_wg_start's checks (taps and win_chunks are not read)
    if (!z || !w || !bias || !X_hi || !X_lo) return T2S_EINVAL;
    if (B <= 0 || L <= 0 || C <= 0 || n_half <= 0 || n_half > 8 || c_off < 0 || c_off + n_half > n_group) return T2S_EINVAL;
    if (!al16(X_hi) || !al16(X_lo) || Lp < t2s_plane_rows(L, halo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_start(z, w, bias, B, n_group, c_off, n_half, C, L, Lp, halo, (u16*)X_hi, (u16*)X_lo,
                                   (hipStream_t)stream, 0, 0, nullptr, nullptr, lengths));
    return T2S_OK;
}

int t2s_wg_startfold_weights(const float* v_in, const float* g_in, const float* w_start, const float* b_start, int C, int n_half,
                             int taps, int Mpad, int win_chunks, void* A_hi, void* A_lo, void* stream) {
    if (!v_in || !w_start || !b_start || !planes_ok(A_hi, A_lo)) return T2S_EINVAL;
    if (C <= 0 || !win_chunks_ok(taps, n_half, win_chunks)) return T2S_EINVAL;
    if (Mpad % 256 || Mpad < cdiv(C, 128) * 256 || (size_t)C * (n_half + 1) * sizeof(float) > 60 * 1024) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_startfold_weights(v_in, g_in, w_start, b_start, C, n_half, taps, Mpad, win_chunks, (u16*)A_hi, (u16*)A_lo,
                                               (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_in_cond_gate(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                        const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, int B, int C, int n_cond,
                        int taps, int dilation, int L, int Lp, int halo, int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(X_hi, X_lo) || !planes_ok(acts_hi, acts_lo) || !bias || !al16(bias)) return T2S_EINVAL;
    if ((n_cond > 0 && !planes_ok(S_hi, S_lo)) || !gate_shape_ok(B, C, taps, dilation, L, Lp, halo, Mpad)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(X_hi, X_lo, cdiv(C, 32), taps, dilation, S_hi, S_lo, cdiv(n_cond, 32));
    g.output(acts_hi, acts_lo, cdiv(C, 32));
    g.a.C = C;
    T2S_CHECK_HIP(g.launch(EPI_GATE, 2 * C, 256, stream));
    return T2S_OK;
}

int t2s_wg_res_skip(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                    void* X_hi, void* X_lo, float* skip, int B, int C, int n_res, int skip_init, int L, int Lp,
                    int halo, int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(acts_hi, acts_lo) || !bias || !al16(bias) || !skip || !al16(skip)) return T2S_EINVAL;
    if (n_res > 0 && !planes_ok(X_hi, X_lo)) return T2S_EINVAL;
    if (C <= 0 || C % 4 || (n_res != 0 && n_res != C) || !geometry_ok(B, L, Lp, halo, Mpad, n_res + C)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(acts_hi, acts_lo, cdiv(C, 32), 1, 1);
    g.output(X_hi, X_lo, cdiv(C, 32));
    g.a.skip = skip; g.a.C = C; g.a.n_res = n_res; g.a.skip_init = skip_init;
    T2S_CHECK_HIP(g.launch(EPI_RESSKIP, n_res + C, 256, stream));
    return T2S_OK;
}

int t2s_wg_endfold_weights(const t2s_endfold_job* jobs, int n_jobs, int C, void* stream) {
    return endfold_weights(jobs, n_jobs, C, stream, false);
}
int t2s_wg_endfold_weights_h16(const t2s_endfold_job* jobs, int n_jobs, int C, void* stream) {
    return endfold_weights(jobs, n_jobs, C, stream, true);
}

int t2s_wg_gate_tile_rows(int B, int C, int L) {
    if (B <= 0 || C <= 0 || L <= 0) return T2S_EINVAL;
    return gate_tile_rows(B, C, L);
}

int t2s_wg_gate_fold_slots(int B, int C, int L) {
    if (B <= 0 || C <= 0 || L <= 0) return T2S_EINVAL;
    return gate_tile_rows(B, C, L) == 128 ? 2 * cdiv(C, 64) : 2 * cdiv(C, 128);
}

int t2s_wg_in_cond_gate_fold(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                             const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                             float* fold_acc, int fold_init, int B, int C, int n_cond, int taps, int dilation, int L,
                             int Lp, int halo, int Mpad, void* stream) {
    return in_cond_gate_fold(A_hi, A_lo, bias, X_hi, X_lo, S_hi, S_lo, acts_hi, acts_lo, fold_A, fold_acc, fold_init, B, C, n_cond, taps,
                             dilation, L, Lp, halo, Mpad, stream, false);
}
int t2s_wg_in_cond_gate_fold_h16(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                                 const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                                 float* fold_acc, int fold_init, int B, int C, int n_cond, int taps, int dilation, int L,
                                 int Lp, int halo, int Mpad, void* stream) {
    return in_cond_gate_fold(A_hi, A_lo, bias, X_hi, X_lo, S_hi, S_lo, acts_hi, acts_lo, fold_A, fold_acc, fold_init, B, C, n_cond, taps,
                             dilation, L, Lp, halo, Mpad, stream, true);
}
int t2s_wg_in_cond_gate_fold_h16_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                                        const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                                        float* fold_acc, int fold_init, int B, int C, int n_cond, int taps, int dilation, int L,
                                        int Lp, int halo, int Mpad, const int* lengths, void* stream) {
    if (!lengths) return T2S_EINVAL;
    return in_cond_gate_fold(A_hi, A_lo, bias, X_hi, X_lo, S_hi, S_lo, acts_hi, acts_lo, fold_A, fold_acc, fold_init, B, C, n_cond, taps,
                             dilation, L, Lp, halo, Mpad, stream, true, lengths);
}

int t2s_wg_in_win_gate_fold(const void* A_hi, const void* A_lo, const float* bias, const void* W_hi, const void* W_lo,
                            const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                            float* fold_acc, int fold_init, int B, int C, int n_cond, int win_chunks, int L, int Lp, int halo,
                            int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(W_hi, W_lo) || !planes_ok(S_hi, S_lo) || !planes_ok(acts_hi, acts_lo) || !bias ||
        !al16(bias))
        return T2S_EINVAL;
    if (!fold_ok(fold_A, fold_acc, C) || C <= 0 || n_cond <= 0 || halo < 0 || (win_chunks != 2 && win_chunks != 4)) return T2S_EINVAL;
    if (!geometry_ok(B, L, Lp, halo, Mpad, cdiv(C, 128) * 256)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    // the window planes' columns already hold the taps: a 1-tap "convolution" over win_chunks chunks, then the conditioning
    g.k_side(W_hi, W_lo, win_chunks, 1, 1, S_hi, S_lo, cdiv(n_cond, 32));
    g.output(acts_hi, acts_lo, cdiv(C, 32));
    g.fold(fold_A, fold_acc, fold_init);
    g.a.C = C;
    T2S_CHECK_HIP(g.launch(EPI_GATE, 2 * C, gate_tile_rows(B, C, L), stream));
    return T2S_OK;
}

int t2s_wg_upsample_basis(const float* W, const float* bias, int n_mel, int ksize, int stride, int n_group, int Lp, int halo,
                          void* U_hi, void* U_lo, void* stream) {
    if (!W || !bias || !planes_ok(U_hi, U_lo)) return T2S_EINVAL;
    if (n_mel <= 0 || n_group <= 0 || stride <= 0 || ksize <= 0 || ksize % stride || stride % n_group) return T2S_EINVAL;
    const int ncols = (stride / n_group) * (ksize / stride) * n_mel + 1;
    if (halo < 0 || Lp != t2s_plane_rows(ncols, halo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_upbasis_planes(W, bias, n_mel, ksize, stride, n_group, Lp, halo, (u16*)U_hi, (u16*)U_lo,
                                            (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_compose_cond(const float* tmp, const float* bias_in, int rows, int Mpad, int P, int K2, long ld, void* A2_hi,
                        void* A2_lo, float* bias_out, void* stream) {
    if (!tmp || !bias_in || !bias_out || !planes_ok(A2_hi, A2_lo)) return T2S_EINVAL;
    if (rows <= 0 || Mpad % 256 || rows > Mpad || P <= 0 || K2 <= 0 || K2 % 32 || ld < (long)P * K2 + 1) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_compose_pack(tmp, bias_in, rows, Mpad, P, K2, (int)ld, (u16*)A2_hi, (u16*)A2_lo, bias_out,
                                          (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_melwin_planes(const float* mel, int B, int n_mel, int frames, int nlag, int Fp, void* M_hi, void* M_lo, void* stream) {
    if (!mel || !planes_ok(M_hi, M_lo)) return T2S_EINVAL;
    if (B <= 0 || n_mel <= 0 || frames <= 0 || nlag <= 0 || Fp < frames) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_melwin_planes(mel, B, n_mel, frames, nlag, Fp, (u16*)M_hi, (u16*)M_lo, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_in_melwin_gate_fold(const void* A_hi, const void* A_lo, const void* A2_hi, const void* A2_lo, const float* bias,
                               const void* X_hi, const void* X_lo, const void* M_hi, const void* M_lo, void* acts_hi,
                               void* acts_lo, const void* fold_A, float* fold_acc, int fold_init, int B, int C, int K2,
                               int taps, int dilation, int L, int Lp, int halo, int Mpad, int P, int Fp, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(A2_hi, A2_lo) || !planes_ok(X_hi, X_lo) || !planes_ok(M_hi, M_lo) ||
        !planes_ok(acts_hi, acts_lo) || !bias || !al16(bias))
        return T2S_EINVAL;
    if (!fold_ok(fold_A, fold_acc, C) || !gate_shape_ok(B, C, taps, dilation, L, Lp, halo, Mpad)) return T2S_EINVAL;
    if (K2 <= 0 || K2 % 32 || P <= 0) return T2S_EINVAL;
    const int F = cdiv(L, P);
    // the phase tiles are 256 rows high: fold_acc must have been sized (t2s_wg_gate_fold_slots) for that tile height
    if (Fp < F || gate_tile_rows(B, C, L) != 256) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(X_hi, X_lo, cdiv(C, 32), taps, dilation, M_hi, M_lo, K2 / 32);
    g.output(acts_hi, acts_lo, cdiv(C, 32));
    g.fold(fold_A, fold_acc, fold_init);
    g.a.A2_hi = (const u16*)A2_hi; g.a.A2_lo = (const u16*)A2_lo;
    g.a.C = C;
    g.a.n_ttiles = 0;      // a phase tile's 256 columns are (batch entry, frame) pairs, ph_nft tiles per batch entry
    g.a.ph_P = P; g.a.ph_Fp = Fp;
    g.a.ph_FT = F <= 64 ? 64 : (F <= 128 ? 128 : 256);
    g.a.ph_bper = 256 / g.a.ph_FT;
    g.a.ph_nft = cdiv(F, g.a.ph_FT);
    T2S_CHECK_HIP(g.launch(EPI_GATE, 2 * C, 256, stream));
    return T2S_OK;
}

// t2s_wg_res_only and, with `lengths`, t2s_wg_res_only_ragged; with h16 their _h16 partners
static int res_only(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                    void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8, const int* lengths,
                    void* stream, bool h16 = false) {
    if (!a_operand_ok(A_hi, A_lo, h16) || !planes_ok(acts_hi, acts_lo) || !planes_ok(X_hi, X_lo) || !bias || !al16(bias)) return T2S_EINVAL;
    if (C <= 0 || C % 4 || (pair8 && C % 32) || !geometry_ok(B, L, Lp, halo, Mpad, C)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(acts_hi, acts_lo, cdiv(C, 32), 1, 1);
    g.output(X_hi, X_lo, cdiv(C, 32));
    g.a.C = 0; g.a.n_res = C; g.a.pair8 = pair8 ? 1 : 0;
    g.a.lengths = lengths;
    T2S_CHECK_HIP(g.launch(EPI_RESSKIP, C, 128, stream, false, h16));
    return T2S_OK;
}

int t2s_wg_res_only_h16(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                        void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8, void* stream) {
    return res_only(A_hi, A_lo, bias, acts_hi, acts_lo, X_hi, X_lo, B, C, L, Lp, halo, Mpad, pair8, nullptr, stream, true);
}

int t2s_wg_res_only(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                    void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8, void* stream) {
    return res_only(A_hi, A_lo, bias, acts_hi, acts_lo, X_hi, X_lo, B, C, L, Lp, halo, Mpad, pair8, nullptr, stream);
}

int t2s_wg_res_only_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                           void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8, const int* lengths,
                           void* stream) {
    if (!lengths) return T2S_EINVAL;
    return res_only(A_hi, A_lo, bias, acts_hi, acts_lo, X_hi, X_lo, B, C, L, Lp, halo, Mpad, pair8, lengths, stream);
}

int t2s_wg_res_only_h16_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                               void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8,
                               const int* lengths, void* stream) {
    if (!lengths) return T2S_EINVAL;
    return res_only(A_hi, A_lo, bias, acts_hi, acts_lo, X_hi, X_lo, B, C, L, Lp, halo, Mpad, pair8, lengths, stream, true);
}

// t2s_wg_res_only_start and, with `lengths`, t2s_wg_res_only_start_ragged
static int res_only_start(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                          const float* z, const float* w_start, const float* b_start, int n_group, int c_off, int n_half,
                          void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, const int* lengths, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(acts_hi, acts_lo) || !planes_ok(X_hi, X_lo) || !bias || !al16(bias)) return T2S_EINVAL;
    if (!z || !w_start || !b_start || n_half <= 0 || n_half > 4 || c_off < 0 || c_off + n_half > n_group) return T2S_EINVAL;
    if (C <= 0 || C % 32 || !geometry_ok(B, L, Lp, halo, Mpad, C)) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(acts_hi, acts_lo, cdiv(C, 32), 1, 1);
    g.output(X_hi, X_lo, cdiv(C, 32));
    g.a.C = 0; g.a.n_res = C; g.a.pair8 = 1;
    g.a.x0_z = z; g.a.x0_w = w_start; g.a.x0_b = b_start; g.a.x0_G = n_group; g.a.x0_coff = c_off; g.a.x0_nh = n_half;
    g.a.lengths = lengths;
    T2S_CHECK_HIP(g.launch(EPI_RESSKIP, C, 128, stream));
    return T2S_OK;
}

int t2s_wg_res_only_start(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                          const float* z, const float* w_start, const float* b_start, int n_group, int c_off, int n_half,
                          void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, void* stream) {
    return res_only_start(A_hi, A_lo, bias, acts_hi, acts_lo, z, w_start, b_start, n_group, c_off, n_half, X_hi, X_lo, B, C, L, Lp,
                          halo, Mpad, nullptr, stream);
}

int t2s_wg_res_only_start_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                                 const float* z, const float* w_start, const float* b_start, int n_group, int c_off, int n_half,
                                 void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, const int* lengths,
                                 void* stream) {
    if (!lengths) return T2S_EINVAL;
    return res_only_start(A_hi, A_lo, bias, acts_hi, acts_lo, z, w_start, b_start, n_group, c_off, n_half, X_hi, X_lo, B, C, L, Lp,
                          halo, Mpad, lengths, stream);
}

// t2s_wg_flow_boundary and, with `lengths`, t2s_wg_flow_boundary_ragged
static int flow_boundary(const float* z_in, float* z_out, const float* fold_acc, int nslots, const float* bes, int n_layers,
                         const float* b_end, float* log_s, int c_off_prev, int n_half_prev, const float* W, int c_off, int n_rem,
                         int n_half, int B, int n_group, int L, int Lp, int halo, int taps, int win_chunks, void* W_hi, void* W_lo,
                         const int* lengths, void* stream) {
    if (!z_in || !planes_ok(W_hi, W_lo) || z_out == z_in || ((fold_acc || W) && !z_out)) return T2S_EINVAL;
    if (B <= 0 || L <= 0 || n_group <= 0 || n_group > 16 || halo < 0 || Lp < t2s_plane_rows(L, halo)) return T2S_EINVAL;
    // n_half <= 4 like its partner t2s_wg_res_only_start and the folded WN.end (8 rows = b ; log_s of 4 channels)
    if (n_half <= 0 || n_half > 4 || c_off < 0 || c_off + n_half > n_group) return T2S_EINVAL;
    if (!win_chunks_ok(taps, n_half, win_chunks) || taps > t2s_flow_boundary_max_taps()) return T2S_EINVAL;
    if (W && (n_rem < n_half || n_rem > 16 || c_off + n_rem > n_group)) return T2S_EINVAL;
    if (fold_acc) {
        if (!bes || !b_end || nslots <= 0 || n_layers <= 0) return T2S_EINVAL;
        if (n_half_prev <= 0 || n_half_prev > 4 || c_off_prev < 0 || c_off_prev + 2 * n_half_prev > n_group) return T2S_EINVAL;
    }
    FlowBoundaryArgs a;
    memset(&a, 0, sizeof(a));
    a.z_in = z_in; a.z_out = z_out; a.fold_acc = fold_acc; a.bes = bes; a.b_end = b_end; a.log_s = fold_acc ? log_s : nullptr;
    a.W = W; a.W_hi = (u16*)W_hi; a.W_lo = (u16*)W_lo;
    a.nslots = nslots; a.n_layers = n_layers; a.c_off_prev = c_off_prev; a.nh_prev = n_half_prev;
    a.c_off = c_off; a.n_rem = n_rem; a.nh = n_half;
    a.G = n_group; a.L = L; a.Lp = Lp; a.halo = halo; a.taps = taps; a.nwc = win_chunks;
    a.lengths = lengths;
    T2S_CHECK_HIP(t2s_launch_flow_boundary(a, B, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_flow_boundary(const float* z_in, float* z_out, const float* fold_acc, int nslots, const float* bes, int n_layers,
                         const float* b_end, float* log_s, int c_off_prev, int n_half_prev, const float* W, int c_off, int n_rem,
                         int n_half, int B, int n_group, int L, int Lp, int halo, int taps, int win_chunks, void* W_hi, void* W_lo,
                         void* stream) {
    return flow_boundary(z_in, z_out, fold_acc, nslots, bes, n_layers, b_end, log_s, c_off_prev, n_half_prev, W, c_off, n_rem, n_half,
                         B, n_group, L, Lp, halo, taps, win_chunks, W_hi, W_lo, nullptr, stream);
}

int t2s_wg_flow_boundary_ragged(const float* z_in, float* z_out, const float* fold_acc, int nslots, const float* bes, int n_layers,
                                const float* b_end, float* log_s, int c_off_prev, int n_half_prev, const float* W, int c_off,
                                int n_rem, int n_half, int B, int n_group, int L, int Lp, int halo, int taps, int win_chunks,
                                void* W_hi, void* W_lo, const int* lengths, void* stream) {
    if (!lengths) return T2S_EINVAL;
    return flow_boundary(z_in, z_out, fold_acc, nslots, bes, n_layers, b_end, log_s, c_off_prev, n_half_prev, W, c_off, n_rem, n_half,
                         B, n_group, L, Lp, halo, taps, win_chunks, W_hi, W_lo, lengths, stream);
}

int t2s_wg_end_fold_affine(const float* fold_acc, int nslots, const float* bes, int n_layers, const float* b_end,
                           float* z, float* log_s, float* wn_out, int B, int n_group, int c_off, int n_half, int L, int reverse,
                           void* stream) {
    if (!fold_acc || !bes || !b_end || !z || nslots <= 0 || n_layers <= 0) return T2S_EINVAL;
    if (B <= 0 || L <= 0 || n_half <= 0 || n_half > 4 || c_off < 0 || c_off + 2 * n_half > n_group) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_end_fold_affine(fold_acc, nslots, bes, n_layers, b_end, z, log_s, wn_out, B, n_group, c_off, n_half,
                                             L, reverse, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_wg_end_affine(const float* skip, const float* w_end, const float* b_end, float* z, float* log_s,
                      float* wn_out, int B, int n_group, int c_off, int n_half, int C, int L, int Lp, int halo, int reverse, void* stream) {
    if (!skip || !w_end || !b_end || !z) return T2S_EINVAL;
    if (B <= 0 || L <= 0 || C <= 0 || n_half <= 0 || n_half > 8 || c_off < 0 || c_off + 2 * n_half > n_group) return T2S_EINVAL;
    if (Lp < t2s_plane_rows(L, halo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_end_affine(skip, w_end, b_end, z, log_s, wn_out, B, n_group, c_off, n_half, C, L, Lp, halo,
                                        reverse, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_conv_bias_act(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                      void* O_hi, void* O_lo, float* out_f32, int f32_channel_last, int B, int Cin, int Cout, int taps,
                      int dilation, int act, int L, int Lp, int halo, int Mpad, void* stream) {
    if (!planes_ok(A_hi, A_lo) || !planes_ok(X_hi, X_lo) || !bias || !al16(bias)) return T2S_EINVAL;
    if ((O_hi || O_lo) && !planes_ok(O_hi, O_lo)) return T2S_EINVAL;
    if (!O_hi && !out_f32) return T2S_EINVAL;
    if (Cin <= 0 || Cout <= 0 || Cout % 4 || !taps_ok(taps, dilation, halo) || !geometry_ok(B, L, Lp, halo, Mpad, Cout)) return T2S_EINVAL;
    if (act < T2S_ACT_NONE || act > T2S_ACT_TANH) return T2S_EINVAL;
    ConvGemm g(A_hi, A_lo, bias);
    g.geometry(B, L, Lp, halo, Mpad);
    g.k_side(X_hi, X_lo, cdiv(Cin, 32), taps, dilation);
    g.output(O_hi, O_lo, cdiv(Cout, 32));
    g.a.out_f32 = out_f32; g.a.C = Cout; g.a.act = act; g.a.f32_cl = f32_channel_last;
    T2S_CHECK_HIP(g.launch(EPI_BIAS_ACT, Cout, bias_act_tile_rows(B, Cout, L), stream));
    return T2S_OK;
}

}  // extern "C"
