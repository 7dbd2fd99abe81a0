// extern "C" boundary of the Tacotron-2 kernels: validation, argument blocks, and the decode-step driver.
#include "../../include/t2s_hip.h"
#include "t2s_kernels.h"
#include "t2s_api_common.h"
#include "tacotron_ops.h"
#include "t2s_handoff.h"

#include <stdlib.h>
#include <string.h>


// one fused attention launch per step (one workgroup per batch element) up to this batch; beyond it the three-kernel form
constexpr int ATT_FUSED_MAX_B = 8;
// streamed gate partials (t2s_taco_decoder::gate_part) up to this batch
constexpr int DECODE_STREAM_MAX_B = 4;
// teacher-forced decode with the decoder cells on the helper stream, unpaced: attention-chain steps per event
constexpr int DECODE_CHUNK = 16;

static int gemv_args_ok(const GemvArgs& a) {
    if (!a.W1 || !a.x1 || !a.y || a.rows <= 0 || a.items <= 0) return 0;
    const int K = a.n1 + a.n2 + a.n3;
    if (K != a.k1 + a.k2 || K > 4096) return 0;
    if ((a.n1 | a.n2 | a.n3 | a.k1 | a.k2 | a.ld1 | a.ld2) & 3) return 0;
    if ((a.sx1 | a.sx2 | a.sx3) & 3) return 0;
    if (!al16(a.W1) || !al16(a.x1) || (a.W2 && !al16(a.W2)) || (a.x2 && !al16(a.x2)) || (a.x3 && !al16(a.x3))) return 0;
    if ((a.n2 > 0 && !a.x2) || (a.n3 > 0 && !a.x3) || (a.k2 > 0 && !a.W2)) return 0;
    return 1;
}

extern "C" {

int t2s_gemv(const float* W1, int ld1, int k1, const float* W2, int ld2, int k2, const float* x1, int n1, long sx1,
             const float* x2, int n2, long sx2, const float* x3, int n3, long sx3, const float* bias1,
             const float* bias2, float* y, long sy_item, long sy_row, int rows, int items, int act,
             const unsigned char* mask, long smask_item, float mask_scale, void* stream) {
    GemvArgs a;
    memset(&a, 0, sizeof(a));
    a.W1 = W1; a.ld1 = ld1; a.k1 = k1; a.W2 = W2; a.ld2 = ld2; a.k2 = k2;
    a.x1 = x1; a.n1 = n1; a.sx1 = sx1; a.x2 = x2; a.n2 = n2; a.sx2 = sx2; a.x3 = x3; a.n3 = n3; a.sx3 = sx3;
    a.bias1 = bias1; a.bias2 = bias2; a.y = y; a.sy_item = sy_item; a.sy_row = sy_row; a.rows = rows; a.items = items;
    a.act = act; a.mask = mask; a.smask_item = smask_item; a.mask_scale = mask_scale;
    if (!gemv_args_ok(a) || act < 0 || act > 2) return T2S_EINVAL;
    a.split_row = 0; a.y2 = nullptr; a.sy2_item = a.sy2_row = 0; a.act2 = 0; a.mask2 = nullptr; a.smask2_item = 0; a.mask2_scale = 1.f;
    T2S_CHECK_HIP(t2s_launch_gemv(a, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_transpose(const float* in, float* out, int R, int C, void* stream) {
    if (!in || !out || R <= 0 || C <= 0) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_transpose(in, out, R, C, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_embed_planes(const long* ids, const float* emb, int B, int T, int E, int V, int Lp, int halo, void* X_hi,
                     void* X_lo, void* stream) {
    if (!ids || !emb || !X_hi || !X_lo || B <= 0 || T <= 0 || E <= 0 || V <= 0) return T2S_EINVAL;
    if (Lp < t2s_plane_rows(T, halo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_embed_planes(ids, emb, B, T, E, V, Lp, halo, (u16*)X_hi, (u16*)X_lo, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_f32_to_planes(const float* x, int B, int C, int L, int Lp, int halo, void* X_hi, void* X_lo, void* stream) {
    if (!x || !X_hi || !X_lo || B <= 0 || C <= 0 || L <= 0 || Lp < t2s_plane_rows(L, halo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_f32_to_planes(x, B, C, L, Lp, halo, (u16*)X_hi, (u16*)X_lo, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_taco_parse_output(float* mel, float* mel_post, float* gate, const int* lengths, int B, int n_mel, int T, void* stream) {
    if (!mel || !mel_post || !gate || !lengths || B <= 0 || n_mel <= 0 || T <= 0 || B > 65535 || n_mel >= 65535) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_parse_output(mel, mel_post, gate, lengths, B, n_mel, T, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_zero_plane_rows(void* X_hi, void* X_lo, const int* lengths, int B, int C, int T, int Lp, int halo, void* stream) {
    if (!X_hi || !X_lo || !lengths || B <= 0 || C <= 0 || T <= 0 || halo < 0 || B > 65535 || C > (1 << 20) || Lp < t2s_plane_rows(T, halo))
        return T2S_EINVAL;
    if (!al16(X_hi) || !al16(X_lo)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_zero_plane_rows((u16*)X_hi, (u16*)X_lo, lengths, B, (C + 31) / 32, T, Lp, halo, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_zero_rows_f32(float* x, const int* lengths, int B, int N, int row, void* stream) {
    if (!x || !lengths || B <= 0 || N <= 0 || row <= 0 || B > 65535 || (long)N * row > (1L << 36)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_zero_rows_f32(x, lengths, B, N, row, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* conv_bias,
                float eps, int C, float* scale, float* bias_out, void* stream) {
    if (!gamma || !beta || !mean || !var || !scale || !bias_out || C <= 0) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_bn_fold(gamma, beta, mean, var, conv_bias, eps, C, scale, bias_out, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_bn_train(const float* x, const float* gamma, const float* beta, float eps, int act, const unsigned char* mask,
                 float mask_scale, int B, int C, int T, int Lp, int halo, float* mean, float* var, void* O_hi, void* O_lo,
                 float* out_f32, void* stream) {
    if (!x || !gamma || !beta || !mean || !var || B <= 0 || C <= 0 || T <= 0 || act < 0 || act > 2) return T2S_EINVAL;
    if (!O_hi && !out_f32) return T2S_EINVAL;
    if (O_hi && (!O_lo || Lp < t2s_plane_rows(T, halo))) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_bn_train(x, gamma, beta, eps, act, mask, mask_scale, B, C, T, Lp, halo, mean, var,
                                      (u16*)O_hi, (u16*)O_lo, out_f32, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_bn_running_update(const float* mean, const float* var, float* running_mean, float* running_var,
                          long long* num_batches_tracked, float momentum, long long n, int C, void* stream) {
    if (!mean || !var || !running_mean || !running_var || C <= 0 || n <= 0 || !(momentum >= 0.f && momentum <= 1.f)) return T2S_EINVAL;
    const float unbias = n > 1 ? (float)((double)n / (double)(n - 1)) : 1.f;
    T2S_CHECK_HIP(t2s_launch_bn_running_update(mean, var, running_mean, running_var, num_batches_tracked, momentum, unbias, C,
                                               (hipStream_t)stream));
    return T2S_OK;
}

int t2s_zero_fill(void* p, size_t bytes, void* stream) {
    if (!p || ((uintptr_t)p & 15)) return T2S_EINVAL;
    if (bytes == 0) return T2S_OK;
    T2S_CHECK_HIP(t2s_launch_zero_fill(p, bytes, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_taco_encoder_lstm(const float* gx, const float* whhT_fwd, const float* whhT_rev, const int* lengths, float* out,
                          int B, int T, int H, int T_out, float* gates_save, float* c_save, void* stream) {
    if (!gx || !whhT_fwd || !whhT_rev || !out || B <= 0 || T <= 0 || T_out <= 0 || T_out > T || 4 * H != 1024) return T2S_EINVAL;
    if ((gates_save == nullptr) != (c_save == nullptr)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_lstm_seq(gx, whhT_fwd, whhT_rev, lengths, out, B, T, H, T_out, gates_save, c_save, (hipStream_t)stream));
    return T2S_OK;
}

long t2s_taco_lstm_xbuf_bytes(int B) { return B > 0 ? (long)(split_lstm_err_word(B) + 1) * 8 : -1; }

int t2s_taco_encoder_lstm_split(const float* gx, const float* whhT_fwd, const float* whhT_rev, const int* lengths, float* out,
                                int B, int T, int H, int T_out, float* gates_save, float* c_save, void* xbuf, unsigned epoch,
                                void* stream) {
    if (!gx || !whhT_fwd || !whhT_rev || !out || !xbuf || B <= 0 || T <= 0 || T >= SPLIT_LSTM_T_LIMIT || T_out <= 0 || T_out > T || H != 256 ||
        ((uintptr_t)xbuf & 7))
        return T2S_EINVAL;
    if ((gates_save == nullptr) != (c_save == nullptr)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_lstm_seq_split(gx, whhT_fwd, whhT_rev, lengths, out, B, T, T_out, gates_save, c_save,
                                            (unsigned long long*)xbuf, epoch, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_bernoulli_mask(unsigned char* mask, size_t n, unsigned long long seed, unsigned long long offset, float keep_prob,
                       void* stream) {
    if (!mask || n == 0 || !(keep_prob > 0.f && keep_prob <= 1.f)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_bernoulli_mask(mask, n, seed, offset, keep_prob, (hipStream_t)stream));
    return T2S_OK;
}

int t2s_taco_stop_check(const float* mel_gate_out, int B, int n_mel, int T_cap, int step0, int n, float threshold,
                        int* stop_step, void* stream) {
    if (!mel_gate_out || !stop_step || B <= 0 || step0 < 0 || n <= 0 || step0 + n > T_cap) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_stop_check(mel_gate_out + (size_t)n_mel * T_cap, B, (n_mel + 1) * T_cap, step0, n, threshold,
                                        stop_step, (hipStream_t)stream));
    return T2S_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Decoder-step driver.  Which kernels a step launches is decided ONCE per call (DecodePlan, from the struct's null pointers and
// shapes); the four step functions below only fill argument blocks from the plan and launch.  Per step remain the h ping-pong by
// step parity, the `+ s * ...` offsets and the two comparisons against mask_steps.  DESIGN.md section 5b lists the chains.
#define T2S_TRY(expr)                          \
    do {                                       \
        const int _rc = (expr);                \
        if (_rc != T2S_OK) return _rc;         \
    } while (0)

struct DecodePlan {
    bool split;          // teacher forced with att_h_all + hc_all: the decoder cells run on the helper stream ...
    bool paced;          // ... one step behind the attention chain, released by pace_flag (else in chunks of DECODE_CHUNK)
    bool sig_by_kernel;  // paced: the matrix-core attention cell stores the pace word itself (else a launch of its own)
    bool fused_att;      // one attention launch per step (else query + energies [+ softmax / context])
    bool q_parts;        // fused_att: the attention cell's workgroups leave partial queries
    bool q_big;          // three-launch form: the matrix-core attention cell leaves them, the energies kernel sums them (no query GEMV)
    bool one;            // three-launch form: the energies launch also does softmax, cumulative weights and context (att_xbuf)
    bool stream_gates;   // the fused attention launch streams the gate partials of the two cells (gate_part)
    bool fold_pre2;      // with stream_gates: prenet layer 1 inside the attention cell's launch (steps below mask_steps)
    bool use_ploc;       // with stream_gates: the location term comes out of the previous step's projection launch (ploc)
    bool proj_fused;     // projection and the next step's prenet layer 0 are one row block: one launch
    int units;           // hidden units per workgroup of lstm_cell_kernel: 2 with the training saves, else 4
    // not a decision of decode_plan: set by t2s_taco_decode_steps_w16 after it.  The cells and the gate-stream role then read the four
    // LSTM matrices from here as binary16 (the argument blocks carry them in their float pointers, tacotron_ops.h); NULL: f32 from `d`
    const t2s_taco_w16* w16;
};
// element `off` of a binary16 matrix, as the cells' argument blocks carry it
static const float* w16_at(const void* w, size_t off) { return (const float*)((const uint16_t*)w + off); }

static float* att_h_in(const t2s_taco_decoder& d, int s) { return (s & 1) ? d.att_h1 : d.att_h0; }
static float* att_h_out(const t2s_taco_decoder& d, int s) { return (s & 1) ? d.att_h0 : d.att_h1; }
static float* dec_h_in(const t2s_taco_decoder& d, int s) { return (s & 1) ? d.dec_h1 : d.dec_h0; }
static float* dec_h_out(const t2s_taco_decoder& d, int s) { return (s & 1) ? d.dec_h0 : d.dec_h1; }
// one [B][4H] block of gate_part
static size_t gate_block(const t2s_taco_decoder& d) { return (size_t)d.B * 4 * d.att_rnn_dim; }

// 1. attention LSTMCell on [prenet_out | context]
static void fill_att_cell(const t2s_taco_decoder& d, const DecodePlan& p, int s, LstmCellArgs& ca) {
    const int B = d.B, P = d.prenet_dim, E = d.enc_dim, A = d.att_rnn_dim;
    memset(&ca, 0, sizeof(ca));
    ca.W_ih = d.att_w_ih; ca.W_hh = d.att_w_hh; ca.b_ih = d.att_b_ih; ca.b_hh = d.att_b_hh;
    ca.x1 = d.teacher_forced ? d.pre_all + (size_t)s * B * P : d.pre2;
    ca.n1 = P; ca.sx1 = P; ca.x2 = d.ctx; ca.n2 = E; ca.sx2 = E;
    ca.h_in = att_h_in(d, s); ca.h_out = att_h_out(d, s); ca.c = d.att_c; ca.B = B; ca.H = A;
    if (d.att_drop) { ca.drop_mask = d.att_drop + (size_t)s * B * A; ca.drop_scale = d.att_drop_scale; }
    if (d.att_gates_all) { ca.gates_out = d.att_gates_all + (size_t)s * B * 4 * A; ca.c_out = d.att_c_all + (size_t)s * B * A; }
    if (d.att_h_all) { ca.h_copy = d.att_h_all + (size_t)s * B * A; ca.s_copy = A; }
    // small batch: the cell's workgroups emit partial queries (their own hidden units' columns of W_query), so the fused attention
    // kernel sums 128 KB of partials instead of pulling the 512 KB of W_query through one CU.  Large batch (matrix-core cells):
    // the same idea - every cell workgroup (4 hidden units) leaves a partial query and the energies kernel sums the A / 4 = 256 of
    // them - takes the query GEMM off the serial chain.
    if (p.q_parts || p.q_big) { ca.w_q = d.w_query; ca.q_part = d.q_part; ca.q_dim = d.att_dim; }
    // streamed gates: W_hh_att . h_att(s-1) was left in gate_part[2] by the previous step's attention launch (zero at step 0)
    if (p.stream_gates) { ca.h_in = nullptr; ca.pre_a = d.gate_part + 2 * gate_block(d); }
    if (p.paced) { ca.sig_ptr = (unsigned*)d.pace_flag; ca.sig_val = (unsigned)s + 1u; }
    // ... and with it the prenet's second layer folded into this launch (every workgroup recomputes the 256 outputs from pre1 and
    // W_pre2 out of L2) instead of a GEMV launch of its own at the end of the previous step; past the masks the cell reads pre2
    if (p.fold_pre2 && s < d.mask_steps) {
        ca.x1 = nullptr; ca.w_p2 = d.w_pre2T; ca.p1 = d.pre1;
        ca.p2_mask = d.prenet_masks + (size_t)s * B * 2 * P + P; ca.s_p2_mask = 2 * P; ca.p2_scale = 2.0f;
    }
    if (p.w16) { ca.W_ih = w16_at(p.w16->att_w_ih, 0); ca.W_hh = w16_at(p.w16->att_w_hh, 0); }
}

// 2.-4. attention: query, location-sensitive energies, softmax, context, cumulative weights
static void fill_att_args(const t2s_taco_decoder& d, const DecodePlan& p, int s, AttArgs& aa) {
    const int B = d.B, T = d.T_in, E = d.enc_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    memset(&aa, 0, sizeof(aa));
    aa.q = d.q; aa.w_loc_conv = d.w_loc_conv; aa.w_loc_dense = d.w_loc_dense; aa.w_v = d.w_v;
    aa.pmem = d.pmem; aa.memory = d.memory; aa.lengths = d.mem_lengths;
    aa.w_prev = d.att_w; aa.w_cum = d.att_wcum; aa.energies = d.energies; aa.ctx = d.ctx;
    aa.align_out = d.align_out + (size_t)s * T; aa.s_align_b = (long)d.T_cap * T;
    if (d.teacher_forced) { aa.ctx_copy = d.hc_all + (size_t)s * B * (D + E) + D; aa.s_ctx_copy = D + E; }
    aa.B = B; aa.T = T; aa.att_dim = d.att_dim; aa.enc_dim = E; aa.loc_f = d.loc_filters; aa.loc_ks = d.loc_kernel;
    aa.w_query = d.w_query; aa.h_att = att_h_out(d, s); aa.w_loc_denseT = d.w_loc_denseT; aa.att_rnn = A;
    if (d.q_all) aa.q_save = d.q_all + (size_t)s * B * d.att_dim;
    if (d.wcum_all) aa.wcum_save = d.wcum_all + (size_t)s * B * T;
    if (p.q_parts) { aa.q_part = d.q_part; aa.n_part = A / p.units; }
    // the location term of this step came out of the previous step's projection launch (zero at step 0)
    if (p.use_ploc) aa.ploc = d.ploc;
    if (p.fused_att) return;
    if (d.q_all) aa.q = d.q_all + (size_t)s * B * d.att_dim;         // the query goes straight into its save slot
    if (p.q_big) { aa.q_part = d.q_part; aa.n_part = A / 4; aa.q_out = (float*)aa.q; aa.q_save = nullptr; }
    // energies, softmax, cumulative weights and context in ONE launch where the shape allows (t2s_taco_decoder::att_xbuf: the
    // tiles of an element exchange their energies through tagged granules)
    if (p.one) { aa.xbuf = (unsigned long long*)d.att_xbuf; aa.tag = (unsigned)s + 1u; }
}

// the role beside the fused attention launch of step s: W_hh_dec . h_dec(s-1) and W_ih_dec[:, :A] . h_att(s) for this step's
// decoder cell, W_hh_att . h_att(s) for the next step's attention cell
static void fill_gate_stream(const t2s_taco_decoder& d, const DecodePlan& p, int s, GateStreamArgs& gs) {
    const int A = d.att_rnn_dim, D = d.dec_rnn_dim;
    const size_t GP = gate_block(d);
    memset(&gs, 0, sizeof(gs));
    gs.W0 = d.dec_w_hh; gs.ld0 = D; gs.x0 = dec_h_in(d, s); gs.out0 = d.gate_part;
    gs.W1 = d.dec_w_ih; gs.ld1 = A + d.enc_dim; gs.out1 = d.gate_part + GP;
    gs.W2 = d.att_w_hh; gs.ld2 = A; gs.out2 = d.gate_part + 2 * GP; gs.x12 = att_h_out(d, s);
    gs.rows = 4 * A; gs.H = A; gs.B = d.B;
    if (p.w16) { gs.W0 = w16_at(p.w16->dec_w_hh, 0); gs.W1 = w16_at(p.w16->dec_w_ih, 0); gs.W2 = w16_at(p.w16->att_w_hh, 0); }
}

// the query of the three-launch attention, W_query . h_att
static void fill_query_gemv(const AttArgs& aa, GemvArgs& qa) {
    memset(&qa, 0, sizeof(qa));
    qa.W1 = aa.w_query; qa.ld1 = aa.att_rnn; qa.k1 = aa.att_rnn; qa.x1 = aa.h_att; qa.n1 = aa.att_rnn; qa.sx1 = aa.att_rnn;
    qa.y = (float*)aa.q; qa.sy_item = aa.att_dim; qa.sy_row = 1; qa.rows = aa.att_dim; qa.items = aa.B;
}

// what t2s_taco_decode_steps / t2s_taco_decode_plan refuse
static int decode_check(const t2s_taco_decoder* d, int step0, int n_steps) {
    if (!d || step0 < 0 || n_steps <= 0) return T2S_EINVAL;
    const int A = d->att_rnn_dim;
    if (d->B <= 0 || d->T_in <= 0 || A != d->dec_rnn_dim || (A & 3) || (d->prenet_dim & 3) || (d->enc_dim & 3) || d->att_dim > 128 ||
        d->loc_filters > 32 || d->loc_kernel > 63 || !(d->loc_kernel & 1))
        return T2S_EINVAL;
    if (step0 + n_steps > d->T_cap) return T2S_EINVAL;
    if (!d->att_w_ih || !d->att_w_hh || !d->dec_w_ih || !d->dec_w_hh || !d->w_query || !d->w_loc_conv ||
        !d->w_loc_dense || !d->w_v || !d->memory || !d->pmem || !d->att_h0 || !d->att_h1 || !d->att_c || !d->dec_h0 ||
        !d->dec_h1 || !d->dec_c || !d->att_w || !d->att_wcum || !d->ctx || !d->q || !d->energies || !d->align_out)
        return T2S_EINVAL;
    if (d->teacher_forced) {
        if (!d->pre_all || !d->hc_all) return T2S_EINVAL;
    } else {
        if (!d->w_proj || !d->b_proj || !d->w_projpre || !d->b_projpre || !d->w_pre2 || !d->pre1 || !d->pre2 ||
            !d->mel_gate_out || !d->prenet_masks)
            return T2S_EINVAL;
    }
    return T2S_OK;
}

// Validation, then every decision that holds for all steps of the call.  A decision that looks at a ping-pong pointer (the two
// t2s_sbgemm_lstm_ok questions, the gate-stream role's pointer checks) must hold for BOTH step parities.
static int decode_plan(const t2s_taco_decoder* d_, int step0, int n_steps, DecodePlan& p) {
    memset(&p, 0, sizeof(p));
    T2S_TRY(decode_check(d_, step0, n_steps));
    const t2s_taco_decoder& d = *d_;
    const int B = d.B, T = d.T_in, P = d.prenet_dim, E = d.enc_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    LstmCellArgs ca;
    AttArgs aa;
    // Teacher-forced decoding with the per-step saves at hand (training): the decoder cell of step s feeds only the decoder
    // cell of step s + 1 and the projection after the loop - never the attention chain (attention cell -> query -> energies ->
    // softmax + context), whose next prenet input is given.  So it runs on the library's helper stream from the saved copies
    // of h_att[s] and ctx[s] (att_h_all, hc_all), a chunk of steps behind the attention chain, and drops out of the serial chain.
    // With one event per STEP this measured equal (128.0 vs 128.2 ms per train step, profiles/r03_taco_timeline_fwd_split.md: the
    // record opens a 7 us gap on the critical stream); with one event per 16 steps: 95.7 -> 91.9 ms.
    p.split = d.teacher_forced && d.att_h_all && d.hc_all;
    // Paced decoder cells (t2s_taco_decoder::pace_flag): the helper stream's cell of step s - 1 is released by a word the attention
    // cell's launch of step s stores as it STARTS, i.e. when the attention of step s - 1 is complete.  It is enqueued ~4 us later, finds
    // the chip held by that attention cell, and runs as its workgroups retire - beside the attention launch of step s, whose small
    // workgroups share a CU with it - and is over when the next attention cell needs the CUs.  In bursts of 16 (the chunked form) the
    // helper's cells kept the chain's next attention cell from starting: their time ADDED to the chain's.  T2S_DECODE_PACED=0: chunks
    // (for tools that serialise kernels across streams, which would otherwise wait out every bounded spin).
    static const bool want_paced = !(getenv("T2S_DECODE_PACED") && atoi(getenv("T2S_DECODE_PACED")) == 0);
    p.paced = p.split && want_paced && d.pace_flag && B > 8 && !((uintptr_t)d.pace_flag & 7);
    // one fused attention launch per step (one workgroup per batch element) up to this batch; beyond it the three-kernel
    // form (query GEMV, energies, softmax + context) fills the chip better (measured at B = 32, T_in = 256: no difference)
    p.fused_att = B <= ATT_FUSED_MAX_B && T <= 512 && d.w_loc_denseT && d.att_dim <= 128;
    p.units = d.att_gates_all ? 2 : 4;
    p.q_parts = p.fused_att && B <= 8 && d.q_part != nullptr;       // (9+ items: the cells run on sbgemm.hip, no partials)
    if (!p.fused_att && !p.q_parts && d.q_part && A == 1024 && d.att_dim == 128 && d.loc_filters == 32 && d.loc_kernel <= 31 &&
        d.w_loc_denseT) {
        p.q_big = true;
        for (int s = 0; s < 2 && p.q_big; ++s) { fill_att_cell(d, p, s, ca); p.q_big = t2s_sbgemm_lstm_ok(ca); }
    }
    // streamed gates (ABI v4, t2s_taco_decoder::gate_part): autoregressive small-batch decode only
    // (up to 4 items: the role's dot products and reductions are per item - at B = 8 the launch takes longer than the two cells save,
    // 73.9 vs 67.4 us per step; B = 4: 48.2 vs 49.9, B = 2: 36.2 vs 42.0, B = 1: 29.6 vs 37.3; and the role must fit this device: one
    // pass of 3-4 row units per wave over one workgroup per CU - else the plain chain)
    if (d.gate_part && B <= DECODE_STREAM_MAX_B && !d.teacher_forced && p.fused_att && p.q_parts && !d.att_gates_all && A == 1024 &&
        D == 1024) {
        fill_att_args(d, p, 0, aa);
        p.stream_gates = true;
        for (int s = 0; s < 2 && p.stream_gates; ++s) {
            GateStreamArgs gs;
            fill_gate_stream(d, p, s, gs);
            p.stream_gates = t2s_att_fused_stream_ok(aa, gs);
        }
    }
    if (p.paced) {
        p.sig_by_kernel = true;
        for (int s = 0; s < 2 && p.sig_by_kernel; ++s) { fill_att_cell(d, p, s, ca); p.sig_by_kernel = t2s_sbgemm_lstm_ok(ca); }
    }
    p.fold_pre2 = p.stream_gates && d.w_pre2T && P == 256 && E == 512;
    p.use_ploc = p.stream_gates && d.ploc && d.att_dim == 128 && d.loc_filters == 32 && d.loc_kernel <= 31 && !d.q_all && !d.wcum_all;
    if (!p.fused_att && d.att_xbuf) {
        p.one = true;
        fill_att_args(d, p, 0, aa);
        p.one = t2s_att_energy_ctx_ok(aa);
    }
    p.proj_fused = !d.teacher_forced && d.w_projpre == d.w_proj + (size_t)(d.n_mel + 1) * (D + E) && d.b_projpre == d.b_proj + d.n_mel + 1;
    return T2S_OK;
}

static int run_att_cell(const t2s_taco_decoder& d, const DecodePlan& p, int s, hipStream_t stream) {
    LstmCellArgs ca;
    fill_att_cell(d, p, s, ca);
    if (p.paced && !p.sig_by_kernel) T2S_CHECK_HIP(t2s_launch_pace_signal(ca.sig_ptr, ca.sig_val, stream));
    T2S_CHECK_HIP(t2s_launch_lstm_cell(ca, stream, p.w16 != nullptr));
    return T2S_OK;
}

// the fused launch, or query + energies [+ softmax / context]
static int run_attention(const t2s_taco_decoder& d, const DecodePlan& p, int s, hipStream_t stream) {
    AttArgs aa;
    fill_att_args(d, p, s, aa);
    if (p.fused_att) {
        GateStreamArgs gs;
        if (p.stream_gates) fill_gate_stream(d, p, s, gs);
        T2S_CHECK_HIP(t2s_launch_att_fused(aa, stream, p.stream_gates ? &gs : nullptr, p.stream_gates && p.w16));
        return T2S_OK;
    }
    if (!p.q_big) {
        GemvArgs qa;
        fill_query_gemv(aa, qa);
        T2S_CHECK_HIP(t2s_launch_gemv(qa, stream));
    }
    T2S_CHECK_HIP(t2s_launch_att_energy(aa, stream));
    if (!p.one) T2S_CHECK_HIP(t2s_launch_att_softmax_ctx(aa, stream));
    return T2S_OK;
}

// 5. decoder LSTMCell on [h_att | context]; `stream` is the helper stream when the plan is split
static int run_dec_cell(const t2s_taco_decoder& d, const DecodePlan& p, int s, hipStream_t stream) {
    const int B = d.B, E = d.enc_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    LstmCellArgs cd;
    memset(&cd, 0, sizeof(cd));
    cd.W_ih = d.dec_w_ih; cd.W_hh = d.dec_w_hh; cd.b_ih = d.dec_b_ih; cd.b_hh = d.dec_b_hh;
    cd.x1 = att_h_out(d, s); cd.n1 = A; cd.sx1 = A; cd.x2 = d.ctx; cd.n2 = E; cd.sx2 = E;
    if (p.split) {
        cd.x1 = d.att_h_all + (size_t)s * B * A;
        cd.x2 = d.hc_all + (size_t)s * B * (D + E) + D; cd.sx2 = D + E;
    }
    cd.h_in = dec_h_in(d, s); cd.h_out = dec_h_out(d, s); cd.c = d.dec_c; cd.B = B; cd.H = D;
    if (p.stream_gates) {
        // only the context columns of W_ih are left to stream (8.4 MB of 42): W_hh . h_dec(s-1) and W_ih[:, :A] . h_att(s)
        // came out of the attention launch as gate_part[0], gate_part[1]
        cd.W_ih = d.dec_w_ih + A; cd.ld_ih = A + E; cd.x1 = d.ctx; cd.n1 = E; cd.sx1 = E; cd.x2 = nullptr; cd.n2 = 0; cd.sx2 = 0;
        cd.h_in = nullptr; cd.pre_a = d.gate_part; cd.pre_b = d.gate_part + gate_block(d);
    }
    if (d.dec_drop) { cd.drop_mask = d.dec_drop + (size_t)s * B * D; cd.drop_scale = d.dec_drop_scale; }
    if (d.teacher_forced) { cd.h_copy = d.hc_all + (size_t)s * B * (D + E); cd.s_copy = D + E; }
    if (d.dec_gates_all) { cd.gates_out = d.dec_gates_all + (size_t)s * B * 4 * D; cd.c_out = d.dec_c_all + (size_t)s * B * D; }
    if (p.w16) { cd.W_ih = w16_at(p.w16->dec_w_ih, p.stream_gates ? A : 0); cd.W_hh = w16_at(p.w16->dec_w_hh, 0); }
    T2S_CHECK_HIP(t2s_launch_lstm_cell(cd, stream, p.w16 != nullptr));
    return T2S_OK;
}

// the projection launch; with use_ploc it also carries the location term of the NEXT step's attention on the CUs the GEMV leaves
// idle (whatever form the launch takes: the next attention launch reads ploc)
static hipError_t launch_proj(const t2s_taco_decoder& d, const DecodePlan& p, const GemvArgs& g, hipStream_t stream) {
    if (!p.use_ploc) return t2s_launch_gemv(g, stream);
    LocPreArgs lp;
    memset(&lp, 0, sizeof(lp));
    lp.w = d.att_w; lp.w_cum = d.att_wcum; lp.w_loc_conv = d.w_loc_conv; lp.w_loc_denseT = d.w_loc_denseT;
    lp.ploc = d.ploc; lp.B = d.B; lp.T = d.T_in; lp.loc_ks = d.loc_kernel;
    return t2s_launch_gemv_with_loc(g, lp, stream);
}

// 6./7. (autoregressive) mel frame + gate logit = W_proj [h_dec | ctx] + b, and (same launch, second row block) layer 0 of the
//       next step's prenet through the precomposed matrix W_pre0 . W_proj (always-on dropout, modules.py:21), so the mel frame
//       needs no extra hop before the prenet; then prenet layer 1 unless the next attention cell folds it in.
static int run_projection(const t2s_taco_decoder& d, const DecodePlan& p, int s, hipStream_t stream) {
    const int B = d.B, P = d.prenet_dim, E = d.enc_dim, D = d.dec_rnn_dim;
    const bool more = s + 1 < d.mask_steps;
    const unsigned char* mk = d.prenet_masks + (size_t)(s + 1) * B * 2 * P;
    GemvArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.W1 = d.w_proj; pa.ld1 = D + E; pa.k1 = D + E;
    pa.x1 = dec_h_out(d, s); pa.n1 = D; pa.sx1 = D; pa.x2 = d.ctx; pa.n2 = E; pa.sx2 = E;
    pa.bias1 = d.b_proj; pa.y = d.mel_gate_out + s; pa.sy_item = (long)(d.n_mel + 1) * d.T_cap;
    pa.sy_row = d.T_cap; pa.rows = d.n_mel + 1; pa.items = B;
    if (more && p.proj_fused) {
        pa.rows = d.n_mel + 1 + P; pa.split_row = d.n_mel + 1;
        pa.y2 = d.pre1; pa.sy2_item = P; pa.sy2_row = 1; pa.act2 = ACT_RELU;
        pa.mask2 = mk; pa.smask2_item = 2 * P; pa.mask2_scale = 2.0f;
    }
    T2S_CHECK_HIP(launch_proj(d, p, pa, stream));
    if (more && !p.proj_fused) {
        GemvArgs p1;
        memset(&p1, 0, sizeof(p1));
        p1.W1 = d.w_projpre; p1.ld1 = D + E; p1.k1 = D + E;
        p1.x1 = pa.x1; p1.n1 = D; p1.sx1 = D; p1.x2 = d.ctx; p1.n2 = E; p1.sx2 = E;
        p1.bias1 = d.b_projpre; p1.y = d.pre1; p1.sy_item = P; p1.sy_row = 1; p1.rows = P; p1.items = B;
        p1.act = ACT_RELU; p1.mask = mk; p1.smask_item = 2 * P; p1.mask_scale = 2.0f;
        T2S_CHECK_HIP(t2s_launch_gemv(p1, stream));
    }
    if (more && !p.fold_pre2) {
        GemvArgs p2;
        memset(&p2, 0, sizeof(p2));
        p2.W1 = d.w_pre2; p2.ld1 = P; p2.k1 = P; p2.x1 = d.pre1; p2.n1 = P; p2.sx1 = P;
        p2.y = d.pre2; p2.sy_item = P; p2.sy_row = 1; p2.rows = P; p2.items = B;
        p2.act = ACT_RELU; p2.mask = mk + P; p2.smask_item = 2 * P; p2.mask_scale = 2.0f;
        T2S_CHECK_HIP(t2s_launch_gemv(p2, stream));
    }
    return T2S_OK;
}

extern "C" {

int t2s_taco_attention(const float* h_att, const float* memory, const float* pmem, const int* lengths, float* w, float* w_cum,
                       float* ctx, float* q_scratch, float* e_scratch, const float* w_query, const float* w_loc_conv,
                       const float* w_loc_dense, const float* w_loc_denseT, const float* w_v, int B, int T, int att_rnn,
                       int att_dim, int enc_dim, int loc_filters, int loc_kernel, void* stream) {
    if (!h_att || !memory || !pmem || !w || !w_cum || !ctx || !q_scratch || !e_scratch || !w_query || !w_loc_conv || !w_loc_dense ||
        !w_v || B <= 0 || T <= 0 || (att_rnn & 3) || (enc_dim & 3) || att_dim <= 0 || att_dim > 128 || loc_filters <= 0 ||
        loc_filters > 32 || loc_kernel <= 0 || loc_kernel > 63 || !(loc_kernel & 1))
        return T2S_EINVAL;
    // step 0 of a decoder that has nothing but the attention's operands: h_att is the attention cell's output slot of an even step
    t2s_taco_decoder d;
    memset(&d, 0, sizeof(d));
    d.B = B; d.T_in = T; d.enc_dim = enc_dim; d.att_rnn_dim = att_rnn; d.att_dim = att_dim; d.loc_filters = loc_filters;
    d.loc_kernel = loc_kernel; d.w_query = w_query; d.w_loc_conv = w_loc_conv; d.w_loc_dense = w_loc_dense; d.w_v = w_v;
    d.w_loc_denseT = w_loc_denseT; d.memory = memory; d.pmem = pmem; d.mem_lengths = lengths; d.att_h1 = (float*)h_att;
    d.att_w = w; d.att_wcum = w_cum; d.ctx = ctx; d.q = q_scratch; d.energies = e_scratch;
    DecodePlan p;
    memset(&p, 0, sizeof(p));
    // (decode_plan asks att_dim <= 128 only and lets the fused launcher refuse a wider encoder or LSTM; this entry point has the
    // three-launch form to fall back on for them, so it asks the launcher's own limits here)
    p.fused_att = B <= ATT_FUSED_MAX_B && T <= 512 && w_loc_denseT && enc_dim <= 512 && att_rnn <= 1024;
    if (p.fused_att) return run_attention(d, p, 0, (hipStream_t)stream);
    // three launches, with the query GEMV checked first: its operands come straight from the caller
    AttArgs aa;
    GemvArgs qa;
    fill_att_args(d, p, 0, aa);
    fill_query_gemv(aa, qa);
    qa.mask_scale = 1.f;
    if (!gemv_args_ok(qa)) return T2S_EINVAL;
    T2S_CHECK_HIP(t2s_launch_gemv(qa, (hipStream_t)stream));
    T2S_CHECK_HIP(t2s_launch_att_energy(aa, (hipStream_t)stream));
    T2S_CHECK_HIP(t2s_launch_att_softmax_ctx(aa, (hipStream_t)stream));
    return T2S_OK;
}

}  // extern "C"

static unsigned plan_bits(const DecodePlan& p) {
    return (p.split ? T2S_PLAN_SPLIT : 0) | (p.paced ? T2S_PLAN_PACED : 0) | (p.sig_by_kernel ? T2S_PLAN_SIG_BY_KERNEL : 0) |
            (p.fused_att ? T2S_PLAN_FUSED_ATT : 0) | (p.q_parts ? T2S_PLAN_Q_PARTS : 0) | (p.q_big ? T2S_PLAN_Q_BIG : 0) |
            (p.one ? T2S_PLAN_ONE : 0) | (p.stream_gates ? T2S_PLAN_STREAM_GATES : 0) | (p.fold_pre2 ? T2S_PLAN_FOLD_PRE2 : 0) |
            (p.use_ploc ? T2S_PLAN_USE_PLOC : 0) | (p.proj_fused ? T2S_PLAN_PROJ_FUSED : 0) | (p.units == 2 ? T2S_PLAN_UNITS_2 : 0);
}

extern "C" {

int t2s_taco_decode_plan(const t2s_taco_decoder* d, int step0, int n_steps, unsigned* bits) {
    DecodePlan p;
    const int rc = decode_plan(d, step0, n_steps, p);
    if (rc != T2S_OK || !bits) return rc;
    *bits = plan_bits(p);
    return T2S_OK;
}

}  // extern "C"

// elements of attention_rnn.weight_ih / _hh and decoder_rnn.weight_ih / _hh: what the cells (and the gate-stream role) of one step read
static long long lstm_weight_elems(const t2s_taco_decoder& d) {
    const long long P = d.prenet_dim, E = d.enc_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    return 4 * A * (P + E + A) + 4 * D * (A + E + D);
}

// The plan of `d` (the same decisions as for the f32 matrices: only the weight reads differ) with the four LSTM matrices taken from
// `w`.  Refused, never run on the f32 matrices instead: what the fp16 kernels do not cover - teacher forcing, the matrix-core cells of
// 9+ items, the training saves - and matrices whose 4-element slots are not 8-byte loads.
static int decode_plan_w16(const t2s_taco_decoder* d_, const t2s_taco_w16* w, int step0, int n_steps, DecodePlan& p) {
    T2S_TRY(decode_plan(d_, step0, n_steps, p));
    const t2s_taco_decoder& d = *d_;
    if (!w || d.teacher_forced || d.B > 8) return T2S_EINVAL;
    if (d.att_gates_all || d.att_c_all || d.dec_gates_all || d.dec_c_all || d.att_h_all || d.q_all || d.wcum_all) return T2S_EINVAL;
    const void* m[] = {w->att_w_ih, w->att_w_hh, w->dec_w_ih, w->dec_w_hh};
    for (const void* q : m)
        if (!q || ((uintptr_t)q & 7)) return T2S_EINVAL;
    if (((d.prenet_dim + d.enc_dim) | d.att_rnn_dim | (d.att_rnn_dim + d.enc_dim) | d.dec_rnn_dim) & 3) return T2S_EINVAL;
    p.w16 = w;
    return T2S_OK;
}

// Enqueues steps [step0, step0 + n_steps) in one of three schedules: serial (every launch of a step on `stream`); split (teacher
// forced with the saves: the attention chain of 16 steps on `stream`, one event, their decoder cells on the helper stream); paced
// (split at 9+ items with pace_flag: the helper's cell of step s - 1 waits for the word the attention cell of step s stores).
static int decode_steps(const t2s_taco_decoder* d_, const t2s_taco_w16* w16, int step0, int n_steps, void* stream_) {
    DecodePlan p;
    const int rc = w16 ? decode_plan_w16(d_, w16, step0, n_steps, p) : decode_plan(d_, step0, n_steps, p);
    if (rc != T2S_OK) return rc;
    const t2s_taco_decoder& d = *d_;
    hipStream_t stream = (hipStream_t)stream_;
    const int s_end = step0 + n_steps;
    T2sHelperStream hs;
    if (p.split) T2S_CHECK_HIP(t2s_helper_stream_acquire(hs));
    struct Join {           // whatever happens below, the caller's stream waits for the helper before this call returns
        T2sHelperStream& hs; hipStream_t stream; bool on;
        ~Join() {
            if (on && hipEventRecord(hs.ev_join, hs.side) == hipSuccess) (void)hipStreamWaitEvent(stream, hs.ev_join, 0);
        }
    } join{hs, stream, p.split};
    if (p.paced) {
        T2S_CHECK_HIP(hipEventRecord(hs.ev_step, stream));            // everything enqueued so far precedes the helper's first cell
        T2S_CHECK_HIP(hipStreamWaitEvent(hs.side, hs.ev_step, 0));
        unsigned long long* perr = (unsigned long long*)d.pace_flag + 1;
        for (int s = step0; s < s_end; ++s) {
            T2S_TRY(run_att_cell(d, p, s, stream));
            T2S_TRY(run_attention(d, p, s, stream));
            if (s > step0) {
                T2S_CHECK_HIP(t2s_launch_pace_wait((const unsigned*)d.pace_flag, (unsigned)s + 1u, perr, hs.side));
                T2S_TRY(run_dec_cell(d, p, s - 1, hs.side));
            }
        }
        // the last step's cell: after its attention (the chain is over: one event costs nothing now)
        T2S_CHECK_HIP(hipEventRecord(hs.ev_step, stream));
        T2S_CHECK_HIP(hipStreamWaitEvent(hs.side, hs.ev_step, 0));
        T2S_TRY(run_dec_cell(d, p, s_end - 1, hs.side));
    } else if (p.split) {
        // the attention chain of a chunk of steps, ONE event, then the decoder cells of those steps on the helper stream while the
        // caller's stream goes on with the next chunk
        for (int c0 = step0; c0 < s_end; c0 += DECODE_CHUNK) {
            const int c1 = c0 + DECODE_CHUNK < s_end ? c0 + DECODE_CHUNK : s_end;
            for (int s = c0; s < c1; ++s) {
                T2S_TRY(run_att_cell(d, p, s, stream));
                T2S_TRY(run_attention(d, p, s, stream));
            }
            T2S_CHECK_HIP(hipEventRecord(hs.ev_step, stream));        // h_att, ctx of the chunk saved (and all earlier work of the caller)
            T2S_CHECK_HIP(hipStreamWaitEvent(hs.side, hs.ev_step, 0));
            for (int s = c0; s < c1; ++s) T2S_TRY(run_dec_cell(d, p, s, hs.side));
        }
    } else {
        for (int s = step0; s < s_end; ++s) {
            T2S_TRY(run_att_cell(d, p, s, stream));
            T2S_TRY(run_attention(d, p, s, stream));
            T2S_TRY(run_dec_cell(d, p, s, stream));
            if (!d.teacher_forced) T2S_TRY(run_projection(d, p, s, stream));
        }
    }
    return T2S_OK;
}

extern "C" {

int t2s_taco_decode_steps(const t2s_taco_decoder* d, int step0, int n_steps, void* stream) {
    return decode_steps(d, nullptr, step0, n_steps, stream);
}

int t2s_taco_decode_steps_w16(const t2s_taco_decoder* d, const t2s_taco_w16* w, int step0, int n_steps, void* stream) {
    if (!w) return T2S_EINVAL;          // (no fallback to the f32 matrices of `d`: that is t2s_taco_decode_steps)
    return decode_steps(d, w, step0, n_steps, stream);
}

int t2s_taco_decode_plan_w16(const t2s_taco_decoder* d, const t2s_taco_w16* w, int step0, int n_steps, unsigned* bits,
                             long long* lstm_weight_bytes) {
    DecodePlan p;
    const int rc = w ? decode_plan_w16(d, w, step0, n_steps, p) : decode_plan(d, step0, n_steps, p);
    if (rc != T2S_OK) return rc;
    if (bits) *bits = plan_bits(p);
    if (lstm_weight_bytes) *lstm_weight_bytes = lstm_weight_elems(*d) * (w ? 2 : 4);
    return T2S_OK;
}

}  // extern "C"
