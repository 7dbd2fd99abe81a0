/* libt2s_hip — C ABI of the MI355X (gfx950) Tacotron-2 / WaveGlow hot path.
 *
 * The reference (DonggeunYu/Text2Speech) has no FFI of its own: its hot path is
 * the torch op sequence inside waveglow/glow.py and tacotron/tacotron.py.  Each
 * entry point below replaces one such op sequence; the reference lines are cited
 * per function.  The Python side (text2speech_amd/glow.py, .../tacotron.py) binds
 * these with ctypes and keeps the reference's module API.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch allocations);
 *    the library allocates no device memory;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, or
 *    ordered before the point the call leaves it at, and nothing synchronises
 *    with the host;
 *  - return value 0 = success; a negative T2S_E* code otherwise (never throws);
 *  - entry points are re-entrant and thread-safe (autograd calls backward from
 *    another thread), and work on whichever device is current in the calling
 *    thread.  Library-owned state, all of it per device and created on first use
 *    on that device: (a) t2s_taco_bptt_steps keeps two helper streams + five events
 *    per device behind a per-device mutex (it overlaps dependent chains; on every
 *    exit, error exits included, the caller's stream waits for both helpers; with
 *    t2s_taco_decode_steps borrows the first helper the same way for teacher-forced steps with saves);
 *    (b) the GEMM launchers remember per device that they raised the kernel's
 *    dynamic-LDS limit (an idempotent one-bit flag); (c) t2s_last_hip_error()
 *    is per thread.  Nothing else persists between calls.
 *
 * "Planes": activations on the WN path are channel-last, split-bf16:
 *      x ~= float(hi) + float(lo),   plane[b][c/32][row][c%32] (bf16),
 *      row = halo + t, 0 <= row < Lp,  Lp = t2s_plane_rows(L, halo);
 *    rows outside [halo, halo+L) must be zero (allocate zero-filled once; the
 *    kernels never write them).  f32 "skip" planes use the same indexing.
 */
#ifndef T2S_HIP_H
#define T2S_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define T2S_OK 0
#define T2S_EINVAL (-1)  /* bad argument (null pointer, size, alignment) */
#define T2S_EHIP (-2)    /* HIP runtime reported an error at launch */

#define T2S_PERM_NONE 0
#define T2S_PERM_GATE 1  /* rows o<C: tanh half, o>=C: sigmoid half, interleaved per 16 channels */
#define T2S_PERM_PAIR8 2 /* table pack only: rows o < C_gate, per group of 32: packed row 16 m + 4 q + e = channel 8 q + 4 m + e */
#define T2S_ACT_NONE 0
#define T2S_ACT_RELU 1
#define T2S_ACT_TANH 2

int t2s_abi_version(void);
/* ABI v4.  Operand format of the split planes this build computes with: 0 = bf16 hi/lo (the shipped library), 1 = fp16 hi/lo
 * (diagnostic build -DT2S_SPLIT_F16: same three MFMA products per MAC, ~22 instead of ~16 significand bits, but no exponent range
 * to spare - the no-grad WaveGlow forward / infer only; the host side refuses the training path and turns a non-finite result,
 * i.e. an operand plane that overflowed 65504, into an error instead of returning it). */
int t2s_operand_format(void);
/* ABI v4.  sizeof(t2s_taco_decoder) / sizeof(t2s_taco_bptt) as this library was compiled: a binding that mirrors the structs field by
 * field (ctypes, cgo, JNI) checks its own size against these before the first call. */
int t2s_sizeof_taco_decoder(void);
int t2s_sizeof_taco_bptt(void);
const char* t2s_error_string(int code);
/* last HIP error text seen by a failing entry point on this thread ("" if none) */
const char* t2s_last_hip_error(void);

/* rows per 32-channel chunk of a plane holding L time steps with `halo` zero rows either side */
int t2s_plane_rows(int L, int halo);
/* packed row count (multiple of 256) for `rows` GEMM output rows */
int t2s_padded_rows(int rows);

/* weight_norm + pack one conv weight v[O][Cin][Kt] (gain g[O] or NULL) into the GEMM A planes
 * A_hi/A_lo [nk][Mpad][32] bf16 at packed-K offset `koff` (tap-major, tap stride Cin_pad), and its
 * bias into bias_out[Mpad].  g_is_scale=1: g is a plain per-row scale (eval BatchNorm fold) instead of
 * a weight-norm gain.  Replaces torch.nn.utils.weight_norm's per-forward recompute
 * (reference glow.py:123,138,142,151). */
int t2s_pack_conv_weight(const float* v, const float* g, int g_is_scale, const float* bias_in, int O, int Cin, int Kt,
                         int perm, int C_gate, int row_off, int Mpad, int koff, int Cin_pad, void* A_hi, void* A_lo,
                         float* bias_out, int bias_accumulate, void* stream);

/* Table-driven form of t2s_pack_conv_weight: ONE launch packs every listed weight (the per-forward
 * weight-norm recompute of all 288 WN convolutions).  `jobs` is a DEVICE array of t2s_pack_job; a workgroup packs 16
 * consecutive output rows, job i owns workgroups [row_start, row_start + ceil(O/16)), row_start being the running sum of
 * ceil(O/16) and total_groups the grand total.  bias_out[p] = bias_in[o] + bias_in2[o] (either may be NULL); leave bias_out
 * NULL on a job that shares its rows' bias with another. */
typedef struct t2s_pack_job {
    const float *v, *g, *bias_in, *bias_in2;
    void *A_hi, *A_lo;
    float* bias_out;
    long row_start;
    long O, Cin, Kt, perm, C_gate, Mpad, koff, Cin_pad, row_off, g_is_scale;
    float* scale_out; /* optional [O]: per-row factor g/|v| that was applied, kept for the backward pass */
} t2s_pack_job;
int t2s_pack_conv_weight_table(const t2s_pack_job* jobs, int n_jobs, long total_groups, void* stream);

/* w[O][K] = v * g / ||v||  for a small weight-normed 1x1 conv (WN.start; reference glow.py:122-124) */
int t2s_weightnorm_small(const float* v, const float* g, int O, int K, float* w, void* stream);

/* ConvTranspose1d(n_mel,n_mel,ksize,stride) + trim to L*n_group samples + squeeze -> conditioning planes
 * S_hi/S_lo [B][ceil(n_mel*n_group/32)][Lp][32]  (reference glow.py:215-221; infer 252-258). */
int t2s_wg_upsample_squeeze(const float* mel, const float* W, const float* bias, int B, int n_mel, int frames,
                            int ksize, int stride, int n_group, int L, int Lp, int halo, void* S_hi, void* S_lo,
                            void* stream);

/* audio[B][T] -> z[B][n_group][L] (unsqueeze=0, reference glow.py:223) or back (unsqueeze=1, glow.py:291) */
int t2s_wg_audio_squeeze(float* audio, float* z, int B, int T, int n_group, int L, int unsqueeze, void* stream);

/* The kept columns of a vocoded window, written straight into the caller's rows (additive to ABI version 4; streaming.py):
 *   dst[b][dst_off + (k - k0) G + g] = z[b][g][k]   for k0 <= k < k1,   z float [B][G][L] contiguous, dst rows ld_dst floats apart.
 * What the unsqueeze above, a slice and a copy would give, in one launch.  No alignment beyond the element for dst, dst_off or ld_dst.
 * T2S_EINVAL, with nothing launched: a NULL z or dst; B, G, L or ld_dst <= 0; B > 65535; k0 < 0, k0 >= k1 or k1 > L; dst_off < 0;
 * (k1 - k0) G > ld_dst - dst_off. */
int t2s_wg_audio_window(const float* z, int B, int G, int L, int k0, int k1, float* dst, long ld_dst, long dst_off, void* stream);

/* in-place invertible 1x1 conv on channels [c_off, c_off+n_rem) of z[B][n_group][L] (reference glow.py:82-102) */
int t2s_wg_convinv(float* z, const float* W, int B, int n_group, int c_off, int n_rem, int L, void* stream);

/* logdet_out = scale*log(det W) (NaN if det<0) and/or inv_out = W^-1, W is n x n, n<=16
 * (reference glow.py:90-91,100) */
int t2s_small_logdet_inv(const float* W, int n, float scale, float* logdet_out, float* inv_out, void* stream);

/* the same for many small matrices in ONE launch (all 12 flows' 1x1-conv weights): jobs is a DEVICE array */
typedef struct t2s_small_mat_job { const float* W; float* logdet_out; float* inv_out; long n; } t2s_small_mat_job;
int t2s_small_logdet_inv_batch(const t2s_small_mat_job* jobs, int n_jobs, float scale, void* stream);
/* Same, `host_jobs` is a HOST array of at most 16 entries that travels as a kernel argument: no device table to upload. */
int t2s_small_logdet_inv_batch_host(const t2s_small_mat_job* host_jobs, int n_jobs, float scale, void* stream);

/* WN.start: x = w[C][n_half] * z[:, c_off:c_off+n_half] + bias -> planes X_hi/X_lo (reference glow.py:156) */
int t2s_wg_start(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                 int L, int Lp, int halo, void* X_hi, void* X_lo, void* stream);

/* One WN layer, first half: acts = tanh/sigmoid gate of (dilated conv(x) + 1x1 conv(spect) + bias)
 * (reference glow.py:159-162 with fused_add_tanh_sigmoid_multiply glow.py:33-40).
 * A planes hold [taps*xc + sc] K-steps x Mpad rows packed with T2S_PERM_GATE. */
int t2s_wg_in_cond_gate(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                        const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, int B, int C, int n_cond,
                        int taps, int dilation, int L, int Lp, int halo, int Mpad, void* stream);

/* One WN layer, second half: rs = 1x1 conv(acts) + bias; x += rs[:n_res]; skip (+)= rs[n_res:]
 * (reference glow.py:164-174).  n_res = C (layers 0..n-2) or 0 (last layer). */
int t2s_wg_res_skip(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                    void* X_hi, void* X_lo, float* skip, int B, int C, int n_res, int skip_init, int L, int Lp,
                    int halo, int Mpad, void* stream);

/* WN.end + affine coupling on channels [c_off+n_half, c_off+2*n_half) of z; writes log_s[B][n_half][L]
 * and wn_out[B][2*n_half][L] = (b ; log_s) if non-NULL (reference glow.py:175,241-246; reverse=1: glow.py:276-280) */
int t2s_wg_end_affine(const float* skip, const float* w_end, const float* b_end, float* z, float* log_s,
                      float* wn_out, int B, int n_group, int c_off, int n_half, int C, int L, int Lp, int halo, int reverse, void* stream);

/* ---- WN.end folded into the skip path (no-grad forward / infer) ----
 * end(sum_i skip_i) = sum_i (W_end W_skip,i) acts_i + const (reference glow.py:172-175), and W_end W_skip,i is only
 * [2*n_half x C]: the skip half of res_skip_layers and the f32 skip accumulator are never materialised. */
typedef struct t2s_endfold_job {
    const float *w_end, *v_skip, *scale, *b_skip;   /* [nj][C], [C][C] skip rows of weight_v, their g/|v|, their bias */
    void* fold_A;                                   /* out: MFMA A fragments, 8192*ceil(C/128) bf16, zero-initialised */
    float* bes;                                     /* out: [8] */
    long nj, C;
} t2s_endfold_job;
/* jobs: DEVICE array, one per WN layer; run after the weight packing that produced `scale` */
int t2s_wg_endfold_weights(const t2s_endfold_job* jobs, int n_jobs, int C, void* stream);
/* Tile height (256 or 128 packed rows) the folded gate GEMM uses for this shape: 128 where 256-row tiles would leave at least
 * half the chip without a workgroup (short utterances).  t2s_wg_gate_fold_slots follows it; t2s_wg_in_melwin_gate_fold (phase
 * tiles, always 256 rows) returns T2S_EINVAL for shapes where this is 128. */
int t2s_wg_gate_tile_rows(int B, int C, int L);
/* t2s_wg_in_cond_gate plus fold_acc[slot][b][j][t] (+)= (W_end W_skip,i)[j] . acts[:, t] over the slot's channels; C % 16 == 0.
 * fold_acc holds t2s_wg_gate_fold_slots(B, C, L) slots of [B][8][L] floats: 2*ceil(C/128) with the 256-row tiles, 2*ceil(C/64) when
 * the shape takes 128-row tiles (a grid of 256-row tiles that would leave half of the CUs idle: short utterances at B = 1).
 * t2s_wg_end_fold_affine takes the same count as `nslots`. */
int t2s_wg_gate_fold_slots(int B, int C, int L);
int t2s_wg_in_cond_gate_fold(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                             const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                             float* fold_acc, int fold_init, int B, int C, int n_cond, int taps, int dilation, int L,
                             int Lp, int halo, int Mpad, void* stream);
/* ---- WN.start folded into the first gate GEMM of a flow (no-grad forward / infer) ----
 * x0 = W_start a + b_start has C channels but only n_half + 1 independent ones, so in_layers[0](x0) (reference glow.py:156,159) is
 * a `taps`-tap convolution of the n_half audio channels and a constant-one channel (1 inside the utterance, 0 in the zero padding:
 * exact at the edges): ncol = taps * (n_half + 1) <= 32 logical columns, column tap * (n_half + 1) + j = z[c_off + j][t + tap - taps/2]
 * (j = n_half: the ones-channel).  Both factors are carried to f32 accuracy by FOUR column sets of ncol columns: with
 * x = h + l + r (h, l the split pair, r what it leaves) the weight planes hold (h, l) | split(r) | (h, l) | (l, 0) and the window planes
 * (h, l) | (h, l) | split(r) | (l, 0).  win_chunks = 2 (two sets per 32-column chunk, 2 ncol <= 32) or 4 (one set per chunk); the
 * convolution half of that GEMM is win_chunks K-steps instead of taps * C / 32.
 *  t2s_wg_start_window: t2s_wg_start, and next to the X planes the window planes W_hi/W_lo [B][win_chunks][Lp][32] (zero-initialised
 *    by the caller; rows outside [0, L) and unused columns stay zero); C >= 32 * win_chunks.
 *  t2s_wg_startfold_weights: K-chunks 0 .. win_chunks-1 of A_hi/A_lo [win_chunks + ceil(n_cond/32)][Mpad][32] = the composed weights
 *    (g_in / |v_in|) v_in[:, :, tap] . [w_start | b_start] in the same column sets, rows in T2S_PERM_GATE order, accumulated in f32.
 *    v_in [2C][C][taps] and g_in [2C] (NULL: plain weight) are in_layers[0]'s; w_start [C][n_half] is t2s_weightnorm_small's output.
 *    The conditioning weights go behind them with t2s_pack_conv_weight(_table) at koff = 32 * win_chunks.
 *  t2s_wg_in_win_gate_fold: t2s_wg_in_cond_gate_fold for that layer, the window planes in place of X (no taps, no dilation). */
int t2s_wg_start_window(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                        int L, int Lp, int halo, void* X_hi, void* X_lo, int taps, int win_chunks, void* W_hi, void* W_lo,
                        void* stream);
int t2s_wg_startfold_weights(const float* v_in, const float* g_in, const float* w_start, const float* b_start, int C, int n_half,
                             int taps, int Mpad, int win_chunks, void* A_hi, void* A_lo, void* stream);
int t2s_wg_in_win_gate_fold(const void* A_hi, const void* A_lo, const float* bias, const void* W_hi, const void* W_lo,
                            const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                            float* fold_acc, int fold_init, int B, int C, int n_cond, int win_chunks, int L, int Lp, int halo,
                            int Mpad, void* stream);
/* residual half only: x += W_res acts + b  (rows [0, C) of the packed res_skip weights; 128-row tiles) */
/* Composed conditioning for the inverse flow (weights packed once).  The ConvTranspose upsampler is linear and only ksize / stride
 * hops overlap, so cond_layers[i](upsample(mel)) at plane row t = P f + phi (P = stride / n_group) is (W_cond,i U_phi) applied to the
 * mel window [mel(f), mel(f-1), ...] of K2 = (ksize / stride) * n_mel values: the conditioning half of the gate GEMM shrinks from
 * n_mel * n_group to K2 columns (glow.py:159-162,215-221 / :252-258; 640 -> 320 at config.json defaults) and the upsampler goes away.
 *  t2s_wg_upsample_basis: U as conditioning planes [1][n_mel*n_group/32][Lp][32] whose time axis is the column (phi, k), plus a last
 *    column with the expanded bias; Lp = t2s_plane_rows(P * K2 + 1, halo).
 *  (caller: t2s_conv_bias_act with A = the conditioning K-chunks of the packed gate weights, X = U, f32 output [2C][ld])
 *  t2s_wg_compose_cond: that f32 result -> A2[phi][K2/32][Mpad][32] (hi, lo); bias_out = bias_in + its last column.
 *  t2s_wg_melwin_planes: mel [B][n_mel][frames] -> M[B][K2/32][Fp][32], row f = the window of frame f (zeros outside the clip).
 *  t2s_wg_in_melwin_gate_fold: t2s_wg_in_cond_gate_fold with (A2, M) in place of the conditioning weights and planes; always the
 *    256-row tiles (fold_acc: 2*ceil(C/128) slots); Fp >= ceil(L / P). */
int t2s_wg_upsample_basis(const float* W, const float* bias, int n_mel, int ksize, int stride, int n_group, int Lp, int halo,
                          void* U_hi, void* U_lo, void* stream);
int t2s_wg_compose_cond(const float* tmp, const float* bias_in, int rows, int Mpad, int P, int K2, long ld, void* A2_hi,
                        void* A2_lo, float* bias_out, void* stream);
int t2s_wg_melwin_planes(const float* mel, int B, int n_mel, int frames, int nlag, int Fp, void* M_hi, void* M_lo, void* stream);
int t2s_wg_in_melwin_gate_fold(const void* A_hi, const void* A_lo, const void* A2_hi, const void* A2_lo, const float* bias,
                               const void* X_hi, const void* X_lo, const void* M_hi, const void* M_lo, void* acts_hi,
                               void* acts_lo, const void* fold_A, float* fold_acc, int fold_init, int B, int C, int K2,
                               int taps, int dilation, int L, int Lp, int halo, int Mpad, int P, int Fp, void* stream);
/* pair8 = 1: the residual rows of A / bias were packed with perm = 2 (T2S_PERM_PAIR8: in every group of 32 channels packed row
 * 16 m + 4 q + e holds channel 8 q + 4 m + e), which lets the epilogue touch x in 16-byte pieces; C % 32 == 0 */
int t2s_wg_res_only(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                    void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8, void* stream);
/* t2s_wg_res_only(pair8 = 1) for the first layer of a flow when nothing wrote x0 = WN.start's output to the X planes: the epilogue
 * rebuilds x0[c][t] = b_start[c] + sum_j w_start[c][j] * z[b][c_off + j][t] (t2s_wg_start's operation order, rounded to the (hi, lo)
 * pair as the planes would hold it) and stores x0 + W_res acts + b; the X planes are only written.  n_half <= 4, C % 32 == 0. */
int t2s_wg_res_only_start(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                          const float* z, const float* w_start, const float* b_start, int n_group, int c_off, int n_half,
                          void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, void* stream);
/* ---- ABI v4, fp16 vocoder planes: WaveGlow.infer for a model whose WN parameters are fp16 (.half()) ----
 * The effective weight of an in / cond / res_skip convolution of such a model, rounded to fp16, IS the GEMM's A operand: one plane,
 * no lo.  Activation planes (X, acts, conditioning) are split-fp16 hi + lo, and each MAC is A.B_hi + A.B_lo accumulated in f32 -
 * two v_mfma_f32_16x16x32_f16 where the split-bf16 entry points spend three.  Biases, the fold sums, WN.start / WN.end, the 1x1
 * convolutions and the coupling stay f32.  Every entry point takes its partner's argument list and checks; the A-operand lo
 * pointer is never read and may be NULL.  An fp16 plane overflows at |x| > 65504 (the caller checks its result for non-finite
 * values).  The plain chain only: no window planes (folded WN.start), no flow-boundary launch, no composed conditioning - their
 * composed weights are not exact in fp16 and have no one-plane form.  (A ragged batch: the _h16_ragged entry points further down.)
 *  t2s_pack_conv_weight_table_h16: the same job table; A_hi receives fp16 (round to nearest even) of the f32 effective weight in the
 *    same permuted layout, A_lo is not touched, bias_out / scale_out as before.
 *  t2s_wg_endfold_weights_h16: fold_A as fp16 hi / lo fragments (a composed matrix: it keeps both planes and three products); bes f32.
 *  t2s_wg_upsample_squeeze_h16, t2s_wg_start_h16: fp16 hi / lo conditioning and X planes; halo and channel-padding rules unchanged.
 *  t2s_wg_in_cond_gate_fold_h16: both tile heights; t2s_wg_gate_tile_rows / t2s_wg_gate_fold_slots decide as for the partner.
 *  t2s_wg_res_only_h16: both pair8 row orders.
 * t2s_wg_end_fold_affine, t2s_wg_convinv, t2s_wg_audio_squeeze and t2s_weightnorm_small are f32 and serve both formats. */
int t2s_pack_conv_weight_table_h16(const t2s_pack_job* jobs, int n_jobs, long total_groups, void* stream);
int t2s_wg_endfold_weights_h16(const t2s_endfold_job* jobs, int n_jobs, int C, void* stream);
int t2s_wg_upsample_squeeze_h16(const float* mel, const float* W, const float* bias, int B, int n_mel, int frames,
                                int ksize, int stride, int n_group, int L, int Lp, int halo, void* S_hi, void* S_lo,
                                void* stream);
int t2s_wg_start_h16(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                     int L, int Lp, int halo, void* X_hi, void* X_lo, void* stream);
int t2s_wg_in_cond_gate_fold_h16(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                                 const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                                 float* fold_acc, int fold_init, int B, int C, int n_cond, int taps, int dilation, int L,
                                 int Lp, int halo, int Mpad, void* stream);
int t2s_wg_res_only_h16(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                        void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8, void* stream);
/* One flow boundary of the no-grad forward in one launch, column by column of z_in [B][n_group][L]:
 *  - fold_acc != NULL: the forward coupling of the flow before, t2s_wg_end_fold_affine(reverse = 0) with (c_off_prev, n_half_prev
 *    <= 4); log_s (may be NULL) is that flow's;
 *  - W != NULL: this flow's 1x1 convolution on channels [c_off, c_off + n_rem), as t2s_wg_convinv;
 *  - all n_group <= 16 channels go to z_out (a second buffer: z_in stays as it was);
 *  - the window planes W_hi / W_lo of the folded WN.start over channels [c_off, c_off + n_half) of the finished columns, as
 *    t2s_wg_start_window writes them (taps <= 33, n_half <= 4 as in t2s_wg_res_only_start).  No X planes: t2s_wg_res_only_start rebuilds x0.
 * fold_acc == NULL and W == NULL: only the window planes, from z_in (z_out may be NULL). */
int t2s_wg_flow_boundary(const float* z_in, float* z_out, const float* fold_acc, int nslots, const float* bes, int n_layers,
                         const float* b_end, float* log_s, int c_off_prev, int n_half_prev, const float* W, int c_off, int n_rem,
                         int n_half, int B, int n_group, int L, int Lp, int halo, int taps, int win_chunks, void* W_hi, void* W_lo,
                         void* stream);
/* ---- Batched inference of mels of different lengths (ABI v4, compatible addition) ----
 * Within one column the inverse flow is pointwise; an entry of a padded batch reads past its own end only through the taps of the gate
 * GEMM on the X planes and through the taps the window planes hold.  So the writers of those planes take `lengths` ([B] int32 in
 * device memory, in columns; an entry's length is clamped to [0, L]) and the gate GEMMs stay as they are.  Each entry point below takes
 * its partner's arguments and checks plus `lengths` (NULL: T2S_EINVAL); for t < lengths[b] it stores what the partner stores.
 *  t2s_wg_start_ragged: t2s_wg_start_window, or t2s_wg_start when W_hi == W_lo == NULL (taps and win_chunks are not read then).  X rows
 *    lengths[b] <= t < L are stored as zeros, hi and lo (stored: the planes may hold a longer call's rows); a window tap at column
 *    tt >= lengths[b] counts as outside, for the audio columns and the ones-column.
 *  t2s_wg_res_only_ragged, t2s_wg_res_only_start_ragged: X rows lengths[b] <= t < L are stored as zeros, hi and lo.
 *  t2s_wg_flow_boundary_ragged: the window planes as t2s_wg_start_ragged writes them; coupling, convolution and z_out are per column
 *    and cover all L columns as in the partner. */
int t2s_wg_start_ragged(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                        int L, int Lp, int halo, void* X_hi, void* X_lo, int taps, int win_chunks, void* W_hi, void* W_lo,
                        const int* lengths, void* stream);
int t2s_wg_res_only_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                           void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8, const int* lengths,
                           void* stream);
int t2s_wg_res_only_start_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                                 const float* z, const float* w_start, const float* b_start, int n_group, int c_off, int n_half,
                                 void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, const int* lengths,
                                 void* stream);
int t2s_wg_flow_boundary_ragged(const float* z_in, float* z_out, const float* fold_acc, int nslots, const float* bes, int n_layers,
                                const float* b_end, float* log_s, int c_off_prev, int n_half_prev, const float* W, int c_off,
                                int n_rem, int n_half, int B, int n_group, int L, int Lp, int halo, int taps, int win_chunks,
                                void* W_hi, void* W_lo, const int* lengths, void* stream);
/* ---- The two above combined: the fp16 chain on a batch of different lengths (ABI v4, compatible addition) ----
 * Each entry point takes its _h16 partner's arguments and checks with `lengths` ([B] int32, device, columns, clamped to [0, L];
 * NULL: T2S_EINVAL) in front of `stream`.  The names end in `_ragged`: a name that ends in `_h16` promises its partner's exact argument list.
 * Below, len = the clamped lengths[b] and a tile = 256 columns starting at a multiple of 256.
 *  t2s_wg_start_h16_ragged: t2s_wg_start_h16 for rows t < len; rows len <= t < L are stored as zeros, hi and lo.  No window planes.
 *  t2s_wg_res_only_h16_ragged: t2s_wg_res_only_h16 for rows t < len, zeros for len <= t < L.  A tile that starts at or behind len is
 *    not computed: its zeros are stored and nothing is loaded.
 *  t2s_wg_in_cond_gate_fold_h16_ragged: both tile heights.  A tile that starts below len is t2s_wg_in_cond_gate_fold_h16's, bit for
 *    bit, the columns at and past len of a tile the end cuts included.  A tile that starts at or behind len is not computed: its
 *    acts columns are NOT written (t2s_wg_res_only_h16_ragged, their reader, drops the same tiles), and its fold_acc elements are
 *    stored as zeros when fold_init != 0 (t2s_wg_end_fold_affine reads every column) and left alone when fold_init == 0. */
int t2s_wg_start_h16_ragged(const float* z, const float* w, const float* bias, int B, int n_group, int c_off, int n_half, int C,
                            int L, int Lp, int halo, void* X_hi, void* X_lo, const int* lengths, void* stream);
int t2s_wg_in_cond_gate_fold_h16_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                                        const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, const void* fold_A,
                                        float* fold_acc, int fold_init, int B, int C, int n_cond, int taps, int dilation, int L,
                                        int Lp, int halo, int Mpad, const int* lengths, void* stream);
int t2s_wg_res_only_h16_ragged(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                               void* X_hi, void* X_lo, int B, int C, int L, int Lp, int halo, int Mpad, int pair8,
                               const int* lengths, void* stream);
/* WN.end output from the folded accumulators + affine coupling (forward or reverse) */
int t2s_wg_end_fold_affine(const float* fold_acc, int nslots, const float* bes, int n_layers, const float* b_end,
                           float* z, float* log_s, float* wn_out, int B, int n_group, int c_off, int n_half, int L, int reverse,
                           void* stream);

/* Generic split-bf16 conv1d-as-GEMM with bias + activation epilogue:
 *   out[b][o][t] = act(bias[o] + sum_{tap,c} W[o][c][tap] * x[b][c][t + (tap - taps/2)*dil])
 * A planes packed with T2S_PERM_NONE.  Writes planes O_hi/O_lo (may be NULL) and/or out_f32 (may be NULL),
 * laid out [B][C][L], or [B][L][C] when f32_channel_last=1.  Used for the Tacotron-2 encoder / postnet convolutions and LSTM input projections
 * (reference tacotron.py:177-194, modules.py:94-137). */
int t2s_conv_bias_act(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                      void* O_hi, void* O_lo, float* out_f32, int f32_channel_last, int B, int Cin, int Cout, int taps,
                      int dilation, int act, int L, int Lp, int halo, int Mpad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tacotron-2 (reference tacotron/tacotron.py, tacotron/modules.py).  All f32, exact.
 */

/* y[item][row] = act(bias1[row] + bias2[row] + [W1[row] | W2[row]] . [x1 | x2 | x3](item)) * mask * mask_scale
 * One wave per output row (weights in registers), loop over items.  Replaces the small Linear layers:
 * query_layer (tacotron.py:137), linear_projection / gate_layer (:387-392), Prenet (modules.py:19-22),
 * memory_layer (tacotron.py:306).  K = n1+n2+n3 = k1+k2 <= 4096; every n, k, ld and item stride a multiple of 4; W and x
 * 16-byte aligned; act 0..2.  Anything else: T2S_EINVAL, nothing enqueued.  More than 8 items with every n and k1 a multiple of
 * 16 run on the f32 matrix cores (same results up to summation order). */
int t2s_gemv(const float* W1, int ld1, int k1, const float* W2, int ld2, int k2, const float* x1, int n1, long sx1,
             const float* x2, int n2, long sx2, const float* x3, int n3, long sx3, const float* bias1,
             const float* bias2, float* y, long sy_item, long sy_row, int rows, int items, int act,
             const unsigned char* mask, long smask_item, float mask_scale, void* stream);

/* out[c][r] = in[r][c] */
int t2s_transpose(const float* in, float* out, int R, int C, void* stream);

/* embedding lookup -> planes: x[b][:, t] = emb[ids[b][t]]  (tacotron.py:40) */
int t2s_embed_planes(const long* ids, const float* emb, int B, int T, int E, int V, int Lp, int halo, void* X_hi,
                     void* X_lo, void* stream);
/* [B][C][L] f32 -> planes */
int t2s_f32_to_planes(const float* x, int B, int C, int L, int Lp, int halo, void* X_hi, void* X_lo, void* stream);
/* Tacotron.parse_output (reference tacotron.py:67-76): mel[b][:, t] = mel_post[b][:, t] = 0 and gate[b][t] = 1e3 for
 * t >= lengths[b], in place.  mel, mel_post: [B][n_mel][T] f32; gate: [B][T] f32; lengths: [B] int32 in device memory.
 * The reference does this with .data.masked_fill_ AFTER the postnet has run, i.e. on the very tensor the postnet's first
 * convolution saved for its backward pass: its weight gradient sees the masked mel (the training path re-derives that
 * convolution's saved input planes from the masked tensor, text2speech_amd/tacotron/tacotron.py). */
int t2s_taco_parse_output(float* mel, float* mel_post, float* gate, const int* lengths, int B, int n_mel, int T, void* stream);
/* Batched inference of texts of different lengths (ABI v4, compatible addition): planes [B][ceil(C/32)][Lp][32] (hi, lo, 16-byte
 * aligned) get zeros in rows halo + t for lengths[b] <= t < T; the halo rows are left alone.  After the embedding and after each
 * convolution a following convolution then reads zeros past every entry's end, as it reads its halo when the entry runs alone. */
int t2s_zero_plane_rows(void* X_hi, void* X_lo, const int* lengths, int B, int C, int T, int Lp, int halo, void* stream);
/* x[b][t][:] = 0 for lengths[b] <= t < N; x: [B][N][row] f32 (the alignments of a batch past each entry's output length) */
int t2s_zero_rows_f32(float* x, const int* lengths, int B, int N, int row, void* stream);
/* eval BatchNorm folded into the preceding conv: scale = gamma/sqrt(var+eps), bias' = (bias-mean)*scale+beta */
int t2s_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* conv_bias,
                float eps, int C, float* scale, float* bias_out, void* stream);

/* Training-mode BatchNorm1d on a conv output x[B][C][T]: batch mean / biased variance per channel (written to
 * mean/var), affine, activation, optional {0,1} dropout mask * mask_scale; result as planes and/or f32 [B][C][T]
 * (reference tacotron.py:183-184,193-194; modules.py:105-137 in .train() mode) */
int t2s_bn_train(const float* x, const float* gamma, const float* beta, float eps, int act, const unsigned char* mask,
                 float mask_scale, int B, int C, int T, int Lp, int halo, float* mean, float* var, void* O_hi, void* O_lo,
                 float* out_f32, void* stream);

/* nn.BatchNorm1d's bookkeeping in .train() mode after t2s_bn_train: running_x = (1 - momentum) running_x + momentum batch_x, the
 * variance unbiased by n / (n - 1) (n = B * T); *num_batches_tracked (int64, optional) += 1.  One launch per layer. */
int t2s_bn_running_update(const float* mean, const float* var, float* running_mean, float* running_var,
                          long long* num_batches_tracked, float momentum, long long n, int C, void* stream);
/* clears `bytes` bytes at p (16-byte aligned): the single fill of a training step's accumulator arena */
int t2s_zero_fill(void* p, size_t bytes, void* stream);

/* Encoder BiLSTM recurrence with packed-sequence semantics (tacotron.py:199-207).  gx[B][T][8H] = W_ih x + b_ih + b_hh
 * for both directions (fwd gates then reverse gates), whhT_* = W_hh^T [H][4H]; out[B][T_out][2H]; 4H must be 1024.
 * lengths[b] (NULL: all T) is cut to T_out (<= T): an entry longer than out's rows runs over its first T_out positions, as if its
 * length were T_out (all four recurrence entry points).  Rows of gates_save / c_save past an entry's length are not written. */
int t2s_taco_encoder_lstm(const float* gx, const float* whhT_fwd, const float* whhT_rev, const int* lengths, float* out,
                          int B, int T, int H, int T_out, float* gates_save /* [B][T][2][4H] or NULL */,
                          float* c_save /* [B][T][2][H] or NULL */, void* stream);
/* ABI v4.  The same recurrence with W_hh resident on the chip: four workgroups per (batch element, direction), each with a quarter
 * of the matrix in registers for the whole sequence, exchange their 64 new h values per step through tagged 8-byte granules in
 * `xbuf` (t2s_taco_lstm_xbuf_bytes(B) bytes, caller-owned, ZERO before its first use, not shared by launches that may overlap in
 * time; the last 8 bytes are an error word the kernel raises if a bounded wait expires - a caller that wants to know reads it
 * after synchronising).  `epoch` is the caller's launch counter for this buffer (any value that differs from the previous launches'
 * in its low 20 bits): tags of an earlier launch never match.  Same results as t2s_taco_encoder_lstm up to summation order.
 * H must be 256, T < 4095. */
int t2s_taco_encoder_lstm_split(const float* gx, const float* whhT_fwd, const float* whhT_rev, const int* lengths, float* out,
                                int B, int T, int H, int T_out, float* gates_save, float* c_save, void* xbuf, unsigned epoch,
                                void* stream);
long t2s_taco_lstm_xbuf_bytes(int B);
/* BPTT of that recurrence: d_out[B][T_out][2H] -> dgx[B][T][8H], hprev[B][T][2H] (the h each step consumed; the X operand of
 * the W_hh weight-gradient GEMM); rows past each length (cut to T_out as above) are not written - the caller clears them.  whh_*
 * are the natural [4H][H] matrices */
int t2s_taco_encoder_lstm_bwd(const float* d_out, const float* out, const float* gates_save, const float* c_save,
                              const float* whh_fwd, const float* whh_rev, const int* lengths, float* dgx, float* hprev,
                              int B, int T, int H, int T_out, void* stream);
/* ABI v4.  ... and its BPTT in the same form (xbuf / epoch as above; a buffer of its own if a forward may be in flight). */
int t2s_taco_encoder_lstm_bwd_split(const float* d_out, const float* out, const float* gates_save, const float* c_save,
                                    const float* whh_fwd, const float* whh_rev, const int* lengths, float* dgx, float* hprev,
                                    int B, int T, int H, int T_out, void* xbuf, unsigned epoch, void* stream);
/* f32 channel-last rows x[b][t][c] -> planes ; embedding gradient d_emb[v][e] = sum over (b,t) with ids == v of planes */
int t2s_rows_to_planes(const float* x, int B, int T, int C, int Lp, int halo, void* X_hi, void* X_lo, void* stream);
int t2s_embedding_grad(const long* ids, const void* D_hi, const void* D_lo, int B, int T, int E, int V, int Lp, int halo,
                       float* d_emb, void* stream);

/* Bernoulli(keep_prob) bytes (0/1) from a counter hash: dropout masks (the always-on prenet dropout,
 * modules.py:21, and the training-mode dropouts) when the caller does not inject them */
int t2s_bernoulli_mask(unsigned char* mask, size_t n, unsigned long long seed, unsigned long long offset, float keep_prob,
                       void* stream);

/* Decoder state + weights for t2s_taco_decode_steps.  Pointers are device pointers; f32 unless noted. */
typedef struct t2s_taco_decoder {
    int B, T_in, n_mel, prenet_dim, enc_dim, att_rnn_dim, dec_rnn_dim, att_dim, loc_filters, loc_kernel;
    int T_cap;           /* time capacity of mel_gate_out / align_out */
    int teacher_forced;  /* 1: step input = pre_all[step]; projection hoisted (hc_all); 0: autoregressive */
    int mask_steps;      /* autoregressive: number of [B][2][prenet] mask slices in prenet_masks */
    const float *att_w_ih, *att_w_hh, *att_b_ih, *att_b_hh;   /* attention_rnn (tacotron.py:366) */
    const float *dec_w_ih, *dec_w_hh, *dec_b_ih, *dec_b_hh;   /* decoder_rnn   (tacotron.py:380) */
    const float *w_query, *w_loc_conv, *w_loc_dense, *w_v;    /* attention_layer (tacotron.py:96-143) */
    const float *w_proj, *b_proj;        /* [n_mel+1][dec+enc]: linear_projection rows, then the gate_layer row */
    const float *w_projpre, *b_projpre;  /* [prenet][dec+enc] = W_prenet0 . W_proj[:n_mel], W_prenet0 . b_proj[:n_mel];
                                          * stored DIRECTLY BEHIND w_proj / b_proj (one [n_mel+1+prenet] row block) */
    const float *w_loc_denseT;           /* [loc_filters][att_dim] (transpose of w_loc_dense) */
    const float *w_pre2;                 /* [prenet][prenet] = prenet.layers.1 */
    const float *memory, *pmem;          /* [B][T_in][enc], [B][T_in][att_dim] */
    const int *mem_lengths;              /* [B] or NULL */
    const float *pre_all;                /* teacher forced: [T+1][B][prenet] */
    const unsigned char *prenet_masks;   /* autoregressive: [mask_steps][B][2][prenet] 0/1, slice s feeds step s */
    const unsigned char *att_drop, *dec_drop; /* training dropout on the LSTM outputs: [T][B][H] 0/1, or NULL */
    float att_drop_scale, dec_drop_scale;
    float *att_h0, *att_h1, *att_c, *dec_h0, *dec_h1, *dec_c;   /* ping-pong h (step parity), c in place */
    float *att_w, *att_wcum, *ctx, *q, *energies, *pre1, *pre2; /* [B][T_in] x3, [B][enc], [B][att_dim], ... */
    float *q_part;                       /* [att_rnn/2][B][att_dim] scratch: per-workgroup partial queries written by the attention
                                          * cell and summed by the fused attention kernel (B <= 8), or NULL (W_query . h there) */
    float *mel_gate_out;                 /* [B][n_mel+1][T_cap] (autoregressive), row n_mel = gate logit */
    float *align_out;                    /* [B][T_cap][T_in] */
    float *hc_all;                       /* teacher forced: [T][B][dec+enc] */
    /* training saves (teacher forced; all NULL otherwise): per step t */
    float *att_gates_all, *att_c_all;    /* [T][B][4H], [T][B][H] attention-LSTM gates (post-activation i,f,g,o) / cell state */
    float *dec_gates_all, *dec_c_all;    /* same for the decoder LSTM */
    float *att_h_all;                    /* [T][B][H] attention-LSTM output after dropout */
    float *q_all, *wcum_all;             /* [T][B][att_dim] queries, [T][B][T_in] cumulative weights after the step */
    /* ABI v4.  [3][B][4H] scratch, ZERO before step 0, or NULL.  Autoregressive decode at B <= 4 with
     * att_rnn_dim = dec_rnn_dim = 1024: the fused attention launch of step t also streams W_hh_dec . h_dec(t-1), W_ih_dec[:, :att_rnn] . h_att(t) and
     * W_hh_att . h_att(t) on the CUs the attention leaves idle and keeps the products here; the decoder cell of step t and the
     * attention cell of step t+1 then add them instead of streaming those 50 MB themselves.  State like h / c: carried between
     * calls that continue one utterance.  NULL: every cell streams its own weights (ABI v3 behaviour). */
    float *gate_part;
    /* ABI v4.  [prenet][prenet] TRANSPOSE of w_pre2, or NULL.  With gate_part: the prenet's second layer (modules.py:19-22) is
     * folded into the attention cell's launch - every workgroup recomputes its 256 outputs from pre1, as a sparse product (pre1 is
     * ~3/4 exact zeros after ReLU and dropout: one coalesced row of the transpose per nonzero) - instead of a GEMV launch of its own
     * on the serial chain.  NULL: the separate launch. */
    const float *w_pre2T;
    /* ABI v4.  [B][T_in][att_dim] scratch, ZERO before step 0, or NULL.  With gate_part: the location term of the attention
     * (location_dense o location_conv of the current weights / cumulative weights, tacotron.py:96-107) is computed one launch EARLIER,
     * by extra workgroups of the projection launch of the previous step (which leaves ~170 CUs idle), and the fused attention launch
     * only adds the query and the processed memory to it: the two exact-f32 matrix-core stages leave the one workgroup the whole
     * launch waits for (4 us at 128 encoder positions, growing linearly with T_in).  State like gate_part. */
    float *ploc;
    /* ABI v4.  Ignored: kept so that the layout stays v4 (a chunk-GEMM decode path that used it was measured no faster and removed,
     * DESIGN.md section 5d).  Every decoder cell streams all of [W_ih | W_hh]; pass NULL. */
    float *dec_in_part;
    /* ABI v4.  (B * T_in + 1) 8-byte words, ZERO before step 0 of a sequence (state like gate_part: tags are step numbers), or NULL.
     * At 9+ items with attention_dim 128, 32 location filters, T_in <= 512 and enc_dim a multiple of 64, the
     * energies launch also does softmax, cumulative weights and context: the workgroups of a batch element exchange their energies
     * through tagged granules here instead of ending the launch.  The last word is raised if a bounded wait expires.  A buffer
     * serves every step INDEX once per zeroing (the tag of step s is s + 1): callers that revisit step indices pass NULL.
     * NULL: energies and softmax + context stay two launches. */
    void *att_xbuf;
    /* ABI v4.  16 bytes (a step counter and an error word), ZERO before step 0 of a sequence, or NULL.  Teacher forced at 9+ items with
     * att_h_all: instead of running a chunk of 16 steps behind, the helper stream's decoder cell of step s - 1 is released by a word
     * the attention cell's launch of step s stores as it starts, so that it runs beside the attention launch of step s (whose
     * workgroups share a CU with it) and is over when the next attention cell needs the chip.  NULL: chunks (as with the environment variable T2S_DECODE_PACED=0, for tools that serialise
     * kernels across streams). */
    void *pace_flag;
} t2s_taco_decoder;

/* Enqueue decoder steps [step0, step0+n_steps) (Decoder.decode, tacotron.py:355-393, plus in autoregressive mode
 * the projection and the prenet of the next step, tacotron.py:447-461) on `stream` without host synchronisation.
 * Which kernels a step launches is decided once per call from the struct's shapes and NULL pointers (t2s_taco_decode_plan below
 * reports it; DESIGN.md section 5b lists the launches of every plan).  Three schedules:
 *  - serial: attention cell, attention, decoder cell [, projection + next prenet] of each step in turn, all on `stream`;
 *  - split (teacher-forced with att_h_all and hc_all given: training, or the no-grad forward at 9+ items): the decoder cells - which
 *    feed nothing but the next decoder cell and the projection after the loop - are enqueued on a library-owned helper stream, 16 steps
 *    behind the attention chain, reading h_att / ctx from those saves;
 *  - paced (split at 9+ items with pace_flag, unless T2S_DECODE_PACED=0): the helper's cell of step s - 1 is released by the word the
 *    attention cell of step s stores as it starts.
 * With the helper stream in use `stream` has been made to wait for it when the call returns, error returns included. */
int t2s_taco_decode_steps(const t2s_taco_decoder* d, int step0, int n_steps, void* stream);

/* The plan t2s_taco_decode_steps(d, step0, n_steps, .) would follow, as T2S_PLAN_* bits in *bits (may be NULL).  Host only: no
 * pointer of `d` is dereferenced and nothing is enqueued.  Returns what t2s_taco_decode_steps returns from its validation.  The
 * plan does not depend on the step range: decisions that look at a ping-pong buffer (att_h0 / att_h1, dec_h0 / dec_h1) hold only
 * if they hold for both, so calls that continue a sequence follow one plan (ABI v4, compatible addition). */
#define T2S_PLAN_SPLIT 0x001u         /* decoder cells on the helper stream (teacher-forced with att_h_all + hc_all) */
#define T2S_PLAN_PACED 0x002u         /* ... one step behind the chain, released through pace_flag; without it: 16-step chunks */
#define T2S_PLAN_SIG_BY_KERNEL 0x004u /* paced: the matrix-core attention cell stores the pace word; without it: a launch of its own */
#define T2S_PLAN_FUSED_ATT 0x008u     /* one attention launch per step; without it: [query GEMV +] energies [+ softmax / context] */
#define T2S_PLAN_Q_PARTS 0x010u       /* fused attention sums the partial queries of the attention cell's workgroups (q_part) */
#define T2S_PLAN_Q_BIG 0x020u         /* the energies kernel sums those of the matrix-core cell (q_part): no query GEMV */
#define T2S_PLAN_ONE 0x040u           /* the energies launch also does softmax, cumulative weights and context (att_xbuf) */
#define T2S_PLAN_STREAM_GATES 0x080u  /* the fused attention launch streams the cells' gate partials (gate_part) */
#define T2S_PLAN_FOLD_PRE2 0x100u     /* prenet layer 1 inside the attention cell's launch (w_pre2T), steps below mask_steps */
#define T2S_PLAN_USE_PLOC 0x200u      /* the attention's location term comes out of the previous projection launch (ploc) */
#define T2S_PLAN_PROJ_FUSED 0x400u    /* autoregressive: projection and the next prenet layer 0 in one launch */
#define T2S_PLAN_UNITS_2 0x800u       /* the VALU cells take 2 hidden units per workgroup (att_gates_all given); without it: 4 */
int t2s_taco_decode_plan(const t2s_taco_decoder* d, int step0, int n_steps, unsigned* bits);

/* ABI v4, compatible addition.  attention_rnn.weight_ih / _hh and decoder_rnn.weight_ih / _hh as IEEE binary16 (what a .half() model
 * holds): device pointers, 8-byte aligned, shapes and row-major layout those of the f32 members of t2s_taco_decoder with the same
 * names (every row length a multiple of 4). */
typedef struct t2s_taco_w16 {
    const void *att_w_ih, *att_w_hh, *dec_w_ih, *dec_w_hh;
} t2s_taco_w16;

/* t2s_taco_decode_steps with the four LSTM matrices streamed from `w` - half the bytes per step - and widened to f32 in registers.
 * Autoregressive decode of up to 8 items: the two VALU cells, the folded-prenet attention cell and the gate-stream role of the fused
 * attention launch read `w`; everything else (biases, state, inputs, the other weights, `w_pre2T`) stays f32 and comes from `d`, whose
 * four f32 matrix pointers are validated as by t2s_taco_decode_steps and not read.  The plan is chosen as for `d` alone, and a slot
 * of 4 halves sits at the k of the f32 form's float4, so sums run in the same order: the outputs EQUAL those of
 * t2s_taco_decode_steps on the widened matrices bit for bit (fp16 subnormals widen exactly).
 * No fallback: T2S_EINVAL, with nothing enqueued, for what the fp16 kernels do not cover - teacher_forced, B > 8, any training save
 * pointer (att_gates_all, att_c_all, dec_gates_all, dec_c_all, att_h_all, q_all, wcum_all) - and for `w` NULL, a NULL member, a
 * member that is not 8-byte aligned, or a matrix row length that is not a multiple of 4. */
int t2s_taco_decode_steps_w16(const t2s_taco_decoder* d, const t2s_taco_w16* w, int step0, int n_steps, void* stream);

/* Host only, like t2s_taco_decode_plan: returns what t2s_taco_decode_steps_w16(d, w, step0, n_steps, .) returns from its validation;
 * *bits (may be NULL) is exactly what t2s_taco_decode_plan gives for `d`; *lstm_weight_bytes (may be NULL) is the number of bytes of
 * the four LSTM matrices that one decoder step reads (2 bytes per element).  With w == NULL (where the steps call refuses) it
 * accepts every struct t2s_taco_decode_plan accepts and reports the f32 figure of t2s_taco_decode_steps, 4 bytes per element. */
int t2s_taco_decode_plan_w16(const t2s_taco_decoder* d, const t2s_taco_w16* w, int step0, int n_steps, unsigned* bits,
                             long long* lstm_weight_bytes);

/* ABI v4.  One call of the location-sensitive attention alone (Attention.forward, tacotron.py:145-166, with the state update of
 * Decoder.decode around it, tacotron.py:371-379): query = w_query . h_att, energies from the location features of (w, w_cum) and
 * the processed memory, masked softmax over T, context.  IN PLACE: w [B][T] holds the previous weights on entry and the new ones on
 * return, w_cum [B][T] is incremented by them, ctx [B][enc] receives the context.  q_scratch [B][att_dim], e_scratch [B][T].
 * lengths [B] int32 or NULL.  Same kernels as t2s_taco_decode_steps (one fused launch up to 8 items, else
 * query GEMV + energies + softmax/context). */
int t2s_taco_attention(const float* h_att, const float* memory, const float* pmem, const int* lengths, float* w, float* w_cum,
                       float* ctx, float* q_scratch, float* e_scratch, const float* w_query, const float* w_loc_conv,
                       const float* w_loc_dense, const float* w_loc_denseT, const float* w_v, int B, int T, int att_rnn,
                       int att_dim, int enc_dim, int loc_filters, int loc_kernel, void* stream);

/* stop_step[b] = first step in [step0, step0+n) with sigmoid(gate) > threshold, if still -1 (tacotron.py:455) */
int t2s_taco_stop_check(const float* mel_gate_out, int B, int n_mel, int T_cap, int step0, int n, float threshold,
                        int* stop_step, void* stream);

/* ------------------------------------------------------------------------------------------------
 * WaveGlow training step (reference waveglow/train.py:110-124: forward -> WaveGlowLoss -> backward -> Adam;
 * the reference gets its backward from autograd over glow.py:207-249, these are the hand-written equivalents).
 * "time-major planes": tm[b][t/32][row][t%32] bf16 (hi, lo) - the operands of the weight-gradient GEMMs,
 * whose contraction index is time.
 */

/* training-mode forms of the two WN-layer entry points: also save the sigmoid values (G planes; the tanh planes T are optional,
 * pass NULL: the backward pass rebuilds tanh as acts / sigmoid) for the backward pass, and read the residual from R planes so
 * every layer's input stays resident */
int t2s_wg_in_cond_gate_train(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                              const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, void* T_hi, void* T_lo,
                              void* G_hi, void* G_lo, int B, int C, int n_cond, int taps, int dilation, int L, int Lp,
                              int halo, int Mpad, void* stream);
int t2s_wg_res_skip_train(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi,
                          const void* acts_lo, const void* R_hi, const void* R_lo, void* X_hi, void* X_lo, float* skip,
                          int B, int C, int n_res, int skip_init, int L, int Lp, int halo, int Mpad, void* stream);

/* Training forward on the no-grad forward's kernels (round 3).  The skip path only ever feeds WN.end (glow.py:172-175), so the
 * training forward folds it into the gate GEMM's epilogue exactly as the no-grad forward does (t2s_wg_in_cond_gate_fold) and
 * never forms the skip sum; the backward pass, which needs it once per flow for WN.end's weight gradient, rebuilds it with
 * t2s_wg_skip_sum from the saved gate outputs.  What training adds to the forward is only what it saves:
 *   t2s_wg_in_cond_gate_fold_train = t2s_wg_in_cond_gate_fold + the sigmoid planes G (tanh is rebuilt as acts / G) + act_bchunks:
 *     32-channel chunks between batch entries of the acts / G planes (0 = C/32), so that the gate outputs of all layers of a flow
 *     can sit side by side in one plane set;
 *   t2s_wg_res_only_train = t2s_wg_res_only reading the layer input from R and writing the next layer's input to X (both are kept);
 *   t2s_wg_end_fold_affine(wn_out != NULL) also stores (b ; log_s) for the coupling's backward.
 * t2s_wg_skip_sum: skip[b][c][t] = bias[c] + sum_k A[k][c] * acts[b][k][t] over n_k_chunks * 32 K channels - with A the skip rows
 * of a flow's res_skip weights packed one after the other along K (t2s_pack_conv_weight, koff = layer * C) and acts the flow-wide
 * planes, this is sum_i (W_skip,i acts_i + b_skip,i): f32 planes [B][C/32][Lp][32] as t2s_wg_res_skip_train writes them. */
int t2s_wg_in_cond_gate_fold_train(const void* A_hi, const void* A_lo, const float* bias, const void* X_hi, const void* X_lo,
                                   const void* S_hi, const void* S_lo, void* acts_hi, void* acts_lo, void* G_hi, void* G_lo,
                                   int act_bchunks, const void* fold_A, float* fold_acc, int fold_init, int B, int C, int n_cond,
                                   int taps, int dilation, int L, int Lp, int halo, int Mpad, void* stream);
int t2s_wg_res_only_train(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                          int act_bchunks, const void* R_hi, const void* R_lo, void* X_hi, void* X_lo, int B, int C, int L, int Lp,
                          int halo, int Mpad, int pair8, void* stream);
int t2s_wg_skip_sum(const void* A_hi, const void* A_lo, const float* bias, const void* acts_hi, const void* acts_lo,
                    int n_k_chunks, int act_bchunks, float* skip, int B, int C, int L, int Lp, int halo, int Mpad, void* stream);

/* d_pre = gate'(acts, G) * (W_rs^T [d_x ; d_skip]):  data gradient of res_skip_layers[i] fused with the backward of
 * tanh*sigmoid (glow.py:33-40,164), from the layer's saved gate output acts = tanh * sigmoid and G = sigmoid (tanh = acts / G).
 * A = t2s_pack_transposed(W_rs); DX may be NULL (last layer: skip rows only).
 * DP planes have 2C channels (tanh half, then sigmoid half).  dp_bchunks: 32-channel chunks between batch entries of the DP
 * planes (0 = 2C/32): DP may be a slice of a wider plane set - the training path keeps the d_pre of all layers of a flow side
 * by side so that the conditioning gradient is ONE K-concatenated GEMM per flow.  tg_bchunks: the same for the acts / G planes
 * (0 = C/32): the training forward keeps the gate outputs of a flow's layers side by side too (t2s_wg_skip_sum). */
int t2s_wg_bwd_gate_dgrad(const void* A_hi, const void* A_lo, const float* zero_bias, const void* DX_hi,
                          const void* DX_lo, const void* DS_hi, const void* DS_lo, const void* acts_hi, const void* acts_lo,
                          const void* G_hi, const void* G_lo, int tg_bchunks, void* DP_hi, void* DP_lo, int dp_bchunks, int B, int C,
                          int L, int Lp, int halo, int Mpad, int pair8, void* stream);

/* O (+)= conv(X) with packed (transposed) weights: data gradients of in_layers[i] (dilated, taps mirrored) and
 * cond_layers[i].  init=1 stores, init=0 accumulates into the O planes.  x_bchunks: chunks between batch entries of the X
 * planes (0 = Cin/32; X may be a slice of a wider plane set, see t2s_wg_bwd_gate_dgrad). */
int t2s_conv_accumulate(const void* A_hi, const void* A_lo, const float* zero_bias, const void* X_hi, const void* X_lo,
                        int x_bchunks, void* O_hi, void* O_lo, int B, int Cin, int Cout, int taps, int dilation, int init, int L, int Lp,
                        int halo, int Mpad, int pair8, void* stream);

/* out[b*ksplit + s][m][n] = sum over time chunks [k0,k1) (split s of ksplit) of A_tm[b][t][m] * X_tm[b][t][n]:
 * B*ksplit split-K slabs; chunks outside [k0,k1) (the zero halo) are skipped */
int t2s_wgrad_gemm(const void* A_hi, const void* A_lo, const void* X_hi, const void* X_lo, const float* zero_bias,
                   float* out, int B, int M, int N, int Mpad, int Npad, int n_tchunks, int k0, int k1, int ksplit,
                   void* stream);
/* Same contraction with K flattened over (batch element, time chunk): out = [nsplit][M][N] slabs, slab s covering
 * ceil(B*(k1-k0)/nsplit) consecutive flattened K-steps, so the split count can be chosen to fill the chip in one round
 * (nsplit ~ 256 / (ceil(M/256)*ceil(N/256))) instead of being a multiple of B. */
int t2s_wgrad_gemm_flat(const void* A_hi, const void* A_lo, const void* X_hi, const void* X_lo, const float* zero_bias,
                        float* out, int B, int M, int N, int Mpad, int Npad, int n_tchunks, int k0, int k1, int nsplit,
                        void* stream);

/* The same contraction straight from CHANNEL-LAST planes (no time-major copies): the transpose happens in the LDS read
 * (ds_read_b64_tr_b16).  Operands are lists of 32-channel chunks, 8 per 256-row tile (pad with a chunk of zeros):
 *   hi / lo  = device pointers to plane row 0 of that chunk for batch entry 0 (a dilated tap is a row offset folded into the
 *              pointer: the autograd of in_layers[i], glow.py:134-139, needs x shifted by (tap - 1) * dilation);
 *   bstride  = u16 elements between batch entries (0 for constants such as the all-ones bias chunk).
 * out = [nsplit][M][ldp] f32 slabs (ldp >= N floats per row; columns N .. ldp-1 are scratch) over K-blocks [k0, k1) of 32 plane
 * rows of each of the B batch entries, as t2s_wgrad_gemm_flat.  ldp % 4 == 0 (and out 16-byte aligned) selects the ping-pong
 * kernel, whose epilogue stores 16-byte pieces; any other ldp the round-2 lockstep kernel.
 * Every K-block is a WHOLE block of 32 plane rows starting at row 32 k (+ the shift folded into the pointer): the caller makes
 * sure rows [32 k0 - max shift, 32 k1 + max shift) exist in every plane (halo % 32 == 0 does, text2speech_amd/glow.py geom()).
 * bias_cols != 0 (ping-pong kernel only, ldp >= N + 4, N % 256 == 0 - whole N tiles: in a ragged last tile columns N .. N+3 are
 * scratch columns of the tile's own epilogue - else T2S_EINVAL): columns N .. N+3 of every slab also receive four partial sums of the
 * M-side operand's rows over the slab's K range - the bias gradient of a convolution, db[m] = sum_t d_out[m][t], without an
 * all-ones column in the N-side table (t2s_wn_backward adds them: n_bias_cols = 4).
 * Both tables live in device memory ([n_tiles * 8] entries).  Replaces 7 t2s_plane_transpose launches per WN layer. */
typedef struct t2s_wgrad_chunk {
    const void* hi;
    const void* lo;
    long bstride;
} t2s_wgrad_chunk;
int t2s_wgrad_cl(const t2s_wgrad_chunk* a_chunks, int n_a_chunks, const t2s_wgrad_chunk* b_chunks, int n_b_chunks, float* out,
                 int B, int M, int N, int ldp, int k0, int k1, int nsplit, int bias_cols, void* stream);

int t2s_plane_transpose(const void* src_hi, const void* src_lo, int B, int src_chunks, int n_chunks, int Lp, int shift,
                        void* dst_hi, void* dst_lo, int Npad, int n_off, void* stream);
int t2s_tm_ones_row(void* dst_hi, void* dst_lo, int B, int Lp, int halo, int L, int Npad, int n_row, void* stream);
/* A[c][koff + tap'*O_pad + o] = scale[o] * v[o][c][flip ? Kt-1-tap' : tap'] -> (hi, lo) [k/32][Mpad][32] */
int t2s_pack_transposed(const float* v, const float* scale, int O, int Cin, int Kt, int flip, int O_pad, int Mpad,
                        int koff, void* A_hi, void* A_lo, int pair8, void* stream);
/* ABI v4: pair8 (t2s_pack_transposed, t2s_wg_bwd_gate_dgrad, t2s_conv_accumulate).  pair8 = 1 packs the M rows of the transposed
 * operand in PERM_PAIR8 order (within every 32 rows, packed row 16 m + 4 q + e = row 8 q + 4 m + e) and tells the two backward GEMMs
 * that their A operand is packed so: their epilogues then move whole 16-byte pieces per plane (8 consecutive channels per lane)
 * instead of 8-byte ones.  Only the 256-row ping-pong kernels have that epilogue: ask t2s_wg_bwd_pair8_ok(B, rows, L) (rows = Cout of
 * t2s_conv_accumulate / C of t2s_wg_bwd_gate_dgrad) before packing; a GEMM call with pair8 = 1 on a shape that takes the 128-row
 * kernels returns T2S_EINVAL.  T2S_BWD_PAIR8=0: t2s_wg_bwd_pair8_ok answers 0. */
int t2s_wg_bwd_pair8_ok(int B, int rows, int L);
/* per-row scale g/|v| of a weight-normed conv (what the forward pack applied), for t2s_pack_transposed */
int t2s_weightnorm_scale(const float* v, const float* g, int O, int K, float* scale, void* stream);
/* reduce split-K slabs P[nsplit][Prows][Pcols] and apply weight_norm's backward (g NULL: plain weight); the bias gradient is
 * the sum over slabs of columns col_bias .. col_bias + n_bias_cols - 1 (n_bias_cols >= 1) */
int t2s_wn_backward(const float* P, int nsplit, int Prows, int Pcols, int row_off, int col_off, int tap_stride,
                    int col_bias, int n_bias_cols, const float* v, const float* g, int O, int Cin, int Kt, float* dv, float* dg,
                    float* db, int db_accum, void* stream);
/* affine coupling backward + un-apply (glow.py:241-246); wn_out = (b ; log_s) [B][2nh][L], d_out gets (d_b ; d_log_s).
 * g_log_s = upstream gradient of this flow's log_s output: [B][nh][L], or - g_log_s_scalar != 0 - ONE float that stands for
 * every element (WaveGlowLoss's gradient is the constant -1/N broadcast, glow.py:52-58), or NULL for none. */
int t2s_wg_affine_backward(float* z, float* dz, const float* wn_out, const float* g_log_s, int g_log_s_scalar, float* d_out, int B,
                           int n_group, int c_off, int n_half, int L, void* stream);
/* out[r][j] (or [j][r]) = sum_{b,t} P[b][r][t] * Q[b][q_off+j][t], rowsum[r] = sum P; P = planes (hi/lo, or f32).
 * scratch: t2s_small_wgrad_scratch(B, chunks) floats of partial sums (reduced in a fixed order: deterministic). */
long t2s_small_wgrad_scratch(int B, int chunks);
int t2s_small_wgrad(const void* P_hi, const void* P_lo, const float* P_f32, const float* Q, float* out, float* rowsum,
                    float* scratch, int B, int chunks, int Lp, int halo, int L, int R, int J, int Jtot, int q_off, int out_transposed,
                    void* stream);
int t2s_rows_sum(const float* Q, int B, int Jtot, int q_off, int J, int L, float* out, void* stream);
/* d_z[:, c_off:c_off+n_half] += W_start^T d_x */
int t2s_wg_start_dgrad(const void* X_hi, const void* X_lo, const float* w, float* dz, int B, int n_group, int c_off,
                       int n_half, int C, int L, int Lp, int halo, void* stream);
/* dW = d_out . z_in^T + (*gscale_ptr * gmul) * W^-T   (glow.py:100-101) */
int t2s_wg_convinv_wgrad(const float* dz, const float* zin, const float* Winv, const float* gscale_ptr, float gmul,
                         int B, int n_group, int c_off, int n, int L, float* dW, void* stream);
/* ConvTranspose1d weight / bias gradient from the conditioning-plane gradient (glow.py:215-221) */
int t2s_wg_upsample_wgrad(const void* D_hi, const void* D_lo, const float* mel, int B, int n_mel, int frames, int ksize,
                          int stride, int n_group, int L, int Lp, int halo, float* dW, float* db, void* stream);

/* Adam over every parameter in one launch (torch.optim.Adam semantics; waveglow/train.py:79,124).  `jobs` is a
 * DEVICE array; job i owns blocks [blk_start, blk_start + ceil(n/1024)).  gscale multiplies the gradient first. */
typedef struct t2s_adam_job {
    float* p; const float* g; float* m; float* v;
    long n;
    long blk_start;
} t2s_adam_job;
int t2s_adam_table(const t2s_adam_job* jobs, int n_jobs, long total_blocks, float lr, float beta1, float beta2,
                   float eps, int step, float gscale, float weight_decay, void* stream);

/* Global gradient norm, clipping and the non-finite skip over the same job table (torch.nn.utils.clip_grad_norm_ semantics,
 * train.py:228-229), all without a host read.  Added within ABI v4.
 * t2s_grad_norm_table: the L2 norm of every job's `g` (only `g`, `n` and `blk_start` of a job are read).  Squares and sums are in
 * double, per-workgroup partials in `partial` (scratch of t2s_grad_norm_partials() doubles, every slot overwritten), added in a fixed
 * order: the same data gives the same bits.  out[4] (f32, device): out[0] = sqrt(sum) * gscale, the norm of the scaled gradients;
 * out[1] = min(1, max_norm / (out[0] + 1e-6)) in f32, torch's clip coefficient (a NaN norm gives NaN; max_norm = +inf gives exactly 1:
 * report only); out[2] = 1 if out[0] is not finite, else 0; out[3] = 0.  max_norm must be >= 0.
 * t2s_grad_scale_table: g[i] *= clip[1].  It WRITES through the jobs' `g` pointers, which every other entry point only reads.
 * t2s_adam_table_clip: t2s_adam_table with the gradient scale gscale * clip[1], `clip` being the `out` above; with clip[1] == 1 the
 * same bits as t2s_adam_table.  skip_nonfinite != 0 and clip[2] != 0: nothing is written, p, m and v keep their bits. */
int t2s_grad_norm_partials(void);
int t2s_grad_norm_table(const t2s_adam_job* jobs, int n_jobs, long total_blocks, float gscale, float max_norm,
                        double* partial, float* out, void* stream);
int t2s_grad_scale_table(const t2s_adam_job* jobs, int n_jobs, long total_blocks, const float* clip, void* stream);
int t2s_adam_table_clip(const t2s_adam_job* jobs, int n_jobs, long total_blocks, float lr, float beta1, float beta2, float eps,
                        int step, float gscale, float weight_decay, const float* clip, int skip_nonfinite, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tacotron-2 training step, backward (reference: autograd over tacotron/tacotron.py:36-49,355-429 and
 * tacotron/modules.py:19-22,94-137; loop train.py:219-225).  Weight gradients of every Linear / LSTM matrix contract
 * over (step, batch) items and reuse t2s_wgrad_gemm on time-major planes built by t2s_rows_to_tm.
 */
/* x[item - shift][c] (f32 rows, stride ld) -> time-major planes tm[item/32][n_off + c][item%32]; items_pad % 32 == 0 */
int t2s_rows_to_tm(const float* x, long ld, int items, int items_pad, int shift, int C, void* dst_hi, void* dst_lo,
                   int Npad, int n_off, void* stream);
/* the same for nb sets at once: set z reads x + z * x_bstride (floats) and writes its planes at dst + z * dst_bstride (bf16
 * elements) - e.g. one set per batch element in front of a t2s_wgrad_gemm with B = nb */
int t2s_rows_to_tm_batched(const float* x, long ld, long x_bstride, int items, int items_pad, int shift, int C, void* dst_hi,
                           void* dst_lo, long dst_bstride, int Npad, int n_off, int nb, void* stream);
/* LSTMCell backward, pointwise part: dh = (dh1+dh2+dh3)*dropout -> dgates[B][4H] (i,f,g,o), dc_carry updated in place */
int t2s_lstm_cell_bwd(const float* dh1, long s1, const float* dh2, long s2, const float* dh3, long s3,
                      const unsigned char* drop_mask, float drop_scale, const float* gates, const float* c_new,
                      const float* c_prev, float* dc_carry, float* dgates, int B, int H, void* stream);
/* dz = (y > 0) ? scale*dy : 0  (backward of relu followed by dropout-with-scale, e.g. the prenet) */
int t2s_relu_drop_bwd(const float* dy, const float* y, float scale, size_t n, float* dz, void* stream);

typedef struct t2s_att_bwd {
    const float *dctx1; long sc1; const float *dctx2; long sc2; const float *dctx3; long sc3;
    const float *w_cur; long s_wcur;
    const float *w_prev, *wc_prev; long s_wprev, s_wcprev;
    const float *q, *pmem, *memory; const int *lengths;
    const float *w_loc_conv, *w_loc_dense, *w_v;
    float *dw_carry, *dwc_carry, *d_q, *d_pmem, *d_memory;
    float *dD_part, *dK_part, *dv_part;   /* += ; one slot per (batch element, 32-position chunk): [B*ceil(T/32)][...];
                                             dD slots hold the transposed gradient [loc_f][att_dim] */
    float *dw_buf, *df_buf, *dq_part;     /* scratch: [B][T], [B][T][32], [B][ceil(T/32)][att_dim] */
    float *dctx_out;                      /* optional [B][enc]: d_ctx of this step; with it d_memory may be NULL and the caller
                                           * forms d_memory = sum_t w_t (x) d_ctx_t once after the loop */
    int B, T, att_dim, enc_dim, loc_f, loc_ks;
    /* the one-launch form (all three set; needs dctx_out, d_memory NULL, attention_dim 128, 32 filters, kernel <= 31; d_q is then
     * NOT written - sum dq_part over the chunks): the step's saved context [B][.] (row stride s_ctx) and
     * the carry buffers the step WRITES (it reads dw_carry / dwc_carry); all four are then [3][B][T] (see t2s_taco_bptt) */
    const float *ctx; long s_ctx;
    float *dw_carry_out, *dwc_carry_out;
} t2s_att_bwd;
/* one decoder step of the location-sensitive attention, backward (tacotron.py:124-166,379).  T2S_EINVAL, nothing enqueued:
 * att_dim > 128, loc_f > 32, loc_ks even or > 63, enc_dim % 4 != 0 or > 1024, a NULL required pointer, or the one-launch fields
 * with a shape or a d_memory that form does not take (t2s_taco_bptt_steps asks the same of its dimensions) */
int t2s_taco_att_bwd(const t2s_att_bwd* a, void* stream);

/* Reversed decoder loop (BPTT through tacotron.py:355-393,418-427): steps t_hi-1 ... t_lo, newest first.  All buffers are the
 * caller's; histories are [T_out][B][...] unless noted.  W_dT = [W_ih | W_hh]^T of decoder_rnn ([A+E+D][4D]), W_aT the same
 * for attention_rnn ([P+E+A][4A]), w_query = query_layer weight as stored ([att_dim][A]).  out_d / out_a receive d[input | h] of the two
 * cells ([T_out][B][A+E+D] and [T_out][B][P+E+A]); dg_d / dg_a / dq_all keep every step's gate / query gradients for the
 * weight-gradient GEMMs that follow the loop. */
typedef struct t2s_taco_bptt {
    int B, T_in, T_out, T_cap;
    int prenet_dim, enc_dim, att_rnn_dim, dec_rnn_dim, att_dim, loc_filters, loc_kernel;
    const float *W_dT, *W_aT, *w_query, *w_loc_conv, *w_loc_dense, *w_v;
    const float *dec_gates_all, *dec_c_all, *att_gates_all, *att_c_all, *q_all, *wcum_all;
    const float *align;                    /* [B][T_cap][T_in] */
    const float *pmem, *memory; const int *lengths;
    const unsigned char *att_drop, *dec_drop; float att_drop_scale, dec_drop_scale;
    const float *d_hc;                     /* [T_out][B][D+E]: gradient of [h_dec | ctx] from projection + gate */
    float *out_d, *out_a, *dg_d, *dg_a, *dq_all;
    float *dc_d, *dc_a, *dw_c, *dwc_c;                  /* carries: [B][D], [B][A], [B][T_in] x2 (zero-initialised) */
    float *d_pmem, *d_memory;                           /* += [B][T_in][att_dim], [B][T_in][enc] */
    float *dD_part, *dK_part, *dv_part, *dw_buf, *df_buf, *dq_part;   /* as in t2s_att_bwd */
    float *dctx_all;                                    /* optional [T_out][B][enc]: every step's d_ctx; then d_memory is not
                                                         * touched by the loop (deferred, see t2s_att_bwd.dctx_out) */
    /* optional, all or none (needs dctx_all, attention_dim 128, 32 location filters, kernel <= 31): the attention backward of a
     * step in ONE launch.  ctx_all = the forward's contexts, step t / item b at ctx_all + t * s_ctx_step + b * s_ctx_item;
     * dw_c2 / dwc_c2 = a second pair of carry buffers, zero-initialised like dw_c / dwc_c (step t reads the pair of parity
     * t & 1 - dw_c for even t - and writes the other).  With these, all four carry buffers are [3][B][T_in]: slot 0 the part
     * a 32-position chunk computes for itself, slots 1 / 2 the parts reaching in from the chunk to the right / left. */
    const float *ctx_all; long s_ctx_step, s_ctx_item;
    float *dw_c2, *dwc_c2;
    /* ABI v4.  (B * ceil(T_in / 32) * 128 + 3) 8-byte words (the last three: the error word and two unused words), ZERO before a BPTT pass, or NULL.  With the one-launch attention backward
     * (ctx_all ...) and T_in <= 512: the attention LSTMCell's pointwise backward (with W_query^T d_q) runs inside that launch - the
     * chunk workgroups of a batch element exchange their partial d_q through tagged granules here (tag = step + 1), each then takes its
     * share of the hidden units.  The last word is raised if a bounded wait expires.  NULL: a launch of its own. */
    void *att_xbuf;
} t2s_taco_bptt;
/* Launch sequencing only.  The decoder-cell chain and the location-conv part of the
 * attention backward run on two library-owned non-blocking streams (created on first use on the current device, kept for the
 * life of the process), ordered against `stream` with events; everything this call enqueues is complete, as seen from
 * `stream`, once the call's last wait has been passed.  Not re-entrant across host threads for the same device. */
int t2s_taco_bptt_steps(const t2s_taco_bptt* p, int t_hi, int t_lo, void* stream);

/* Tacotron2Loss (tacotron/loss_function.py:3-18): out[0] = mean((mel-target)^2) + mean((post-target)^2) + mean(BCEWithLogits(gate,
 * gate_target)), out[1] = the two mel terms, out[2] = the gate term; d_mel / d_post / d_gate (each optional) receive the
 * gradients for an upstream gradient of 1.  partial = scratch of 256*3 doubles (two-stage, order-independent reduction). */
int t2s_taco_loss(const float* mel, const float* post, const float* target, size_t n_mel, const float* gate,
                  const float* gate_target, size_t n_gate, float* d_mel, float* d_post, float* d_gate, void* partial,
                  float* out, void* stream);

/* WaveGlowLoss (waveglow/glow.py:43-59): out[0] = (sum z^2 / (2 sigma^2) - sum_k sum log_s[k] - sum_k log_det[k]) / n_z.
 * log_s / n_log_s are HOST arrays of n_flows (<= 16) device pointers / element counts, log_det a device array of n_flows
 * floats.  d_z (optional) receives z / (sigma^2 n_z); the gradients w.r.t. log_s and log_det are the constant -1 / n_z.
 * partial = scratch of 256*2 doubles. */
int t2s_waveglow_loss(const float* z, size_t n_z, const float* const* log_s, const size_t* n_log_s, int n_flows,
                      const float* log_det, float sigma, float* d_z, void* partial, float* out, void* stream);

typedef struct t2s_bn_bwd_args {
    const float *x, *mean, *var, *gamma, *beta; float eps;
    const float *dout_f32; const void *dout_hi, *dout_lo;
    const unsigned char *mask; float mask_scale; int act;
    float *dgamma, *dbeta; void *dx_hi, *dx_lo;
    int B, C, T, Lp, halo;
} t2s_bn_bwd_args;
/* training-mode BatchNorm1d backward fused with the backward of activation + dropout; dx as planes.
 * ABI v4: `partial` = scratch of B * C * 2 doubles (the per-batch-element sums S1, S2, added in a fixed order: bitwise reproducible) */
int t2s_bn_bwd(const t2s_bn_bwd_args* a, void* partial, void* stream);
/* out[j] = sum_i in[i][j] ; out = a (+ b) (+ c): b and c optional, so it is also the stream-ordered copy of an f32 buffer */
int t2s_sum_axis0(const float* in, int n0, int n, float* out, void* stream);
int t2s_add3(const float* a, const float* b, const float* c, size_t n, float* out, void* stream);
/* out[i] = (in ? in[i] : 1) * scalar[0] * mul, scalar in DEVICE memory: how a loss hands its saved gradient times the upstream
 * gradient (a 0-dim device tensor in `loss.backward()`, waveglow/train.py:122) to the model's backward without an eager operator */
int t2s_scale_by_scalar(const float* in, size_t n, const float* scalar, float mul, float* out, void* stream);
/* planes -> f32 [B][C][L] (accumulate=1: +=) */
int t2s_planes_to_f32(const void* X_hi, const void* X_lo, int B, int C, int L, int Lp, int halo, float* out,
                      int accumulate, void* stream);

/* ---- audio front-end / back-end ------------------------------------------------------------------
 * Each of the three stages below is one body and one set of kernels behind two entry points: the plain one here is the
 * lengths-free form (every entry has the batch's extent, T samples or F frames) of its _ragged partner further down, with the same
 * checks.  B <= 65535 for t2s_stft_transform and t2s_stft_inverse (the batch index is a grid y / z dimension; a larger B is
 * T2S_EINVAL); ld_mt > 0 for t2s_mel_from_mag.
 * STFT.transform (utils/stft.py:72-99): audio [B][T] -> frames F = T/hop + 1, bins c = n_fft/2 + 1.
 *   fwd_basis [2c][n_fft] (windowed Fourier basis, real rows then imaginary rows); scratch xp [B][ldp] (ldp >= T + n_fft,
 *   ldp % 4 == 0) and ft [B][F][2c]; outputs (each optional) mag / phase [B][c][F] and magT [B*F][ld_mt] (zero padded rows:
 *   the operand of t2s_mel_from_mag, ld_mt % 16 == 0). */
int t2s_stft_transform(const float* audio, int B, int T, const float* fwd_basis, int n_fft, int hop, float* xp, long ldp,
                       float* ft, float* mag, float* phase, float* magT, long ld_mt, void* stream);
/* TacotronSTFT.mel_spectrogram after the STFT (utils/layers.py:76-78): mel [B][n_mel][F] = log(max(mel_basis . mag, clip));
 * mel_basis_p [n_mel][ld_mt] zero padded; clip <= 0 skips the log. */
int t2s_mel_from_mag(const float* magT, long ld_mt, int B, int F, const float* mel_basis_p, int n_mel, float clip, float* mel,
                     void* stream);
/* STFT.inverse (utils/stft.py:101-129) with the Denoiser's spectral subtraction fused when bias != NULL
 * (waveglow/denoiser.py:36-38: m = max(mag - strength * bias[bin], 0)).  inv_basis_t [n_fft][ld_rc] = inverse basis transposed,
 * zero padded to ld_rc >= 2c (% 16 == 0); win_sq [n_fft] squared window or NULL; scratch rc [B*F][ld_rc], frames [B][F][n_fft];
 * out [B][hop * (F - 1)]. */
int t2s_stft_inverse(const float* mag, const float* phase, int B, int F, int n_fft, int hop, const float* inv_basis_t, long ld_rc,
                     const float* bias, float strength, const float* win_sq, float tiny, float* rc, float* frames, float* out,
                     void* stream);
/* ---- The three above on a padded batch whose entries differ in length, and int16 PCM (ABI v4, compatible additions) ----
 * Entry b of the batch holds lengths[b] samples (or frames[b] frames); every entry gets what it gets alone, whatever the padding
 * holds, and +0 behind its end.  Each entry point runs its partner's code with the lengths: it takes the partner's arguments and
 * checks plus the lengths twice: `lengths` /
 * `frames` ([B] int32 in device memory, read by the kernels; NULL: T2S_EINVAL) and `lengths_host` / `frames_host` (the same values
 * in host memory; NULL: T2S_EINVAL).  The host copy is read before the call returns and validated before the first launch (a value
 * out of range: T2S_EINVAL, nothing launched); the contractions are launched per entry with the entry's own item count from it,
 * because the GEMV / matrix-core dispatcher chooses by item count - that is what makes an entry's bits those of its solo call.  The
 * kernels clamp the device values to the validated range.  B <= 65535.
 *  t2s_stft_transform_ragged: audio [B][T], n_fft/2 < lengths[b] <= T; the layouts of t2s_stft_transform at F = T/hop + 1.  Entry b
 *    has F_b = lengths[b]/hop + 1 frames; the reflect padding mirrors about sample lengths[b] - 1 and audio[b][t >= lengths[b]] is
 *    never read.  For f < F_b mag, phase and magT hold, bit for bit, what t2s_stft_transform stores for the entry alone (B = 1,
 *    T = lengths[b], the same ldp and ld_mt); for f >= F_b they are stored as +0.  The scratch xp and ft behind an entry's end are
 *    not written.
 *  t2s_mel_from_mag_ragged: 1 <= frames[b] <= F; columns f < frames[b] are t2s_mel_from_mag's for the entry alone (the double-
 *    precision log-clamp included), columns behind are +0 - not log(clip): zero is what a collate function pads mels with - and
 *    the rows of magT behind are not read.  clip <= 0 skips the log, as in the partner; the zeros are stored all the same.
 *  t2s_stft_inverse_ragged: 2 <= frames[b] <= F; out [B][hop (F - 1)].  Samples n < hop (frames[b] - 1) are t2s_stft_inverse's for
 *    the entry alone: recombination, contraction, overlap-add bounds and window-sum-square all use frames[b], never F.  Samples
 *    behind are +0; mag and phase at f >= frames[b] are never read; the scratch rc and frames_buf ([B][F][n_fft]) are not written
 *    there.
 *  t2s_pcm16: x [B] rows of N samples, ldx elements apart (ldx >= N), f32 (is_half = 0) or fp16 (is_half != 0);
 *    out int16 [B][N] = (int16) trunc(float(x) * 32768.f), saturated to [-32768, 32767] (+1.0 gives 32767; the reference's numpy cast
 *    of an out-of-range float is undefined), NaN gives 0.  lengths ([B] int32, device) may be NULL: every sample; otherwise samples
 *    at or behind lengths[b] give 0 and are not read (any value of lengths[b] is safe: below 0 counts as 0, above N as N).  No
 *    alignment beyond the element: odd N and odd ldx work. */
int t2s_stft_transform_ragged(const float* audio, int B, int T, const int* lengths, const int* lengths_host, const float* fwd_basis,
                              int n_fft, int hop, float* xp, long ldp, float* ft, float* mag, float* phase, float* magT, long ld_mt,
                              void* stream);
int t2s_mel_from_mag_ragged(const float* magT, long ld_mt, int B, int F, const int* frames, const int* frames_host,
                            const float* mel_basis_p, int n_mel, float clip, float* mel, void* stream);
int t2s_stft_inverse_ragged(const float* mag, const float* phase, int B, int F, const int* frames, const int* frames_host, int n_fft,
                            int hop, const float* inv_basis_t, long ld_rc, const float* bias, float strength, const float* win_sq,
                            float tiny, float* rc, float* frames_buf, float* out, void* stream);
int t2s_pcm16(const void* x, int is_half, int B, int N, long ldx, const int* lengths, short* out, void* stream);

/* ---- training batches from a pool of int16 clips in device memory (additive to ABI version 4; text2speech_amd/data.py) ----------------
 *  t2s_pcm16_gather: t2s_pcm16's inverse, with each row's samples taken from anywhere in a pool.  pool: int16 [pool_len] (any 2-byte
 *    alignment); table: int64 [B][2] in device memory, (start, count) per row in samples of pool; out: f32 [B] rows of N, ldo floats
 *    apart (ldo >= N; rows need 4-byte alignment only, 16-byte aligned rows get 16-byte stores).  For row b let c = count clamped to
 *    [0, N] and then so that [start, start + c) lies inside [0, pool_len); a start outside the pool gives c = 0.  Then
 *    out[b][t] = (float)pool[start + t] / max_wav_value for t < c (an IEEE division: with 32768 it is exact, the bits of
 *    tensor.float() / 32768) and +0 for c <= t < N; columns N .. ldo are not written.  Any table value is safe and no sample outside
 *    [0, pool_len) is read (inside the pool, samples next to a row's own may be).  T2S_EINVAL, with nothing launched: a NULL pool,
 *    table or out, pool_len <= 0, B <= 0, B > 65535, N <= 0, ldo < N, max_wav_value not finite or not > 0.
 *  t2s_gate_targets: the stop-token targets of a collated Tacotron batch, gate [B][T] f32 = (t >= frames[b] - 1) ? 1 : 0 (the
 *    reference's gate_padded[i, mel.size(1) - 1:] = 1, utils/data_utils.py:146).  frames: int32 [B] on the device; frames[b] <= 0
 *    makes the whole row 1, frames[b] > T the whole row 0.  T2S_EINVAL: NULL pointers, B <= 0, B > 65535, T <= 0. */
int t2s_pcm16_gather(const short* pool, long pool_len, const long* table, int B, int N, float max_wav_value, float* out, long ldo,
                     void* stream);
int t2s_gate_targets(const int* frames, int B, int T, float* gate, void* stream);

/* ---- sample-rate conversion by up / down in device memory (additive to ABI version 4; audio.py Resampler, data.py PcmPool.resample) ----
 * The polyphase FIR of scipy.signal.resample_poly(x, up, down) with zero extension.  h: the filter, double [n_taps] in device memory
 * (8-byte aligned), n_taps = 2 half + 1, built by the caller (audio.resample_filter restates scipy's default Kaiser design).  A row of
 * n_in samples gives n_out = ceil(n_in up / down) samples
 *     y[m] = sum_k x[k] h[half + m down - k up]        over 0 <= k < n_in with 0 <= half + m down - k up < n_taps,
 * each one loop of its own in double precision: k ascending, one fused multiply-add per tap from +0.  The loop depends on m, n_in and
 * the filter only, so a row's bits are the same alone and in any batch or pool.  An int16 destination stores rint(y) (ties to even)
 * saturated to [-32768, 32767], NaN as 0; an f32 destination the one rounding of the double sum; an f16 source is widened exactly.
 * One kernel serves both entry points and every type pair; a workgroup makes t2s_resample_tile() consecutive outputs of one row.
 *  t2s_resample_tile: host only, that number (1024).
 *  t2s_resample_table: src [src_len] of src_kind (0 int16, 1 f32, 2 f16); dst [dst_len] of dst_kind (0 int16, 1 f32); table: int64
 *    [n_rows][4] in device memory, (src_start, src_count, dst_start, dst_cap) per row, in samples.  Row r's input is its own
 *    src_count samples from src_start - nothing next to them enters its sums.  It gets v = min(ceil(src_count up / down), dst_cap)
 *    samples of y at dst_start and +0 behind them up to dst_cap.  Any table value is safe: a negative src_count or a src_start
 *    outside [0, src_len) counts as no samples (the row is all +0), a src_count that runs past src_len is cut there; dst_cap is cut
 *    to max_out and to what dst holds behind dst_start, and a negative one or a dst_start outside [0, dst_len) writes nothing.
 *    Nothing outside [0, src_len) is read and nothing outside a row's [dst_start, dst_start + dst_cap) is written; rows whose
 *    destination ranges overlap are the caller's error.  max_out bounds the grid: ceil(max_out / tile) x n_rows workgroups.
 *    out_lengths: NULL, or int32 [n_rows] in device memory that receives every row's v.  No alignment beyond the element.
 *  t2s_resample_batch: the padded-batch form.  x [B] rows of N samples, ldx elements apart, f32 (is_half = 0) or f16; out f32 [B]
 *    rows of N_out, ldo apart: table rows (b ldx, lengths[b], b ldo, N_out).  lengths: int32 [B] in device memory, clamped to
 *    [0, N]; NULL: every row holds N.  Samples at or behind lengths[b] are never read.
 *  T2S_EINVAL, with nothing launched: a NULL src / x, table, h or dst / out; src_len, dst_len, n_rows, B, N, N_out or max_out <= 0;
 *    n_rows or B > 65535; max_out > 2^40; up or down < 1, gcd(up, down) != 1, max(up, down) > 512; n_taps even or < 3, or so long that
 *    its phase table, up (ceil(n_taps / up) | 1) doubles, exceeds 96 KB of LDS (half_width 10 needs 84 KB at most); ldx < N or
 *    ldo < N_out; a kind out of range; h not 8-byte aligned. */
int t2s_resample_tile(void);
int t2s_resample_table(const void* src, int src_kind, long src_len, const long* table, int n_rows, const double* h, int n_taps, int up,
                       int down, void* dst, int dst_kind, long dst_len, long max_out, int* out_lengths, void* stream);
int t2s_resample_batch(const void* x, int is_half, int B, int N, long ldx, const int* lengths, const double* h, int n_taps, int up,
                       int down, float* out, int N_out, long ldo, int* out_lengths, void* stream);

/* ---- peak rescaling and silence trimming in device memory (additive to ABI version 4; audio.py Trimmer, data.py PcmPool.rescale_trim) ----
 * librosa.effects.trim's decision and the reference's `wav / abs(wav).max() * rescaling_max` (datasets/kss.py:68-74).  For a row of n
 * samples x, frame length fl, hop h, pad = fl / 2 samples of padding at both ends (pad_mode 0: reflected about the first and the last
 * sample, needs n > pad; pad_mode 1: zeros): n_frames = 1 + (n + 2 pad - fl) / h, E_f = the sum of the squares of padded samples
 * f h .. f h + fl - 1, peak = max |x| (a non-finite sample counts as +inf), peak_eff = max(peak, peak_floor), and the view gain g =
 * rescaling_max / peak_eff with rescaling and peak_eff > 0, else 1 / 32768 for an int16 source and 1 for floats.  Frame f is loud iff
 *     max(E_f, F) > rho max(E_max, F)        rho = 10^(-top_db / 10), F = 1e-10 fl / g^2, E_max = max_f E_f,
 * evaluated in double - librosa's 10 log10(max(1e-10, g^2 E_f / fl)) - 10 log10(max(1e-10, g^2 E_max / fl)) > -top_db without the
 * logarithms.  start = h (the first loud frame), end = min(n, h (the last loud frame + 1)); no loud frame, a non-finite sample in the
 * row, a pad_mode 0 row with n <= pad or a row of zeros (E_max = 0: no frame counts as loud, where librosa's floor would keep the row
 * whole) give (0, 0).  Every E_f is one double-precision sum in an order that depends on fl alone
 * (an int16 row's is the exact integer), so a row's energies, bounds and samples are the same bits alone and in any batch or pool.
 * Tables are int64 in device memory and any value in them is safe: a negative src_count or a src_start outside [0, src_len) counts
 * as no samples, a src_count that runs past src_len is cut there; nothing outside [0, src_len) is read.  src_kind 0 int16, 1 f32,
 * 2 f16; no alignment beyond the element (tables, energy, stats and bounds: 8 bytes).
 *  t2s_trim_tile: host only, the frames one workgroup of the energy pass makes (64).
 *  t2s_trim_energy: table [n_rows][3] = (src_start, src_count, energy_start).  Writes row r's E_f to energy[energy_start + f] - as many
 *    frames as max_frames and the scratch behind energy_start allow (an energy_start outside [0, energy_len): none) - and
 *    stats[r] = (peak, E_max), which the call zeroes first; a pad_mode 0 row with 0 < n <= pad gets no frames and E_max = -1.
 *    energy = NULL: the peaks only.  max_frames bounds the grid: ceil(max_frames / tile) x n_rows workgroups.
 *  t2s_trim_bounds: from the same table, energies and stats, bounds[r] = (start, end), int64.  rescale 0 / 1: whether g carries the
 *    peak (rescaling_max is ignored without).
 *  t2s_trim_gather: table [n_rows][4] = (src_start, src_count, dst_start, dst_cap), as t2s_resample_table's.  bounds (or NULL: the
 *    whole row) narrows row r's source to [src_start + start, src_start + end), cut to the row; stats (or NULL: no rescaling) makes
 *    every sample x -> x s with s = rescaling_max / peak_eff formed in double (int16: s = rescaling_max 32768 / peak_eff), where
 *    peak_eff > 0.  int16 -> int16 stores rint((double)x s), ties to even, saturated; f32 / f16 -> f32 stores (float)((double)x s);
 *    without rescaling samples are copied bit for bit (f16 widened exactly).  dst_kind must be 0 for an int16 source and 1 for a
 *    float one.  The row gets v = min(kept, dst_cap) samples at dst_start and +0 behind them up to dst_cap; dst_cap is cut to max_out
 *    and to what dst holds; out_lengths: NULL or int32 [n_rows] that receives v.  src and dst must not overlap.
 *  T2S_EINVAL, with nothing launched: a NULL src, table, stats (energy, bounds pass), energy (bounds pass), bounds (bounds pass) or
 *    dst; src_len, dst_len, n_rows, energy_len, max_frames or max_out <= 0; n_rows > 65535; max_frames or max_out > 2^40;
 *    frame_length outside [2, 8192]; hop outside [1, frame_length]; pad_mode not 0 or 1; a kind out of range or a pair other than
 *    the three above; top_db, rescaling_max or peak_floor negative or not finite; rescaling (rescale = 1, or stats given) with
 *    rescaling_max = 0; a misaligned table, energy, stats or bounds; overlapping src and dst. */
int t2s_trim_tile(void);
int t2s_trim_energy(const void* src, int src_kind, long src_len, const long* table, int n_rows, int frame_length, int hop, int pad_mode,
                    long max_frames, double* energy, long energy_len, double* stats, void* stream);
int t2s_trim_bounds(const long* table, int n_rows, int src_kind, long src_len, int frame_length, int hop, int pad_mode, long max_frames,
                    const double* energy, long energy_len, const double* stats, double top_db, int rescale, double rescaling_max,
                    double peak_floor, long* bounds, void* stream);
int t2s_trim_gather(const void* src, int src_kind, long src_len, const long* table, int n_rows, const long* bounds, const double* stats,
                    double rescaling_max, double peak_floor, void* dst, int dst_kind, long dst_len, long max_out, int* out_lengths,
                    void* stream);

/* ---- programme loudness in device memory (additive to ABI version 4; audio.py Loudness, data.py PcmPool.loudness /
 *      normalize_loudness, longform.py normalize_long) ----
 * ITU-R BS.1770-4 / EBU R128 gated loudness of a mono row, and the gain that brings it to a target.  For a row of n samples x at
 * the integer rate fs (an int16 row counts as x / 32768, an f16 row is widened exactly; the filter starts from zero state at the
 * row's first sample, and only the row's own samples enter):
 *  - K-weighting: y = the shelf biquad, then the high-pass biquad, applied to x in double (transposed direct form II).  The caller
 *    forms the coefficients in double; audio.py loudness_coefficients states the formulas.
 *  - Hops: h = floor(fs / 10 + 1 / 2) samples; z_k = the sum of y^2 over samples k h .. (k + 1) h - 1, for k < n / h (an incomplete
 *    trailing hop is dropped).  Blocks: ms_j = (((z_j + z_(j+1)) + z_(j+2)) + z_(j+3)) / (4 h), j < J = max(0, n / h - 3).
 *  - Gates, linear, in double: A = { j : ms_j > gate_abs }, R = { j in A : ms_j > 0.1 mean(A) }, ms = mean(R),
 *    lufs = -0.691 + 10 log10(ms).  (gate_abs = 10^((-70 + 0.691) / 10) is the standard's.)
 *  - Gain: g = sqrt(target_T / ms), target_T = 10^((target_lufs + 0.691) / 10) formed by the caller; peak = max |x| (in the units
 *    above; a non-finite sample counts as +inf); with peak_limit > 0 and peak g > peak_limit: g = peak_limit / peak.
 *  - flags: 1 J = 0 (the row is shorter than 0.4 s); 2 A is empty (J > 0, every sample finite); 4 the peak limit set the gain;
 *    8 a non-finite sample lies inside the row (|A| and |R| then count as 0).  Any of 1, 2, 8 gives g = 1, ms = 0, lufs = -inf
 *    (NaN with 8).
 * The filter runs in parallel along the row (csrc/loudness.hip): segments of t2s_loud_segment() samples, 256 to a tile, every
 * one counted from the row's first sample, and every sum in one order that depends on n and h alone; no atomics.  A row's
 * statistics and samples are therefore the same bits alone and at any place of any batch or pool, at any alignment, whatever lies
 * behind its length.  Tables are int64 in device memory and any value in them is safe, as t2s_trim_gather's: a negative src_count
 * or a src_start outside [0, src_len) counts as no samples, a src_count that runs past src_len is cut there; nothing outside
 * [0, src_len) is read.  src_kind 0 int16, 1 f32, 2 f16; no alignment beyond the element (tables, coef, scratch, stats: 8 bytes).
 *  t2s_loud_tile / t2s_loud_segment: host only, the samples of one workgroup's tile (8192) and of one lane's segment (32).
 *  t2s_loud_scratch: host only, the doubles of scratch t2s_loud_measure needs for n_rows rows of at most max_count samples
 *    (-1 for arguments t2s_loud_measure would refuse).
 *  t2s_loud_measure: table [n_rows][2] = (src_start, src_count); a row longer than max_count is cut there.  fs_hop is h.
 *    coef: 160 doubles in device memory - [0, 5) b0 b1 b2 a1 a2 of the shelf, [5, 10) of the high-pass, [10, 16) unused,
 *    [16 + 16 k, 32 + 16 k) for k = 0 .. 7 the 4 x 4 row-major matrix P_S^(2^k), [144, 160) P_tile = P_S^256, where P_S = M^S and M
 *    is the zero-input map of one sample on the state (s1, s2 of the shelf, s1, s2 of the high-pass).  stats: double [n_rows][4] =
 *    (ms, lufs, peak, g); counts: int32 [n_rows][4] = (J, |A|, |R|, flags).  Four launches on the stream; nothing waits across
 *    workgroups.  peak_limit <= 0: none.
 *  t2s_loud_apply: table [n_rows][4] = (src_start, src_count, dst_start, dst_cap), as t2s_trim_gather's; g is stats[r][3].
 *    int16 -> int16 stores rint((double)x g), ties to even, saturated; f32 / f16 -> f32 stores (float)((double)x g); g = 1 copies
 *    bit for bit (f16 widened exactly).  The row gets min(n, dst_cap) samples at dst_start and +0 behind them up to dst_cap; dst_cap
 *    is cut to max_out and to what dst holds; out_lengths: NULL or int32 [n_rows] that receives the count.
 *  T2S_EINVAL, with nothing launched: a NULL src, table, coef, scratch, stats, counts or dst; src_len, dst_len, n_rows, max_count or
 *    max_out <= 0; n_rows > 65535; max_count > 2^31 - 1; max_out > 2^40; fs_hop outside [400, 38400] or below the segment; a kind
 *    out of range or a pair other than int16 -> int16, f32 -> f32, f16 -> f32; gate_abs negative or not finite; target_T not
 *    finite or <= 0; peak_limit NaN; a misaligned table, coef, scratch, stats or counts; scratch_len below t2s_loud_scratch's;
 *    overlapping src and dst. */
int t2s_loud_tile(void);
int t2s_loud_segment(void);
long t2s_loud_scratch(int n_rows, long max_count);
int t2s_loud_measure(const void* src, int src_kind, long src_len, const long* table, int n_rows, long max_count, int fs_hop,
                     const double* coef, double* scratch, long scratch_len, double gate_abs, double target_T, double peak_limit,
                     double* stats, int* counts, void* stream);
int t2s_loud_apply(const void* src, int src_kind, long src_len, const long* table, int n_rows, const double* stats, void* dst,
                   int dst_kind, long dst_len, long max_out, int* out_lengths, void* stream);

/* ---- true-peak metering and a look-ahead limiter in device memory (additive to ABI version 4; audio.py Limiter, data.py
 *      PcmPool.true_peak / limit, longform.py limit_long) ----
 * The last stage of a delivery chain: no output sample above a ceiling, the gain taken down smoothly around each peak only.  For a
 * mono row of n samples x and a row gain g (gains[r], or 1 without gains; an int16 row counts as x / 32768, an f16 row is widened
 * exactly), all in double: u[i] = (double)x[i] g inside the row and 0 outside it (zero extension, as t2s_resample_table's).
 *  1. Envelope.  os is 1, 2 or 4; h is the caller's interpolation filter of n_taps = 2 half_width os + 1 taps, half = half_width os
 *     (audio.py resample_filter(1, os, half_width, beta): scipy.signal.resample_poly(x, os, 1)'s own filter - the project's filter,
 *     not the 48-tap table printed in BS.1770 Annex 2, which is one admissible interpolator among others).
 *     y[m] = sum_j u[j] h[m - os j + half] over the j whose tap index lies in [0, n_taps), in ascending j, one fused multiply-add a
 *     tap; p[i] = max(|u[i]|, max_(q < os) |y[os i + q]|).  With os = 1: p[i] = |u[i]| and h is not read.
 *  2. Required gain.  r[i] = c / p[i] where p[i] > c, else 1; r = 1 outside the row.  c is the ceiling, a float32 value.
 *  3. Look-ahead.  m[i] = min over |k| <= L of r[i + k], for every i (outside the row too).  0 <= L <= t2s_limit_max_lookahead().
 *  4. Smoothing.  s[i] = min(r[i], sum_(k = -L .. L) w[k] m[i + k]), in ascending k, one fused multiply-add a tap.  w is the
 *     caller's window of 2 L + 1 doubles, w[k] = 1/2 + 1/2 cos(pi k / (L + 1)) normalised; its sum in ascending order must not come
 *     out below 1 (audio.py limiter_window sees to that), so that s is exactly 1 wherever every m in reach is 1: the kernels skip
 *     the sum for a tile with no r below 1 in reach, and for a row with none at all.
 *  5. Output.  o[i] = u[i] s[i].  f32 / f16 -> f32 stores (float)o[i]; int16 -> int16 stores rint(32768 o[i]), ties to even,
 *     saturated.  The row gets min(n, dst_cap) samples at dst_start and +0 behind them up to dst_cap (cut to max_out and to what dst
 *     holds), as t2s_loud_apply's.  With g = 1 a row with nothing over the ceiling is copied bit for bit.
 *  6. stats: double [n_rows][4] = (true_peak = max p, sample_peak = max |u|, s_min = min s, 0); counts: int32 [n_rows][2] =
 *     (the number of i with p[i] > c, flags).  flags: 1 the row was limited (the count is not 0); 8 a u inside the row is not
 *     finite: then both peaks are +inf, s_min 1, the count 0, and t2s_limit_apply copies the row WITHOUT its gain.
 * Guaranteed: |stored sample| <= c, exactly (s <= r <= c / |u| up to one rounding in double, and rounding to float32 is monotone
 * and c is a float32; int16: |code| <= rint(32768 c)).  NOT guaranteed: the true peak of the output - a gain that moves changes
 * the values between the samples; profiles/limiter_tests.md records what it came to.  o[i] depends on x over
 * [i - R, i + R] only, R = 2 L + half_width.  Every sum has one order that depends on the row alone, min and max are order-free and
 * tiles are counted from the row's first sample: a row's statistics and samples are the same bits alone and at any place of any
 * batch or pool, at any alignment, whatever lies behind its length.  Tables are int64 in device memory and any value in them is
 * safe, as t2s_loud_apply's; nothing outside [0, src_len) is read and stores land only inside [dst_start, dst_start + dst_cap).
 *  t2s_limit_tile / t2s_limit_max_lookahead / t2s_limit_max_half_width: host only; the outputs of one workgroup (1024), the largest L
 *    (1024) and the largest half_width (32).
 *  t2s_limit_scratch: host only, the doubles of scratch t2s_limit_measure needs (four per tile; -1 for arguments it would refuse).
 *  t2s_limit_measure: table [n_rows][2] = (src_start, src_count); a row longer than max_count is cut there.  Two launches.
 *  t2s_limit_apply: table [n_rows][4] = (src_start, src_count, dst_start, dst_cap); counts are the measure call's; the envelope is
 *    computed again, not stored in between.  out_lengths: NULL or int32 [n_rows] that receives the count.  One launch.
 *  T2S_EINVAL, with nothing launched: a NULL src, table, h, w, scratch, stats, counts or dst; src_len, dst_len, n_rows, max_count or
 *    max_out <= 0; n_rows > 65535; max_count > 2^31 - 1; max_out > 2^40; os not 1, 2 or 4; half_width outside [1, max];
 *    n_taps != 2 half_width os + 1; L outside [0, max]; c not finite, <= 0 or not a float32 value; a kind out of range or a pair
 *    other than int16 -> int16, f32 -> f32, f16 -> f32; a misaligned table, gains, h, w, scratch, stats (8 bytes) or counts (4);
 *    scratch_len below t2s_limit_scratch's; overlapping src and dst. */
int t2s_limit_tile(void);
int t2s_limit_max_lookahead(void);
int t2s_limit_max_half_width(void);
long t2s_limit_scratch(int n_rows, long max_count);
int t2s_limit_measure(const void* src, int src_kind, long src_len, const long* table, int n_rows, long max_count, const double* gains,
                      const double* h, int n_taps, int os, int half_width, const double* w, int lookahead, double ceiling,
                      double* scratch, long scratch_len, double* stats, int* counts, void* stream);
int t2s_limit_apply(const void* src, int src_kind, long src_len, const long* table, int n_rows, const double* gains, const double* h,
                    int n_taps, int os, int half_width, const double* w, int lookahead, double ceiling, const int* counts, void* dst,
                    int dst_kind, long dst_len, long max_out, int* out_lengths, void* stream);

/* ---- delivery inside a stream: the resampler and the limiter window by window, G.711 (additive to ABI version 4; audio.py
 *      DeliveryStream, to_ulaw / to_alaw; streaming.py synthesize_stream(delivery=); csrc/delivery.hip) ----
 * A stream hands over the row of an utterance piece by piece.  Both stages are local, so a stream keeps the last C samples of what
 * it has seen - the carry, f32 [B][C], packed - and each output is the whole-row entry point's own loop over carry | piece: the
 * windows of a stream, concatenated, are t2s_resample_batch's / t2s_limit_apply's row bit for bit, for any piece lengths.  All
 * positions are global sample indices of the stream's row, host scalars; the host knows every piece length and nothing is read
 * back.  Rows: carry_in / carry_out [B][C]; piece f32 (is_half = 0) or f16 [B] rows of n samples, ldp elements apart, at global
 * position K0 (N0); out f32 [B] rows, ldo apart.  carry_in holds the samples K0 - C .. K0 - 1 and is only read; carry_out (another
 * buffer: ping-pong) receives the last C samples of carry | piece, an f16 sample widened exactly; a piece shorter than C shifts the
 * old carry.  Samples below index 0 do not exist (they are never read: a new stream's carry may hold anything); with `final`,
 * samples at or beyond K0 + n do not exist either.  n = 0 is allowed (piece may then be NULL), and with `final` flushes what the
 * carry still owes.  One launch each; a workgroup makes 1024 outputs, one more per row writes the carry.
 *  t2s_resample_window_carry: host only.  C_r = ceil(n_taps / up); -1 for n_taps < 3 or up < 1.
 *  t2s_resample_window_end: host only.  The M1 of a window that ends at source sample K1 = K0 + n:
 *    not final  M1 = max(M0, ceil((K1 up - half) / down)), half = n_taps / 2 - every output whose last tap lies below K1;
 *    final      M1 = max(M0, ceil(K1 up / down)) - t2s_resample_table's n_out.           -1 for arguments the call would refuse.
 *  t2s_resample_window: writes y[m], M0 <= m < M1, to out[b][m - M0]: t2s_resample_table's sum - k ascending, one double fused
 *    multiply-add per tap from +0, rounded to f32 once - over the samples that exist.  M0 is the M1 of the window before (0 at
 *    first).
 *  t2s_limit_window_carry: host only.  C_l = 2 (2 lookahead + half_width) = 2 reach; -1 outside the limits.
 *  t2s_limit_window_end: host only.  not final: O1 = max(O0, N1 - reach); final: O1 = max(O0, N1), N1 = N0 + n.
 *  t2s_limit_window: writes o[i], O0 <= i < O1, to out[b][i - O0]: steps 1 - 5 of the limiter above over [O0 - reach, N1) - the same
 *    sums in the same order, the same sliding minimum and window sum, r = 1 outside the row; f32 / f16 -> f32.  gains: double [B] in
 *    device memory or NULL; h, n_taps, os, half_width, w, lookahead, ceiling as t2s_limit_apply's.  There is no measure pass and no
 *    counts: a window sum is skipped only for a tile with no r < 1 in reach, where s is exactly 1.
 *    state: 40 bytes a row, 8-byte aligned, kept by the caller from window to window and updated through integer atomics only:
 *    words 0 - 2 the bit patterns of the largest p, the largest |u| and the smallest s over the delivered i (non-negative doubles
 *    order as their bit patterns), word 3 zero, then int32 the number of delivered i with p[i] > c and int32 flags.  A new stream
 *    sets it to (0, 0, the bits of 1.0, 0, 0, 0).  After the final window, read as double [4] and int32 [2], it is
 *    t2s_limit_measure's stats and counts of the whole row.
 *    NOT FINITE: the whole-row call copies such a row; a stream has already delivered, so it mutes instead.  A u that is not
 *    finite, or an interpolated y that is not, counts as p = +inf: r = 0 there, the gain goes to 0 around it, o[i] = +0 where u[i]
 *    itself is not finite, every stored sample is finite, and flag 8 is raised (the recorded peaks are then +inf and s_min 0).
 *  t2s_g711: int16 codes [n] -> bytes [n], ITU-T G.711.  law 0, mu-law: v = x >> 2 (arithmetic, 14 bits); v < 0: v = -v and the
 *    sign mask is 0x7F, else 0xFF; v = min(v, 8159) + 33 (the 16-bit form's clip 32635 and bias 132, >> 2); seg = the first of the
 *    ends 0x3F, 0x7F, 0xFF .. 0x1FFF with v <= end; byte = ((seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask, and 0x7F ^ mask where no
 *    end holds v.  law 1, A-law: v = x >> 3 (13 bits); v >= 0: mask 0xD5, else v = -v - 1 and mask 0x55; seg = the first of the ends
 *    0x1F, 0x3F, 0x7F .. 0xFFF with v <= end; byte = ((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 15)) ^ mask.  No alignment beyond
 *    the element.
 *  T2S_EINVAL, with nothing launched and nothing written: a NULL carry_in, carry_out, h, w or state, a NULL piece with n > 0, a NULL
 *    out where the window has outputs; carry_in and carry_out overlapping; B <= 0 or > 65535; n < 0 or > 2^31 - 1; ldp < n; a
 *    position below 0 or above 2^40; O0 > N1; more outputs than out_cap or ldo; the filter, window and ceiling conditions of
 *    t2s_resample_table / t2s_limit_apply; a misaligned h, w, gains, state (8 bytes), carry or out (4), piece (its element);
 *    t2s_g711: a NULL pcm or out, n <= 0 or > 2^40, law other than 0 or 1. */
int t2s_resample_window_carry(int n_taps, int up);
long t2s_resample_window_end(long K1, long M0, int n_taps, int up, int down, int final);
int t2s_resample_window(const float* carry_in, float* carry_out, const void* piece, int is_half, int B, long n, long ldp, long K0,
                        long M0, int final, const double* h, int n_taps, int up, int down, float* out, long out_cap, long ldo,
                        void* stream);
int t2s_limit_window_carry(int lookahead, int half_width);
long t2s_limit_window_end(long N1, long O0, int lookahead, int half_width, int final);
int t2s_limit_window(const float* carry_in, float* carry_out, const void* piece, int is_half, int B, long n, long ldp, long N0, long O0,
                     int final, const double* gains, const double* h, int n_taps, int os, int half_width, const double* w,
                     int lookahead, double ceiling, float* out, long out_cap, long ldo, void* state, void* stream);
int t2s_g711(const short* pcm, long n, int law, unsigned char* out, void* stream);

/* ---- joining the rows of padded batches into one utterance in device memory (additive to ABI version 4; audio.py join_batches,
 *      longform.py synthesize_long) ----
 * Sentence after sentence, a pause of zeros between them, a linear ramp at the joints; no length is read by the host.
 *  - n segments are numbered by position p = 0 .. n-1.
 *  - Segment p is row order[p] of the sources, or row p when order is NULL.
 *  - Its length len_p is read from the device.  It is clamped to [0, N] of its row, so any value is safe.
 *  - Its pause is g_p >= 0 samples, for p < n-1.  Pauses come from an int32 array by position, or one uniform gap.  g_{n-1} counts
 *    as 0.
 * With int64 arithmetic:
 *     off_0 = 0,   off_{p+1} = off_p + len_p + g_p,   total = off_{n-1} + len_{n-1}
 *     dst[off_p + i] = w_p(i) x_p[i]        0 <= i < len_p
 *     dst[j] = +0                           every other j in [0, dst_cap)
 * The fade is F >= 0 samples.
 *  - The ramp is r(k) = (float)((double)(2k + 1) / (double)(2F)) for 0 <= k < F.  It is one double division, rounded once.
 *  - The leading ramp applies to segment p when p > 0 or fade_ends is set.  The trailing ramp applies when p < n-1 or fade_ends is
 *    set.
 *  - y = x (f16 widened exactly).
 *  - If the leading ramp applies and i < F: y = y r(i), one f32 multiply.
 *  - Then, if the trailing ramp applies and len_p - 1 - i < F: y = y r(len_p - 1 - i).
 *  - A segment shorter than 2F gets both factors, in that order.
 *  - F = 0 copies bit for bit.
 * Because of this, a segment's samples in the output depend on its own samples, F, and whether it is first or last.  They do not
 * depend on the batch it came from or on its row.  Elements at or beyond dst_cap are never written.  offsets[0 .. n] is reported
 * unclipped, with offsets[n] = total.  length = min(total, dst_cap) is reported as int32.
 *  t2s_join_tile: host only, the samples of one row that one workgroup of the gather handles (2048).
 *  t2s_join_offsets: the scan.  lengths, row_caps (the N of each row's batch): int32 [n] in device memory, by row; order: int32 [n],
 *    position -> row, or NULL (an entry outside [0, n) counts as an empty segment); gaps: int32 [n - 1] by position (a negative one
 *    counts as 0), or NULL: `gap` everywhere.  Writes offsets (int64 [n + 1], 8-byte aligned) and length (int32 [1]) from one
 *    workgroup in integer arithmetic, for any n up to 65535.  It also stores +0 to all of dst[0 : dst_cap), on the same stream and
 *    before the scan: the pauses and the tail are this call's business, so after it and the gathers every element of
 *    dst[0 : dst_cap) is defined, whatever it held before.
 *  t2s_join_gather: one source batch.  src: B rows of N samples, ldx elements apart (ldx >= N), src_kind 1 f32 or 2 f16 (as
 *    t2s_trim_gather's); lengths: int32 [B] of these rows; pos: int32 [B], pos[b] the position of row b - a negative or >= n value
 *    means the row is not part of the join and writes nothing; offsets: the scan's.  Row b's len samples (lengths[b] clamped to
 *    [0, N]) go to dst[offsets[pos[b]] + i] with the ramps above, where that index lies in [0, dst_cap); nothing else is written
 *    and samples at or behind a row's length are never read.  The grid is ceil(N / tile) x B workgroups.  Several batches are
 *    several calls with the same offsets, n, fade and dst; their order does not matter.
 *  T2S_EINVAL, with nothing launched: a NULL required pointer (all but order, gaps and stream); n, B, N or dst_cap <= 0; n or
 *    B > 65535; dst_cap > 2^31 - 1; fade < 0 or > 65536; gap < 0; a src_kind other than 1 or 2; ldx < N; src overlapping dst; offsets
 *    not 8-byte aligned.  No alignment is required beyond the element otherwise. */
int t2s_join_tile(void);
int t2s_join_offsets(const int* lengths, const int* row_caps, const int* order, const int* gaps, int gap, int n, float* dst,
                     long dst_cap, long* offsets, int* length, void* stream);
int t2s_join_gather(const void* src, int src_kind, int B, int N, long ldx, const int* lengths, const int* pos, const long* offsets,
                    int n, int fade, int fade_ends, float* dst, long dst_cap, void* stream);

/* ---- keyed sampling: random draws that are a function of (the entry's seed, the element's index) only (additive to ABI version 4;
 *      tacotron.py inference_batch(seeds=), glow.py infer(seed=) / infer_batch(seeds=) / draw_noise) ----
 * An entry of a batch draws the same bits alone and in any batch: nothing depends on B, on the entry's place, on the padded length
 * or on a generator's state.  seeds: unsigned 64-bit [B] in device memory, one per entry.  All arithmetic below is wrapping uint64;
 *     mix(x):  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31      (splitmix64's finaliser)
 *     GOLD = 0x9E3779B97F4A7C15.
 *  t2s_bernoulli_mask_keyed: mask unsigned char [n_steps][B][row].  mask[t][b][j] = (mix((t row + j) GOLD + seeds[b]) >> 40) <
 *    (unsigned)(keep_prob 2^24) - exactly what t2s_bernoulli_mask(buf, n_steps row, seeds[b], 0, keep_prob) stores at index
 *    t row + j.  B = 1 with seed s is therefore that call bit for bit, and entry b of any batch is its solo mask.
 *    T2S_EINVAL, with nothing launched: a NULL pointer; n_steps, B or row <= 0; B > 65535; n_steps row > (2^31 - 1) 256; keep_prob outside
 *    (0, 1].
 *  t2s_wg_noise_keyed: z float [B][G][L], contiguous (the buffer WaveGlow's inverse flow starts from, glow.py:260-267,284-289).
 *    key_b = mix(seeds[b] GOLD + 0x5741564547)  (the constant keeps this domain apart from the mask hash: one user seed feeds both).
 *    For channel c and column t:  p = (c << 40) | (t >> 1),  a = mix((2 p) GOLD + key_b),  h = mix((2 p + 1) GOLD + key_b),
 *        u1 = ((a >> 11) + 1) 2^-53  in (0, 1],   u2 = (h >> 11) 2^-53  in [0, 1),   r = sqrt(-2 ln u1),
 *        n = r cos(2 pi u2) for even t,  r sin(2 pi u2) for odd t        (evaluated in double precision, sincospi(2 u2)),
 *        z[b][c][t] = sigma_b * (float)n        (one f32 rounding of n, then one f32 multiply),
 *    sigma_b = sigmas[b] where sigmas (NULL, or float [B] in device memory) is given, else sigma.  |n| <= sqrt(106 ln 2) = 8.58: no
 *    inf, no NaN.  The value depends on (seeds[b], c, t) only.  sigmas' values are not read on the host and so not checked.
 *    T2S_EINVAL, with nothing launched: a NULL z or seeds; B, G or L <= 0; B or G > 65535; L >= 2^40; B G L > 2^60; a sigma that is
 *    not finite or < 0.  No alignment beyond the element.
 *  t2s_wg_noise_keyed_at: a window of those columns.  z float [B][G][L]; z[b][c][j] is exactly what t2s_wg_noise_keyed stores at
 *    column c0_b + j of a buffer long enough to hold it, c0_b = col0s[b] where col0s (NULL, or long long [B] in device memory) is
 *    given, else col0.  Any parity of c0_b and of L: the member of a Box-Muller pair that lies outside the window is not stored.
 *    col0s' values are not read on the host and so not checked; whatever they hold, only z[b][c][0 .. L) is written.
 *    T2S_EINVAL, with nothing launched: as t2s_wg_noise_keyed, and col0 < 0 or col0 + L >= 2^40.
 *  t2s_noise_tile: host only, the columns of one row that a workgroup of the noise kernel makes (1024). */
int t2s_bernoulli_mask_keyed(unsigned char* mask, int n_steps, int B, int row, const unsigned long long* seeds, float keep_prob,
                             void* stream);
int t2s_noise_tile(void);
int t2s_wg_noise_keyed(float* z, int B, int G, long L, const unsigned long long* seeds, float sigma, const float* sigmas, void* stream);
int t2s_wg_noise_keyed_at(float* z, int B, int G, long L, long col0, const long long* col0s, const unsigned long long* seeds, float sigma,
                          const float* sigmas, void* stream);

/* ---- the alignment check: where every decoder frame attends, and whether that path is the text (additive to ABI version 4;
 *      alignment.py alignment_report, longform.py synthesize_long(check=); csrc/align.hip) ----
 * Inputs
 *  - A: B entries of N rows of T_in columns.
 *     - Row stride is ld_row >= T_in.
 *     - Entry stride is ld_entry >= N * ld_row.
 *     - src_kind is 1 for f32 or 2 for f16, as in t2s_join_gather.
 *  - in_len, out_len: int32 [B] in device memory.
 *     - out_len may be NULL, which means N.  in_len may be NULL, which means T_in.
 *  - Clamped values: S_b = clamp(in_len[b], 1, T_in) and F_b = clamp(out_len[b], 0, N).
 * Row pass (t2s_align_rows).  For every b and t < F_b:
 *  - pos[b,t] is the smallest j in [0, S_b) at which A[b,t,j] is largest.
 *     - The scan starts at best = -inf, j = 0 and updates on v > best.  A NaN is therefore never chosen, and a row of NaN gives
 *       pos = 0 with peak -inf.
 *  - peak[b,t] is that value, widened to f32 exactly.
 *  - bad[b,t] = 1 if any of the S_b values is not finite, otherwise 0.
 * For t >= F_b: pos = -1, peak = 0, bad = 0.  The row is not loaded, so the ragged tail costs nothing.
 * Outputs: pos int32 [B, N], peak f32 [B, N], bad uint8 [B, N].
 * One wave per row, lanes striding the columns, four rows per workgroup; the grid covers the B N rows.
 * Entry pass (t2s_align_stats).  One workgroup per entry, walking t in blocks of 256 frames with a carry.  Outputs:
 * stats, int32 [B, 8]:
 *   0 frames         F_b
 *   1 symbols        S_b
 *   2 max_skip       max(pos_t - pos_{t-1}) over 1 <= t < F_b, not below 0.  0 if F_b < 2.
 *   3 max_back       max(pos_{t-1} - pos_t), same convention
 *   4 longest_stall  longest run of consecutive frames with equal pos.  0 if F_b = 0.
 *   5 last_pos       pos_{F_b - 1}.  -1 if F_b = 0.
 *   6 covered        number of j < S_b with dur[b,j] > 0
 *   7 bad_rows       sum of bad
 * focus, f64 [B]:
 *  - The mean of peak over the entry's frames.  It is summed in double, in an order fixed by F_b alone (thread i of 256 adds frames
 *    i, i + 256, ... in that order, then a fixed tree joins the 256 sums).  An entry's bits are then the same alone, in any batch
 *    and at any place.
 *  - 0 if F_b = 0.
 *  - If a peak is not finite, the result is whatever IEEE gives.  bad_rows reports it.
 * dur, int32 [B, T_in]:
 *  - The number of frames with pos = j.
 *  - 0 for j >= S_b.
 * flags, int32 [B].  The thresholds reach the kernel in a by-value struct:
 *     1 TRUNCATED   max_frames > 0 && F_b >= max_frames
 *     2 SKIP        max_skip > skip_max
 *     4 BACK        max_back > back_max
 *     8 STALL       longest_stall > stall_max
 *    16 UNFINISHED  last_pos < S_b - 1 - end_slack
 *    32 DIFFUSE     !(focus >= min_focus), so a NaN sets it
 *    64 NONFINITE   bad_rows > 0
 *   128 EMPTY       F_b == 0
 *  - A negative integer threshold switches its bit off.
 *  - min_focus <= 0 switches DIFFUSE off (a NaN min_focus as well).
 * t2s_align_stats reads the row pass's pos, peak and bad ([B, N], the first F_b of each entry) and the same two length arrays.  It
 * stores +0 to all of dur on the same stream before its kernel.  It trusts no pos it reads: a value outside [0, S_b) is counted in no
 * dur.
 * Memory safety: every length is clamped; nothing outside the stated outputs is written; nothing is read past S_b columns or F_b
 * rows.  T_in of any positive size works.  The one limit is B N <= 2^31 - 1 (rows are numbered in an int).
 * T2S_EINVAL, with nothing launched: a NULL A, pos, peak, bad, stats, focus, dur or flags; a pointer that is not aligned to its
 * element (A to 4 bytes for f32 and 2 for f16, the int32 and f32 arrays to 4, focus to 8; in_len and out_len where given); B, N or
 * T_in < 1; B N > 2^31 - 1; ld_row < T_in; ld_entry < N ld_row; a src_kind other than 1 or 2. */
int t2s_align_rows(const void* A, int src_kind, int B, int N, int T_in, long ld_row, long ld_entry, const int* in_len,
                   const int* out_len, int* pos, float* peak, unsigned char* bad, void* stream);
int t2s_align_stats(const int* pos, const float* peak, const unsigned char* bad, int B, int N, int T_in, const int* in_len,
                    const int* out_len, int max_frames, int skip_max, int back_max, int stall_max, int end_slack, double min_focus,
                    int* stats, double* focus, int* dur, int* flags, void* stream);

/* ---- speaking rate and symbol timestamps: a mel warped in time, and the spans of its symbols (additive to ABI version 4;
 *      rate.py warp_mel / symbol_spans, longform.py synthesize_long_timed(speed=, timestamps=); csrc/warp.hip) ----
 * Speed is changed between the two models: stretching the frame axis of the mel and letting the vocoder make more or fewer samples
 * keeps pitch and timbre.  The same cumulative map that drives the warp tells where every symbol went.  Everything discrete is an
 * exact integer, so it cannot differ between the device, a restatement, a solo run and a batch.
 * Stretch per frame
 *  - Q = 2^20.  Source frame f of entry b has a stretch s[b,f]: an int64 count of output frames in units of 1 / Q.
 *  - One rate r for all, or one per entry: s = rint(Q / r), formed on the host in double.  It reaches the map kernel by value
 *    (`stretch`) or as int64 [B] in device memory (`stretches`, each value clamped to [Q / 8, 8 Q] on the device).
 *  - Per-symbol rates: `rates` f32 [B, T_in] and `path` int32 [B, F] (t2s_align_rows' pos).
 *      s[b,f] = rint(Q / clamp((double)rates[b, path[b,f]], min_rate, max_rate)), formed on the device, ties to even.
 *    A frame is at rate 1 (s = Q) when its path value lies outside [0, S_b), S_b = clamp(in_len[b], 1, T_in), or when its table value
 *    is a NaN.  +-inf, 0 and negative values clamp.  min_rate <= max_rate are host doubles within [1 / 8, 8].
 * Cumulative map
 *  - F_b = clamp(lengths[b], 0, F).
 *  - c[b,0] = 0, c[b,f+1] = c[b,f] + s[b,f] for f < F_b: int64 [B, F + 1].  Entries behind F_b repeat c[b,F_b].
 * Output length
 *  - F'_b = 0 if F_b = 0, else clamp((c[b,F_b] + Q / 2) >> 20, 1, cap).
 * Output frame j < F'_b
 *  - p = (2j + 1) Q, and m[f] = c[f] + c[f+1] is the doubled centre of source frame f.  Let f be the largest index with m[f] <= p.
 *  - If there is none, out = x[0].  If f >= F_b - 1, out = x[F_b - 1].
 *  - Otherwise a = (double)(p - m[f]) / (double)(m[f+1] - m[f]).  If a == 0, out = x[f] bit for bit and x[f+1] is not read.  Else
 *    out = (T)((1 - a) (double)x[f] + a (double)x[f+1]): one double expression, rounded once to the mel's type T (f32 or f16).
 *  - The same f and a serve all C channels.  Columns F'_b .. cap - 1 of the output are +0.
 *  So rate 1 is the identity bit for bit (f = j, a = 0), any stretches give np.interp(j + 0.5, m / 2Q, x) with end clamping, and a
 *  uniform rate r reads the coordinate (j + 0.5) r - 0.5.
 * Symbol spans
 *  - For symbol k < S_b: first is the smallest and last the largest f < F_b with path[b,f] == k; t0 = c[first], t1 = c[last + 1].
 *  - In vocoder samples u = (t hop) >> 20.  With a monotone path neighbouring spans abut exactly.
 *  - Then, for both ends, each step where its argument is given: u = clamp(u - trim_start[b], 0, trim_len[b]); u += offsets[b];
 *    u = min((u up) / down, total), an integer floor division.
 *  - spans int64 [B, T_in, 2] holds (-1, -1) for a symbol no frame attends to, for a symbol at or behind S_b and for every symbol of
 *    an entry with F_b = 0.
 *  t2s_warp_block: host only, the frames of one step of the map's walk and the output frames of one tile of the gather (256).
 *  t2s_warp_map: one workgroup per entry walks the frames in blocks with a carried int64 sum, for any F.  lengths, in_len: int32 [B] in
 *    device memory or NULL (F, T_in).  path rows are ld_path >= F apart, rates rows ld_rates >= T_in apart; rates needs path, takes
 *    stretch = Q and no stretches.  Writes, each where its pointer is given (one at least): cum = c; out_len int32 [B] = F'_b;
 *    first_last int32 [B, T_in, 2] = (first, last), (-1, -1) for a symbol without a frame (needs path; the call sets it to -1 on the
 *    same stream before the kernel, whose integer minima and maxima are exact in any order).
 *  t2s_warp_gather: x is B entries of C rows of F frames, rows ld_row >= F and entries ld_entry >= C ld_row elements apart (a view of a
 *    wider mel goes in as it is), src_kind 1 f32 or 2 f16; cum and out_len are the map's.  Writes all of out [B, C, cap], dense and of
 *    x's type.  The grid runs over tiles of output frames x entries x groups of 16 channels; a column finds its f once, by bisection
 *    in the entry's row of c, and stores are coalesced along time.
 *  t2s_warp_spans: one thread per (entry, symbol).  trim_start and trim_end (both or neither: a Trimmer's cut points, trim_len =
 *    trim_end - trim_start), offsets, total_dev (int64 [1], in the place of `total`): int64 in device memory or NULL; no step is
 *    skipped by a value, up = down = 1 and total = 2^62 leave u as it is.
 * Memory safety: every length is clamped; a path value is used only inside [0, S_b); the gather's f lies in [0, F_b) whatever cum
 * holds, samples at or behind F_b are never read and a store goes only inside [0, cap); first / last are used only inside [0, F_b).
 * T2S_EINVAL, with nothing launched: a NULL x, cum (gather, spans), out_len (gather), out, first_last (spans) or spans; no output at
 *    all (map); rates or first_last without path, rates with stretches or with stretch != Q; a pointer that is not aligned to its
 *    element (int64 arrays to 8); B < 1 or > 65535; F < 1 or > 2^30; cap < 1; C < 1; T_in < 1 where a path or spans are asked for;
 *    B T_in > 2^31 - 1; ld_path < F, ld_rates < T_in, ld_row < F, ld_entry < C ld_row; a src_kind other than 1 or 2; x overlapping
 *    out; a stretch outside [Q / 8, 8 Q]; min_rate or max_rate outside [1 / 8, 8] or min_rate > max_rate; hop, up or down outside
 *    [1, 2^20]; F hop > 2^39; total < 0; one of trim_start and trim_end without the other. */
int t2s_warp_block(void);
int t2s_warp_map(const int* lengths, int B, int F, long stretch, const long* stretches, const int* path, long ld_path,
                 const float* rates, long ld_rates, const int* in_len, int T_in, double min_rate, double max_rate, int cap, long* cum,
                 int* out_len, int* first_last, void* stream);
int t2s_warp_gather(const void* x, int src_kind, int B, int C, int F, long ld_row, long ld_entry, const int* lengths, const long* cum,
                    const int* out_len, void* out, int cap, void* stream);
int t2s_warp_spans(const long* cum, const int* first_last, int B, int F, int T_in, const int* in_len, const int* lengths, int hop,
                   const long* trim_start, const long* trim_end, const long* offsets, long up, long down, long total,
                   const long* total_dev, long* spans, void* stream);

/* ---- control inside a stream: the alignment check and the time warp, pushed piece by piece (additive to ABI version 4;
 *      alignment.py AlignmentStream, rate.py WarpStream, streaming.py synthesize_stream(control=); csrc/align.hip, csrc/warp.hip) ----
 * Both computations above are prefix computations, so a stream carries them in HBM.  Notation: all buffers hold N_cap frames (the
 * decoder's max_decoder_steps); n0 frames were seen before this push and n after it, 0 <= n0 <= n <= N_cap.  The guarantee: after
 * every push the outputs are what the whole-row entry points give for the prefix [0, n), bit for bit, whatever the cuts.
 * t2s_align_window
 *  - A: B entries of n - n0 rows of T_in columns, the frames [n0, n); rows ld_row >= T_in and entries ld_entry >= (n - n0) ld_row
 *    elements apart; src_kind 1 f32, 2 f16.  NULL is allowed where n == n0.  S_b = clamp(in_len[b], 1, T_in), in_len NULL: T_in.
 *  - Row pass: t2s_align_rows' scan (ties to the smaller column, a NaN is never chosen) writes pos / peak / bad at columns [n0, n) of
 *    the [B, N_cap] buffers, which persist over the stream.  Columns at and behind n are not written.
 *  - Entry pass: one workgroup per entry walks the new frames 256 at a time.  Its running values live in a state block per entry
 *    (t2s_align_window_state() bytes each, 8-byte aligned): the run-start carry, the maxima of skip / back / stall, covered and
 *    bad_rows, and 256 double partial sums of the peaks.  A push with n0 == 0 initialises the block, and stores +0 to all of dur on
 *    the same stream before its kernels; later pushes add to dur by the same integer atomics.
 *  - Peak sums: frame t is added into partial t % 256 in ascending t, whatever the cuts; the 256-way tree of t2s_align_stats is
 *    formed on every push from the current partials.  focus is therefore t2s_align_stats' bits for the prefix on every push.
 *  - Stall: a run still open at frame n - 1 counts with its current length, as t2s_align_stats counts its last run.
 *  - Outputs, rewritten on every push: stats [B, 8], focus [B] and flags [B] of the prefix [0, n), F_b = n.  On a push with
 *    last == 0, flags carries only the live bits SKIP, BACK, STALL and NONFINITE; with last == 1 all eight, max_frames for TRUNCATED.
 *  - An empty push (n == n0) launches the entry pass alone: the outputs are rewritten, e.g. with the bits of last == 1.
 *  Memory safety as t2s_align_stats: every length is clamped, n0 and n as well; no pos that was read back is trusted.
 *  T2S_EINVAL, with nothing launched and nothing written: a NULL pos, peak, bad, state, stats, focus, dur or flags; A NULL with n > n0;
 *  a pointer not aligned to its element (state and focus to 8); B, T_in or N_cap < 1; N_cap > 2^30; B N_cap > 2^31 - 1; n0 < 0, n < n0
 *  or n > N_cap; ld_row < T_in; ld_entry < (n - n0) ld_row; a src_kind other than 1 or 2; a last other than 0 or 1.
 * t2s_warp_window_map
 *  - t2s_warp_map's step over the frames [n0, n), one stretch per entry for this push: `stretch`, or stretches int64 [B] in device
 *    memory, each clamped to [Q / 8, 8 Q] on the device.  It may differ from push to push.
 *  - cum int64 [B, N_cap + 1] persists and is the carry: cum[b, n0 + 1 .. n] is extended from the stored cum[b, n0]; n0 == 0 writes
 *    cum[b, 0] = 0.  Entries behind n are not written.
 *  - With path (int32, rows ld_path >= n apart - t2s_align_window's pos) and first_last int32 [B, T_in, 2]: frames [n0, n) apply
 *    t2s_warp_map's two tests with F_b = n.  A run's first frame is f == 0 or path[f - 1] != k, its last frame so far f == n - 1 or
 *    path[f + 1] != k; first only ever decreases, last only ever increases, so after any push first_last is t2s_warp_map's for the
 *    prefix.  The call sets first_last to -1 where n0 == 0 only.  t2s_warp_spans reads cum and first_last as they are, with F =
 *    N_cap and lengths = n.
 *  T2S_EINVAL: a NULL cum; first_last without path; path with T_in < 1 or ld_path < n; a pointer not aligned to its element; B < 1 or
 *  > 65535; B T_in > 2^31 - 1; the frames as above; without stretches, a stretch outside [Q / 8, 8 Q].
 * t2s_warp_window_gather
 *  - Writes output columns [j0, j1) of the warped mel to out [B, C, j1 - j0], dense and of x's type: t2s_warp_gather's expression
 *    exactly, with F_b = n.  x is the mel known so far, B entries of C rows of >= n frames, rows ld_row >= n and entries ld_entry >=
 *    C ld_row elements apart.  A column j is settled - no later frame changes it - when (2j + 1) Q <= c[n - 1] + c[n]; a caller who
 *    asks only for settled columns never reaches the clamp at F_b - 1 before the utterance's last push.
 *  - j1 == j0 launches nothing.
 *  T2S_EINVAL: a NULL cum; j0 < 0, j1 < j0, j1 > 2^31 - 1; and where j1 > j0: a NULL x or out, n < 1, ld_row < n, ld_entry < C ld_row,
 *  misaligned x or out, x overlapping out; C < 1; a src_kind other than 1 or 2; B and the frames as above. */
int t2s_align_window_state(void);
int t2s_align_window(const void* A, int src_kind, int B, int N_cap, int T_in, int n0, int n, int last, long ld_row, long ld_entry,
                     const int* in_len, int max_frames, int skip_max, int back_max, int stall_max, int end_slack, double min_focus,
                     int* pos, float* peak, unsigned char* bad, void* state, int* stats, double* focus, int* dur, int* flags,
                     void* stream);
int t2s_warp_window_map(int B, int N_cap, int n0, int n, long stretch, const long* stretches, const int* path, long ld_path,
                        const int* in_len, int T_in, long* cum, int* first_last, void* stream);
int t2s_warp_window_gather(const void* x, int src_kind, int B, int C, int N_cap, int n, long ld_row, long ld_entry, const long* cum,
                           long j0, long j1, void* out, void* stream);

/* ---- IIR filtering in device memory: cascades of second-order sections (additive to ABI version 4; audio.py SosFilter /
 *      FilterStream, data.py PcmPool.filter, DeliveryStream(pre_filter=, post_filter=), longform.py filter_long; csrc/sosfilt.hip) ----
 * A filter is n sections, 1 <= n <= t2s_sos_max_sections() (8: order 16), scipy.signal.sosfilt's: rows b0 b1 b2 a0 a1 a2 with
 * a0 = 1.  For a mono row of samples v[i] (int16, f32 or f16, each widened to double exactly) and a row gain g (gains[r], or 1
 * without gains), all in double:
 *     x[i] = v[i] g, and +0.0 where that product is not finite (a NaN or an infinity would otherwise reach the end of the row, and
 *            a stream cannot take back what it has delivered).  Each such i is counted in the row's `nonfinite`.
 *     every section, transposed direct form II, from a zero state at the row's first sample:
 *            y = b0 x + s1,    s1 = b1 x - a1 y + s2,    s2 = b2 x - a2 y        (each product-and-sum one fused multiply-add)
 *     the output of section j is the input of section j + 1.
 *     f32 destination: (float)y, one rounding.  int16 destination: rint(y), ties to even, saturated to [-32768, 32767]; each i with
 *            rint(y) outside that range is counted in the row's `clipped`.  An int16 row is filtered in the code domain unless a
 *            gain scales it (1 / 32768 brings it to [-1, 1) for an f32 destination).
 * The recursion runs in parallel along the row (csrc/sosfilt.hip): segments of t2s_sos_segment() samples, 256 to a tile of
 * t2s_sos_tile(), counted from the row's first sample.  Section by section, every segment is filtered from a zero state, the 256
 * end states are chained by a scan with the powers of the section's zero-input map, and the segment is filtered again from the
 * state in front of it; tiles are chained by the cascade's 2n x 2n zero-input map across a kernel boundary.  This is NOT the
 * sequential recursion's rounding: the result differs from scipy.signal.sosfilt in double by the reordering, which
 * profiles/filter_tests.md records (a pole pair at a few Hz, e.g. a 5 Hz high-pass at 48 kHz, is the kind of filter that direct-form
 * double arithmetic itself does not hold to a float32 ulp).  Every sum has one order that depends on the row's length alone, so a
 * row's samples and counts are the same bits alone and at any place of any batch or pool, at any alignment, whatever lies behind
 * its length.  The kernels do not judge stability; audio.py refuses a pole of radius >= 1.
 *  tab: t2s_sos_table_doubles() (552) doubles in device memory, built on the host in double by running the recurrence on unit states
 *    with zero input (audio.py sos_table): [5 j, 5 j + 5) b0 b1 b2 a1 a2 of section j; [40 + 32 j + 4 k, + 4) the 2 x 2 row-major
 *    zero-input map of section j's state (s1, s2) over segment 2^k samples, k = 0 .. 7; [296, 296 + (2 n)^2) the 2n x 2n row-major
 *    map of the cascade's state (s1, s2 of section 0, s1, s2 of section 1, ...) over a tile.
 *  t2s_sos_tile / t2s_sos_segment / t2s_sos_max_sections / t2s_sos_table_doubles: host only (4096, 16, 8, 552).
 *  t2s_sos_scratch: host only, the doubles of scratch for n_rows rows of at most max_count samples: 2 n per tile (-1 for arguments
 *    the call would refuse).
 *  t2s_sos_filter: table [n_rows][4] = (src_start, src_count, dst_start, dst_cap), int64 in device memory, any value safe as
 *    t2s_loud_apply's: nothing outside [0, src_len) is read, a row longer than max_count is cut there, stores land only inside
 *    [dst_start, dst_start + dst_cap) cut to max_out and to [0, dst_len).  The row gets min(count, dst_cap) samples and +0 behind
 *    them up to dst_cap.  src_kind 0 int16, 1 f32, 2 f16; dst_kind 0 int16 (from int16 only), 1 f32.  counts: int32 [n_rows][2] =
 *    (nonfinite over the row's samples, clipped over the stored ones); the call zeroes them on the stream first.  Two or three
 *    launches (no tile pass where max_count is below a tile); nothing waits across workgroups.
 *  The stream form.  carry: t2s_sos_window_carry(n) bytes a row (16 n + 4 tile), 8-byte aligned, [B] rows packed: the cascade's state
 *    at the start of the row's current tile (2n doubles), then the row's samples since then as f32 (fewer than a tile).  A new
 *    stream's carry is all zero bytes; its counts are zero and accumulate.
 *  t2s_sos_window: piece f32 (is_half 0) or f16 [B] rows of n >= 0 samples, ldp apart, at global position N0 of the row (the host
 *    knows it: the sum of the pieces so far); out f32 [B] rows of n, ldo apart.  The window stages carry | piece from the tile's
 *    start, N0 % tile samples back, and runs the same kernels, the chain starting from the carried state; a scanned state depends
 *    only on the lanes in front of it and an output only on the samples in front of it, so the piece's outputs are the whole row's
 *    bits for ANY piece lengths, and after the last piece counts are the whole row's.  carry_out (another buffer: ping-pong)
 *    receives the next carry; n = 0 copies it.  scratch: t2s_sos_scratch(B, N0 % tile + n, n_sections) doubles.  A causal filter
 *    holds nothing back: there is no final flag.
 *  T2S_EINVAL, with nothing launched and nothing written: a NULL src, table, tab, scratch, dst, counts, carry_in or carry_out, a NULL
 *    piece or out with n > 0; src_len, dst_len, n_rows, B, max_count or max_out <= 0; n_rows or B > 65535; max_count or N0 % tile + n
 *    > 2^31 - 1; max_out or N0 > 2^40; n < 0; ldp or ldo < n; n_sections outside [1, 8]; a kind out of range or f32 / f16 -> int16;
 *    scratch_len below t2s_sos_scratch's; a misaligned table, gains, tab, scratch, carry (8 bytes), counts or out (4), src, dst or
 *    piece (its element); src overlapping dst; carry_in overlapping carry_out. */
int t2s_sos_tile(void);
int t2s_sos_segment(void);
int t2s_sos_max_sections(void);
int t2s_sos_table_doubles(void);
long t2s_sos_scratch(int n_rows, long max_count, int n_sections);
int t2s_sos_filter(const void* src, int src_kind, long src_len, const long* table, int n_rows, long max_count, const double* gains,
                   const double* tab, int n_sections, double* scratch, long scratch_len, void* dst, int dst_kind, long dst_len,
                   long max_out, int* counts, void* stream);
int t2s_sos_window_carry(int n_sections);
int t2s_sos_window(const void* carry_in, void* carry_out, const void* piece, int is_half, int B, long n, long ldp, long N0,
                   const double* gains, const double* tab, int n_sections, double* scratch, long scratch_len, float* out, long ldo,
                   int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
