// Host only (t2s_api.hip, t2s_api_train.hip): how the C-ABI entry points check their arguments, fill ConvGemmArgs and launch the
// matrix-core GEMMs.  The derived fields - nk_x, nk, n_ttiles, n_mtiles - are each computed in one place below.
#pragma once
#include "../../include/t2s_hip.h"
#include "t2s_api_common.h"
#include "t2s_kernels.h"

#include <string.h>

// ---- tile heights: each a measured decision, by how many workgroups 256-row tiles would put on the chip's 256 CUs

// Gate GEMM tile height for a shape: 256-row tiles (the ping-pong kernel) unless they leave at least half of the chip's 256 CUs
// without a workgroup - short utterances at B = 1 - where 128-row tiles give twice the workgroups at half the work each.
static inline int gate_tile_rows(int B, int C, int L) {
    const long wg256 = (long)cdiv(C, 128) * cdiv(L, 256) * B;
    return (wg256 <= 128 && C % 64 == 0) ? 128 : 256;
}
// t2s_conv_bias_act: a grid of at most 64 workgroups is latency-bound per K-step: 128-row tiles with three LDS stages (conv_gemm.hip)
static inline int bias_act_tile_rows(int B, int Cout, int L) { return (long)cdiv(Cout, 256) * cdiv(L, 256) * B <= 64 ? 128 : 256; }
// t2s_wg_skip_sum and the lockstep t2s_wg_bwd_gate_dgrad: 128-row tiles when 256-row tiles would leave half the CUs without a
// workgroup (C = 512: 2 x 64 tiles)
static inline int lockstep_tile_rows(int B, int C, int L) { return cdiv(C, 256) * cdiv(L, 256) * B < 200 ? 128 : 256; }
// the lockstep t2s_conv_accumulate: 128-row tiles when 256-row tiles would leave most CUs without a workgroup
static inline int accumulate_tile_rows(int B, int Cout, int L) {
    const int wg256 = cdiv(Cout, 256) * cdiv(L, 256) * B;
    return (wg256 <= 128 || Cout % 256 == 0) && wg256 < 200 ? 128 : 256;
}
// The accumulate / gate-backward GEMMs of the training backward: 256-row tiles on the ping-pong schedule (csrc/gate_gemm_pp.hip)
// once they give at least ~100 workgroups - M = 512 at 8 x 16000 is 128, half the chip, and the rest is taken by the
// weight-gradient stream that runs beside them - else the lockstep kernels on 128-row tiles (twice the workgroups).
static inline bool bwd_pp256(const ConvGemmArgs& a, int rows) {
    return t2s_pp_shape_ok(a) && (long)cdiv(rows, 256) * a.n_ttiles * a.B >= 100;
}

// ---- argument checks that repeat

// B x L columns on planes of Lp rows; Mpad packed weight rows, of which the GEMM uses `rows`
static inline bool geometry_ok(int B, int L, int Lp, int halo, int Mpad, int rows) {
    return B > 0 && L > 0 && Lp == t2s_plane_rows(L, halo) && Mpad % 256 == 0 && Mpad >= rows;
}
static inline bool taps_ok(int taps, int dilation, int halo) {
    return taps > 0 && (taps & 1) && dilation > 0 && (taps / 2) * dilation <= halo;
}
// the gate GEMMs: C channels packed as tanh / sigmoid halves of 256-row tiles
static inline bool gate_shape_ok(int B, int C, int taps, int dilation, int L, int Lp, int halo, int Mpad) {
    return C > 0 && C % 4 == 0 && taps_ok(taps, dilation, halo) && geometry_ok(B, L, Lp, halo, Mpad, cdiv(C, 128) * 256);
}
// WN.end folded into the gate: MFMA fragments of 16 channels
static inline bool fold_ok(const void* fold_A, const float* fold_acc, int C) { return fold_A && fold_acc && al16(fold_A) && C % 16 == 0; }

// ---- the argument block: zeroed (memset: it goes to the kernel by value, padding included), then filled side by side
struct ConvGemm {
    ConvGemmArgs a;

    ConvGemm(const void* A_hi, const void* A_lo, const float* bias) {
        memset(&a, 0, sizeof(a));
        a.A_hi = (const u16*)A_hi; a.A_lo = (const u16*)A_lo; a.bias = bias;
    }
    void geometry(int B, int L, int Lp, int halo, int Mpad) {
        a.B = B; a.L = L; a.Lp = Lp; a.halo = halo; a.Mpad = Mpad;
        a.n_ttiles = cdiv(L, 256);
    }
    // K = taps x xc chunks of the X planes, then sc chunks of the optional S planes; xbs: see ConvGemmArgs
    void k_side(const void* X_hi, const void* X_lo, int xc, int taps, int dil, const void* S_hi = nullptr, const void* S_lo = nullptr,
                int sc = 0, int xbs = 0) {
        a.X_hi = (const u16*)X_hi; a.X_lo = (const u16*)X_lo; a.xc = xc; a.xbs = xbs;
        a.S_hi = (const u16*)S_hi; a.S_lo = (const u16*)S_lo; a.sc = sc;
        a.taps = taps; a.dil = dil;
        a.nk_x = taps * xc; a.nk = a.nk_x + sc;
    }
    void output(void* O_hi, void* O_lo, int oc) { a.O_hi = (u16*)O_hi; a.O_lo = (u16*)O_lo; a.oc = oc; }
    // WN.end folded into the gate; fold_acc holds t2s_wg_gate_fold_slots(B, C, L) slots
    void fold(const void* fold_A, float* fold_acc, int fold_init) {
        a.fold_A = (const u16*)fold_A; a.fold_acc = fold_acc; a.fold_init = fold_init;
    }
    // `rows` packed output rows (a gate GEMM has 2 C) on tiles mt_rows high: n_mtiles follows from the two, here and nowhere else.
    // Phase mode exists only on the ping-pong gate schedule; bwd_pp: the caller found bwd_pp256 true (mt_rows = 256).
    // h16: fp16 planes, one-plane A operand (the _h16 entry points; the folded gate and the residual-only GEMM have that form).
    hipError_t launch(int epi, int rows, int mt_rows, void* stream, bool bwd_pp = false, bool h16 = false) {
        a.n_mtiles = cdiv(rows, mt_rows);
        if (h16) return t2s_launch_conv_gemm(a, epi, (hipStream_t)stream, mt_rows, true);
        if (a.ph_P > 0) return t2s_launch_gate_gemm_pp(a, (hipStream_t)stream);
        if (bwd_pp) return t2s_launch_bwd_gemm_pp(a, epi, (hipStream_t)stream);
        return t2s_launch_conv_gemm(a, epi, (hipStream_t)stream, mt_rows);
    }
};
