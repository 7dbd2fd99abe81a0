"""The composed-conditioning path of WaveGlow.infer (include/t2s_hip.h, t2s_wg_upsample_basis and the three
entry points behind it) restated in float64 with stock torch: the upsampled and squeezed spectrogram, the upsampler's basis U_phi,
the mel windows, the composed weights W_cond U_phi - and the plane layouts the kernels write, each with the inverse indexing that
reads it back.  tests/test_compose_ref_cpu.py pins it; tests/test_waveglow_compose_kernels_gpu.py compares the kernels with it.  A
plain module, imported by the tests; nothing here touches the GPU.

With P = stride / G, nlag = ksize / stride and K2 = nlag * n_mel, plane row t = P f + phi of the squeezed spectrogram is
    spect[co G + g][t] = bias[co] + sum_{j, ci} W[ci][co][stride j + G phi + g] mel[ci][f - j] = (U_phi window(f))[c] + bias_exp[c],
so a 1x1 convolution W_cond of it is (W_cond U_phi) window(f) + (b + W_cond bias_exp)."""
import torch
import torch.nn.functional as F

from text2speech_amd import planes
from wg_fwd_util import _gate_row


def geometry(n_mel, ksize, stride, G):
    """(P, nlag, K2) of an upsampler ConvTranspose1d(n_mel, n_mel, ksize, stride) squeezed by G"""
    assert ksize % stride == 0 and stride % G == 0, (ksize, stride, G)
    return stride // G, ksize // stride, (ksize // stride) * n_mel


def plane_rows(L, halo):
    """rows of a plane of L data rows (include/t2s_hip.h: t2s_plane_rows)"""
    return -(-L // 256) * 256 + 2 * halo


# ---------------------------------------------------------------------------------------------- the operation
def upsample_squeezed(mel, W, bias, stride, G, L):
    """mel [B, n_mel, frames], W [n_mel, n_mel, ksize], bias [n_mel] -> float64 [B, n_mel G, L]: F.conv_transpose1d cut to G L
    samples and squeezed; channel co G + g at column t is sample G t + g"""
    y = F.conv_transpose1d(mel.double(), W.double(), bias.double(), stride=stride)
    assert G * L <= y.size(2), "the mel is too short for L"
    B, M = y.shape[:2]
    return y[:, :, :G * L].reshape(B, M, L, G).permute(0, 1, 3, 2).reshape(B, M * G, L).contiguous()


def basis(W, bias, stride, G):
    """(U [P, n_mel G, K2], bias_exp [n_mel G]) float64: U[phi][co G + g][j n_mel + ci] = W[ci][co][stride j + G phi + g],
    bias_exp[c] = bias[c // G]"""
    M, _, ksize = W.shape
    P, nlag, K2 = geometry(M, ksize, stride, G)
    w = W.double().reshape(M, M, nlag, P, G)                 # [ci, co, j, phi, g]: the tap is stride j + G phi + g
    U = w.permute(3, 1, 4, 2, 0).reshape(P, M * G, K2).contiguous()
    return U, bias.double().repeat_interleave(G)


def mel_windows(mel, nlag, Fp):
    """mel [B, n_mel, frames] -> float64 [B, nlag n_mel, Fp]: row j n_mel + ci at frame f is mel[b][ci][f - j], zero outside
    [0, frames)"""
    B, M, Fr = mel.shape
    out = torch.zeros(B, nlag * M, Fp, dtype=torch.float64)
    for j in range(nlag):
        n = min(Fr, Fp - j)
        if n > 0:
            out[:, j * M:(j + 1) * M, j:j + n] = mel.double()[:, :, :n]
    return out


def composed(w_cond_eff, b_sum, U, bias_exp):
    """(A2 [P, 2C, K2], b [2C]) float64 in channel order: A2_phi = W_cond U_phi, b = b_sum + W_cond bias_exp"""
    w = w_cond_eff.double().reshape(w_cond_eff.size(0), -1)
    return torch.einsum("oc,pck->pok", w, U), b_sum.double() + w @ bias_exp


def phase_columns(A2, win, L):
    """A2 [P, O, K2], windows [B, K2, >= ceil(L / P)] -> [B, O, L]: column P f + phi is A2_phi @ window(f)"""
    P = A2.size(0)
    nF = -(-L // P)
    v = torch.einsum("pok,bkf->bofp", A2, win[:, :, :nF])
    return v.reshape(v.size(0), v.size(1), nF * P)[:, :, :L]


# ---------------------------------------------------------------------------------------------- the gate GEMM that reads them
WN_KS, WN_NH = 3, 4         # kernel size and n_half of the seeded WN of every gate case


def wn_seed(C, nl):
    return 1000 * C + 10 * nl + WN_KS + WN_NH


def gate_case(C, n_mel, ksize, stride, G, B, L, nl):
    """One seeded gate case, float64 on the CPU: a WN (wg_fwd_util.wn_state, n_cond = n_mel G), audio, a mel of ceil(L / P) frames,
    an upsampler whose weights are scaled by 1 / sqrt(nlag n_mel) (spect stays near unit variance), spect = upsample_squeezed of
    them, and the oracle's per-layer expectation (wg_fwd_util.layer_expect; layer i has dilation 2^i)."""
    import wg_fwd_util as Wf
    P, nlag, K2 = geometry(n_mel, ksize, stride, G)
    n_cond = n_mel * G
    sd = Wf.wn_state(C, nl, WN_KS, WN_NH, n_cond, wn_seed(C, nl))
    cfg = Wf.wn_cfg(C, nl, WN_KS)
    gen = torch.Generator().manual_seed(7 * L + B + n_mel)
    nF = -(-L // P)
    audio = torch.randn(B, WN_NH, L, generator=gen).double()
    mel = torch.randn(B, n_mel, nF, generator=gen).double()
    W_up = (torch.randn(n_mel, n_mel, ksize, generator=gen) / (nlag * n_mel) ** 0.5).double()
    b_up = (0.1 * torch.randn(n_mel, generator=gen)).double()
    spect = upsample_squeezed(mel, W_up, b_up, stride, G, L)
    layers, _ = Wf.layer_expect(sd, cfg, audio, spect)
    U, bias_exp = basis(W_up, b_up, stride, G)
    return dict(C=C, B=B, L=L, P=P, nlag=nlag, K2=K2, F=nF, n_cond=n_cond, sd=sd, cfg=cfg, audio=audio, mel=mel, W_up=W_up, b_up=b_up,
                spect=spect, layers=layers, U=U, bias_exp=bias_exp)


def gate_operands(case, i):
    """(w_in [2C, C, ks], A2 [P, 2C, K2], b [2C]) float64 of layer i: the effective in-layer weights, the composed conditioning
    weights and the composed bias (in-layer bias + conditioning bias + W_cond bias_exp)"""
    import wg_fwd_util as Wf
    sd = case["sd"]
    w_in = Wf.eff(sd, "in_layers.%d" % i)
    w_cond = Wf.eff(sd, "cond_layers.%d" % i)[:, :, 0]
    b_sum = sd["WN.0.in_layers.%d.bias" % i] + sd["WN.0.cond_layers.%d.bias" % i]
    A2, b = composed(w_cond, b_sum, case["U"], case["bias_exp"])
    return w_in, A2, b


def gate_acts(case, i, w_in, A2, b, x, win):
    """tanh * sigmoid of in_layers[i](x) + the composed conditioning of the windows + b, in float64"""
    C, d = case["C"], 2 ** i
    s = F.conv1d(x, w_in, None, dilation=d, padding=(WN_KS * d - d) // 2) + phase_columns(A2, win, case["L"]) + b[None, :, None]
    return torch.tanh(s[:, :C]) * torch.sigmoid(s[:, C:])


def gate_floor(case, i):
    """(acts floor, fold floor), each (norm-relative, max-relative), from the reference alone: the float64 gate with A2, M, X and the
    in-layer weights replaced by the values their (hi, lo) planes hold, against the unrounded oracle; and the fold product of the
    rounded F_i with those acts as planes hold them, in the kernel's three products (wg_bwd_util.split3_floor's arithmetic),
    against the oracle's fold."""
    import wg_bwd_util as Ub
    from wg_fwd_util import plane_round
    ly = case["layers"][i]
    w_in, A2, b = gate_operands(case, i)
    win = mel_windows(case["mel"], case["nlag"], case["F"])
    exact = gate_acts(case, i, w_in, A2, b, ly["x"], win)
    assert Ub.rel(exact, ly["acts"]) < 1e-12, "the composed gate is not the oracle's"
    acts_r = gate_acts(case, i, plane_round(w_in), plane_round(A2), b, plane_round(ly["x"]), plane_round(win))
    fa, fb = plane_round(ly["F"]), plane_round(acts_r)

    def split(x):
        hi = x.to(torch.float32).to(torch.bfloat16).double()
        return hi, x - hi
    (ah, al), (bh, bl) = split(fa), split(fb)
    eq = "jc,bct->bjt"
    emu = torch.einsum(eq, ah, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, al, bh)
    return (Ub.rel(acts_r, ly["acts"]), Ub.maxrel(acts_r, ly["acts"])), (Ub.rel(emu, ly["fold"]), Ub.maxrel(emu, ly["fold"]))


# ---------------------------------------------------------------------------------------------- layouts: write
def _split(x):
    """float64 -> (hi, lo) bf16 of its f32 value (exact where x is an f32 value: what a kernel that gathers f32 values holds)"""
    return planes.split_bf16(x.to(torch.float32))


def u_planes(U, bias_exp, halo):
    """(hi, lo) [1, ceil(n_chan / 32), Lp, 32]: channel c of row halo + phi K2 + k is U[phi][c][k], row halo + P K2 is the expanded
    bias, everything else zero; Lp = plane_rows(P K2 + 1, halo)"""
    P, n_chan, K2 = U.shape
    cols = torch.cat([U.permute(1, 0, 2).reshape(n_chan, P * K2), bias_exp.reshape(n_chan, 1)], 1)
    return planes.to_planes(cols.to(torch.float32)[None], halo, plane_rows(P * K2 + 1, halo))


def rows_planes(T, Mpad):
    """T [P, rows, K2] (rows already in packed order, K2 % 32 == 0) -> (hi, lo) [P, K2 / 32, Mpad, 32], rows >= `rows` zero"""
    P, rows, K2 = T.shape
    assert K2 % 32 == 0 and rows <= Mpad
    full = torch.zeros(P, Mpad, K2, dtype=torch.float64)
    full[:, :rows] = T
    return _split(full.reshape(P, Mpad, K2 // 32, 32).permute(0, 2, 1, 3).contiguous())


def a2_planes(A2, C, Mpad):
    """A2 [P, 2C, K2] in channel order -> the planes the gate GEMM reads: output channel o in packed row _gate_row(o, C)"""
    P, O, K2 = A2.shape
    assert O == 2 * C
    r = _gate_row(torch.arange(O), C)
    T = torch.zeros(P, int(r.max()) + 1, K2, dtype=torch.float64)
    T[:, r] = A2.double()
    return rows_planes(T, Mpad)


def bias_rows(b, C, Mpad):
    """b [2C] in channel order -> f32 [Mpad] in packed rows, zero elsewhere"""
    out = torch.zeros(Mpad, dtype=torch.float32)
    out[_gate_row(torch.arange(2 * C), C)] = b.to(torch.float32)
    return out


def m_planes(win, Fp):
    """mel windows [B, K2, Fp] -> (hi, lo) [B, ceil(K2 / 32), Fp, 32], columns past K2 zero"""
    assert win.size(2) == Fp
    return planes.to_planes(win.to(torch.float32), 0, Fp)


# ---------------------------------------------------------------------------------------------- layouts: read back
def _val(hi, lo):
    return hi.double().cpu() + lo.double().cpu()


def u_decode(hi, lo, P, K2, n_chan, halo):
    """(U [P, n_chan, K2], bias_exp [n_chan]) float64 from the U planes, by the kernels' own index arithmetic"""
    v = _val(hi, lo)
    c = torch.arange(n_chan)
    U = torch.empty(P, n_chan, K2, dtype=torch.float64)
    for phi in range(P):
        for k in range(K2):
            U[phi, :, k] = v[0, c >> 5, halo + phi * K2 + k, c & 31]
    return U, v[0, c >> 5, halo + P * K2, c & 31]


def rows_decode(hi, lo, rows):
    """[P, rows, K2] float64 from A2 planes [P, K2 / 32, Mpad, 32], rows in packed order"""
    v = _val(hi, lo)
    k = torch.arange(v.size(1) * 32)
    return torch.stack([v[:, k >> 5, m, k & 31] for m in range(rows)], 1)


def a2_decode(hi, lo, C):
    """[P, 2C, K2] float64 in channel order from A2 planes"""
    v = _val(hi, lo)
    k = torch.arange(v.size(1) * 32)
    r = _gate_row(torch.arange(2 * C), C)
    return torch.stack([v[:, k >> 5, int(m), k & 31] for m in r], 1)


def bias_decode(b, C):
    """[2C] float64 in channel order from packed bias rows"""
    return b.double().cpu()[_gate_row(torch.arange(2 * C), C)]


def m_decode(hi, lo, K2):
    """[B, K2, Fp] float64 from mel-window planes"""
    v = _val(hi, lo)
    k = torch.arange(K2)
    return torch.stack([v[:, k >> 5, f, k & 31] for f in range(v.size(2))], 2)
