"""tests/compose_ref.py against stock torch, in float64 on the CPU: the identity the composed-conditioning path rests on - a 1x1
convolution of the upsampled, squeezed spectrogram at plane row P f + phi is the composed weights of phase phi applied to the mel
window of frame f - and the plane layouts, written and read back with the inverse indexing."""
import pytest
import torch
import torch.nn.functional as F

import compose_ref as R
from text2speech_amd import planes
from wg_fwd_util import _gate_row

G = 8
# (n_mel, ksize, stride)
GEOMS = [(8, 256, 64), (16, 256, 128), (5, 32, 8), (80, 1024, 256)]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _setup(n_mel, ksize, stride, B, L, extra_frames, seed):
    P, nlag, K2 = R.geometry(n_mel, ksize, stride, G)
    gen = torch.Generator().manual_seed(seed)
    frames = -(-L // P) + extra_frames
    mel = torch.randn(B, n_mel, frames, generator=gen).double()
    W = (torch.randn(n_mel, n_mel, ksize, generator=gen) / (nlag * n_mel) ** 0.5).double()
    bias = (0.1 * torch.randn(n_mel, generator=gen)).double()
    return P, nlag, K2, gen, mel, W, bias


@pytest.mark.parametrize("ragged", [False, True], ids=["L-multiple-of-P", "L-ragged"])
@pytest.mark.parametrize("n_mel,ksize,stride", GEOMS, ids=["%d-%d-%d" % g for g in GEOMS])
def test_composed_weights_on_windows_are_the_conditioning_convolution(n_mel, ksize, stride, ragged):
    """conv1d(upsample_squeezed(mel), W_cond, b)[:, :, P f + phi] == A2_phi @ window(f) + b_composed to 1e-12 relative, over every
    column - frames 0 .. nlag - 1, whose windows reach in front of the clip, and the last frame among them - and at those frames
    one by one"""
    P = stride // G
    F_ = 6
    L = P * F_ - (P // 2 if ragged and P > 1 else 0) - (1 if ragged and P == 1 else 0)
    B, rows = 2, 12
    P, nlag, K2, gen, mel, W, bias = _setup(n_mel, ksize, stride, B, L, 1 if ragged else 0, seed=n_mel + stride)
    nF = -(-L // P)
    assert nF > nlag and (L % P != 0) == (ragged and P > 1)
    w_cond = torch.randn(rows, n_mel * G, generator=gen).double()
    b = torch.randn(rows, generator=gen).double()
    spect = R.upsample_squeezed(mel, W, bias, stride, G, L)
    assert spect.shape == (B, n_mel * G, L) and spect.dtype == torch.float64
    want = F.conv1d(spect, w_cond[:, :, None], b)
    U, bias_exp = R.basis(W, bias, stride, G)
    assert U.shape == (P, n_mel * G, K2)
    A2, bc = R.composed(w_cond, b, U, bias_exp)
    win = R.mel_windows(mel, nlag, nF)
    assert win.shape == (B, K2, nF)
    got = torch.empty_like(want)
    for phi in range(P):
        cols = torch.arange(phi, L, P)
        got[:, :, cols] = torch.einsum("ok,bkf->bof", A2[phi], win[:, :, :cols.numel()]) + bc[None, :, None]
    assert _rel(got, want) < 1e-12, _rel(got, want)
    scale = float(want.abs().max())
    for f in list(range(nlag)) + [nF - 1]:
        for phi in range(P):
            t = P * f + phi
            if t < L:
                assert float((got[:, :, t] - want[:, :, t]).abs().max()) < 1e-12 * scale, (f, phi)
    # the spectrogram itself, through the basis: U_phi window(f) + bias_exp
    for phi in (0, P - 1):
        cols = torch.arange(phi, L, P)
        s = torch.einsum("ck,bkf->bcf", U[phi], win[:, :, :cols.numel()]) + bias_exp[None, :, None]
        assert _rel(s, spect[:, :, cols]) < 1e-12


@pytest.mark.parametrize("C,geom,B,L,i", [(16, (8, 256, 64), 2, 21, 1), (32, (16, 256, 128), 3, 40, 0)], ids=["C16-P8", "C32-P16"])
def test_gate_reference_is_the_oracles_gate(C, geom, B, L, i):
    """compose_ref.gate_case / gate_acts: the composed gate of the windows is the oracle's acts_i (gate_floor asserts 1e-12), its
    floor is a rounding-sized figure, and a window one frame late, the next phase's weights or a zeroed batch entry each move the
    acts and the fold product far beyond the GEMM bars (2e-5 / 1e-4)"""
    import wg_bwd_util as Ub
    cs = R.gate_case(C, *geom, G, B, L, 2)
    assert L % cs["P"] != 0 and cs["F"] == -(-L // cs["P"]) and cs["spect"].shape == (B, geom[0] * G, L)
    (fn, fm), (gn, gm) = R.gate_floor(cs, i)
    assert 1e-7 < fn < 2e-5 and fn <= fm < 1e-4 and 1e-7 < gn < 2e-5 and gm < 1e-4
    ly = cs["layers"][i]
    w_in, A2, b = R.gate_operands(cs, i)
    win = R.mel_windows(cs["mel"], cs["nlag"], cs["F"])
    late = torch.zeros_like(win)
    late[:, :, 1:] = win[:, :, :-1]
    dropped = ly["acts"].clone()
    dropped[B - 1] = 0
    for wrong in (R.gate_acts(cs, i, w_in, A2, b, ly["x"], late), R.gate_acts(cs, i, w_in, torch.roll(A2, -1, 0), b, ly["x"], win), dropped):
        fold = torch.einsum("jc,bct->bjt", ly["F"], wrong)
        assert Ub.rel(wrong, ly["acts"]) > 0.1 and Ub.maxrel(wrong, ly["acts"]) > 0.1
        assert Ub.rel(fold, ly["fold"]) > 0.1 and Ub.maxrel(fold, ly["fold"]) > 0.1


def test_upsample_squeezed_channel_order():
    """channel co G + g at column t is sample G t + g of the transposed convolution, written out by hand"""
    n_mel, ksize, stride, L = 3, 16, 8, 5
    P, nlag, K2, gen, mel, W, bias = _setup(n_mel, ksize, stride, 1, L, 1, seed=1)
    spect = R.upsample_squeezed(mel, W, bias, stride, G, L)
    for co, g, t in [(0, 0, 0), (2, 7, 4), (1, 3, 2)]:
        s = G * t + g
        v = float(bias[co])
        for ci in range(n_mel):
            for f in range(mel.size(2)):
                if 0 <= s - stride * f < ksize:
                    v += float(mel[0, ci, f] * W[ci, co, s - stride * f])
        assert abs(float(spect[0, co * G + g, t]) - v) < 1e-12


def test_mel_windows_edges():
    """zero in front of the clip and behind it; the tail lags of rows frames .. frames + nlag - 2 are still the clip's last frames"""
    mel = torch.arange(1, 2 * 3 * 5 + 1, dtype=torch.float64).reshape(2, 3, 5)
    win = R.mel_windows(mel, 4, 10)
    for b in range(2):
        for j in range(4):
            for ci in range(3):
                for f in range(10):
                    want = float(mel[b, ci, f - j]) if 0 <= f - j < 5 else 0.0
                    assert float(win[b, j * 3 + ci, f]) == want
    assert float(win[:, :, 8:].abs().max()) == 0.0 and float(win[:, 9:, 7].abs().min()) > 0.0
    assert R.mel_windows(mel, 4, 5).shape == (2, 12, 5) and torch.equal(R.mel_windows(mel, 4, 5), win[:, :, :5])
    assert torch.equal(R.mel_windows(mel[:, :, :1], 4, 3)[:, :, 0], torch.cat([mel[:, :, 0], torch.zeros(2, 9, dtype=torch.float64)], 1))


@pytest.mark.parametrize("n_mel,ksize,stride,halo", [(8, 256, 64, 0), (5, 32, 8, 128), (16, 256, 128, 0)])
def test_u_planes_round_trip(n_mel, ksize, stride, halo):
    P, nlag, K2, gen, mel, W, bias = _setup(n_mel, ksize, stride, 1, 8, 0, seed=stride)
    W, bias = W.float().double(), bias.float().double()        # f32 values: the planes hold them to the (hi, lo) pair
    U, bias_exp = R.basis(W, bias, stride, G)
    hi, lo = R.u_planes(U, bias_exp, halo)
    n_chan, ncols = n_mel * G, P * K2 + 1
    assert hi.shape == (1, -(-n_chan // 32), R.plane_rows(ncols, halo), 32) and hi.dtype == torch.bfloat16
    U2, be2 = R.u_decode(hi, lo, P, K2, n_chan, halo)
    h, l = planes.split_bf16(U.float())
    assert torch.equal(U2, h.double() + l.double())
    h, l = planes.split_bf16(bias_exp.float())
    assert torch.equal(be2, h.double() + l.double())
    assert float((U2 - U).abs().max()) <= 2.0 ** -15 * float(U.abs().max())
    # rows outside [halo, halo + ncols) and channels past n_chan are zero
    for p in (hi, lo):
        assert float(p[:, :, :halo].float().abs().max() if halo else 0.0) == 0.0
        assert float(p[:, :, halo + ncols:].float().abs().max()) == 0.0
        if n_chan % 32:
            assert float(p[:, -1, :, n_chan % 32:].float().abs().max()) == 0.0
    # one element by the definition: U[phi][co G + g][j n_mel + ci] = W[ci][co][stride j + G phi + g]
    phi, co, g, j, ci = P - 1, n_mel - 1, 5, nlag - 1, 1
    assert float(U[phi, co * G + g, j * n_mel + ci]) == float(W[ci, co, stride * j + G * phi + g])
    assert float(bias_exp[co * G + g]) == float(bias[co])


@pytest.mark.parametrize("C,P,K2", [(48, 8, 32), (80, 1, 64), (160, 2, 32)])
def test_a2_planes_round_trip(C, P, K2):
    gen = torch.Generator().manual_seed(C)
    A2 = torch.randn(P, 2 * C, K2, generator=gen).double()
    b = torch.randn(2 * C, generator=gen).float()
    Mpad = -(-C // 128) * 256
    hi, lo = R.a2_planes(A2, C, Mpad)
    assert hi.shape == (P, K2 // 32, Mpad, 32)
    h, l = planes.split_bf16(A2.float())
    assert torch.equal(R.a2_decode(hi, lo, C), h.double() + l.double())
    # every row that is no channel's packed row is zero
    used = torch.zeros(Mpad, dtype=torch.bool)
    used[_gate_row(torch.arange(2 * C), C)] = True
    assert float(hi[:, :, ~used].float().abs().max() if (~used).any() else 0.0) == 0.0
    # packed-order rows: rows_planes / rows_decode are each other's inverse, padding rows zero
    T = torch.randn(P, 96, K2, generator=gen).double()
    rh, rl = R.rows_planes(T, 256)
    h, l = planes.split_bf16(T.float())
    assert torch.equal(R.rows_decode(rh, rl, 96), h.double() + l.double())
    assert float(rh[:, :, 96:].float().abs().max()) == 0.0 and float(rl[:, :, 96:].float().abs().max()) == 0.0
    bp = R.bias_rows(b.double(), C, Mpad)
    assert torch.equal(R.bias_decode(bp, C), b.double()) and float(bp[~used].abs().max() if (~used).any() else 0.0) == 0.0


@pytest.mark.parametrize("B,n_mel,frames,nlag,Fp", [(3, 8, 5, 4, 5), (2, 5, 9, 4, 64), (1, 80, 3, 4, 256)])
def test_m_planes_round_trip(B, n_mel, frames, nlag, Fp):
    mel = torch.randn(B, n_mel, frames, generator=torch.Generator().manual_seed(frames)).double()
    win = R.mel_windows(mel, nlag, Fp)
    K2 = nlag * n_mel
    hi, lo = R.m_planes(win, Fp)
    assert hi.shape == (B, -(-K2 // 32), Fp, 32)
    h, l = planes.split_bf16(win.float())
    assert torch.equal(R.m_decode(hi, lo, K2), h.double() + l.double())
    if K2 % 32:
        assert float(hi[:, -1, :, K2 % 32:].float().abs().max()) == 0.0
