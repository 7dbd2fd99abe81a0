"""The composed-conditioning kernels of WaveGlow.infer (T2S_COND_COMPOSE=1), one by one
through the C entry points, against float64 (tests/compose_ref.py, which tests/test_compose_ref_cpu.py pins):

  t2s_wg_upsample_basis, t2s_wg_compose_cond, t2s_wg_melwin_planes    layout kernels: gathered f32 values, split into (hi, lo) - bit-exact
  t2s_wg_in_melwin_gate_fold                                          the phase-tile gate GEMM (gate_gemm_pp_kernel<PH = true>)
  the weight chain basis -> t2s_conv_bias_act -> compose_cond -> gate   once, end to end
  t2s_wg_upsample_squeeze (bf16)                                      the default conditioning writer, both of its kernels

Every output is a guarded allocation and the guards are asserted after each call.  Every kernel reads host-built operands, never
the output of another kernel under test - test_weight_chain_end_to_end is the one exception, and is there for that.  The in-layer
weights and fold_A come from the engine's pack entry points exactly as in tests/test_waveglow_fwd_kernels_gpu.py (its _WN), whose
own tests cover them.

Bars: wg_bwd_util.GEMM_NORM / GEMM_MAX for plane outputs and fold sums (the bars of test_in_cond_gate_fold, whose arithmetic this
is).  Each gate case prints its floor - compose_ref.gate_floor: the float64 gate with A2, M, X and the in-layer weights as their
planes hold them against the unrounded oracle, no output of the code under test - and takes 4 x the floor as a bar where the floor
exceeds a quarter of that bar (_fold_bars).  The norm-relative floors are 4.2e-6 .. 4.6e-6 against a quarter bar of 5e-6: that bar
stays.  The max-relative floors are 1.7e-5 .. 2.9e-5 against 2.5e-5: two-m-tiles (2.53e-5 -> 1.01e-4) and by-grid-size (2.93e-5 ->
1.17e-4) take the raised bar, and the kernel's figures are inside the unraised one there too
(profiles/waveglow_compose_kernel_tests.md has every figure)."""
import math

import pytest
import torch

import compose_ref as R
import test_waveglow_fwd_kernels_gpu as K
import wg_bwd_util as U
from text2speech_amd import _lib, planes

pytestmark = pytest.mark.gpu

DEV = U.DEV
HALO = K.HALO
G8 = 8
EINVAL = -1


def _bits16(t):
    return t.cpu().contiguous().view(torch.int16)


def _assert_planes_equal(label, got, want):
    """bit patterns of a guarded (hi, lo) pair against the host-built pair; guards intact"""
    for name, g, w in zip(("hi", "lo"), got, want):
        assert g.t.shape == w.shape, (label, name, g.t.shape, w.shape)
        same = _bits16(g.t) == _bits16(w)
        assert bool(same.all()), "%s: %d elements of the %s plane differ, first at %r" % (
            label, int((~same).sum()), name, tuple(int(v) for v in (~same).nonzero()[0]))
        g.assert_guards(label + " " + name)


# ---------------------------------------------------------------------------------------------- (a) the layout kernels, bit-exact
def _upsampler(n_mel, ksize, stride, seed):
    """(W [n_mel, n_mel, ksize], bias [n_mel]) f32 on the CPU, scaled so that the upsampled spectrogram stays near unit variance"""
    gen = torch.Generator().manual_seed(seed)
    nlag = ksize // stride
    return torch.randn(n_mel, n_mel, ksize, generator=gen) / (nlag * n_mel) ** 0.5, 0.1 * torch.randn(n_mel, generator=gen)


@pytest.mark.parametrize("n_mel,ksize,stride,halo", [(8, 256, 64, 0), (16, 256, 128, 0), (5, 32, 8, 0), (8, 256, 64, 128)],
                         ids=["8-256-64", "16-256-128", "5-32-8-quarter-chunk", "8-256-64-halo128"])
def test_upsample_basis(n_mel, ksize, stride, halo):
    """U as planes whose time axis is the column (phi, k): every element the split of the gathered f32 weight, the expanded bias in
    the last column, the rows behind it, the halo rows and the channels past n_mel * 8 (5 mels: 40 of 64) zero."""
    _lib.load()
    P, nlag, K2 = R.geometry(n_mel, ksize, stride, G8)
    W, bias = _upsampler(n_mel, ksize, stride, seed=n_mel + stride)
    Ub, bias_exp = R.basis(W, bias, stride, G8)
    want = R.u_planes(Ub, bias_exp, halo)
    n_chan, ncols = n_mel * G8, P * K2 + 1
    sc, Lp = -(-n_chan // 32), _lib.plane_rows(ncols, halo)
    assert Lp == R.plane_rows(ncols, halo) and want[0].shape == (1, sc, Lp, 32)
    out = K._plane_pair(1, sc, Lp)
    W_d, bias_d = U.dev(W), U.dev(bias)
    label = "upsample_basis %d-%d-%d halo %d" % (n_mel, ksize, stride, halo)
    _lib.call("t2s_wg_upsample_basis", _lib.ptr(W_d), _lib.ptr(bias_d), n_mel, ksize, stride, G8, Lp, halo, _lib.ptr(out[0].t),
              _lib.ptr(out[1].t), _lib.current_stream())
    K._sync()
    _assert_planes_equal(label, out, want)
    # what the equality above contains, spelled out: the bias column is the last one, nothing behind it, nothing past the channels
    c = torch.arange(n_chan)
    bh, bl = planes.split_bf16(bias_exp.float())
    last = halo + ncols - 1
    assert torch.equal(out[0].t.cpu()[0, c >> 5, last, c & 31], bh) and torch.equal(out[1].t.cpu()[0, c >> 5, last, c & 31], bl)
    assert float(bh.float().abs().min()) > 0.0
    for p in out:
        assert float(p.t[:, :, last + 1:].float().abs().max()) == 0.0, label + ": rows behind the bias column"
        if halo:
            assert float(p.t[:, :, :halo].float().abs().max()) == 0.0, label + ": halo rows"
        if n_chan % 32:
            assert float(p.t[:, -1, :, n_chan % 32:].float().abs().max()) == 0.0, label + ": channels past n_mel * 8"
    # Lp must be the rows of exactly P K2 + 1 columns
    assert _lib.load().t2s_wg_upsample_basis(_lib.ptr(W_d), _lib.ptr(bias_d), n_mel, ksize, stride, G8, Lp + 256, halo,
                                             _lib.ptr(out[0].t), _lib.ptr(out[1].t), _lib.current_stream()) == EINVAL


@pytest.mark.parametrize("rows,Mpad", [(96, 256), (320, 512), (256, 256)])
def test_compose_cond(rows, Mpad):
    """tmp [rows][ld] f32 -> A2[phi][K2 / 32][Mpad][32]: the split of tmp[m][phi K2 + k], rows rows .. Mpad - 1 zero; bias_out = bias_in
    + the last column in f32 (one add: bit-exact), bias_in above `rows`.  K2 32 and 64, P 1 and 8, ld = P K2 + 1 and larger."""
    _lib.load()
    gen = torch.Generator().manual_seed(rows + Mpad)
    for K2 in (32, 64):
        for P in (1, 8):
            for extra in (0, 7):
                ncols = P * K2 + 1
                ld = ncols + extra
                label = "compose_cond rows %d Mpad %d K2 %d P %d ld %d" % (rows, Mpad, K2, P, ld)
                tmp = torch.randn(rows, ld, generator=gen)
                bias_in = torch.randn(Mpad, generator=gen)
                T = tmp[:, :P * K2].reshape(rows, P, K2).permute(1, 0, 2).double()
                want = R.rows_planes(T, Mpad)
                want_b = bias_in.clone()
                want_b[:rows] = bias_in[:rows] + tmp[:, P * K2]
                out = (K._BF(P, K2 // 32, Mpad, 32), K._BF(P, K2 // 32, Mpad, 32))
                for o in out:           # not zero beforehand: the padding rows are the kernel's to write
                    o.t.fill_(0.75)
                bias_out = U.Guarded(Mpad)
                tmp_d, bias_d = U.dev(tmp), U.dev(bias_in)
                _lib.call("t2s_wg_compose_cond", _lib.ptr(tmp_d), _lib.ptr(bias_d), rows, Mpad, P, K2, ld, _lib.ptr(out[0].t),
                          _lib.ptr(out[1].t), _lib.ptr(bias_out.t), _lib.current_stream())
                K._sync()
                _assert_planes_equal(label, out, want)
                if rows < Mpad:
                    for o in out:
                        assert float(o.t[:, :, rows:].float().abs().max()) == 0.0, label + ": padding rows"
                assert torch.equal(bias_out.t.cpu().view(torch.int32), want_b.view(torch.int32)), label + ": bias_out"
                bias_out.assert_guards(label)


# (B, n_mel, frames, nlag, Fp)
_MELWIN = [(3, 8, 5, 4, 5), (2, 16, 70, 2, 256), (1, 8, 1, 4, 64), (2, 5, 9, 4, 64), (1, 80, 3, 4, 256)]


@pytest.mark.parametrize("B,n_mel,frames,nlag,Fp", _MELWIN, ids=["B%d-M%d-F%d-lag%d-Fp%d" % c for c in _MELWIN])
def test_melwin_planes(B, n_mel, frames, nlag, Fp):
    """M[b][k / 32][f][k % 32] = mel[b][ci][f - j], k = j n_mel + ci: zeros in the first frames' lags, the tail lags of rows frames ..
    frames + nlag - 2 still the clip's last frames, zero behind them.  K2 = 20 (5 mels; the engine never passes it): the header sets
    no rule on K2 here, the entry point accepts it and writes ceil(K2 / 32) chunks with the columns past K2 zero."""
    _lib.load()
    K2 = nlag * n_mel
    mc = -(-K2 // 32)
    mel = torch.randn(B, n_mel, frames, generator=torch.Generator().manual_seed(frames + Fp))
    win = R.mel_windows(mel, nlag, Fp)
    want = R.m_planes(win, Fp)
    out = (K._BF(B, mc, Fp, 32), K._BF(B, mc, Fp, 32))
    for o in out:
        o.t.fill_(0.75)                 # every row of the planes is the kernel's to write
    mel_d = U.dev(mel)
    label = "melwin_planes B%d M%d frames %d nlag %d Fp %d" % (B, n_mel, frames, nlag, Fp)
    rc = _lib.load().t2s_wg_melwin_planes(_lib.ptr(mel_d), B, n_mel, frames, nlag, Fp, _lib.ptr(out[0].t), _lib.ptr(out[1].t),
                                          _lib.current_stream())
    assert rc == 0, label
    K._sync()
    _assert_planes_equal(label, out, want)
    got = R.m_decode(out[0].t, out[1].t, K2)
    # the edges, spelled out: lag j of row f is a frame of the clip (non-zero: randn) where 0 <= f - j < frames and zero elsewhere -
    # the leading zeros of rows 0 .. nlag - 2, the tail lags of rows frames .. frames + nlag - 2
    for f in range(min(frames + nlag - 1, Fp)):
        for j in range(nlag):
            v = got[:, j * n_mel:(j + 1) * n_mel, f].abs()
            if 0 <= f - j < frames:
                assert float(v.min()) > 0.0, (label, f, j)
            else:
                assert float(v.max()) == 0.0, (label, f, j)
    if frames + nlag - 1 < Fp:
        assert float(got[:, :, frames + nlag - 1:].abs().max()) == 0.0, label + ": rows behind the tail lags"
    if K2 % 32:
        for o in out:
            assert float(o.t[:, -1, :, K2 % 32:].float().abs().max()) == 0.0, label + ": columns past K2"
    # Fp below the frames is refused and writes nothing
    keep = [o.t.clone() for o in out]
    assert _lib.load().t2s_wg_melwin_planes(_lib.ptr(mel_d), B, n_mel, frames, nlag, frames - 1, _lib.ptr(out[0].t), _lib.ptr(out[1].t),
                                            _lib.current_stream()) == EINVAL
    K._sync()
    assert all(torch.equal(o.t, k) for o, k in zip(out, keep))


# ---------------------------------------------------------------------------------------------- (b) t2s_wg_in_melwin_gate_fold
# name, C, (n_mel, ksize, stride), B, L, Fp, dilation, fold_init, (ph_FT, ph_bper, ph_nft), fold slots
GATE_CASES = [
    ("ft64-ragged-batch", 48, (8, 256, 64), 5, 37, 256, 2, 1, (64, 4, 1), 2),       # second tile 1 of 4 entries, L % P != 0
    ("ft64-full", 48, (8, 256, 64), 4, 512, 64, 1, 0, (64, 4, 1), 2),               # a full tile, Fp == F, running sums
    ("ft128", 48, (16, 256, 128), 3, 1590, 256, 4, 1, (128, 2, 1), 2),              # odd batch
    ("ft256-two-tiles", 48, (8, 256, 64), 2, 2053, 257, 1, 1, (256, 1, 2), 2),      # second tile one frame, Fp == F
    ("two-k-chunks", 80, (16, 256, 64), 2, 300, 256, 2, 0, (64, 4, 1), 2),          # K2 / 32 = 2, C past one 64-group
    ("two-m-tiles", 160, (8, 256, 64), 2, 560, 256, 8, 1, (128, 2, 1), 4),          # n_mtiles 2
    ("by-grid-size", 128, (8, 256, 64), 5, 6660, 1024, 1, 1, (256, 1, 4), 2),       # 256-row tiles because the grid is large
]


def phase_tiles(L, P):
    """(ph_FT, ph_bper, ph_nft) of t2s_wg_in_melwin_gate_fold for L columns in P phases (text2speech_amd/csrc/t2s_api.hip)"""
    nF = -(-L // P)
    FT = 64 if nF <= 64 else (128 if nF <= 128 else 256)
    return FT, 256 // FT, -(-nF // FT)


_cases = {}


def _gate_setup(C, geom, B, L, dil):
    """the float64 case (compose_ref.gate_case) and the same seeded WN with its packed operands: computed once, never modified"""
    key = (C, geom, B, L, dil)
    if key not in _cases:
        if len(_cases) >= 3:
            _cases.pop(next(iter(_cases)))
        i = int(math.log2(dil))
        assert 2 ** i == dil
        nl = max(i + 1, 2)
        cs = R.gate_case(C, *geom, G8, B, L, nl)
        wn = K._WN(C, nl, R.WN_KS, R.WN_NH, cs["n_cond"], seed=R.wn_seed(C, nl))
        assert all(torch.equal(wn.sd[k], v) for k, v in cs["sd"].items())
        _cases[key] = (cs, wn, i)
    return _cases[key]


def _host_operands(cs, wn, i, Fp):
    """(A2 planes, composed bias, M planes) of layer i on the device, laid out on the host from float64"""
    _, A2, b = R.gate_operands(cs, i)
    A2p = tuple(U.dev(p) for p in R.a2_planes(A2, wn.C, wn.Mpad1))
    Mp = tuple(U.dev(p) for p in R.m_planes(R.mel_windows(cs["mel"], cs["nlag"], Fp), Fp))
    return A2p, U.dev(R.bias_rows(b, wn.C, wn.Mpad1)), Mp


def _run_gate(label, cs, wn, i, A2p, b1c, Mp, Fp, fold_init, nslots):
    """One launch on the oracle's x_i as planes.  fold_init = 1: fold_acc full of the NaN sentinel; 0: seeded previous contents."""
    B, C, L = cs["B"], wn.C, cs["L"]
    Lp = _lib.plane_rows(L, HALO)
    xc = -(-C // 32)
    Xp = planes.to_planes(U.dev(cs["layers"][i]["x"].float()), HALO, Lp)
    Ah, Al, _ = wn.gate(i)
    fold_A = wn.fold(i)[0]
    out = K._plane_pair(B, xc, Lp)
    prev = None
    if not fold_init:
        prev = 0.1 * torch.randn(nslots, B, 8, L, generator=torch.Generator().manual_seed(L + nslots))
    fold_acc = U.Guarded(nslots, B, 8, L, fill=None if prev is None else U.dev(prev))
    _lib.call("t2s_wg_in_melwin_gate_fold", _lib.ptr(Ah), _lib.ptr(Al), _lib.ptr(A2p[0]), _lib.ptr(A2p[1]), _lib.ptr(b1c),
              _lib.ptr(Xp[0]), _lib.ptr(Xp[1]), _lib.ptr(Mp[0]), _lib.ptr(Mp[1]), _lib.ptr(out[0].t), _lib.ptr(out[1].t),
              _lib.ptr(fold_A), _lib.ptr(fold_acc.t), fold_init, B, C, cs["K2"], R.WN_KS, 2 ** i, L, Lp, HALO, wn.Mpad1, cs["P"], Fp,
              _lib.current_stream())
    K._sync()
    return out, fold_acc, prev


def _check_gate(label, cs, wn, i, out, fold_acc, prev):
    """acts planes against the oracle's acts_i, the sum of fold_acc over its slots (less the seeded previous contents) against the
    oracle's F_i . acts_i; halo rows, rows >= L and channels past C zero; guards intact.  Returns the four error figures."""
    C, L = wn.C, cs["L"]
    ly = cs["layers"][i]
    fl_a, fl_f = R.gate_floor(cs, i)
    bars = K._fold_bars(fl_a)           # the case's floor is the gate's; the fold product's own is printed beside it
    print("PARITY %-60s norm-rel %.3e  max-rel %.3e  -> bars %.1e / %.1e" % (label + " FLOOR", *fl_a, *bars))
    print("INFO   %-60s norm-rel %.3e  max-rel %.3e" % (label + " fold floor", *fl_f))
    pair = (out[0].t, out[1].t)
    ea = U.check(label + " acts", U.plane_values(pair, C, L, HALO), ly["acts"], *bars)
    U.assert_halo_zero(pair, L, HALO, label)
    for p in out:
        if C % 32:
            assert float(p.t[:, -1, :, C % 32:].float().abs().max()) == 0.0, label + ": channels past C were written"
        p.assert_guards(label)
    fsum = fold_acc.t.double().sum(0).cpu()          # NaN if any element of any slot was not written
    if prev is not None:
        fsum = fsum - prev.double().sum(0)
    ef = U.check(label + " fold (sum over %d slots)" % fold_acc.t.size(0), fsum, ly["fold"], *bars)
    fold_acc.assert_guards(label)
    return ea + ef


@pytest.mark.parametrize("name,C,geom,B,L,Fp,dil,fold_init,tiles,nslots", GATE_CASES, ids=[c[0] for c in GATE_CASES])
def test_in_melwin_gate_fold(name, C, geom, B, L, Fp, dil, fold_init, tiles, nslots):
    """t2s_wg_in_melwin_gate_fold on host-built A2, bias and M (compose_ref, float64) and the engine's packed in-layer weights, at the
    phase-tile packings the ids name: 64- and 128-frame tiles with several batch entries in one column tile, a batch that does not
    fill its last tile, L % P != 0, Fp == F, fold_init = 0, two K-chunks of the mel window, two M tiles, four frame tiles."""
    K._assert_tiles(B, C, L, 256, nslots)
    P = geom[2] // G8
    assert phase_tiles(L, P) == tiles and Fp >= -(-L // P)
    cs, wn, i = _gate_setup(C, geom, B, L, dil)
    label = "melwin %s B%d C%d L%d P%d K2 %d d%d" % (name, B, C, L, P, cs["K2"], dil)
    A2p, b1c, Mp = _host_operands(cs, wn, i, Fp)
    out, fold_acc, prev = _run_gate(label, cs, wn, i, A2p, b1c, Mp, Fp, fold_init, nslots)
    _check_gate(label, cs, wn, i, out, fold_acc, prev)


def test_in_melwin_gate_fold_validation():
    """T2S_EINVAL with nothing launched - real pointers, the outputs' sentinels stay - for K2 % 32 != 0, P <= 0, Fp below ceil(L / P)
    and a shape whose tile height is 128 rows; the tuple the broken ones are made from is itself accepted (zero operands)."""
    lib = _lib.load()
    Pt = _lib.ptr
    B, C, K2, L, P, Fp = 1, 48, 32, 300, 8, 64
    Lp = _lib.plane_rows(L, HALO)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    A = torch.zeros(3 * 2 + 1, 256, 32, **bf)
    A2 = torch.zeros(P, 1, 256, 32, **bf)
    bias = torch.zeros(256, device=DEV)
    Xp, Mp = torch.zeros(B, 2, Lp, 32, **bf), torch.zeros(B, 1, Fp, 32, **bf)
    fold_A = torch.zeros(8192, **bf)
    SENT = 0.375
    outs = [torch.full((B, 2, Lp, 32), SENT, **bf) for _ in range(2)]
    acc = U.Guarded(2, B, 8, L)

    def call(**ch):
        a = dict(A_hi=Pt(A), A_lo=Pt(A), A2_hi=Pt(A2), A2_lo=Pt(A2), bias=Pt(bias), X_hi=Pt(Xp), X_lo=Pt(Xp), M_hi=Pt(Mp), M_lo=Pt(Mp),
                 acts_hi=Pt(outs[0]), acts_lo=Pt(outs[1]), fold_A=Pt(fold_A), fold_acc=Pt(acc.t), fold_init=1, B=B, C=C, K2=K2, taps=3,
                 dilation=1, L=L, Lp=Lp, halo=HALO, Mpad=256, P=P, Fp=Fp, stream=_lib.current_stream())
        a.update(ch)
        return lib.t2s_wg_in_melwin_gate_fold(*a.values())

    assert -(-L // P) == 38 and lib.t2s_wg_gate_tile_rows(1, 64, 300) == 128 and lib.t2s_wg_gate_tile_rows(B, C, L) == 256
    for ch in (dict(K2=20), dict(K2=48), dict(K2=0), dict(P=0), dict(P=-1), dict(Fp=37), dict(C=64)):
        assert call(**ch) == EINVAL, "accepted %r" % (ch,)
        K._sync()
        assert all(bool((o == SENT).all()) for o in outs) and bool(acc.untouched(acc.t).all()), "wrote something with %r" % (ch,)
    assert call() == 0 and call(Fp=38) == 0
    K._sync()
    assert not bool(acc.untouched(acc.t).any())
    acc.assert_guards("validation")


# ---------------------------------------------------------------------------------------------- (d) the weight chain, end to end
# C, (n_mel, ksize, stride), B, L, Fp, dilation, fold slots: the first is GATE_CASES' ft64-ragged-batch; the table has no case with
# C = 80 on the (16, 256, 128) upsampler, so the second is two-k-chunks' shape on that geometry (P 16, K2 32, 19 frames)
_CHAIN = [(48, (8, 256, 64), 5, 37, 256, 2, 2), (80, (16, 256, 128), 2, 300, 256, 2, 2)]


@pytest.mark.parametrize("C,geom,B,L,Fp,dil,nslots", _CHAIN, ids=["C48-8-256-64", "C80-16-256-128"])
def test_weight_chain_end_to_end(C, geom, B, L, Fp, dil, nslots):
    """The one test that feeds a kernel's output to the next: t2s_wg_upsample_basis -> t2s_conv_bias_act on the conditioning
    K-chunks of the packed gate weights -> t2s_wg_compose_cond, as WaveGlow's engine chains them (glow.py, compose_cond).  The
    planes and the bias it leaves are read back (compose_ref's decode) and compared with compose_ref.composed at the GEMM bars,
    then exactly these planes go to t2s_wg_in_melwin_gate_fold with the outputs held to what the host-built case is held to."""
    K._assert_tiles(B, C, L, 256, nslots)
    n_mel, ksize, stride = geom
    cs, wn, i = _gate_setup(C, geom, B, L, dil)
    P, K2 = cs["P"], cs["K2"]
    label = "chain C%d %d-%d-%d" % ((C,) + geom)
    st = _lib.current_stream()
    ncols = P * K2 + 1
    sc, Lp_u = wn.Spad // 32, _lib.plane_rows(ncols, 0)
    Up = K._plane_pair(1, sc, Lp_u)
    W_d, b_d = U.dev(cs["W_up"].float()), U.dev(cs["b_up"].float())
    _lib.call("t2s_wg_upsample_basis", _lib.ptr(W_d), _lib.ptr(b_d), n_mel, ksize, stride, G8, Lp_u, 0, _lib.ptr(Up[0].t),
              _lib.ptr(Up[1].t), st)
    Ah, Al, b1 = wn.gate(i)
    cond_off = (wn.ks * wn.Cpad // 32) * wn.Mpad1 * 32 * 2          # bytes: the conditioning K-chunks of the packed gate weights
    tmp = U.Guarded(2 * C, ncols)
    zb = torch.zeros(wn.Mpad1, device=DEV)
    _lib.call("t2s_conv_bias_act", _lib.c_vp(Ah.data_ptr() + cond_off), _lib.c_vp(Al.data_ptr() + cond_off), _lib.ptr(zb),
              _lib.ptr(Up[0].t), _lib.ptr(Up[1].t), None, None, _lib.ptr(tmp.t), 0, 1, cs["n_cond"], 2 * C, 1, 1, 0, ncols, Lp_u, 0,
              wn.Mpad1, st)
    A2o = (K._BF(P, K2 // 32, wn.Mpad1, 32), K._BF(P, K2 // 32, wn.Mpad1, 32))
    b1c = U.Guarded(wn.Mpad1)
    _lib.call("t2s_wg_compose_cond", _lib.ptr(tmp.t), _lib.ptr(b1), 2 * C, wn.Mpad1, P, K2, ncols, _lib.ptr(A2o[0].t),
              _lib.ptr(A2o[1].t), _lib.ptr(b1c.t), st)
    K._sync()
    for g in Up + A2o + (tmp, b1c):
        g.assert_guards(label)
    _, A2, b = R.gate_operands(cs, i)
    U.check(label + " A2", R.a2_decode(A2o[0].t, A2o[1].t, C), A2, U.GEMM_NORM, U.GEMM_MAX)
    U.check(label + " composed bias", R.bias_decode(b1c.t, C), b, U.GEMM_NORM, U.GEMM_MAX)
    if 2 * C < wn.Mpad1:
        assert float(A2o[0].t[:, :, 2 * C:].float().abs().max()) == 0.0 and float(A2o[1].t[:, :, 2 * C:].float().abs().max()) == 0.0
    Mp = tuple(U.dev(p) for p in R.m_planes(R.mel_windows(cs["mel"], cs["nlag"], Fp), Fp))
    out, fold_acc, prev = _run_gate(label, cs, wn, i, (A2o[0].t, A2o[1].t), b1c.t, Mp, Fp, 1, nslots)
    _check_gate(label + " gate", cs, wn, i, out, fold_acc, prev)


# ---------------------------------------------------------------------------------------------- t2s_wg_upsample_squeeze, bf16
# (n_mel, ksize, stride), B, L, mel frames beyond ceil(8 L / stride); the vector kernel, then the matrix-core kernel (n_group 8,
# ksize = 4 stride, stride % 64 == 0, n_mel % 4 == 0)
_UPSQ = [
    ("vec", (5, 32, 8), 2, 300, 5),             # more mel frames than L needs; 40 of 64 channels
    ("vec", (5, 32, 8), 1, 1, 0),
    ("vec", (5, 32, 8), 9, 70, 0),              # B = 9 crosses the batch block of 8
    ("mfma", (4, 256, 64), 2, 300, 0),
    ("mfma", (4, 256, 64), 1, 1, 0),
    ("mfma", (36, 256, 64), 3, 40, 0),          # 9 (position block, chunk) pairs: one past the 8 XCD slots, the others return early
    ("mfma", (8, 512, 128), 2, 257, 0),         # two position blocks per hop
]


@pytest.mark.parametrize("kind,geom,B,L,extra", _UPSQ, ids=["%s-%d-%d-%d-B%d-L%d" % ((c[0],) + c[1] + c[2:4]) for c in _UPSQ])
def test_upsample_squeeze_bf16(kind, geom, B, L, extra):
    """t2s_wg_upsample_squeeze against compose_ref.upsample_squeezed (F.conv_transpose1d, float64) at the GEMM bars: halo rows, rows
    >= L and channels past n_mel * 8 zero, guards intact."""
    _lib.load()
    n_mel, ksize, stride = geom
    assert (kind == "mfma") == (ksize == 4 * stride and stride % 64 == 0 and n_mel % 4 == 0)
    frames = -(-G8 * L // stride) + extra
    W, bias = _upsampler(n_mel, ksize, stride, seed=n_mel + L)
    mel = torch.randn(B, n_mel, frames, generator=torch.Generator().manual_seed(B + L))
    want = R.upsample_squeezed(mel, W, bias, stride, G8, L)
    n_chan = n_mel * G8
    Lp = _lib.plane_rows(L, HALO)
    out = K._plane_pair(B, -(-n_chan // 32), Lp)
    mel_d, W_d, bias_d = U.dev(mel), U.dev(W), U.dev(bias)
    label = "upsample_squeeze %s %d-%d-%d B%d L%d frames %d" % (kind, n_mel, ksize, stride, B, L, frames)
    _lib.call("t2s_wg_upsample_squeeze", _lib.ptr(mel_d), _lib.ptr(W_d), _lib.ptr(bias_d), B, n_mel, frames, ksize, stride, G8, L, Lp,
              HALO, _lib.ptr(out[0].t), _lib.ptr(out[1].t), _lib.current_stream())
    K._sync()
    pair = (out[0].t, out[1].t)
    U.check(label, U.plane_values(pair, n_chan, L, HALO), want, U.GEMM_NORM, U.GEMM_MAX)
    U.assert_halo_zero(pair, L, HALO, label)
    for p in out:
        if n_chan % 32:
            assert float(p.t[:, -1, :, n_chan % 32:].float().abs().max()) == 0.0, label + ": channels past n_mel * 8 were written"
        p.assert_guards(label)
