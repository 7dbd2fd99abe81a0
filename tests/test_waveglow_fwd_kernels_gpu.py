"""The GEMM kernels of the WaveGlow forward that the no-grad path and the training forward launch, one by one through the C entry
points, against float64 (oracle.waveglow_oracle.wn_forward through tests/wg_fwd_util.py, which tests/test_wg_fwd_util_cpu.py pins):

  t2s_wg_in_cond_gate_fold(_train)   acts (and sigmoid) planes, and WN.end folded into the epilogue: fold_acc[slot][b][j][t]
  t2s_wg_in_win_gate_fold            the same for layer 0 through the window planes of the folded WN.start
  t2s_wg_res_only(_train / _start)   x + W_res . acts + b
  t2s_wg_end_fold_affine             WN.end from the folded sums and the affine coupling, forward and reverse

Every kernel reads the ORACLE's input of that kernel, rounded to planes (planes.to_planes), never another kernel's output; the
weights come from the engine's own pack entry points (tests/test_weight_prep_kernels_gpu.py, tests/test_start_fold_gpu.py and
tests/test_waveglow_gpu.py test those).  Layer i of the oracle has dilation 2^i, so a case with dilation d runs layer log2(d).
Each gate case first asserts the tile height (256-row ping-pong kernel of csrc/gate_gemm_pp.hip or the 128-row tiles of
csrc/conv_gemm.hip) and the slot count it was written for.  Of fold_acc only the sum over the slots is contract.

Bars are tests/wg_bwd_util.py's: GEMM_* for plane outputs and for the fold product (the same three-product arithmetic, f32
accumulation, K = C <= 512), F32_* for the coupling.  The fold product's own floor (U.split3_floor of fold_A's values and the
oracle's acts as planes hold them: no output of the code under test) is printed with every fold case; a case whose floor exceeds
a quarter of a bar takes 4 x its floor as that bar (_fold_bars: none does - the floors are 1.2e-6 .. 3.7e-6 norm-relative and
1.1e-6 .. 3.8e-6 max-relative against quarter bars of 5e-6 and 2.5e-5, and the kernels' fold sums sit on their floors;
profiles/waveglow_fwd_kernel_tests.md has every figure)."""
import functools
import math

import pytest
import torch

import wg_bwd_util as U
import wg_fwd_util as W
from text2speech_amd import _lib, planes

pytestmark = pytest.mark.gpu

DEV = U.DEV
HALO = 128
G8 = 8                  # n_group of every z in this file
PAD = 1024              # bf16 elements in front of and behind every plane output
_GUARD_BF = -1.5        # what those hold


class _BF:
    """A bf16 device buffer of `shape`, zeroed, with PAD elements of _GUARD_BF either side; `.t` is the buffer (16-byte aligned)."""

    def __init__(self, *shape):
        self.n = math.prod(shape)
        self.raw = torch.full((self.n + 2 * PAD,), _GUARD_BF, dtype=torch.bfloat16, device=DEV)
        self.t = self.raw[PAD:PAD + self.n].view(*shape)
        self.t.zero_()

    def assert_guards(self, label):
        assert bool((self.raw[:PAD] == _GUARD_BF).all()), "%s: wrote in front of the output" % label
        assert bool((self.raw[PAD + self.n:] == _GUARD_BF).all()), "%s: wrote behind the output" % label


def _plane_pair(B, nc, Lp, src=None):
    """two guarded plane buffers [B, nc, Lp, 32], optionally holding a copy of the (hi, lo) pair src"""
    pair = (_BF(B, nc, Lp, 32), _BF(B, nc, Lp, 32))
    if src is not None:
        pair[0].t.copy_(src[0])
        pair[1].t.copy_(src[1])
    return pair


def _f32(t):
    return None if t is None else U.dev(t.to(torch.float32))


def _sync():
    torch.cuda.synchronize()


def _pack_table(jobs):
    """t2s_pack_conv_weight_table over jobs (v, g, bias_in, bias_in2, A_hi, A_lo, bias_out, O, Cin, Kt, perm, C_gate, Mpad, koff,
    Cin_pad, scale_out), laid out as text2speech_amd/glow.py lays them out"""
    dp = lambda t: 0 if t is None else t.data_ptr()
    rows, row_start = [], 0
    for (v, g, b1, b2, Ah, Al, bo, O_, Cin, Kt, perm, Cg, Mpad, koff, Cin_pad, so) in jobs:
        rows.append([dp(v), dp(g), dp(b1), dp(b2), dp(Ah), dp(Al), dp(bo), row_start, O_, Cin, Kt, perm, Cg, Mpad, koff, Cin_pad, 0, 0, dp(so)])
        row_start += -(-O_ // 16)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    _lib.call("t2s_pack_conv_weight_table", _lib.ptr(table), len(rows), row_start, _lib.current_stream())
    _sync()


class _WN:
    """One seeded WN (wg_fwd_util.wn_state) and its packed operands, built on demand with the engine's own entry points."""

    def __init__(self, C, nl, ks, nh, n_cond, seed, bias_shift=None):
        self.C, self.nl, self.ks, self.nh, self.n_cond = C, nl, ks, nh, n_cond
        self.sd = W.wn_state(C, nl, ks, nh, n_cond, seed)
        if bias_shift is not None:          # (layer, [(gate row, shift)])
            i, shifts = bias_shift
            for o, s in shifts:
                self.sd["WN.0.in_layers.%d.bias" % i][o] += s
        self.cfg = W.wn_cfg(C, nl, ks)
        self.Cpad, self.Spad = -(-C // 32) * 32, -(-n_cond // 32) * 32
        self.Mpad1 = -(-C // 128) * 256
        self.d = {k: _f32(v.flatten() if k.endswith("weight_g") else v) for k, v in self.sd.items()}

    def p(self, name):
        return self.d["WN.0." + name]

    def _zeros_bf(self, *shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device=DEV)

    @functools.lru_cache(maxsize=None)
    def gate(self, i):
        """(A1h, A1l, b1) of layer i: in_layers[i] then cond_layers[i] along K, T2S_PERM_GATE rows, the two biases added"""
        C, ks = self.C, self.ks
        nk1 = ks * self.Cpad // 32 + self.Spad // 32
        Ah, Al, b1 = self._zeros_bf(nk1, self.Mpad1, 32), self._zeros_bf(nk1, self.Mpad1, 32), torch.zeros(self.Mpad1, device=DEV)
        li, lc = "in_layers.%d." % i, "cond_layers.%d." % i
        jobs = [(self.p(li + "weight_v"), self.p(li + "weight_g"), self.p(li + "bias"), self.p(lc + "bias") if self.n_cond else None,
                 Ah, Al, b1, 2 * C, C, ks, 1, C, self.Mpad1, 0, self.Cpad, None)]
        if self.n_cond:
            jobs.append((self.p(lc + "weight_v"), self.p(lc + "weight_g"), None, None, Ah, Al, None, 2 * C, self.n_cond, 1, 1, C,
                         self.Mpad1, ks * self.Cpad, self.Spad, None))
        _pack_table(jobs)
        return Ah, Al, b1

    @functools.lru_cache(maxsize=None)
    def res(self, i, pair8):
        """(A2h, A2l, b2, Mpad2, scale) of res_skip_layers[i]; pair8: the residual rows in the T2S_PERM_PAIR8 order"""
        C = self.C
        rows2 = 2 * C if i < self.nl - 1 else C
        Mpad2 = _lib.padded_rows(rows2)
        Ah, Al, b2 = self._zeros_bf(self.Cpad // 32, Mpad2, 32), self._zeros_bf(self.Cpad // 32, Mpad2, 32), torch.zeros(Mpad2, device=DEV)
        s_rs = torch.empty(rows2, device=DEV)
        lr = "res_skip_layers.%d." % i
        _pack_table([(self.p(lr + "weight_v"), self.p(lr + "weight_g"), self.p(lr + "bias"), None, Ah, Al, b2, rows2, C, 1,
                      2 if pair8 else 0, C if pair8 else 0, Mpad2, 0, self.Cpad, s_rs)])
        return Ah, Al, b2, Mpad2, s_rs

    @functools.lru_cache(maxsize=None)
    def fold(self, i):
        """(fold_A, bes [8]) of layer i from t2s_wg_endfold_weights, with the scales the pack wrote"""
        C = self.C
        s_rs = self.res(i, False)[4]
        r0 = C if i < self.nl - 1 else 0
        lr = "res_skip_layers.%d." % i
        w_end = self.p("end.weight").view(2 * self.nh, C)
        fold_A = self._zeros_bf(-(-C // 128) * 8192)
        bes = torch.zeros(8, device=DEV)
        table = torch.tensor([[w_end.data_ptr(), self.p(lr + "weight_v").data_ptr() + 4 * r0 * C, s_rs.data_ptr() + 4 * r0,
                               self.p(lr + "bias").data_ptr() + 4 * r0, fold_A.data_ptr(), bes.data_ptr(), 2 * self.nh, C]],
                             dtype=torch.int64).to(DEV)
        _lib.call("t2s_wg_endfold_weights", _lib.ptr(table), 1, C, _lib.current_stream())
        _sync()
        return fold_A, bes

    @functools.lru_cache(maxsize=None)
    def w_start(self):
        w = torch.empty(self.C, self.nh, device=DEV)
        _lib.call("t2s_weightnorm_small", _lib.ptr(self.p("start.weight_v")), _lib.ptr(self.p("start.weight_g")), self.C, self.nh,
                  _lib.ptr(w), _lib.current_stream())
        _sync()
        return w

    @functools.lru_cache(maxsize=None)
    def win_gate(self, nwc):
        """(A0h, A0l, b1) of layer 0 through the folded WN.start: the composed block, then the conditioning weights"""
        C = self.C
        nk = nwc + self.Spad // 32
        Ah, Al, b1 = self._zeros_bf(nk, self.Mpad1, 32), self._zeros_bf(nk, self.Mpad1, 32), torch.zeros(self.Mpad1, device=DEV)
        _lib.call("t2s_wg_startfold_weights", _lib.ptr(self.p("in_layers.0.weight_v")), _lib.ptr(self.p("in_layers.0.weight_g")),
                  _lib.ptr(self.w_start()), _lib.ptr(self.p("start.bias")), C, self.nh, self.ks, self.Mpad1, nwc, _lib.ptr(Ah),
                  _lib.ptr(Al), _lib.current_stream())
        _pack_table([(self.p("cond_layers.0.weight_v"), self.p("cond_layers.0.weight_g"), self.p("in_layers.0.bias"),
                      self.p("cond_layers.0.bias"), Ah, Al, b1, 2 * C, self.n_cond, 1, 1, C, self.Mpad1, 32 * nwc, self.Spad, None)])
        return Ah, Al, b1


@functools.lru_cache(maxsize=4)
def _case(C, nl, ks, nh, n_cond, B, L, bias_shift=None):
    """the seeded WN of a shape, its inputs and the oracle's per-layer expectation: computed once, shared, never modified"""
    wn = _WN(C, nl, ks, nh, n_cond, seed=1000 * C + 10 * nl + ks + nh, bias_shift=bias_shift)
    audio, spect = W.wn_inputs(B, nh, n_cond, L, seed=L + 7 * B)
    layers, out = W.layer_expect(wn.sd, wn.cfg, audio, spect)
    return wn, audio, spect, layers, out


def _fold_bars(floor):
    """GEMM bars of a fold case: the project's, unless the arithmetic's own floor exceeds a quarter of one - then 4 x that floor"""
    fn, fm = floor
    return (U.GEMM_NORM if fn <= U.GEMM_NORM / 4 else 4 * fn), (U.GEMM_MAX if fm <= U.GEMM_MAX / 4 else 4 * fm)


def _assert_tiles(B, C, L, tile, nslots):
    lib = _lib.load()
    assert lib.t2s_wg_gate_tile_rows(B, C, L) == tile, "the tile-height rule moved this case off the %d-row kernel" % tile
    assert lib.t2s_wg_gate_fold_slots(B, C, L) == nslots, (lib.t2s_wg_gate_fold_slots(B, C, L), nslots)


def _slice_ptr(buf, first, Lp):
    """pointer to chunk `first` of batch entry 0 of a plane buffer [B, chunks, Lp, 32]"""
    return _lib.c_vp(buf.t.data_ptr() + 2 * first * Lp * 32)


_NEIGHBOUR = 1.5        # what the neighbouring layers' chunks of a wide plane set hold


class _ActPlanes:
    """The acts (and, training, sigmoid) outputs of a gate launch: guarded planes of xc chunks, or - wide - the middle third of a
    plane set of 3 xc chunks per batch entry whose other chunks must stay as they are."""

    def __init__(self, B, xc, Lp, train, wide):
        self.xc, self.Lp, self.wide = xc, Lp, wide
        self.first = xc if wide else 0
        self.bchunks = 3 * xc if wide else 0
        n = 4 if train else 2
        self.bufs = [_BF(B, 3 * xc if wide else xc, Lp, 32) for _ in range(n)]
        if wide:
            for b in self.bufs:
                b.t[:, :xc] = _NEIGHBOUR
                b.t[:, 2 * xc:] = _NEIGHBOUR

    def ptrs(self):
        return [_slice_ptr(b, self.first, self.Lp) for b in self.bufs]

    def acts(self):
        return self.bufs[0].t[:, self.first:self.first + self.xc], self.bufs[1].t[:, self.first:self.first + self.xc]

    def sig(self):
        return self.bufs[2].t[:, self.first:self.first + self.xc], self.bufs[3].t[:, self.first:self.first + self.xc]

    def check_frame(self, C, L, label):
        """halo rows, rows t >= L and channels [C, Cpad) zero; the neighbours and the guards untouched"""
        pairs = [self.acts()] + ([self.sig()] if len(self.bufs) == 4 else [])
        for pair in pairs:
            U.assert_halo_zero(pair, L, HALO, label)
            if C % 32:
                for p in pair:
                    assert float(p[:, -1, :, C % 32:].float().abs().max()) == 0.0, label + ": channels past C were written"
        for b in self.bufs:
            b.assert_guards(label)
            if self.wide:
                assert bool((b.t[:, :self.xc] == _NEIGHBOUR).all()) and bool((b.t[:, 2 * self.xc:] == _NEIGHBOUR).all()), \
                    label + ": a neighbouring layer's chunks changed"


def _launch_cond(wn, i, Xp, Sp, out, fold_acc, fold_init, B, L, Lp, train):
    Ah, Al, b1 = wn.gate(i)
    fold_A = wn.fold(i)[0]
    S = (None, None) if Sp is None else (_lib.ptr(Sp[0]), _lib.ptr(Sp[1]))
    o = out.ptrs()
    tail = (_lib.ptr(fold_A), _lib.ptr(fold_acc.t), fold_init, B, wn.C, wn.n_cond, wn.ks, 2 ** i, L, Lp, HALO, wn.Mpad1,
            _lib.current_stream())
    if train:
        _lib.call("t2s_wg_in_cond_gate_fold_train", _lib.ptr(Ah), _lib.ptr(Al), _lib.ptr(b1), _lib.ptr(Xp[0]), _lib.ptr(Xp[1]), S[0],
                  S[1], o[0], o[1], o[2], o[3], out.bchunks, *tail)
    else:
        _lib.call("t2s_wg_in_cond_gate_fold", _lib.ptr(Ah), _lib.ptr(Al), _lib.ptr(b1), _lib.ptr(Xp[0]), _lib.ptr(Xp[1]), S[0], S[1],
                  o[0], o[1], *tail)
    _sync()


def _z_with(audio, c_off, seed):
    """f32 device z [B, 8, L]: the audio channels at c_off, seeded noise everywhere else"""
    B, nh, L = audio.shape
    z = torch.randn(B, G8, L, generator=torch.Generator().manual_seed(seed))
    z[:, c_off:c_off + nh] = audio.float()
    return U.dev(z)


def _launch_win(wn, nwc, audio, c_off, Sp, out, fold_acc, fold_init, B, L, Lp):
    """the window planes by t2s_wg_start_window from the oracle's audio, then t2s_wg_in_win_gate_fold"""
    C = wn.C
    z = _z_with(audio, c_off, seed=L)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    Xh, Xl = torch.zeros(B, wn.Cpad // 32, Lp, 32, **bf), torch.zeros(B, wn.Cpad // 32, Lp, 32, **bf)
    Wh, Wl = torch.zeros(B, nwc, Lp, 32, **bf), torch.zeros(B, nwc, Lp, 32, **bf)
    st = _lib.current_stream()
    _lib.call("t2s_wg_start_window", _lib.ptr(z), _lib.ptr(wn.w_start()), _lib.ptr(wn.p("start.bias")), B, G8, c_off, wn.nh, C, L, Lp,
              HALO, _lib.ptr(Xh), _lib.ptr(Xl), wn.ks, nwc, _lib.ptr(Wh), _lib.ptr(Wl), st)
    Ah, Al, b1 = wn.win_gate(nwc)
    o = out.ptrs()
    _lib.call("t2s_wg_in_win_gate_fold", _lib.ptr(Ah), _lib.ptr(Al), _lib.ptr(b1), _lib.ptr(Wh), _lib.ptr(Wl), _lib.ptr(Sp[0]),
              _lib.ptr(Sp[1]), o[0], o[1], _lib.ptr(wn.fold(0)[0]), _lib.ptr(fold_acc.t), fold_init, B, C, wn.n_cond, nwc, L, Lp, HALO,
              wn.Mpad1, st)
    _sync()


def _check_gate_outputs(label, wn, i, layers, out, fold_acc, L, train, before=None):
    """The assertions on one gate launch of layer i.  Returns the float64 fold product of what fold_A and the acts planes hold
    (plus `before`, the products of the launches this one accumulated on)."""
    C, nh = wn.C, wn.nh
    assert bool(torch.isfinite(out.acts()[0].float()).all()) and bool(torch.isfinite(out.acts()[1].float()).all()), label
    got = U.plane_values(out.acts(), C, L, HALO)
    U.check(label + " acts", got, layers[i]["acts"], U.GEMM_NORM, U.GEMM_MAX)
    if train:
        U.check(label + " sigmoid", U.plane_values(out.sig(), C, L, HALO), layers[i]["sig"], U.GEMM_NORM, U.GEMM_MAX)
    out.check_frame(C, L, label)
    # the fold: the sum over the slots against fold_A's values times the acts planes' values
    Fd = W._endfold_decode(wn.fold(i)[0], C)[:8, :C]
    assert float(Fd[2 * nh:].abs().max()) == 0.0 if nh < 4 else True
    want = torch.einsum("jc,bct->bjt", Fd, got)
    if before is not None:
        want = want + before
    floor = U.split3_floor(Fd[:2 * nh], W.plane_round(layers[i]["acts"]), "jc,bct->bjt")
    nb, mb = _fold_bars(floor)
    print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e  -> bars %.1e / %.1e" % (label + " fold", floor[0], floor[1], nb, mb))
    fsum = fold_acc.t.double().sum(0).cpu()         # NaN if any element of any slot was not written
    U.check(label + " fold (sum over %d slots)" % fold_acc.t.size(0), fsum[:, :2 * nh], want[:, :2 * nh], nb, mb)
    if before is None:      # beside it, not asserted: the same sum against the oracle's own F_i . acts_i (weights and acts unrounded)
        print("INFO   %-60s norm-rel %.3e  max-rel %.3e" % (label + " fold vs oracle", U.rel(fsum[:, :2 * nh], layers[i]["fold"]),
                                                            U.maxrel(fsum[:, :2 * nh], layers[i]["fold"])))
    if nh < 4:
        assert float(fsum[:, 2 * nh:].abs().max()) == 0.0, label + ": fold rows j >= 2 n_half are not zero"
    fold_acc.assert_guards(label)
    return want


def _gate_case(label, kind, B, C, n_cond, L, ks, i, tile, nh=4, c_off=0, nwc=None, train=False, wide=False, bias_shift=None):
    """One gate case: the launch under test with fold_init = 1 on a fold_acc full of the NaN sentinel, every assertion of
    _check_gate_outputs, then another layer's launch with fold_init = 0 on top and the float64 sum of both products."""
    _lib.load()
    xc = -(-C // 32)
    nslots = 2 * (C // 64) if tile == 128 else 2 * (-(-C // 128))
    _assert_tiles(B, C, L, tile, nslots)
    nl = max(i + 1, 2)
    wn, audio, spect, layers, _ = _case(C, nl, ks, nh, n_cond, B, L, bias_shift)
    Lp = _lib.plane_rows(L, HALO)
    Sp = planes.to_planes(U.dev(spect.float()), HALO, Lp) if n_cond else None
    fold_acc = U.Guarded(nslots, B, 8, L)           # exactly [nslots][B][8][L]: a store at t >= L lands in a neighbour or a guard
    out = _ActPlanes(B, xc, Lp, train, wide)
    if kind == "win":
        _launch_win(wn, nwc, audio, c_off, Sp, out, fold_acc, 1, B, L, Lp)
    else:
        Xp = planes.to_planes(U.dev(layers[i]["x"].float()), HALO, Lp)
        _launch_cond(wn, i, Xp, Sp, out, fold_acc, 1, B, L, Lp, train)
    first = _check_gate_outputs(label, wn, i, layers, out, fold_acc, L, train)
    # a second layer on top (fold_init = 0): the oracle's input of that layer, its weights, its dilation
    j = i - 1 if i > 0 else 1
    Xp = planes.to_planes(U.dev(layers[j]["x"].float()), HALO, Lp)
    _launch_cond(wn, j, Xp, Sp, out, fold_acc, 0, B, L, Lp, train)
    _check_gate_outputs(label + " + layer %d" % j, wn, j, layers, out, fold_acc, L, train, before=first)


# ---------------------------------------------------------------------------------------------- (a) t2s_wg_in_cond_gate_fold
# (B, C, n_cond, L, dilation, kernel size, tile rows)
def _sat(C):
    """layer 0: +30, -30, +120, -120 on the tanh rows of channels 0 .. 3 and on the sigmoid rows of channels 4 .. 7"""
    return 0, tuple(zip((0, 1, 2, 3, C + 4, C + 5, C + 6, C + 7), (30.0, -30.0, 120.0, -120.0) * 2))


COND_CASES = [
    ("128-ragged", 2, 64, 640, 300, 1, 3, 128, None),
    ("128-exact", 1, 128, 96, 256, 4, 3, 128, None),
    ("128-three-mtiles", 3, 192, 40, 257, 32, 3, 128, None),
    ("128-16slots", 2, 512, 640, 520, 128, 3, 128, None),
    ("128-one-column", 1, 64, 32, 1, 128, 3, 128, None),
    ("256-C16", 2, 16, 32, 5, 1, 3, 256, None),
    ("256-C80", 3, 80, 96, 300, 2, 3, 256, None),
    ("256-C144", 1, 144, 640, 257, 128, 3, 256, None),
    ("256-C48", 2, 48, 40, 256, 16, 3, 256, None),
    ("256-129wg", 3, 64, 64, 10757, 8, 3, 256, None),
    ("256-130wg", 1, 256, 64, 16385, 1, 3, 256, None),
    ("256-nk1", 2, 16, 0, 37, 1, 1, 256, None),
    ("256-nk2", 2, 16, 32, 37, 1, 1, 256, None),
    ("256-nk3", 2, 32, 64, 37, 1, 1, 256, None),
    ("256-taps5", 2, 80, 96, 300, 4, 5, 256, None),
    ("128-saturated", 2, 64, 96, 300, 1, 3, 128, _sat(64)),
    ("256-saturated", 2, 80, 96, 300, 1, 3, 256, _sat(80)),       # beside the listed cases: the ping-pong epilogue has a gate of its own
]


@pytest.mark.parametrize("name,B,C,n_cond,L,dil,ks,tile,shift", COND_CASES, ids=[c[0] for c in COND_CASES])
def test_in_cond_gate_fold(name, B, C, n_cond, L, dil, ks, tile, shift):
    """t2s_wg_in_cond_gate_fold at the smallest shape of each family (the ids name them; 129wg / 130wg: a C % 64 == 0 model on the
    ping-pong kernel by its grid, 129 workgroups = the block remap's remainder branch; nk1..3: K loops of 1, 2, 3 steps;
    saturated: +-30 and +-120 on the gate biases of eight channels - finite outputs at the same bars)."""
    i = int(math.log2(dil))
    assert 2 ** i == dil
    if shift is not None:       # the shifted channels really saturate: tanh at +-1, sigmoid at 0 / 1
        _, _, _, layers, _ = _case(C, 2, ks, 4, n_cond, B, L, shift)
        a = layers[0]["acts"]
        assert float(a[:, 3].abs().max()) > 0.0 and float((a[:, 0].abs() - layers[0]["sig"][:, 0]).abs().max()) < 1e-12
        assert float(a[:, 7].abs().max()) < 1e-40 and float(layers[0]["sig"][:, 6].min()) == 1.0
    _gate_case("cond %s B%d C%d S%d L%d d%d k%d" % (name, B, C, n_cond, L, dil, ks), "cond", B, C, n_cond, L, ks, i, tile, bias_shift=shift)


# ---------------------------------------------------------------------------------------------- (b) t2s_wg_in_win_gate_fold
# (B, C, n_cond, L, kernel size, n_half, c_off, win_chunks, tile rows); win_chunks = 4 needs C > 96 (four 32-channel chunks)
WIN_CASES = [
    (2, 64, 32, 300, 3, 4, 0, 2, 128),          # nk = 3
    (1, 80, 640, 257, 3, 3, 2, 2, 256),
    (3, 64, 640, 5, 3, 1, 6, 2, 128),
    (2, 80, 32, 1, 3, 4, 0, 2, 256),            # nk = 3 on the ping-pong kernel, one column
    (1, 80, 32, 300, 3, 1, 6, 2, 256),
    (2, 64, 640, 257, 3, 3, 2, 2, 128),
    (1, 128, 32, 257, 5, 4, 0, 4, 128),         # five taps: one column set per chunk
    (2, 112, 640, 300, 5, 4, 0, 4, 256),
]


@pytest.mark.parametrize("B,C,n_cond,L,ks,nh,c_off,nwc,tile", WIN_CASES,
                         ids=["B%d-C%d-S%d-L%d-k%d-nh%d-off%d-w%d" % c[:8] for c in WIN_CASES])
def test_in_win_gate_fold(B, C, n_cond, L, ks, nh, c_off, nwc, tile):
    """Layer 0 through the window planes (t2s_wg_start_window from the oracle's audio, t2s_wg_startfold_weights): the oracle's
    layer-0 acts come from x0 = W_start a + b_start with zero padding.  Same assertions as the conditioned gate."""
    assert nwc == (2 if 2 * ks * (nh + 1) <= 32 else 4)
    _gate_case("win B%d C%d S%d L%d k%d nh%d off%d w%d" % (B, C, n_cond, L, ks, nh, c_off, nwc), "win", B, C, n_cond, L, ks, 0, tile,
               nh=nh, c_off=c_off, nwc=nwc)


# ---------------------------------------------------------------------------------------------- (e) the training gate
@pytest.mark.parametrize("wide", [False, True], ids=["own-planes", "wide-planes"])
@pytest.mark.parametrize("B,C,n_cond,L,dil,tile", [(2, 64, 96, 300, 2, 128), (3, 80, 96, 300, 2, 256)], ids=["128", "256"])
def test_in_cond_gate_fold_train(B, C, n_cond, L, dil, tile, wide):
    """t2s_wg_in_cond_gate_fold_train: everything the no-grad form is held to, the G planes against the oracle's sigmoid, and
    act_bchunks = 0 or a plane set three layers wide whose other two layers' chunks stay untouched."""
    _gate_case("train %d-row B%d C%d L%d %s" % (tile, B, C, L, "wide" if wide else "own"), "cond", B, C, n_cond, L, 3, int(math.log2(dil)),
               tile, train=True, wide=wide)


# ---------------------------------------------------------------------------------------------- (c) the residual GEMMs
_BL = [(2, 300), (1, 257), (3, 5), (1, 1)]


def _res_setup(C, B, L, nh=4):
    wn, audio, spect, layers, _ = _case(C, 2, 3, nh, 32, B, L)
    Lp = _lib.plane_rows(L, HALO)
    xc = -(-C // 32)
    return wn, audio, layers[0], Lp, xc


def _check_x(label, X, C, L, want):
    U.check(label, U.plane_values((X[0].t, X[1].t), C, L, HALO), want, U.GEMM_NORM, U.GEMM_MAX)
    U.assert_halo_zero((X[0].t, X[1].t), L, HALO, label)
    for p in X:
        if C % 32:
            assert float(p.t[:, -1, :, C % 32:].float().abs().max()) == 0.0, label + ": channels past C were written"
        p.assert_guards(label)


@pytest.mark.parametrize("B,L", _BL)
@pytest.mark.parametrize("C,pair8", [(32, 0), (32, 1), (36, 0), (128, 0), (128, 1), (160, 0), (160, 1)])
def test_res_only(C, pair8, B, L):
    """t2s_wg_res_only in place on the oracle's x_0 and acts_0: x_1 = x_0 + W_res . acts_0 + b in float64 at the GEMM bars, halo
    rows and channels past C zero, guards intact; both row orders."""
    _lib.load()
    wn, _, ly, Lp, xc = _res_setup(C, B, L)
    A2h, A2l, b2, Mpad2, _ = wn.res(0, bool(pair8))
    Ap = planes.to_planes(U.dev(ly["acts"].float()), HALO, Lp)
    X = _plane_pair(B, xc, Lp, planes.to_planes(U.dev(ly["x"].float()), HALO, Lp))
    _lib.call("t2s_wg_res_only", _lib.ptr(A2h), _lib.ptr(A2l), _lib.ptr(b2), _lib.ptr(Ap[0]), _lib.ptr(Ap[1]), _lib.ptr(X[0].t),
              _lib.ptr(X[1].t), B, C, L, Lp, HALO, Mpad2, pair8, _lib.current_stream())
    _sync()
    _check_x("res_only C%d pair8=%d B%d L%d" % (C, pair8, B, L), X, C, L, ly["x_next"])


@pytest.mark.parametrize("c_off,nh", [(0, 4), (2, 3), (6, 1)])
@pytest.mark.parametrize("B,L", _BL)
@pytest.mark.parametrize("C", [32, 128, 160])
def test_res_only_start(C, B, L, c_off, nh):
    """t2s_wg_res_only_start: x_0 rebuilt from z in the epilogue.  The X planes' data rows hold NaN beforehand, so a kernel that
    read them could not give a finite x_1: they are only written."""
    _lib.load()
    wn, audio, ly, Lp, xc = _res_setup(C, B, L, nh)
    A2h, A2l, b2, Mpad2, _ = wn.res(0, True)
    Ap = planes.to_planes(U.dev(ly["acts"].float()), HALO, Lp)
    X = _plane_pair(B, xc, Lp)
    for p in X:
        p.t[:, :, HALO:HALO + L] = float("nan")
    z = _z_with(audio, c_off, seed=C + L)
    _lib.call("t2s_wg_res_only_start", _lib.ptr(A2h), _lib.ptr(A2l), _lib.ptr(b2), _lib.ptr(Ap[0]), _lib.ptr(Ap[1]), _lib.ptr(z),
              _lib.ptr(wn.w_start()), _lib.ptr(wn.p("start.bias")), G8, c_off, nh, _lib.ptr(X[0].t), _lib.ptr(X[1].t), B, C, L, Lp, HALO,
              Mpad2, _lib.current_stream())
    _sync()
    _check_x("res_only_start C%d B%d L%d off%d nh%d" % (C, B, L, c_off, nh), X, C, L, ly["x_next"])


@pytest.mark.parametrize("wide", [False, True], ids=["own-planes", "wide-planes"])
@pytest.mark.parametrize("C,pair8,B,L", [(128, 1, 2, 300), (160, 0, 1, 257)])
def test_res_only_train(C, pair8, B, L, wide):
    """t2s_wg_res_only_train: the layer input is read from R and stays bit for bit, x_1 goes to X (NaN in its data rows
    beforehand); the acts come from their own planes or from the middle of a plane set three layers wide."""
    _lib.load()
    wn, _, ly, Lp, xc = _res_setup(C, B, L)
    A2h, A2l, b2, Mpad2, _ = wn.res(0, bool(pair8))
    acts = planes.to_planes(U.dev(ly["acts"].float()), HALO, Lp)
    if wide:        # the neighbouring layers' chunks hold values that would wreck the sum if they were read
        Ap = [torch.full((B, 3 * xc, Lp, 32), 100.0, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        for w, a in zip(Ap, acts):
            w[:, xc:2 * xc] = a
        a_ptr = [_lib.c_vp(w.data_ptr() + 2 * xc * Lp * 32) for w in Ap]
    else:
        Ap, a_ptr = acts, [_lib.ptr(a) for a in acts]
    R = planes.to_planes(U.dev(ly["x"].float()), HALO, Lp)
    R_keep = [r.clone() for r in R]
    X = _plane_pair(B, xc, Lp)
    for p in X:
        p.t[:, :, HALO:HALO + L] = float("nan")
    _lib.call("t2s_wg_res_only_train", _lib.ptr(A2h), _lib.ptr(A2l), _lib.ptr(b2), a_ptr[0], a_ptr[1], 3 * xc if wide else 0,
              _lib.ptr(R[0]), _lib.ptr(R[1]), _lib.ptr(X[0].t), _lib.ptr(X[1].t), B, C, L, Lp, HALO, Mpad2, pair8, _lib.current_stream())
    _sync()
    _check_x("res_only_train C%d pair8=%d B%d L%d %s" % (C, pair8, B, L, "wide" if wide else "own"), X, C, L, ly["x_next"])
    assert torch.equal(R[0], R_keep[0]) and torch.equal(R[1], R_keep[1]), "R changed"


# ---------------------------------------------------------------------------------------------- (d) t2s_wg_end_fold_affine
# (nslots, n_layers, n_half, c_off, L)
_END = [(2, 1, 1, 6, 1), (6, 4, 3, 2, 255), (16, 8, 4, 0, 257), (2, 4, 4, 0, 255), (6, 8, 1, 6, 257), (16, 1, 3, 2, 1),
        (2, 8, 3, 2, 257), (6, 1, 4, 0, 1), (16, 4, 1, 6, 255)]


@pytest.mark.parametrize("reverse", [0, 1], ids=["forward", "reverse"])
@pytest.mark.parametrize("nslots,nl,nh,c_off,L", _END)
def test_end_fold_affine(nslots, nl, nh, c_off, L, reverse):
    """WN.end from random slots, bes and b_end, and the coupling exp(ls) a1 + bb (reverse: (a1 - bb) / exp(ls)) in float64 at the
    f32 bars, with log_s and wn_out each given or NULL; every other channel of z bit-identical, guards intact."""
    _lib.load()
    B = 2
    gen = torch.Generator().manual_seed(100 * nslots + 10 * nl + nh + L)
    acc = 0.1 * torch.randn(nslots, B, 8, L, generator=gen)
    bes = 0.1 * torch.randn(nl, 8, generator=gen)
    b_end = 0.1 * torch.randn(2 * nh, generator=gen)
    z0 = torch.randn(B, G8, L, generator=gen)
    tot = acc.double().sum(0) + bes.double().sum(0)[None, :, None]
    bb = tot[:, :nh] + b_end.double()[None, :nh, None]
    ls = tot[:, nh:2 * nh] + b_end.double()[None, nh:, None]
    a1 = z0.double()[:, c_off + nh:c_off + 2 * nh]
    want = (a1 - bb) / torch.exp(ls) if reverse else torch.exp(ls) * a1 + bb
    acc_d, bes_d, b_end_d = U.dev(acc), U.dev(bes), U.dev(b_end)
    touched = torch.zeros(G8, dtype=torch.bool)
    touched[c_off + nh:c_off + 2 * nh] = True
    for with_ls, with_out in ((True, True), (False, False), (True, False), (False, True)):
        label = "end_fold_affine %s slots%d layers%d nh%d L%d log_s=%s wn_out=%s" % ("rev" if reverse else "fwd", nslots, nl, nh, L,
                                                                                    with_ls, with_out)
        z = U.Guarded(B, G8, L, fill=U.dev(z0))
        log_s = U.Guarded(B, nh, L) if with_ls else None
        wn_out = U.Guarded(B, 2 * nh, L) if with_out else None
        _lib.call("t2s_wg_end_fold_affine", _lib.ptr(acc_d), nslots, _lib.ptr(bes_d), nl, _lib.ptr(b_end_d), _lib.ptr(z.t),
                  None if log_s is None else _lib.ptr(log_s.t), None if wn_out is None else _lib.ptr(wn_out.t), B, G8, c_off, nh, L,
                  reverse, _lib.current_stream())
        _sync()
        zc = z.t.cpu()
        U.check(label + " a1", zc[:, touched], want, U.F32_NORM, U.F32_MAX)
        assert torch.equal(zc[:, ~touched], z0[:, ~touched]), label + ": another channel of z changed"
        z.assert_guards(label)
        if with_ls:
            U.check(label + " log_s", log_s.t, ls, U.F32_NORM, U.F32_MAX)
            log_s.assert_guards(label)
        if with_out:
            U.check(label + " wn_out", wn_out.t, torch.cat([bb, ls], 1), U.F32_NORM, U.F32_MAX)
            wn_out.assert_guards(label)


# ---------------------------------------------------------------------------------------------- (f) argument checks
def test_argument_validation_without_launching():
    """Every broken rule returns T2S_EINVAL before anything is launched and leaves the outputs' sentinel in place (the pointers
    are real, and the tuples the broken ones are made from are themselves accepted)."""
    lib = _lib.load()
    P = _lib.ptr
    B, C, n_cond, L, taps, nwc = 1, 64, 32, 40, 3, 2
    Lp = _lib.plane_rows(L, HALO)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    A = torch.zeros(taps * 2 + 1, 256, 32, **bf)
    bias = torch.zeros(256, device=DEV)
    Xp, Sp = torch.zeros(B, 2, Lp, 32, **bf), torch.zeros(B, 1, Lp, 32, **bf)
    Wp = torch.zeros(B, 4, Lp, 32, **bf)
    fold_A = torch.zeros(8192, **bf)
    z, ws, bs = torch.zeros(B, G8, L, device=DEV), torch.zeros(C, 4, device=DEV), torch.zeros(C, device=DEV)
    SENT = 0.375
    outs = [torch.full((B, 2, Lp, 32), SENT, **bf) for _ in range(4)]        # acts hi / lo, G hi / lo (X hi / lo of the residual forms)
    acc = U.Guarded(2, B, 8, L)
    st = _lib.current_stream()

    def unchanged():
        _sync()
        return all(bool((o == SENT).all()) for o in outs) and bool(acc.untouched(acc.t).all())

    def cond(**ch):
        a = dict(A_hi=P(A), A_lo=P(A), bias=P(bias), X_hi=P(Xp), X_lo=P(Xp), S_hi=P(Sp), S_lo=P(Sp), acts_hi=P(outs[0]), acts_lo=P(outs[1]),
                 fold_A=P(fold_A), fold_acc=P(acc.t), fold_init=1, B=B, C=C, n_cond=n_cond, taps=taps, dilation=1, L=L, Lp=Lp, halo=HALO,
                 Mpad=256, stream=st)
        a.update(ch)
        return lib.t2s_wg_in_cond_gate_fold(*a.values())

    def cond_train(**ch):
        a = dict(A_hi=P(A), A_lo=P(A), bias=P(bias), X_hi=P(Xp), X_lo=P(Xp), S_hi=P(Sp), S_lo=P(Sp), acts_hi=P(outs[0]), acts_lo=P(outs[1]),
                 G_hi=P(outs[2]), G_lo=P(outs[3]), act_bchunks=0, fold_A=P(fold_A), fold_acc=P(acc.t), fold_init=1, B=B, C=C, n_cond=n_cond,
                 taps=taps, dilation=1, L=L, Lp=Lp, halo=HALO, Mpad=256, stream=st)
        a.update(ch)
        return lib.t2s_wg_in_cond_gate_fold_train(*a.values())

    def win(**ch):
        a = dict(A_hi=P(A), A_lo=P(A), bias=P(bias), W_hi=P(Wp), W_lo=P(Wp), S_hi=P(Sp), S_lo=P(Sp), acts_hi=P(outs[0]), acts_lo=P(outs[1]),
                 fold_A=P(fold_A), fold_acc=P(acc.t), fold_init=1, B=B, C=C, n_cond=n_cond, win_chunks=nwc, L=L, Lp=Lp, halo=HALO, Mpad=256,
                 stream=st)
        a.update(ch)
        return lib.t2s_wg_in_win_gate_fold(*a.values())

    def res(**ch):
        a = dict(A_hi=P(A), A_lo=P(A), bias=P(bias), acts_hi=P(Xp), acts_lo=P(Xp), X_hi=P(outs[0]), X_lo=P(outs[1]), B=B, C=C, L=L, Lp=Lp,
                 halo=HALO, Mpad=256, pair8=1, stream=st)
        a.update(ch)
        return lib.t2s_wg_res_only(*a.values())

    def res_train(**ch):
        a = dict(A_hi=P(A), A_lo=P(A), bias=P(bias), acts_hi=P(Xp), acts_lo=P(Xp), act_bchunks=0, R_hi=P(Xp), R_lo=P(Xp), X_hi=P(outs[0]),
                 X_lo=P(outs[1]), B=B, C=C, L=L, Lp=Lp, halo=HALO, Mpad=256, pair8=1, stream=st)
        a.update(ch)
        return lib.t2s_wg_res_only_train(*a.values())

    def res_start(**ch):
        a = dict(A_hi=P(A), A_lo=P(A), bias=P(bias), acts_hi=P(Xp), acts_lo=P(Xp), z=P(z), w_start=P(ws), b_start=P(bs), n_group=G8, c_off=0,
                 n_half=4, X_hi=P(outs[0]), X_lo=P(outs[1]), B=B, C=C, L=L, Lp=Lp, halo=HALO, Mpad=256, stream=st)
        a.update(ch)
        return lib.t2s_wg_res_only_start(*a.values())

    bad = [(cond, dict(C=24)), (cond, dict(C=40)), (cond_train, dict(C=24)), (win, dict(C=24)),
           (cond, dict(Lp=Lp + 1)), (cond, dict(Lp=Lp - 1)), (cond_train, dict(Lp=Lp + 1)), (win, dict(Lp=Lp - 1)), (res, dict(Lp=Lp + 1)),
           (res_train, dict(Lp=Lp - 1)), (res_start, dict(Lp=Lp + 1)),
           (cond, dict(dilation=HALO + 1)), (cond, dict(taps=5, dilation=HALO // 2 + 1)), (cond_train, dict(dilation=HALO + 1)),
           (win, dict(win_chunks=3)),
           (res, dict(C=48, pair8=1)), (res_train, dict(C=48, pair8=1)), (res_start, dict(C=48))]
    for fn, ch in bad:
        assert fn(**ch) == -1, "%s accepted %r" % (fn.__name__, ch)
        assert unchanged(), "%s wrote something with %r" % (fn.__name__, ch)
    # the tuples themselves are accepted (zero operands: the launches are harmless), C = 48 too where it is the pair8 order that is not
    for fn in (cond, cond_train, win, res, res_train, res_start):
        assert fn() == 0, fn.__name__
    assert res(C=48, pair8=0) == 0 and res_train(C=48, pair8=0) == 0
    _sync()
