"""The _h16 entry points (fp16 vocoder planes, include/t2s_hip.h) one by one through the C ABI against float64:

  t2s_pack_conv_weight_table_h16    one fp16 plane of the effective weight (round to nearest even), A_lo untouched
  t2s_wg_endfold_weights_h16        the folded WN.end as fp16 hi / lo fragments
  t2s_wg_start_h16, t2s_wg_upsample_squeeze_h16     fp16 hi / lo X and conditioning planes
  t2s_wg_in_cond_gate_fold_h16      A . B_hi + A . B_lo with a one-plane A operand (A_lo = NULL), both tile heights
  t2s_wg_res_only_h16               the same for the residual GEMM, both row orders

Every kernel reads the ORACLE's input of that kernel (oracle.waveglow_oracle.wn_forward through tests/wg_fwd_util.py) rounded to
fp16 planes, never another kernel's output, and every expectation is float64 arithmetic on the DECODED values of what the kernel
reads: the packed fp16 weights and f32 biases as they sit in memory, the planes' hi + lo.  Against those values the two-product
arithmetic drops nothing (A is one plane, B is hi + lo exactly): what is left is the f32 accumulation and the rounding of the
result to an fp16 (hi, lo) pair.  That floor is computed per case on the CPU from the same decoded values (_two_product_floor: the
two products contracted in float32) and printed; a case whose floor exceeds a quarter of a bar takes 4 x its floor as that bar,
the rule of tests/test_waveglow_fwd_kernels_gpu.py::_fold_bars.  Bars are tests/wg_bwd_util.py's GEMM_NORM / GEMM_MAX.  The folded
WN.end keeps hi + lo and three products; its floor is the three-product one in fp16 (_split3_floor_f16)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import wg_bwd_util as U
import wg_fwd_util as W
from text2speech_amd import _lib, planes

pytestmark = pytest.mark.gpu

DEV = U.DEV
HALO = 128
G8 = 8
PAD = 1024              # fp16 elements in front of and behind every plane output
_GUARD_H = -1.5         # what those hold
H16 = dict(dtype=torch.float16, device=DEV)


class _HB:
    """An fp16 device buffer of `shape`, zeroed, with PAD elements of _GUARD_H either side; `.t` is the buffer (16-byte aligned)."""

    def __init__(self, *shape):
        self.n = math.prod(shape)
        self.raw = torch.full((self.n + 2 * PAD,), _GUARD_H, **H16)
        self.t = self.raw[PAD:PAD + self.n].view(*shape)
        self.t.zero_()

    def assert_guards(self, label):
        assert bool((self.raw[:PAD] == _GUARD_H).all()), "%s: wrote in front of the output" % label
        assert bool((self.raw[PAD + self.n:] == _GUARD_H).all()), "%s: wrote behind the output" % label


def _f32(t):
    return None if t is None else U.dev(t.to(torch.float32))


def _sync():
    torch.cuda.synchronize()


def _to_h16(x, Lp):
    """float64 / f32 CPU [B, C, L] -> fp16 (hi, lo) device planes"""
    return planes.to_planes(U.dev(x.float()), HALO, Lp, fmt="f16")


def _bars(floor):
    fn, fm = floor
    return (U.GEMM_NORM if fn <= U.GEMM_NORM / 4 else 4 * fn), (U.GEMM_MAX if fm <= U.GEMM_MAX / 4 else 4 * fm)


def _two_product_floor(a, b, contract):
    """The floor of A . B_hi + A . B_lo with f32 accumulation: a (float64, fp16-exact) and b (float64 plane values, hi + lo exactly)
    contracted by `contract(a, b)` in float32 for each plane, against the float64 contraction of a and b."""
    bh = b.to(torch.float16).double()
    bl = b - bh
    assert torch.equal(bl.to(torch.float16).double(), bl), "a plane value is not hi + lo of two fp16 numbers"
    exact = contract(a, b)
    emu = contract(a.float(), bh.float()).double() + contract(a.float(), bl.float()).double()
    return U.rel(emu, exact), U.maxrel(emu, exact)


def _split3_floor_f16(a, b, eq):
    """U.split3_floor with fp16 hi planes: hi.hi + hi.lo + lo.hi against the exact contraction (the lo.lo term is what it drops)"""
    def split(x):
        hi = x.to(torch.float32).to(torch.float16).double()
        return hi, x - hi
    ah, al = split(a)
    bh, bl = split(b)
    exact = torch.einsum(eq, a, b)
    emu = torch.einsum(eq, ah, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, al, bh)
    return U.rel(emu, exact), U.maxrel(emu, exact)


def _pack_table(jobs, h16=True):
    """t2s_pack_conv_weight_table(_h16) over jobs laid out as text2speech_amd/glow.py lays them out"""
    dp = lambda t: 0 if t is None else t.data_ptr()
    rows, row_start = [], 0
    for (v, g, b1, b2, Ah, Al, bo, O_, Cin, Kt, perm, Cg, Mpad, koff, Cin_pad, so) in jobs:
        rows.append([dp(v), dp(g), dp(b1), dp(b2), dp(Ah), dp(Al), dp(bo), row_start, O_, Cin, Kt, perm, Cg, Mpad, koff, Cin_pad, 0, 0, dp(so)])
        row_start += -(-O_ // 16)
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    _lib.call("t2s_pack_conv_weight_table_h16" if h16 else "t2s_pack_conv_weight_table", _lib.ptr(table), len(rows), row_start,
              _lib.current_stream())
    _sync()


def _unpair8(v, rows):
    """rows of a packed operand back in channel order (packed row 16 m + 4 q + e of a group of 32 = channel 8 q + 4 m + e)"""
    c = torch.arange(rows)
    w = c & 31
    return v[(c & ~31) + ((w >> 2) & 1) * 16 + (w >> 3) * 4 + (w & 3)]


class _WN:
    """One seeded WN (wg_fwd_util.wn_state) and its fp16 operands, built on demand with the _h16 pack entry points (A_lo = NULL)."""

    def __init__(self, C, nl, ks, nh, n_cond, seed, bias_shift=None):
        self.C, self.nl, self.ks, self.nh, self.n_cond = C, nl, ks, nh, n_cond
        self.sd = W.wn_state(C, nl, ks, nh, n_cond, seed)
        if bias_shift is not None:
            i, shifts = bias_shift
            for o, s in shifts:
                self.sd["WN.0.in_layers.%d.bias" % i][o] += s
        self.cfg = W.wn_cfg(C, nl, ks)
        self.Cpad, self.Spad = -(-C // 32) * 32, -(-n_cond // 32) * 32
        self.Mpad1 = -(-C // 128) * 256
        self.d = {k: _f32(v.flatten() if k.endswith("weight_g") else v) for k, v in self.sd.items()}

    def p(self, name):
        return self.d["WN.0." + name]

    @functools.lru_cache(maxsize=None)
    def gate(self, i):
        """(A1h, b1) of layer i: in_layers[i] then cond_layers[i] along K, T2S_PERM_GATE rows, the two biases added"""
        C, ks = self.C, self.ks
        nk1 = ks * self.Cpad // 32 + self.Spad // 32
        Ah, b1 = torch.zeros(nk1, self.Mpad1, 32, **H16), torch.zeros(self.Mpad1, device=DEV)
        li, lc = "in_layers.%d." % i, "cond_layers.%d." % i
        jobs = [(self.p(li + "weight_v"), self.p(li + "weight_g"), self.p(li + "bias"), self.p(lc + "bias") if self.n_cond else None,
                 Ah, None, b1, 2 * C, C, ks, 1, C, self.Mpad1, 0, self.Cpad, None)]
        if self.n_cond:
            jobs.append((self.p(lc + "weight_v"), self.p(lc + "weight_g"), None, None, Ah, None, None, 2 * C, self.n_cond, 1, 1, C,
                         self.Mpad1, ks * self.Cpad, self.Spad, None))
        _pack_table(jobs)
        return Ah, b1

    def gate_decoded(self, i):
        """float64 (w_in [2C, C, ks], w_cond [2C, n_cond] or None, bias [2C]) as the packed operand of layer i holds them"""
        C, ks = self.C, self.ks
        Ah, b1 = self.gate(i)
        v = Ah.double().cpu().permute(1, 0, 2).reshape(self.Mpad1, -1)
        row = W._gate_row(torch.arange(2 * C), C)
        w_in = torch.stack([v[row][:, t * self.Cpad:t * self.Cpad + C] for t in range(ks)], 2)
        w_cond = v[row][:, ks * self.Cpad:ks * self.Cpad + self.n_cond] if self.n_cond else None
        return w_in, w_cond, b1.double().cpu()[row]

    @functools.lru_cache(maxsize=None)
    def res(self, i, pair8):
        """(A2h, b2, Mpad2, scale) of res_skip_layers[i]; pair8: the residual rows in the T2S_PERM_PAIR8 order"""
        C = self.C
        rows2 = 2 * C if i < self.nl - 1 else C
        Mpad2 = _lib.padded_rows(rows2)
        Ah, b2 = torch.zeros(self.Cpad // 32, Mpad2, 32, **H16), torch.zeros(Mpad2, device=DEV)
        s_rs = torch.empty(rows2, device=DEV)
        lr = "res_skip_layers.%d." % i
        _pack_table([(self.p(lr + "weight_v"), self.p(lr + "weight_g"), self.p(lr + "bias"), None, Ah, None, b2, rows2, C, 1,
                      2 if pair8 else 0, C if pair8 else 0, Mpad2, 0, self.Cpad, s_rs)])
        return Ah, b2, Mpad2, s_rs

    def res_decoded(self, i, pair8):
        """float64 (w_res [C, C], b_res [C]): the residual rows as the packed operand holds them, in channel order"""
        C = self.C
        Ah, b2, Mpad2, _ = self.res(i, pair8)
        v = Ah.double().cpu().permute(1, 0, 2).reshape(Mpad2, -1)[:, :C]
        b = b2.double().cpu()
        if pair8:
            return _unpair8(v, C), _unpair8(b, C)
        return v[:C], b[:C]

    @functools.lru_cache(maxsize=None)
    def fold(self, i):
        """(fold_A fp16, bes [8]) of layer i from t2s_wg_endfold_weights_h16, with the scales the pack wrote"""
        C = self.C
        s_rs = self.res(i, False)[3]
        r0 = C if i < self.nl - 1 else 0
        lr = "res_skip_layers.%d." % i
        w_end = self.p("end.weight").view(2 * self.nh, C)
        fold_A = torch.zeros(-(-C // 128) * 8192, **H16)
        bes = torch.zeros(8, device=DEV)
        table = torch.tensor([[w_end.data_ptr(), self.p(lr + "weight_v").data_ptr() + 4 * r0 * C, s_rs.data_ptr() + 4 * r0,
                               self.p(lr + "bias").data_ptr() + 4 * r0, fold_A.data_ptr(), bes.data_ptr(), 2 * self.nh, C]],
                             dtype=torch.int64).to(DEV)
        _lib.call("t2s_wg_endfold_weights_h16", _lib.ptr(table), 1, C, _lib.current_stream())
        _sync()
        return fold_A, bes

    @functools.lru_cache(maxsize=None)
    def w_start(self):
        w = torch.empty(self.C, self.nh, device=DEV)
        _lib.call("t2s_weightnorm_small", _lib.ptr(self.p("start.weight_v")), _lib.ptr(self.p("start.weight_g")), self.C, self.nh,
                  _lib.ptr(w), _lib.current_stream())
        _sync()
        return w


@functools.lru_cache(maxsize=4)
def _case(C, nl, ks, nh, n_cond, B, L, bias_shift=None):
    """the seeded WN of a shape, its inputs and the oracle's per-layer expectation: computed once, shared, never modified"""
    wn = _WN(C, nl, ks, nh, n_cond, seed=1000 * C + 10 * nl + ks + nh, bias_shift=bias_shift)
    audio, spect = W.wn_inputs(B, nh, n_cond, L, seed=L + 7 * B)
    layers, out = W.layer_expect(wn.sd, wn.cfg, audio, spect)
    return wn, audio, spect, layers, out


# ---------------------------------------------------------------------------------------------- (a) the pack
def _check_one_plane(label, got, w64):
    """|decode(A_hi) - w64| <= 2^-11 |w64| (1 + 1e-3) + 2^-25 for every element: half an fp16 ulp plus the f32 effective weight's own
    rounding"""
    err = (got - w64).abs()
    bound = 2.0 ** -11 * w64.abs() * (1 + 1e-3) + 2.0 ** -25
    worst = float((err / bound).max())
    print("PACK   %-60s worst |err| / bound %.3f over %d elements" % (label, worst, err.numel()))
    assert bool((err <= bound).all()), "%s: an element is off by %.3f x its bound" % (label, worst)


@pytest.mark.parametrize("C", [36, 160])
def test_pack_one_fp16_plane(C):
    """Gate and residual tables at ks = 3: every element of the decoded hi plane within half an fp16 ulp of the float64 effective
    weight, rows and K columns outside the job zero, bias_out bit for bit the split-bf16 pack's, and a real A_lo buffer handed in
    the job keeps its sentinel."""
    _lib.load()
    ks, nh, n_cond, nl = 3, 4, 40, 2
    wn = _WN(C, nl, ks, nh, n_cond, seed=77 + C)
    # -- gate: in_layers.0 then cond_layers.0
    w_in, w_cond, _ = wn.gate_decoded(0)
    _check_one_plane("gate C%d in_layers" % C, w_in, W.eff(wn.sd, "in_layers.0"))
    _check_one_plane("gate C%d cond_layers" % C, w_cond, W.eff(wn.sd, "cond_layers.0")[:, :, 0])
    Ah, b1 = wn.gate(0)
    v = Ah.double().cpu().permute(1, 0, 2).reshape(wn.Mpad1, -1)
    used = torch.zeros_like(v, dtype=torch.bool)
    row = W._gate_row(torch.arange(2 * C), C)
    for t in range(ks):
        used[row[:, None], (t * wn.Cpad + torch.arange(C))[None]] = True
    used[row[:, None], (ks * wn.Cpad + torch.arange(n_cond))[None]] = True
    assert float(v[~used].abs().max()) == 0.0, "gate C%d: padding rows / columns were written" % C
    # the same jobs through the split-bf16 pack: the biases agree bit for bit
    nk1 = ks * wn.Cpad // 32 + wn.Spad // 32
    bf = dict(dtype=torch.bfloat16, device=DEV)
    Bh, Bl, bb = torch.zeros(nk1, wn.Mpad1, 32, **bf), torch.zeros(nk1, wn.Mpad1, 32, **bf), torch.zeros(wn.Mpad1, device=DEV)
    li, lc = "in_layers.0.", "cond_layers.0."
    _pack_table([(wn.p(li + "weight_v"), wn.p(li + "weight_g"), wn.p(li + "bias"), wn.p(lc + "bias"), Bh, Bl, bb, 2 * C, C, ks, 1, C,
                  wn.Mpad1, 0, wn.Cpad, None)], h16=False)
    assert torch.equal(bb.view(torch.int32), b1.view(torch.int32)), "gate C%d: bias_out differs from the split-bf16 pack's" % C
    # -- residual / skip table, both row orders where the pair8 order exists
    for pair8 in ([False, True] if C % 32 == 0 else [False]):
        w_res, b_res = wn.res_decoded(0, pair8)
        w64 = W.eff(wn.sd, "res_skip_layers.0")[:, :, 0]
        _check_one_plane("res C%d pair8=%d residual rows" % (C, pair8), w_res, w64[:C])
        A2h, b2, Mpad2, _ = wn.res(0, pair8)
        v2 = A2h.double().cpu().permute(1, 0, 2).reshape(Mpad2, -1)
        _check_one_plane("res C%d pair8=%d skip rows" % (C, pair8), v2[C:2 * C, :C], w64[C:])
        assert float(v2[2 * C:].abs().max()) == 0.0 and (C % 32 == 0 or float(v2[:, C:].abs().max()) == 0.0)
        lr = "res_skip_layers.0."
        Rh, Rl, rb = torch.zeros(wn.Cpad // 32, Mpad2, 32, **bf), torch.zeros(wn.Cpad // 32, Mpad2, 32, **bf), torch.zeros(Mpad2, device=DEV)
        _pack_table([(wn.p(lr + "weight_v"), wn.p(lr + "weight_g"), wn.p(lr + "bias"), None, Rh, Rl, rb, 2 * C, C, 1,
                      2 if pair8 else 0, C if pair8 else 0, Mpad2, 0, wn.Cpad, None)], h16=False)
        assert torch.equal(rb.view(torch.int32), b2.view(torch.int32)), "res C%d: bias_out differs from the split-bf16 pack's" % C
    # -- A_lo given: untouched
    lo = torch.full((wn.Cpad // 32, Mpad2, 32), _GUARD_H, **H16)
    hi = _HB(wn.Cpad // 32, Mpad2, 32)
    _pack_table([(wn.p(lr + "weight_v"), wn.p(lr + "weight_g"), wn.p(lr + "bias"), None, hi.t, lo, torch.zeros(Mpad2, device=DEV),
                  2 * C, C, 1, 0, 0, Mpad2, 0, wn.Cpad, None)])
    assert bool((lo == _GUARD_H).all()), "the _h16 pack wrote A_lo"
    assert torch.equal(hi.t, wn.res(0, False)[0])
    hi.assert_guards("pack C%d" % C)


# ---------------------------------------------------------------------------------------------- (b) the folded WN.end fragments
@pytest.mark.parametrize("C,nj", [(48, 6), (160, 8)])
def test_endfold_weights_h16(C, nj):
    """Decoded hi + lo against float64 (W_end . diag(scale)) . V_skip at the plane bars tests/test_weight_prep_kernels_gpu.py holds the
    split-bf16 form to; rows nj .. 15 and columns past C zero; bes at the f32 bars."""
    _lib.load()
    gen = torch.Generator().manual_seed(C + nj)
    w_end, v = U.dev(torch.randn(nj, C, generator=gen) * 0.05), U.dev(torch.randn(C, C, generator=gen))
    scale, b = U.dev(torch.rand(C, generator=gen) + 0.5), U.dev(torch.randn(C, generator=gen))
    fold = _HB(-(-C // 128) * 8192)
    bes = U.Guarded(8)
    table = torch.tensor([[w_end.data_ptr(), v.data_ptr(), scale.data_ptr(), b.data_ptr(), fold.t.data_ptr(), bes.t.data_ptr(), nj, C]],
                         dtype=torch.int64).to(DEV)
    _lib.call("t2s_wg_endfold_weights_h16", _lib.ptr(table), 1, C, _lib.current_stream())
    _sync()
    label = "endfold_h16 C%d nj%d" % (C, nj)
    want = (w_end.double().cpu() * scale.double().cpu()[None]) @ v.double().cpu()
    got = W._endfold_decode(fold.t, C)
    U.check(label + " fold_A", got[:nj, :C], want, U.GEMM_NORM, U.GEMM_MAX)
    assert float(got[nj:].abs().max()) == 0.0, label + ": rows nj .. 15 are not zero"
    if got.size(1) > C:
        assert float(got[:, C:].abs().max()) == 0.0, label + ": columns past C are not zero"
    fold.assert_guards(label)
    U.check(label + " bes", bes.t.double().cpu()[:nj], w_end.double().cpu() @ b.double().cpu(), U.F32_NORM, U.F32_MAX)
    bes.assert_guards(label)


# ---------------------------------------------------------------------------------------------- (c) the plane writers
_BL = [(2, 300), (1, 1)]


def _check_planes(label, pair, C, L, want):
    U.check(label, U.plane_values((pair[0].t, pair[1].t), C, L, HALO), want, U.GEMM_NORM, U.GEMM_MAX)
    U.assert_halo_zero((pair[0].t, pair[1].t), L, HALO, label)
    for p in pair:
        if C % 32:
            assert float(p.t[:, -1, :, C % 32:].float().abs().max()) == 0.0, label + ": channels past C were written"
        p.assert_guards(label)


@pytest.mark.parametrize("c_off,nh", [(0, 4), (6, 1)])
@pytest.mark.parametrize("B,L", _BL)
def test_start_h16(B, L, c_off, nh):
    """x = W_start z[c_off : c_off + n_half] + b as fp16 hi / lo planes against float64 of the f32 weights the kernel reads"""
    _lib.load()
    C = 36
    wn = _WN(C, 2, 3, nh, 32, seed=5 + nh)
    Lp = _lib.plane_rows(L, HALO)
    z = U.dev(torch.randn(B, G8, L, generator=torch.Generator().manual_seed(L + c_off)))
    X = (_HB(B, 2, Lp, 32), _HB(B, 2, Lp, 32))
    _lib.call("t2s_wg_start_h16", _lib.ptr(z), _lib.ptr(wn.w_start()), _lib.ptr(wn.p("start.bias")), B, G8, c_off, nh, C, L, Lp, HALO,
              _lib.ptr(X[0].t), _lib.ptr(X[1].t), _lib.current_stream())
    _sync()
    want = torch.einsum("cj,bjt->bct", wn.w_start().double().cpu(), z.double().cpu()[:, c_off:c_off + nh]) + \
        wn.p("start.bias").double().cpu()[None, :, None]
    _check_planes("start_h16 B%d L%d off%d nh%d" % (B, L, c_off, nh), X, C, L, want)


@pytest.mark.parametrize("B,L", _BL)
@pytest.mark.parametrize("n_mel,ksize,stride", [(4, 256, 64), (5, 32, 8)], ids=["matrix-core", "vector"])
def test_upsample_squeeze_h16(n_mel, ksize, stride, B, L):
    """ConvTranspose1d + squeeze by 8 as fp16 hi / lo conditioning planes against float64, on both kernels behind the entry point"""
    _lib.load()
    frames = max(1, -(-(8 * L - ksize) // stride) + 1)
    gen = torch.Generator().manual_seed(n_mel + L)
    mel, Wt, bias = torch.randn(B, n_mel, frames, generator=gen), 0.1 * torch.randn(n_mel, n_mel, ksize, generator=gen), \
        0.1 * torch.randn(n_mel, generator=gen)
    Lp = _lib.plane_rows(L, HALO)
    nchan = n_mel * 8
    nc = -(-nchan // 32)
    S = (_HB(B, nc, Lp, 32), _HB(B, nc, Lp, 32))
    mel_d, W_d, bias_d = U.dev(mel), U.dev(Wt), U.dev(bias)       # hold references: a freed temporary's block is reused at once
    _lib.call("t2s_wg_upsample_squeeze_h16", _lib.ptr(mel_d), _lib.ptr(W_d), _lib.ptr(bias_d), B, n_mel, frames, ksize,
              stride, 8, L, Lp, HALO, _lib.ptr(S[0].t), _lib.ptr(S[1].t), _lib.current_stream())
    _sync()
    up = F.conv_transpose1d(mel.double(), Wt.double(), bias.double(), stride=stride)[:, :, :8 * L]
    want = up.reshape(B, n_mel, L, 8).permute(0, 1, 3, 2).reshape(B, nchan, L)           # channel co * 8 + g at column t = up[co][8 t + g]
    _check_planes("upsample_squeeze_h16 mel%d k%d s%d B%d L%d" % (n_mel, ksize, stride, B, L), S, nchan, L, want)


# ---------------------------------------------------------------------------------------------- (d) the folded gate GEMM
def _assert_tiles(B, C, L, tile, nslots):
    lib = _lib.load()
    assert lib.t2s_wg_gate_tile_rows(B, C, L) == tile, "the tile-height rule moved this case off the %d-row kernel" % tile
    assert lib.t2s_wg_gate_fold_slots(B, C, L) == nslots, (lib.t2s_wg_gate_fold_slots(B, C, L), nslots)


def _gate_pre(w_in, w_cond, bias, x, s, dil, ks):
    """float64 (or float32: the floor) pre-activations [B, 2C, L] of decoded weights on plane values"""
    y = F.conv1d(x, w_in.to(x.dtype), None, dilation=dil, padding=(ks * dil - dil) // 2)
    if w_cond is not None:
        y = y + F.conv1d(s, w_cond.to(x.dtype)[:, :, None])
    return y + bias.to(x.dtype)[None, :, None]


def _launch_gate(wn, i, Xp, Sp, acts, fold_acc, fold_init, B, L, Lp):
    Ah, b1 = wn.gate(i)
    S = (None, None) if Sp is None else (_lib.ptr(Sp[0]), _lib.ptr(Sp[1]))
    _lib.call("t2s_wg_in_cond_gate_fold_h16", _lib.ptr(Ah), None, _lib.ptr(b1), _lib.ptr(Xp[0]), _lib.ptr(Xp[1]), S[0], S[1],
              _lib.ptr(acts[0].t), _lib.ptr(acts[1].t), _lib.ptr(wn.fold(i)[0]), _lib.ptr(fold_acc.t), fold_init, B, wn.C, wn.n_cond,
              wn.ks, 2 ** i, L, Lp, HALO, wn.Mpad1, _lib.current_stream())
    _sync()


def _check_gate(label, wn, i, Xp, Sp, acts, fold_acc, L, before=None):
    C, nh, ks = wn.C, wn.nh, wn.ks
    w_in, w_cond, bias = wn.gate_decoded(i)
    xv = U.plane_values(Xp, C, L, HALO)
    sv = U.plane_values(Sp, wn.n_cond, L, HALO) if wn.n_cond else None
    pre = _gate_pre(w_in, w_cond, bias, xv, sv, 2 ** i, ks)
    want = torch.tanh(pre[:, :C]) * torch.sigmoid(pre[:, C:])
    # the floor of the two-product accumulation, carried through the gate: the same pre-activations with each plane contracted in f32
    xh = xv.to(torch.float16).double()
    sh = sv.to(torch.float16).double() if sv is not None else None
    zb = torch.zeros_like(bias)
    pre32 = _gate_pre(w_in, w_cond, bias, xh.float(), None if sh is None else sh.float(), 2 ** i, ks).double() + \
        _gate_pre(w_in, w_cond, zb, (xv - xh).float(), None if sh is None else (sv - sh).float(), 2 ** i, ks).double()
    emu = torch.tanh(pre32[:, :C]) * torch.sigmoid(pre32[:, C:])
    floor = (U.rel(emu, want), U.maxrel(emu, want))
    nb, mb = _bars(floor)
    print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e  -> bars %.1e / %.1e" % (label + " acts (two products, f32)", floor[0], floor[1], nb, mb))
    pair = (acts[0].t, acts[1].t)
    assert bool(torch.isfinite(pair[0].float()).all()) and bool(torch.isfinite(pair[1].float()).all()), label
    got = U.plane_values(pair, C, L, HALO)
    U.check(label + " acts", got, want, nb, mb)
    U.assert_halo_zero(pair, L, HALO, label)
    for p in acts:
        if C % 32:
            assert float(p.t[:, -1, :, C % 32:].float().abs().max()) == 0.0, label + ": channels past C were written"
        p.assert_guards(label)
    # the fold (fp16 hi + lo, three products): the sum over the slots against fold_A's values times the acts planes' values
    Fd = W._endfold_decode(wn.fold(i)[0], C)[:8, :C]
    wantf = torch.einsum("jc,bct->bjt", Fd, got)
    if before is not None:
        wantf = wantf + before
    ffloor = _split3_floor_f16(Fd[:2 * nh], want.float().double(), "jc,bct->bjt")
    fnb, fmb = _bars(ffloor)
    print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e  -> bars %.1e / %.1e" % (label + " fold (three products)", ffloor[0], ffloor[1], fnb, fmb))
    fsum = fold_acc.t.double().sum(0).cpu()         # NaN if any element of any slot was not written
    U.check(label + " fold (sum over %d slots)" % fold_acc.t.size(0), fsum[:, :2 * nh], wantf[:, :2 * nh], fnb, fmb)
    if nh < 4:
        assert float(fsum[:, 2 * nh:].abs().max()) == 0.0, label + ": fold rows j >= 2 n_half are not zero"
    fold_acc.assert_guards(label)
    return wantf


def _sat(C):
    """layer 0: +30, -30, +120, -120 on the tanh rows of channels 0 .. 3 and on the sigmoid rows of channels 4 .. 7"""
    return 0, tuple(zip((0, 1, 2, 3, C + 4, C + 5, C + 6, C + 7), (30.0, -30.0, 120.0, -120.0) * 2))


# (name, B, C, n_cond, L, dilation, kernel size, tile rows, bias shift)
GATE_CASES = [
    ("128-ragged", 2, 64, 640, 300, 1, 3, 128, None),
    ("128-one-column", 1, 64, 32, 1, 128, 3, 128, None),
    ("128-three-mtiles", 3, 192, 40, 257, 32, 3, 128, None),
    ("256-C16", 2, 16, 32, 5, 1, 3, 256, None),
    ("256-C80", 3, 80, 96, 300, 2, 3, 256, None),
    ("256-C144", 1, 144, 640, 257, 128, 3, 256, None),
    ("256-nk1", 2, 16, 0, 37, 1, 1, 256, None),         # K loops of 1, 2 and 3 steps: the prologue's and the tail's wait counts
    ("256-nk2", 2, 16, 32, 37, 1, 1, 256, None),
    ("256-nk3", 2, 32, 64, 37, 1, 1, 256, None),         # the first K-step that runs the counted waits of the main loop
    ("256-saturated", 2, 80, 96, 300, 1, 3, 256, _sat(80)),
]


@pytest.mark.parametrize("name,B,C,n_cond,L,dil,ks,tile,shift", GATE_CASES, ids=[c[0] for c in GATE_CASES])
def test_in_cond_gate_fold_h16(name, B, C, n_cond, L, dil, ks, tile, shift):
    """The launch under test with fold_init = 1 on a fold_acc full of the NaN sentinel, then another layer's launch with
    fold_init = 0 on top and the float64 sum of both products; the tile height is asserted first."""
    _lib.load()
    i = int(math.log2(dil))
    assert 2 ** i == dil
    nslots = 2 * (C // 64) if tile == 128 else 2 * (-(-C // 128))
    _assert_tiles(B, C, L, tile, nslots)
    nl = max(i + 1, 2)
    wn, audio, spect, layers, _ = _case(C, nl, ks, 4, n_cond, B, L, shift)
    label = "gate_h16 %s B%d C%d S%d L%d d%d k%d" % (name, B, C, n_cond, L, dil, ks)
    Lp = _lib.plane_rows(L, HALO)
    xc = -(-C // 32)
    Sp = _to_h16(spect, Lp) if n_cond else None
    fold_acc = U.Guarded(nslots, B, 8, L)
    acts = (_HB(B, xc, Lp, 32), _HB(B, xc, Lp, 32))
    Xp = _to_h16(layers[i]["x"], Lp)
    _launch_gate(wn, i, Xp, Sp, acts, fold_acc, 1, B, L, Lp)
    first = _check_gate(label, wn, i, Xp, Sp, acts, fold_acc, L)
    j = i - 1 if i > 0 else 1
    Xp = _to_h16(layers[j]["x"], Lp)
    _launch_gate(wn, j, Xp, Sp, acts, fold_acc, 0, B, L, Lp)
    _check_gate(label + " + layer %d" % j, wn, j, Xp, Sp, acts, fold_acc, L, before=first)


# ---------------------------------------------------------------------------------------------- (e) the residual GEMM
@pytest.mark.parametrize("B,L", _BL)
@pytest.mark.parametrize("C,pair8", [(32, 0), (32, 1), (36, 0), (160, 0), (160, 1)])
def test_res_only_h16(C, pair8, B, L):
    """In place on the oracle's x_0 and acts_0 as fp16 planes: x_0 + W_res . acts_0 + b in float64 of the decoded operands"""
    _lib.load()
    wn, _, _, layers, _ = _case(C, 2, 3, 4, 32, B, L)
    ly = layers[0]
    Lp = _lib.plane_rows(L, HALO)
    xc = -(-C // 32)
    A2h, b2, Mpad2, _ = wn.res(0, bool(pair8))
    Ap = _to_h16(ly["acts"], Lp)
    X0 = _to_h16(ly["x"], Lp)
    X = (_HB(B, xc, Lp, 32), _HB(B, xc, Lp, 32))
    X[0].t.copy_(X0[0])
    X[1].t.copy_(X0[1])
    _lib.call("t2s_wg_res_only_h16", _lib.ptr(A2h), None, _lib.ptr(b2), _lib.ptr(Ap[0]), _lib.ptr(Ap[1]), _lib.ptr(X[0].t),
              _lib.ptr(X[1].t), B, C, L, Lp, HALO, Mpad2, pair8, _lib.current_stream())
    _sync()
    label = "res_only_h16 C%d pair8=%d B%d L%d" % (C, pair8, B, L)
    w_res, b_res = wn.res_decoded(0, bool(pair8))
    av, xv = U.plane_values(Ap, C, L, HALO), U.plane_values(X0, C, L, HALO)
    mm = lambda a, b: torch.einsum("oc,bct->bot", a, b)
    want = xv + mm(w_res, av) + b_res[None, :, None]
    floor = _two_product_floor(w_res, av, mm)
    print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e (of W_res . acts alone)" % (label, floor[0], floor[1]))
    nb, mb = _bars(floor)
    U.check(label, U.plane_values((X[0].t, X[1].t), C, L, HALO), want, nb, mb)
    U.assert_halo_zero((X[0].t, X[1].t), L, HALO, label)
    for p in X:
        if C % 32:
            assert float(p.t[:, -1, :, C % 32:].float().abs().max()) == 0.0, label + ": channels past C were written"
        p.assert_guards(label)


# ---------------------------------------------------------------------------------------------- (f) argument checks
def test_argument_validation_without_launching():
    """NULL planes, C % 16 != 0 and a misaligned pointer return T2S_EINVAL with nothing enqueued: the outputs keep their sentinel.
    The tuples the broken ones are made from are themselves accepted, with A_lo = NULL."""
    lib = _lib.load()
    P = _lib.ptr
    B, C, n_cond, L, taps = 1, 64, 32, 40, 3
    Lp = _lib.plane_rows(L, HALO)
    A = torch.zeros(taps * 2 + 1, 256, 32, **H16)
    bias = torch.zeros(256, device=DEV)
    Xp, Sp = torch.zeros(B, 2, Lp, 32, **H16), torch.zeros(B, 1, Lp, 32, **H16)
    fold_A = torch.zeros(8192, **H16)
    SENT = 0.375
    outs = [torch.full((B, 2, Lp, 32), SENT, **H16) for _ in range(2)]
    acc = U.Guarded(2, B, 8, L)
    st = _lib.current_stream()
    off2 = lambda t: _lib.c_vp(t.data_ptr() + 2)          # two bytes past a 16-byte boundary

    def unchanged():
        _sync()
        return all(bool((o == SENT).all()) for o in outs) and bool(acc.untouched(acc.t).all())

    def gate(**ch):
        a = dict(A_hi=P(A), A_lo=None, bias=P(bias), X_hi=P(Xp), X_lo=P(Xp), S_hi=P(Sp), S_lo=P(Sp), acts_hi=P(outs[0]), acts_lo=P(outs[1]),
                 fold_A=P(fold_A), fold_acc=P(acc.t), fold_init=1, B=B, C=C, n_cond=n_cond, taps=taps, dilation=1, L=L, Lp=Lp, halo=HALO,
                 Mpad=256, stream=st)
        a.update(ch)
        return lib.t2s_wg_in_cond_gate_fold_h16(*a.values())

    def res(**ch):
        a = dict(A_hi=P(A), A_lo=None, bias=P(bias), acts_hi=P(Xp), acts_lo=P(Xp), X_hi=P(outs[0]), X_lo=P(outs[1]), B=B, C=C, L=L, Lp=Lp,
                 halo=HALO, Mpad=256, pair8=1, stream=st)
        a.update(ch)
        return lib.t2s_wg_res_only_h16(*a.values())

    z, ws, bs = torch.zeros(B, G8, L, device=DEV), torch.zeros(C, 4, device=DEV), torch.zeros(C, device=DEV)

    def start(**ch):
        a = dict(z=P(z), w=P(ws), bias=P(bs), B=B, n_group=G8, c_off=0, n_half=4, C=C, L=L, Lp=Lp, halo=HALO, X_hi=P(outs[0]), X_lo=P(outs[1]),
                 stream=st)
        a.update(ch)
        return lib.t2s_wg_start_h16(*a.values())

    bad = [(gate, dict(A_hi=None)), (gate, dict(X_hi=None)), (gate, dict(X_lo=None)), (gate, dict(S_lo=None)), (gate, dict(acts_hi=None)),
           (gate, dict(acts_lo=None)), (gate, dict(fold_A=None)), (gate, dict(fold_acc=None)), (gate, dict(bias=None)),
           (gate, dict(C=24)), (gate, dict(C=40)),
           (gate, dict(A_hi=off2(A))), (gate, dict(X_lo=off2(Xp))), (gate, dict(acts_hi=off2(outs[0]))), (gate, dict(fold_A=off2(fold_A))),
           (gate, dict(Lp=Lp + 1)), (gate, dict(dilation=HALO + 1)),
           (res, dict(A_hi=None)), (res, dict(acts_lo=None)), (res, dict(X_hi=None)), (res, dict(X_lo=None)), (res, dict(bias=None)),
           (res, dict(A_hi=off2(A))), (res, dict(X_hi=off2(outs[0]))), (res, dict(C=48, pair8=1)), (res, dict(C=30, pair8=0)),
           (res, dict(Lp=Lp - 1)),
           (start, dict(X_hi=None)), (start, dict(X_lo=None)), (start, dict(X_lo=off2(outs[1]))), (start, dict(z=None)),
           (start, dict(Lp=Lp - 1))]
    for fn, ch in bad:
        assert fn(**ch) == -1, "%s accepted %r" % (fn.__name__, ch)
        assert unchanged(), "%s wrote something with %r" % (fn.__name__, ch)
    assert lib.t2s_pack_conv_weight_table_h16(None, 1, 1, st) == -1 and lib.t2s_wg_endfold_weights_h16(None, 1, C, st) == -1
    # the tuples themselves are accepted (zero operands: the launches are harmless)
    for fn in (gate, res, start):
        assert fn() == 0, fn.__name__
    assert res(C=48, pair8=0) == 0
    _sync()
