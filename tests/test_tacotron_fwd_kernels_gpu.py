"""The Tacotron forward kernels one by one through the C ABI (run with -m gpu on an MI355X), each against a plain float64
restatement of the same operation on the CPU (never another kernel of this library), off the model's reference shape: at the
kernels' tile edges, at K loops shorter than their pipelines and at the sizes where the launchers change kernels.  Every compared
output goes through wg_bwd_util.check (norm-relative error AND the maximum error relative to the expectation's largest element)
after a `PARITY ...` line with both figures; f32 outputs live in Guarded buffers (NaN sentinel inside, guard words either side);
plane outputs start from marked planes, so rows and padded channels that must not be written are compared by bits.

Which kernel a case launches:
  conv_gemm_kernel<EPI_BIAS_ACT, 128, false, 3>  section 1, every case of _CONV with B < 65 (at most 64 workgroups of 256-row tiles);
                                                 its three-stage prologue at 1, 2, 3 K-steps: the rows marked nk = 1 / 2 / 3
  conv_gemm_kernel<EPI_BIAS_ACT, 256>            section 1, the B = 65 rows (65 workgroups: one past bias_act_tile_rows' switch)
  gemv_rows_kernel<1>, grid.y 1 / 16 / 64        section 2, K = 20 with 63 / 64, 65 / 4100 items
  gemv_rows_kernel<1 2 4 7 10 16>                section 2, 3 items, K on both sides of 256 / 512 / 1024 / 1792 / 2560, and 4096
  sbgemm_plain_kernel<16 | 32> and their 16-item forms  section 2, 9 / 32 / 33 items with K = 16 and 48 (16 + 16 + 16) and K = 96 (32 + 32 + 32);
                                                 2100 rows x 33 items: the form with 32 items per workgroup, second block one item deep
  f32_to_planes / embed_planes / transpose / zero_plane_rows / zero_rows_f32 / parse_output / bn_fold / bernoulli_mask /
  stop_check kernels                             section 3, one test each, and their refusals
  t2s_taco_decode_steps                          section 4: the table in front of it

Bars: the split-bf16 GEMM at wg_bwd_util.GEMM_NORM = 2e-5 / GEMM_MAX = 1e-4 against float64 of the values its operand planes hold;
the f32 kernels at F32_NORM = 1e-5 / F32_MAX = 1e-4.  A plane pair against the f32 value it was split from: per element
|x - (hi + lo)| <= 2^-16 |x| + 2^-133, from split_bf16 as written (t2s_common.h): hi = bf16(x) rounds to nearest with an 8-bit
significand, so r = x - hi (exact in f32) has |r| <= 2^-8 |x|; lo = bf16(r) rounds r the same way, |r - lo| <= 2^-8 |r|, or half of
bf16's smallest subnormal (2^-134) where r is below its normal range.  profiles/tacotron_fwd_kernel_parity.md has the measured
figures."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wg_bwd_util as U
from taco_ref_util import att_step, lstm, ragged
from text2speech_amd import _lib
from text2speech_amd.tacotron.tacotron import _DecoderStruct
from wg_bwd_util import DEV, F32_MAX, F32_NORM, GEMM_MAX, GEMM_NORM, Guarded, check, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
ptr = _lib.ptr
_PLANE_MARK = 7.0           # what plane outputs hold before a call: a written halo row or an unwritten data row shows
_SPLIT_REL, _SPLIT_ABS = 2.0 ** -16, 2.0 ** -133


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _sync():
    torch.cuda.synchronize()


def _st():
    return _lib.current_stream()


class _Checks:
    """Every check of a case runs (and prints its figures); done() then fails with all that missed."""

    def __init__(self, norm_bar=F32_NORM, max_bar=F32_MAX):
        self.failed, self.bars = [], (norm_bar, max_bar)

    def __call__(self, label, got, want):
        try:
            check(label, got, want, *self.bars)
        except AssertionError as e:
            self.failed.append(str(e))

    def ok(self, cond, msg):
        if not bool(cond):
            self.failed.append(msg)

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def _marked_planes(B, C, Lp):
    mk = lambda: torch.full((B, -(-C // 32), Lp, 32), _PLANE_MARK, dtype=torch.bfloat16, device=DEV)
    return mk(), mk()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _planes_untouched_outside(ck, pair, C, L, halo, tag, pad_zero):
    """Rows in front of and behind the data still hold the mark; channels C .. 32 ceil(C / 32) of the data rows are zero
    (pad_zero: the kernel is documented to clear them) or still hold the mark (it must not write them)."""
    for p in pair:
        ck.ok(bool((p[:, :, :halo].float() == _PLANE_MARK).all()) and bool((p[:, :, halo + L:].float() == _PLANE_MARK).all()),
              tag + ": rows outside [halo, halo + L) were written")
        if C % 32:
            pad = p[:, -1, halo:halo + L, C % 32:].float()
            ck.ok(bool((pad == (0.0 if pad_zero else _PLANE_MARK)).all()),
                  tag + (": channels past C are not zero" if pad_zero else ": channels past C were written"))


def _split_ok(ck, pair, src, C, L, halo, tag):
    """hi + lo of the data rows against the f32 values they were split from, element by element."""
    got = U.plane_values(pair, C, L, halo)
    src = torch.as_tensor(src).double().cpu()
    err = (got - src).abs()
    bound = src.abs() * _SPLIT_REL + _SPLIT_ABS
    print("PARITY %-60s worst |x - (hi + lo)| / |x| %.3e (bound %.3e)" % (tag, float((err / (src.abs() + 1e-300)).max()), _SPLIT_REL))
    ck.ok(bool(torch.isfinite(got).all()) and bool((err <= bound).all()), tag + ": hi + lo is further from its f32 source than split_bf16 allows")


# ============================================================================================================ 1. t2s_conv_bias_act
# (B, Cin, Cout, taps, dilation, halo, L, act, outputs); nk = taps * ceil(Cin / 32) K-steps.  128-row tiles with three LDS stages
# unless B = 65 (65 workgroups of 256-row tiles: the two-stage 256-row kernel).
_CONV = [
    # the three-stage prologue: nk = 1, 2, 3, then 4, 5 and 20
    (1, 8, 4, 1, 1, 0, 17, 0, "f32"),                # nk 1
    (1, 40, 80, 1, 1, 0, 33, 1, "planes"),           # nk 2
    (1, 8, 132, 3, 1, 1, 50, 2, "cl"),               # nk 3
    (1, 100, 80, 1, 1, 0, 31, 0, "planes+cl"),       # nk 4
    (1, 20, 260, 5, 1, 2, 40, 1, "f32"),             # nk 5
    (1, 100, 132, 5, 1, 2, 64, 2, "planes"),         # nk 20
    # Cin 33 / 80: a padded last chunk; halo wider than the taps need; dilation 4
    (2, 33, 80, 5, 1, 2, 70, 0, "planes+cl"),
    (2, 80, 4, 5, 1, 8, 20, 1, "f32"),
    (1, 80, 260, 3, 4, 4, 100, 2, "cl"),
    (2, 33, 132, 3, 4, 4, 19, 0, "planes"),
    # 256-row tiles: B = 65, L = 5
    (65, 8, 260, 1, 1, 0, 5, 0, "planes+cl"),
    (65, 8, 8, 1, 1, 0, 5, 1, "f32"),
    (65, 33, 260, 3, 1, 1, 5, 2, "planes"),
    (65, 40, 8, 5, 1, 2, 5, 0, "cl"),
    (65, 100, 132, 1, 1, 0, 5, 1, "planes+cl"),
    (65, 8, 4, 3, 4, 4, 5, 2, "f32"),
    # the time-tile edge and the batch stride: L = 1, 255, 256, 257 at B = 2
    (2, 33, 80, 5, 1, 2, 1, 0, "planes+cl"),
    (2, 33, 80, 5, 1, 2, 255, 1, "f32"),
    (2, 33, 80, 5, 1, 2, 256, 2, "planes"),
    (2, 33, 80, 5, 1, 2, 257, 0, "cl"),
    (2, 8, 132, 3, 4, 4, 1, 1, "f32"),
    (2, 8, 132, 3, 4, 4, 255, 2, "planes+cl"),
    (2, 8, 132, 3, 4, 4, 256, 0, "cl"),
    (2, 8, 132, 3, 4, 4, 257, 1, "planes"),
    (2, 80, 260, 1, 1, 0, 1, 2, "cl"),
    (2, 80, 260, 1, 1, 0, 255, 0, "planes"),
    (2, 80, 260, 1, 1, 0, 256, 1, "planes+cl"),
    (2, 80, 260, 1, 1, 0, 257, 2, "f32"),
    # every output form and activation at the short K loops
    (1, 8, 80, 1, 1, 0, 16, 2, "planes"),
    (1, 8, 260, 1, 1, 0, 48, 1, "cl"),
    (1, 40, 4, 1, 1, 0, 15, 2, "planes+cl"),
    (1, 40, 132, 1, 1, 0, 257, 0, "f32"),
    (1, 8, 80, 3, 1, 1, 255, 0, "planes"),
    (1, 8, 260, 3, 4, 4, 256, 1, "planes+cl"),
    (3, 100, 4, 1, 1, 0, 7, 2, "cl"),
    (1, 20, 80, 5, 1, 8, 33, 2, "f32"),
    (1, 80, 132, 5, 1, 2, 257, 1, "planes+cl"),
    (2, 80, 80, 5, 1, 2, 64, 0, "cl"),
    (1, 33, 260, 1, 1, 0, 1, 0, "planes"),
    (1, 20, 8, 5, 1, 2, 256, 2, "cl"),
]


def _act64(v, act):
    return (v, torch.relu(v), torch.tanh(v))[act]


@pytest.mark.parametrize("B,Cin,Cout,taps,dil,halo,L,act,outs", _CONV)
def test_conv_bias_act(lib, B, Cin, Cout, taps, dil, halo, L, act, outs):
    """Operands through t2s_f32_to_planes and t2s_pack_conv_weight (PERM_NONE); the expectation is float64 conv1d of the values
    the X planes and the packed A hold (channels below Cin only: what pads the last chunk must contribute nothing)."""
    g = torch.Generator().manual_seed(11000 + B + 3 * Cin + 5 * Cout + 7 * taps + 11 * dil + 13 * halo + 17 * L + act)
    Cpad, Mpad, Lp = -(-Cin // 32) * 32, _lib.padded_rows(Cout), _lib.plane_rows(L, halo)
    w = torch.randn(Cout, Cin, taps, generator=g) / (Cin * taps) ** 0.5
    bias, x = torch.randn(Cout, generator=g) * 0.3, torch.randn(B, Cin, L, generator=g)
    A = [torch.zeros(taps * Cpad // 32, Mpad, 32, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    bias_d = torch.zeros(Mpad, device=DEV)
    d_w, d_b, d_x = dev(w), dev(bias), dev(x)
    _lib.call("t2s_pack_conv_weight", ptr(d_w), None, 0, ptr(d_b), Cout, Cin, taps, 0, 0, 0, Mpad, 0, Cpad, ptr(A[0]), ptr(A[1]),
              ptr(bias_d), 0, _st())
    X = [torch.zeros(B, Cpad // 32, Lp, 32, dtype=torch.bfloat16, device=DEV) for _ in range(2)]      # (the halo is the zero padding)
    _lib.call("t2s_f32_to_planes", ptr(d_x), B, Cin, L, Lp, halo, ptr(X[0]), ptr(X[1]), _st())
    _sync()
    Wv = U.packed_values(A[0], A[1], Cout, taps * Cpad).view(Cout, taps, Cpad)[:, :, :Cin].permute(0, 2, 1).contiguous()
    Xv = U.plane_values(X, Cin, L, halo)
    want = _act64(F.conv1d(Xv, Wv, bias_d[:Cout].double().cpu(), padding=(taps // 2) * dil, dilation=dil), act)      # [B, Cout, L]
    tag = "conv_bias_act[B=%d Cin=%d Cout=%d taps=%d dil=%d halo=%d L=%d act=%d %s]" % (B, Cin, Cout, taps, dil, halo, L, act, outs)
    ck = _Checks(GEMM_NORM, GEMM_MAX)
    cl = outs in ("cl", "planes+cl")

    def run(with_planes, with_f32):
        O = _marked_planes(B, Cout, Lp) if with_planes else (None, None)
        out = (Guarded(B, L, Cout) if cl else Guarded(B, Cout, L)) if with_f32 else None
        _lib.call("t2s_conv_bias_act", ptr(A[0]), ptr(A[1]), ptr(bias_d), ptr(X[0]), ptr(X[1]), ptr(O[0]), ptr(O[1]),
                  ptr(out.t) if out else None, int(cl), B, Cin, Cout, taps, dil, act, L, Lp, halo, Mpad, _st())
        _sync()
        return O, out

    O, out = run(outs != "f32" and outs != "cl", outs != "planes")
    if out is None:         # planes only: the f32 values they were split from come out of a second call on the same operands
        _, out = run(False, True)
    got = out.t.permute(0, 2, 1) if cl else out.t
    ck(tag + " out_f32", got, want)
    out.assert_guards(tag + " out_f32")
    if O[0] is not None:
        _split_ok(ck, O, got, Cout, L, halo, tag + " planes vs out_f32")
        _planes_untouched_outside(ck, O, Cout, L, halo, tag + " planes", pad_zero=False)
    ck.done()


def test_conv_bias_act_refusals(lib):
    """T2S_EINVAL in front of the launch, nothing written: a halo narrower than the taps reach, Cout not a multiple of 4, Lp that is
    not t2s_plane_rows(L, halo), Mpad not a multiple of 256, act = 3, no output at all, O_hi without O_lo."""
    B, Cin, Cout, L, halo = 1, 8, 8, 9, 2
    Mpad, Lp = _lib.padded_rows(Cout), _lib.plane_rows(L, halo)
    A = [torch.zeros(5, Mpad, 32, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    X = [torch.zeros(B, 1, Lp + 64, 32, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    bias = torch.zeros(Mpad, device=DEV)
    O, out = _marked_planes(B, Cout, Lp + 64), Guarded(B, Cout, L)
    base = dict(O_hi=ptr(O[0]), O_lo=ptr(O[1]), out=ptr(out.t), Cout=Cout, taps=5, dil=1, act=0, Lp=Lp, halo=halo, Mpad=Mpad)
    for name, change in (("halo < reach", dict(dil=2)), ("Cout % 4", dict(Cout=6)), ("Lp", dict(Lp=Lp + 64)), ("Mpad", dict(Mpad=128)),
                         ("act", dict(act=3)), ("no output", dict(O_hi=None, O_lo=None, out=None)), ("O_lo NULL", dict(O_lo=None)),
                         ("even taps", dict(taps=4))):
        a = dict(base, **change)
        rc = lib.t2s_conv_bias_act(ptr(A[0]), ptr(A[1]), ptr(bias), ptr(X[0]), ptr(X[1]), a["O_hi"], a["O_lo"], a["out"], 0, B, Cin,
                                   a["Cout"], a["taps"], a["dil"], a["act"], L, a["Lp"], a["halo"], a["Mpad"], _st())
        _sync()
        assert rc == EINVAL, (name, rc)
        assert bool(out.untouched(out.t).all()) and all(bool((p.float() == _PLANE_MARK).all()) for p in O), name + ": written on refusal"
    out.assert_guards("conv_bias_act refusals")


# ===================================================================================================================== 2. t2s_gemv
def _flat_rows(g, n_rows, n, stride, scale=1.0):
    """A flat f32 buffer whose row i is buf[i * stride : i * stride + n] (stride < n: the rows overlap), and the rows as [n_rows, n]."""
    buf = torch.randn((n_rows - 1) * stride + n, generator=g) * scale
    return buf, torch.as_strided(buf, (n_rows, n), (stride, 1))


def _gemv(lib, tag, rows, items, ns, k1, ld_extra=(4, 8), sx=None, act=0, bias=(True, False), mask=False, transposed=False, seed=0):
    """One t2s_gemv call against float64.  ns = (n1, n2, n3) input segments, W1 holds the first k1 columns (row stride k1 +
    ld_extra[0]), W2 the rest; sx: item strides of the segments (default n + 4); transposed: sy_row = items, sy_item = 1; mask:
    bytes with an item stride of rows + 3 and mask_scale 2."""
    K = sum(ns)
    k2 = K - k1
    g = torch.Generator().manual_seed(21000 + seed + rows + 3 * items + 5 * K + act)
    sx = sx or tuple(n + 4 for n in ns)
    W1 = torch.randn(rows, k1 + ld_extra[0], generator=g) / K ** 0.5
    W2 = torch.randn(rows, k2 + ld_extra[1], generator=g) / K ** 0.5 if k2 else None
    segs = [_flat_rows(g, items, n, s) if n else (None, None) for n, s in zip(ns, sx)]
    b = [torch.randn(rows, generator=g) * 0.3 if on else None for on in bias]
    m = (torch.rand(items, rows + 3, generator=g) >= 0.4).to(torch.uint8) if mask else None
    Wfull = torch.cat([W1[:, :k1]] + ([W2[:, :k2]] if k2 else []), 1).double()
    xfull = torch.cat([v for _, v in segs if v is not None], 1).double()
    want = xfull @ Wfull.t() + sum(t.double() for t in b if t is not None) if any(bias) else xfull @ Wfull.t()
    want = _act64(want, act)
    if mask:
        want = want * m[:, :rows].double() * 2.0
    sy_item, sy_row = (1, items) if transposed else (rows + 5, 1)
    n_out = (items - 1) * sy_item + (rows - 1) * sy_row + 1
    y = Guarded(n_out)
    d = [None if t is None else dev(t) for t in (W1, W2, segs[0][0], segs[1][0], segs[2][0], b[0], b[1], m)]
    _lib.call("t2s_gemv", ptr(d[0]), W1.size(1), k1, ptr(d[1]), W2.size(1) if k2 else 0, k2, ptr(d[2]), ns[0], sx[0], ptr(d[3]), ns[1],
              sx[1] if ns[1] else 0, ptr(d[4]), ns[2], sx[2] if ns[2] else 0, ptr(d[5]), ptr(d[6]), ptr(y.t), sy_item, sy_row, rows, items,
              act, ptr(d[7]), rows + 3 if mask else 0, 2.0 if mask else 1.0, _st())
    _sync()
    got = torch.as_strided(y.t, (items, rows), (sy_item, sy_row))
    ck = _Checks()
    ck(tag, got, want)
    if mask:
        ck.ok(float(got.cpu()[m[:, :rows] == 0].abs().sum()) == 0.0, tag + ": a masked output is not exactly 0")
    written = torch.zeros(n_out, dtype=torch.bool)
    torch.as_strided(written, (items, rows), (sy_item, sy_row)).fill_(True)
    ck.ok(bool(y.untouched(y.t).cpu()[~written].all()), tag + ": wrote between the outputs")
    y.assert_guards(tag)
    ck.done()


@pytest.mark.parametrize("items", [63, 64, 65, 4100])
def test_gemv_wave_per_row_many_items(lib, items):
    """K = 20 is no multiple of 16, so more than 8 items stay on gemv_rows_kernel: grid.y = 1 (63), 16 (64, 65), 64 (4100)."""
    _gemv(lib, "gemv[K=20 rows=5 items=%d]" % items, 5, items, (20, 0, 0), 20, act=1)


def _three_way(K):
    """K as three segments (multiples of 4) over two weight blocks whose boundary lies inside the second segment."""
    n1, n2 = (K // 3) & ~3, (K // 4) & ~3
    return (n1, n2, K - n1 - n2), n1 + ((n2 // 2) & ~3)


@pytest.mark.parametrize("K", [256, 260, 512, 516, 1024, 1028, 1792, 1796, 2560, 2564, 4096])
def test_gemv_register_tile_boundaries(lib, K):
    """gemv_rows_kernel<NV4> for NV4 = ceil(K / 256) rounded up to 1, 2, 4, 7, 10, 16: K at and 4 past each boundary, 3 items,
    7 rows (the second workgroup has one idle wave)."""
    ns, k1 = _three_way(K)
    _gemv(lib, "gemv[K=%d=%d+%d+%d k1=%d rows=7 items=3]" % (K, *ns, k1), 7, 3, ns, k1, bias=(True, True))


@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemv_epilogue(lib, act):
    """bias1 + bias2, the activation, and a mask whose item stride is wider than the rows, scaled by 2."""
    _gemv(lib, "gemv[K=40 rows=6 items=5 act=%d mask bias2]" % act, 6, 5, (16, 12, 12), 24, act=act, bias=(True, True), mask=True)
    _gemv(lib, "gemv[K=40 rows=6 items=5 act=%d no bias]" % act, 6, 5, (16, 12, 12), 24, act=act, bias=(False, False), seed=1)


def test_gemv_strides(lib):
    """Transposed output (sy_row = items, sy_item = 1), and items that overlap in memory (sx1 = 8 < n1 = 32: the framing of
    audio_ops.hip)."""
    _gemv(lib, "gemv[transposed output]", 6, 5, (32, 8, 0), 40, transposed=True, bias=(True, False))
    _gemv(lib, "gemv[sx1=8 < n1=32]", 6, 70, (32, 0, 0), 32, sx=(8, 0, 0), ld_extra=(4, 0), act=2)
    _gemv(lib, "gemv[sx1=8 < n1=32, K=36: wave per row]", 6, 70, (36, 0, 0), 36, sx=(8, 0, 0), ld_extra=(4, 0), seed=2)


@pytest.mark.parametrize("items", [9, 32, 33])
@pytest.mark.parametrize("ns,k1", [((16, 0, 0), 16), ((16, 16, 16), 32), ((32, 32, 32), 64)])
def test_gemv_matrix_core(lib, items, ns, k1):
    """K % 16 == 0 and more than 8 items: sbgemm_plain_kernel (16 k per step; 32 where every segment is a multiple of 32), 17 rows:
    the second 16-row tile holds one row.  Epilogue as above; the output transposed for the three-segment shapes."""
    K = sum(ns)
    _gemv(lib, "gemv[mfma K=%d items=%d rows=17]" % (K, items), 17, items, ns, k1, act=2 if K == 16 else 1, bias=(True, True),
          mask=True, transposed=K != 16)


@pytest.mark.parametrize("n", [16, 32])
def test_gemv_matrix_core_full_item_blocks(lib, n):
    """2100 rows x 33 items: too many workgroups for the 16-item form, so 32 items per workgroup and a second block one item deep."""
    _gemv(lib, "gemv[mfma K=%d items=33 rows=2100]" % (3 * n), 2100, 33, (n, n, n), 2 * n, bias=(True, False))


def test_gemv_refusals(lib):
    """T2S_EINVAL with the output untouched: K = 4100, an n that is no multiple of 4, k1 + k2 != K, act = 3, an x1 that is not
    16-byte aligned."""
    W, x, y = torch.zeros(2, 4200, device=DEV), torch.zeros(3 * 4200 + 8, device=DEV), Guarded(3, 2)

    def call(K=32, n1=None, k1=None, act=0, x_off=0):
        n1 = K if n1 is None else n1
        rc = lib.t2s_gemv(ptr(W), 4200, K if k1 is None else k1, None, 0, 0, ctypes.c_void_p(x.data_ptr() + x_off), n1, 4200, None, 0, 0,
                          None, 0, 0, None, None, ptr(y.t), 2, 1, 2, 3, act, None, 0, 1.0, _st())
        _sync()
        return rc

    for name, kw in (("K = 4100", dict(K=4100)), ("n1 = 18", dict(K=18)), ("k1 + k2 != K", dict(K=32, k1=28)), ("act = 3", dict(act=3)),
                     ("x1 + 4 bytes", dict(x_off=4))):
        assert call(**kw) == EINVAL, name
        assert bool(y.untouched(y.t).all()), name + ": written on refusal"
    assert call() == 0 and not bool(y.untouched(y.t).any())        # (the same call without the fault goes through)
    y.assert_guards("gemv refusals")


# ==================================================================================================== 3. the small forward kernels
@pytest.mark.parametrize("halo", [0, 2])
@pytest.mark.parametrize("L", [1, 63, 64, 65])
@pytest.mark.parametrize("C", [1, 33, 80])
def test_f32_to_planes(lib, C, L, halo):
    B, Lp = 2, _lib.plane_rows(L, halo)
    x = torch.randn(B, C, L, generator=torch.Generator().manual_seed(31000 + C + L))
    d_x, X = dev(x), _marked_planes(B, C, Lp)
    _lib.call("t2s_f32_to_planes", ptr(d_x), B, C, L, Lp, halo, ptr(X[0]), ptr(X[1]), _st())
    _sync()
    tag, ck = "f32_to_planes[C=%d L=%d halo=%d]" % (C, L, halo), _Checks()
    _split_ok(ck, X, x, C, L, halo, tag)
    _planes_untouched_outside(ck, X, C, L, halo, tag, pad_zero=True)
    ck.done()


@pytest.mark.parametrize("halo", [0, 2])
@pytest.mark.parametrize("T", [1, 63, 64, 65])
@pytest.mark.parametrize("E", [1, 33, 80])
def test_embed_planes(lib, E, T, halo):
    """Ids with repeats (11 symbols); an id past the table and a negative id read row 0 (embed_planes_kernel clamps them there)."""
    B, V, Lp = 2, 11, _lib.plane_rows(T, halo)
    g = torch.Generator().manual_seed(32000 + E + T)
    emb, ids = torch.randn(V, E, generator=g), torch.randint(0, V, (B, T), generator=g)
    ids[0, 0], ids[1, -1] = V + 5, -3
    want = emb[torch.where((ids < 0) | (ids >= V), torch.zeros_like(ids), ids)].permute(0, 2, 1)          # [B, E, T]
    d_e, d_i, X = dev(emb), dev(ids), _marked_planes(B, E, Lp)
    _lib.call("t2s_embed_planes", ptr(d_i), ptr(d_e), B, T, E, V, Lp, halo, ptr(X[0]), ptr(X[1]), _st())
    _sync()
    tag, ck = "embed_planes[E=%d T=%d halo=%d]" % (E, T, halo), _Checks()
    _split_ok(ck, X, want, E, T, halo, tag)
    _planes_untouched_outside(ck, X, E, T, halo, tag, pad_zero=True)
    ck.done()


@pytest.mark.parametrize("R,C", [(1, 1), (31, 33), (32, 32), (33, 65), (513, 7)])
def test_transpose(lib, R, C):
    x = torch.randn(R, C, generator=torch.Generator().manual_seed(33000 + R))
    d_x, out = dev(x), Guarded(C, R)
    _lib.call("t2s_transpose", ptr(d_x), ptr(out.t), R, C, _st())
    _sync()
    assert torch.equal(out.t.cpu(), x.t().contiguous()), "transpose[%d x %d] is not exact" % (R, C)
    out.assert_guards("transpose")


def _ragged_lengths(T):
    """0, T, past T, one that ends inside a 64-row block, and the block edge itself where T reaches it."""
    return [0, T, T + 9, min(T, 100) if T > 128 else T // 2, min(T, 64)]


@pytest.mark.parametrize("T", [1, 64, 65, 257])
def test_zero_plane_rows(lib, T):
    B, C, halo = 5, 40, 3
    Lp = _lib.plane_rows(T, halo)
    g = torch.Generator().manual_seed(34000 + T)
    lens = _ragged_lengths(T)
    X = [dev(torch.randn(B, 2, Lp, 32, generator=g).bfloat16()) for _ in range(2)]         # halo rows hold values too
    before = [p.clone() for p in X]
    d_len = dev(torch.tensor(lens, dtype=torch.int32))
    _lib.call("t2s_zero_plane_rows", ptr(X[0]), ptr(X[1]), ptr(d_len), B, C, T, Lp, halo, _st())
    _sync()
    for p, p0 in zip(X, before):
        want = p0.clone()
        for b, n in enumerate(lens):
            want[b, :, halo + min(n, T):halo + T] = 0
        assert torch.equal(_bits(p), _bits(want)), "zero_plane_rows[T=%d]: a kept row changed or a row past the length is not zero" % T


@pytest.mark.parametrize("T", [1, 64, 65, 257])
def test_zero_rows_f32_and_parse_output(lib, T):
    B, row, n_mel = 5, 7, 5
    g = torch.Generator().manual_seed(35000 + T)
    lens = _ragged_lengths(T)
    d_len = dev(torch.tensor(lens, dtype=torch.int32))
    keep = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]                            # [B, T]
    x0 = torch.randn(B, T, row, generator=g)
    x = Guarded(B, T, row, fill=dev(x0))
    _lib.call("t2s_zero_rows_f32", ptr(x.t), ptr(d_len), B, T, row, _st())
    mel0, post0, gate0 = torch.randn(B, n_mel, T, generator=g), torch.randn(B, n_mel, T, generator=g), torch.randn(B, T, generator=g)
    mel, post, gate = Guarded(B, n_mel, T, fill=dev(mel0)), Guarded(B, n_mel, T, fill=dev(post0)), Guarded(B, T, fill=dev(gate0))
    _lib.call("t2s_taco_parse_output", ptr(mel.t), ptr(post.t), ptr(gate.t), ptr(d_len), B, n_mel, T, _st())
    _sync()
    z = torch.zeros(())
    assert torch.equal(x.t.cpu(), torch.where(keep[:, :, None], x0, z)), "zero_rows_f32[T=%d]" % T
    assert torch.equal(mel.t.cpu(), torch.where(keep[:, None, :], mel0, z)), "parse_output[T=%d] mel" % T
    assert torch.equal(post.t.cpu(), torch.where(keep[:, None, :], post0, z)), "parse_output[T=%d] mel_post" % T
    assert torch.equal(gate.t.cpu(), torch.where(keep, gate0, torch.full((), 1e3))), "parse_output[T=%d] gate" % T
    for name, gd in (("x", x), ("mel", mel), ("mel_post", post), ("gate", gate)):
        gd.assert_guards("zero_rows_f32 / parse_output " + name)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_bn_fold(lib, C, with_bias):
    g = torch.Generator().manual_seed(36000 + C)
    gamma, beta, mean = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g), torch.randn(C, generator=g)
    var, cb, eps = torch.rand(C, generator=g) + 0.05, torch.randn(C, generator=g), 1e-5
    d = [dev(t) for t in (gamma, beta, mean, var, cb)]
    scale, bias = Guarded(C), Guarded(C)
    _lib.call("t2s_bn_fold", ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]) if with_bias else None, eps, C, ptr(scale.t),
              ptr(bias.t), _st())
    _sync()
    s64 = gamma.double() / torch.sqrt(var.double() + float(np.float32(eps)))
    tag, ck = "bn_fold[C=%d bias=%d]" % (C, with_bias), _Checks()
    ck(tag + " scale", scale.t, s64)
    ck(tag + " bias", bias.t, ((cb.double() if with_bias else 0.0) - mean.double()) * s64 + beta.double())
    scale.assert_guards(tag + " scale")
    bias.assert_guards(tag + " bias")
    ck.done()


def _hash_mask(n, seed, offset, keep_prob):
    """bernoulli_mask_kernel's counter hash in numpy uint64 (wrapping arithmetic): 24 bits of the mixed counter against
    keep_prob * 2^24 evaluated in float32."""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(offset)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    thr = np.uint64(int(np.float32(keep_prob) * np.float32(16777216.0)))
    return ((x >> np.uint64(40)) < thr).astype(np.uint8)


def _device_mask(n, seed, offset, keep_prob):
    """The kernel's bytes, written into the middle of a buffer of 0xAB bytes whose 64 bytes either side must not change."""
    buf = torch.full((n + 128,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.call("t2s_bernoulli_mask", ctypes.c_void_p(buf.data_ptr() + 64), n, seed, offset, keep_prob, _st())
    _sync()
    buf = buf.cpu().numpy()
    assert (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all(), "bernoulli_mask[n=%d]: wrote outside the mask" % n
    return buf[64:64 + n]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_bernoulli_mask_bits(lib, n):
    seed, k = 0x123456789ABCDEF, 1000
    for p in (0.5, 0.9):
        got = _device_mask(n, seed, 0, p)
        assert np.array_equal(got, _hash_mask(n, seed, 0, p)), "bernoulli_mask[n=%d p=%.1f] differs from the hash" % (n, p)
        # offset continuity: mask(n, offset = k)[i] == mask(n + k, offset = 0)[i + k]
        assert np.array_equal(_device_mask(n, seed, k, p), _device_mask(n + k, seed, 0, p)[k:]), "bernoulli_mask[n=%d]: offset" % n
    assert (_device_mask(n, seed, 0, 1.0) == 1).all(), "bernoulli_mask[n=%d]: keep_prob = 1 is not all ones" % n


@pytest.mark.parametrize("p", [0.5, 0.9])
def test_bernoulli_mask_mean(lib, p):
    """2^20 draws: the mean within 5 standard deviations sqrt(p (1 - p) / n) of p (the threshold is p to within 2^-24)."""
    n = 1 << 20
    mean = float(_device_mask(n, 77, 0, p).mean())
    sd = (p * (1 - p) / n) ** 0.5
    print("PARITY bernoulli_mask mean at keep_prob %.1f: %.6f (5 sd = %.6f)" % (p, mean, 5 * sd))
    assert abs(mean - p) < 5 * sd


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_stop_check(lib, n):
    """Gates at -5 (sigmoid 0.007) except the hits at +5 (0.993), threshold 0.5; the mel rows and the gate row outside
    [step0, step0 + n) hold +5 everywhere: a read of the wrong row or step shows as a hit that is not there."""
    B, n_mel, step0 = 6, 3, 3
    T_cap = step0 + n + 2
    mg = torch.full((B, n_mel + 1, T_cap), 5.0)
    mg[:, n_mel, step0:step0 + n] = -5.0
    second = step0 + (64 + 3 if n > 67 else n // 2)          # in the second 64-lane pass where there is one
    hits = [step0, step0 + n - 1, None, second, step0, step0 + n - 1]
    for b, h in enumerate(hits):
        if h is not None:
            mg[b, n_mel, h] = 5.0
    mg[3, n_mel, second + 1:step0 + n] = 5.0                  # later hits do not move the first one
    start = [-1, -1, -1, -1, 2, 0]                            # entries 4 and 5 are decided already: left alone
    want = [h if s < 0 and h is not None else s for h, s in zip(hits, start)]
    d_mg = dev(mg)
    stop = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    stop[1:B + 1] = torch.tensor(start, dtype=torch.int32)
    _lib.call("t2s_taco_stop_check", ptr(d_mg), B, n_mel, T_cap, step0, n, 0.5, ctypes.c_void_p(stop.data_ptr() + 4), _st())
    _sync()
    assert stop.cpu().tolist() == [-7] + want + [-7], "stop_check[n=%d]" % n


def test_small_kernel_refusals(lib):
    """What the entry points of t2s_api_taco.hip refuse: T2S_EINVAL and nothing written."""
    f, planes = Guarded(64), _marked_planes(1, 32, 256 + 4)
    src = torch.zeros(4096, device=DEV)
    ids, lens = torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    bytes_ = torch.full((64,), 0xAB, dtype=torch.uint8, device=DEV)
    stop = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    P, S, st = ptr(planes[0]), ptr(src), _st()
    off2 = ctypes.c_void_p(planes[0].data_ptr() + 2)
    calls = [
        ("transpose in NULL", lambda: lib.t2s_transpose(None, ptr(f.t), 4, 4, st)),
        ("transpose R = 0", lambda: lib.t2s_transpose(S, ptr(f.t), 0, 4, st)),
        ("embed ids NULL", lambda: lib.t2s_embed_planes(None, S, 1, 4, 8, 4, 260, 2, P, ptr(planes[1]), st)),
        ("embed T = 0", lambda: lib.t2s_embed_planes(ptr(ids), S, 1, 0, 8, 4, 260, 2, P, ptr(planes[1]), st)),
        ("embed Lp short", lambda: lib.t2s_embed_planes(ptr(ids), S, 1, 4, 8, 4, 259, 2, P, ptr(planes[1]), st)),
        ("embed X_lo NULL", lambda: lib.t2s_embed_planes(ptr(ids), S, 1, 4, 8, 4, 260, 2, P, None, st)),
        ("f32_to_planes C = 0", lambda: lib.t2s_f32_to_planes(S, 1, 0, 4, 260, 2, P, ptr(planes[1]), st)),
        ("f32_to_planes Lp short", lambda: lib.t2s_f32_to_planes(S, 1, 8, 4, 259, 2, P, ptr(planes[1]), st)),
        ("parse_output lengths NULL", lambda: lib.t2s_taco_parse_output(ptr(f.t), ptr(f.t), ptr(f.t), None, 1, 2, 4, st)),
        ("parse_output T = 0", lambda: lib.t2s_taco_parse_output(ptr(f.t), ptr(f.t), ptr(f.t), ptr(lens), 1, 2, 0, st)),
        ("zero_plane_rows unaligned", lambda: lib.t2s_zero_plane_rows(off2, ptr(planes[1]), ptr(lens), 1, 32, 4, 260, 2, st)),
        ("zero_plane_rows Lp short", lambda: lib.t2s_zero_plane_rows(P, ptr(planes[1]), ptr(lens), 1, 32, 4, 259, 2, st)),
        ("zero_plane_rows halo < 0", lambda: lib.t2s_zero_plane_rows(P, ptr(planes[1]), ptr(lens), 1, 32, 4, 260, -1, st)),
        ("zero_rows_f32 N = 0", lambda: lib.t2s_zero_rows_f32(ptr(f.t), ptr(lens), 1, 0, 4, st)),
        ("zero_rows_f32 lengths NULL", lambda: lib.t2s_zero_rows_f32(ptr(f.t), None, 1, 4, 4, st)),
        ("bn_fold C = 0", lambda: lib.t2s_bn_fold(S, S, S, S, None, 1e-5, 0, ptr(f.t), ptr(f.t), st)),
        ("bn_fold gamma NULL", lambda: lib.t2s_bn_fold(None, S, S, S, None, 1e-5, 4, ptr(f.t), ptr(f.t), st)),
        ("bernoulli n = 0", lambda: lib.t2s_bernoulli_mask(ptr(bytes_), 0, 1, 0, 0.5, st)),
        ("bernoulli keep_prob = 0", lambda: lib.t2s_bernoulli_mask(ptr(bytes_), 8, 1, 0, 0.0, st)),
        ("bernoulli keep_prob = 1.5", lambda: lib.t2s_bernoulli_mask(ptr(bytes_), 8, 1, 0, 1.5, st)),
        ("stop_check past T_cap", lambda: lib.t2s_taco_stop_check(S, 4, 2, 8, 4, 5, 0.5, ptr(stop), st)),
        ("stop_check n = 0", lambda: lib.t2s_taco_stop_check(S, 4, 2, 8, 0, 0, 0.5, ptr(stop), st)),
        ("stop_check step0 < 0", lambda: lib.t2s_taco_stop_check(S, 4, 2, 8, -1, 4, 0.5, ptr(stop), st)),
    ]
    for name, fn in calls:
        rc = fn()
        _sync()
        assert rc == EINVAL, (name, rc)
        assert bool(f.untouched(f.t).all()) and all(bool((p.float() == _PLANE_MARK).all()) for p in planes), name + ": written on refusal"
        assert bool((bytes_ == 0xAB).all()) and bool((stop == -1).all()), name + ": written on refusal"
    f.assert_guards("small kernel refusals")


# ============================================================================== 4. t2s_taco_decode_steps against a float64 decoder loop
# Which chain a case reaches (asserted from t2s_taco_decode_plan before every call, so that no case passes on another chain):
#   small autoregressive, B = 1 / 3, w_loc_denseT given   FUSED_ATT: att_fused_mfma_kernel (attention_dim 128 / 32 filters) or att_fused_kernel
#                                                         (64 / 16 / kernel 33); Q_PARTS with q_part (partial queries, q_dim 128 and 64), clear
#                                                         without; lstm_cell_kernel<1, 4, false>; PROJ_FUSED with w_projpre behind w_proj (one
#                                                         launch of n_mel + 1 + P = 53 rows, split_row 21), clear with it apart (three GEMVs)
#   ... w_loc_denseT NULL                                 FUSED_ATT clear at small B: query GEMV + att_energy_kernel + att_softmax_ctx_kernel
#   small autoregressive, B = 9 / 33                      sbgemm_lstm_kernel<32> (P + E + A = 224 = 7 x 32) for both cells, 33: a second 32-item
#                                                         block one item deep; query GEMV on sbgemm_plain; att_energy_mfma_kernel or att_energy_kernel
#   small autoregressive, P = 36, B = 9 / 65              the attention cell on lstm_cell_kernel (36 % 16 != 0), 65: a second 64-item chunk;
#                                                         the decoder cell on sbgemm_lstm_kernel<32> (n1 = 128, n2 = 64, K = 320)
#   teacher forced, B = 3, no saves                       the serial schedule (SPLIT clear)
#   teacher forced, B = 3, all saves, dropout masks       SPLIT in 16-step chunks, UNITS_2: lstm_cell_kernel<1, 2, true>; once more as calls of 1
#                                                         and 17 steps, so that one call spans two chunks
#   teacher forced, B = 9, all saves, pace_flag           SPLIT + PACED (+ SIG_BY_KERNEL: the matrix-core cell stores the pace word)
#   teacher forced, B = 9, all saves, att_xbuf            ONE: att_energy_mfma_kernel<true> does softmax, cumulative weights and context
#   reference sizes, B = 2, autoregressive                STREAM_GATES + FOLD_PRE2 + USE_PLOC: lstm_cell_p2_kernel, att_fused_mfma_kernel<true, true>,
#                                                         lstm_cell_kernel<., 4, false, true>, gemv_rows_loc_kernel; mask_steps = 4: steps 4 and 5 read pre2
#   reference sizes, B = 9, teacher forced, saves         Q_BIG + ONE: sbgemm_lstm_kernel with partial queries, no query GEMV
# Bars: F32_NORM / F32_MAX for every output.  Each output's float32 floor is printed too (`FLOOR ...`: the same loop in float32 on the
# CPU against the float64 one); eighteen autoregressive steps leave it at 1e-7 to 1e-6, so no bar had to be derived from it.
_PLAN_BITS = dict(SPLIT=0x001, PACED=0x002, SIG_BY_KERNEL=0x004, FUSED_ATT=0x008, Q_PARTS=0x010, Q_BIG=0x020, ONE=0x040,
                  STREAM_GATES=0x080, FOLD_PRE2=0x100, USE_PLOC=0x200, PROJ_FUSED=0x400, UNITS_2=0x800)
_DSMALL = dict(P=32, E=64, A=128, n_mel=20, T_in=40, T_cap=20)
_DREF = dict(P=256, E=512, A=1024, n_mel=80, T_in=48, T_cap=8)
_CALLS_SMALL, _CALLS_REF = ((0, 7), (7, 11)), ((0, 3), (3, 3))
_DEC_W = {}


def _dec_weights(dims, ad, F_, KS):
    """Seeded random decoder weights (f32 on the CPU) for one set of sizes, scaled so that no gate saturates."""
    key = (tuple(sorted(dims.items())), ad, F_, KS)
    if key in _DEC_W:
        return _DEC_W[key]
    P, E, A, n_mel = (dims[k] for k in ("P", "E", "A", "n_mel"))
    D = A
    g = torch.Generator().manual_seed(41000 + P + E + A + ad + F_ + KS)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    sa, sd = min(0.08, 1.5 / (P + E + A) ** 0.5), min(0.08, 1.5 / (A + E + D) ** 0.5)
    w = types.SimpleNamespace(
        att_w_ih=r(4 * A, P + E, sc=sa), att_w_hh=r(4 * A, A, sc=sa), att_b_ih=r(4 * A, sc=0.07), att_b_hh=r(4 * A, sc=0.07),
        dec_w_ih=r(4 * D, A + E, sc=sd), dec_w_hh=r(4 * D, D, sc=sd), dec_b_ih=r(4 * D, sc=0.07), dec_b_hh=r(4 * D, sc=0.07),
        w_query=r(ad, A, sc=1.0 / A ** 0.5), w_loc_conv=r(F_, 2, KS, sc=0.2), w_loc_dense=r(ad, F_, sc=0.2), w_v=r(ad, sc=0.3),
        w_proj=r(n_mel + 1, D + E, sc=1.0 / (D + E) ** 0.5), b_proj=r(n_mel + 1, sc=0.1),
        w_pre0=r(P, n_mel, sc=1.5 / n_mel ** 0.5), w_pre2=r(P, P, sc=1.5 / P ** 0.5))
    # prenet layer 0 composed with the projection in float64, rounded once to f32: what both the library and the loop use
    w.w_projpre = (w.w_pre0.double() @ w.w_proj[:n_mel].double()).float()
    w.b_projpre = (w.w_pre0.double() @ w.b_proj[:n_mel].double()).float()
    _DEC_W[key] = w
    return w


def _decoder_loop(c, dtype):
    """tacotron.py:355-393 (attention cell, attention, decoder cell) for steps 0 .. n - 1, and in autoregressive mode
    tacotron.py:447-461: the projection, and the prenet of the next step from the composed matrix with the injected masks.  The
    prenet buffers behave as the struct documents them: pre1 / pre2 start at zero (the go frame), the projection of step s fills
    them for step s + 1 while s + 1 < mask_steps, and with the folded prenet layer 1 (FOLD_PRE2) pre2 is never written - the
    attention cell computes it from pre1 below mask_steps and reads the buffer from there on.  Returns every stack the struct saves."""
    w, B, n = c.w, c.B, c.n_steps
    P, E, A, T_in = (c.dims[k] for k in ("P", "E", "A", "T_in"))
    cv = lambda t: t.to(dtype)
    Wa, ba = cv(torch.cat([w.att_w_ih, w.att_w_hh], 1)), cv(w.att_b_ih) + cv(w.att_b_hh)
    Wd, bd = cv(torch.cat([w.dec_w_ih, w.dec_w_hh], 1)), cv(w.dec_b_ih) + cv(w.dec_b_hh)
    Wq, K, Dl, v, Wp, bp, Wpp, bpp, Wp2 = map(cv, (w.w_query, w.w_loc_conv, w.w_loc_dense, w.w_v, w.w_proj, w.b_proj, w.w_projpre,
                                                  w.b_projpre, w.w_pre2))
    pmem, memory = cv(c.pmem), cv(c.memory)
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    h_a, c_a, h_d, c_d, ctx, wt, wc = z(B, A), z(B, A), z(B, A), z(B, A), z(B, E), z(B, T_in), z(B, T_in)
    pre1, pre2 = z(B, P), z(B, P)
    names = ("att_gates", "att_c", "att_h", "q", "w", "wcum", "dec_gates", "dec_c", "hc", "mel_gate")
    sv = {k: [] for k in names}
    for s in range(n):
        if c.teacher:
            x1 = cv(c.pre_all[s])
        elif c.fold and s < c.mask_steps:
            x1 = torch.relu(pre1 @ Wp2.t()) * cv(c.mk[s, :, 1]) * 2.0
        else:
            x1 = pre2
        _, ga, c_a, h = lstm(torch.cat([x1, ctx, h_a], 1), Wa, ba, c_a)
        h_a = h * cv(c.m_att[s]) * c.s_att if c.drops else h
        q = h_a @ Wq.t()
        wt, ctx, wc = att_step(q, pmem, memory, wt, wc, K, Dl, v, c.lengths)
        _, gd, c_d, h = lstm(torch.cat([h_a, ctx, h_d], 1), Wd, bd, c_d)
        h_d = h * cv(c.m_dec[s]) * c.s_dec if c.drops else h
        hc = torch.cat([h_d, ctx], 1)
        mg = hc @ Wp.t() + bp
        if not c.teacher and s + 1 < c.mask_steps:
            pre1 = torch.relu(hc @ Wpp.t() + bpp) * cv(c.mk[s + 1, :, 0]) * 2.0
            if not c.fold:
                pre2 = torch.relu(pre1 @ Wp2.t()) * cv(c.mk[s + 1, :, 1]) * 2.0
        for k, val in zip(names, (ga, c_a, h_a, q, wt, wc, gd, c_d, hc, mg)):
            sv[k].append(val)
    out = {k: torch.stack(val) for k, val in sv.items()}
    out.update(f_att_w=wt, f_att_wcum=wc, f_ctx=ctx, f_att_c=c_a, f_dec_c=c_d, f_att_h=h_a, f_dec_h=h_d)
    return out


def _decode_case(dims, calls, B, teacher, ad=128, F_=32, KS=31, q_part=True, adjacent=True, denseT=True, saves=False, drops=False,
                 pace=False, xbuf=False, stream=False, mask_steps=None, plan=None):
    P, E, A, n_mel, T_in, T_cap = (dims[k] for k in ("P", "E", "A", "n_mel", "T_in", "T_cap"))
    c = types.SimpleNamespace(dims=dims, calls=calls, B=B, teacher=teacher, ad=ad, F=F_, KS=KS, q_part=q_part, adjacent=adjacent,
                              denseT=denseT, saves=saves, drops=drops, pace=pace, xbuf=xbuf, stream=stream, plan=plan or {})
    c.n_steps = calls[-1][0] + calls[-1][1]
    c.mask_steps = T_cap if mask_steps is None else mask_steps
    c.fold = stream                 # (asserted from the plan: FOLD_PRE2)
    c.w = _dec_weights(dims, ad, F_, KS)
    g = torch.Generator().manual_seed(42000 + B + 3 * ad + 7 * teacher + 11 * saves + P)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    c.lengths = torch.tensor(ragged(B, T_in), dtype=torch.int32)
    c.pmem, c.memory = r(B, T_in, ad, sc=0.5), r(B, T_in, E)
    c.pre_all = r(T_cap + 1, B, P).clamp_min(0.0) * 2.0
    c.mk = (torch.rand(c.mask_steps, B, 2, P, generator=g) >= 0.5).to(torch.uint8)
    c.m_att = (torch.rand(T_cap, B, A, generator=g) >= 0.1).to(torch.uint8)
    c.m_dec = (torch.rand(T_cap, B, A, generator=g) >= 0.1).to(torch.uint8)
    c.s_att = c.s_dec = 1.0 / 0.9
    c.ref = _decoder_loop(c, torch.float64)
    ref32 = _decoder_loop(c, torch.float32)
    c.floor = {k: (U.rel(ref32[k], val), U.maxrel(ref32[k], val)) for k, val in c.ref.items()}
    return c


def _run_decode(lib, c, tag):
    w, B, n, teacher = c.w, c.B, c.n_steps, c.teacher
    P, E, A, n_mel, T_in, T_cap = (c.dims[k] for k in ("P", "E", "A", "n_mel", "T_in", "T_cap"))
    D, ad = A, c.ad
    keep = []                       # device tensors the struct points into

    def dv(t):
        keep.append(dev(t))
        return keep[-1]

    d = _DecoderStruct()
    for k, val in dict(B=B, T_in=T_in, n_mel=n_mel, prenet_dim=P, enc_dim=E, att_rnn_dim=A, dec_rnn_dim=D, att_dim=ad, loc_filters=c.F,
                       loc_kernel=c.KS, T_cap=T_cap, teacher_forced=int(teacher), mask_steps=0 if teacher else c.mask_steps).items():
        setattr(d, k, val)
    for name in ("att_w_ih", "att_w_hh", "att_b_ih", "att_b_hh", "dec_w_ih", "dec_w_hh", "dec_b_ih", "dec_b_hh", "w_query", "w_loc_conv",
                 "w_loc_dense", "w_v", "w_pre2"):
        setattr(d, name, dv(getattr(w, name)).data_ptr())
    if c.adjacent:                  # one [n_mel + 1 + P] row block
        w_all, b_all = dv(torch.cat([w.w_proj, w.w_projpre], 0)), dv(torch.cat([w.b_proj, w.b_projpre], 0))
        d.w_proj, d.b_proj = w_all.data_ptr(), b_all.data_ptr()
        d.w_projpre, d.b_projpre = w_all.data_ptr() + (n_mel + 1) * (D + E) * 4, b_all.data_ptr() + (n_mel + 1) * 4
    else:
        for name in ("w_proj", "b_proj", "w_projpre", "b_projpre"):
            setattr(d, name, dv(getattr(w, name)).data_ptr())
    if c.denseT:
        d.w_loc_denseT = dv(w.w_loc_dense.t()).data_ptr()
    d.memory, d.pmem, d.mem_lengths = dv(c.memory).data_ptr(), dv(c.pmem).data_ptr(), dv(c.lengths).data_ptr()
    if teacher:
        d.pre_all = dv(c.pre_all).data_ptr()
    else:
        d.prenet_masks = dv(c.mk).data_ptr()
    d.att_drop_scale = d.dec_drop_scale = 1.0
    if c.drops:
        d.att_drop, d.dec_drop, d.att_drop_scale, d.dec_drop_scale = dv(c.m_att).data_ptr(), dv(c.m_dec).data_ptr(), c.s_att, c.s_dec
    o = types.SimpleNamespace()
    zg = lambda *s: Guarded(*s, fill=torch.zeros(*s, device=DEV))
    for name, sh in dict(att_h0=(B, A), att_h1=(B, A), att_c=(B, A), dec_h0=(B, D), dec_h1=(B, D), dec_c=(B, D), att_w=(B, T_in),
                         att_wcum=(B, T_in), ctx=(B, E), q=(B, ad), energies=(B, T_in), pre1=(B, P), pre2=(B, P)).items():
        setattr(o, name, zg(*sh))
    if c.q_part:
        o.q_part = zg(A // 2, B, ad)
    o.align_out = Guarded(B, T_cap, T_in)
    if teacher:
        o.hc_all = Guarded(T_cap, B, D + E)
    else:
        o.mel_gate_out = Guarded(B, n_mel + 1, T_cap)
    if c.saves:
        for name, sh in dict(att_gates_all=(T_cap, B, 4 * A), att_c_all=(T_cap, B, A), dec_gates_all=(T_cap, B, 4 * D),
                             dec_c_all=(T_cap, B, D), att_h_all=(T_cap, B, A), q_all=(T_cap, B, ad), wcum_all=(T_cap, B, T_in)).items():
            setattr(o, name, Guarded(*sh))
    if c.stream:
        o.gate_part, o.ploc = zg(3, B, 4 * A), zg(B, T_in, ad)
        d.w_pre2T = dv(w.w_pre2.t()).data_ptr()
    for name, gd in vars(o).items():
        setattr(d, name, gd.t.data_ptr())
    xbuf = torch.zeros(B * T_in + 1, dtype=torch.int64, device=DEV) if c.xbuf else None
    pace = torch.zeros(2, dtype=torch.int64, device=DEV) if c.pace else None
    d.att_xbuf, d.pace_flag = None if xbuf is None else xbuf.data_ptr(), None if pace is None else pace.data_ptr()
    seen = 0
    for step0, n_call in c.calls:
        bits = ctypes.c_uint(0)
        assert lib.t2s_taco_decode_plan(ctypes.byref(d), step0, n_call, ctypes.byref(bits)) == 0, tag + ": the plan refuses the struct"
        for name, on in c.plan.items():
            assert bool(bits.value & _PLAN_BITS[name]) == on, "%s: plan bit %s is %s (plan 0x%x)" % (tag, name, "clear" if on else "set", bits.value)
        seen |= bits.value
        _lib.call("t2s_taco_decode_steps", ctypes.byref(d), step0, n_call, _st())
    _sync()
    ref, ck = c.ref, _Checks()

    def cmp(name, got, key):
        print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e" % ("%s %s" % (tag, name), *c.floor[key]))
        ck("%s %s" % (tag, name), got, ref[key])

    def rest_untouched(name, gd, view):
        ck.ok(bool(gd.untouched(view).all()), "%s: %s written past the last step" % (tag, name))

    cmp("align_out", o.align_out.t[:, :n].permute(1, 0, 2), "w")
    rest_untouched("align_out", o.align_out, o.align_out.t[:, n:])
    if teacher:
        cmp("hc_all", o.hc_all.t[:n], "hc")
        rest_untouched("hc_all", o.hc_all, o.hc_all.t[n:])
    else:
        cmp("mel_gate_out", o.mel_gate_out.t[:, :, :n].permute(2, 0, 1), "mel_gate")
        rest_untouched("mel_gate_out", o.mel_gate_out, o.mel_gate_out.t[:, :, n:])
    if c.saves:
        for name, key in (("att_gates_all", "att_gates"), ("att_c_all", "att_c"), ("dec_gates_all", "dec_gates"), ("dec_c_all", "dec_c"),
                          ("att_h_all", "att_h"), ("q_all", "q"), ("wcum_all", "wcum")):
            gd = getattr(o, name)
            cmp(name, gd.t[:n], key)
            rest_untouched(name, gd, gd.t[n:])
    last_odd = (n - 1) & 1          # the step's output slot: h1 after an even step, h0 after an odd one
    for name, gd, key in (("att_w", o.att_w, "f_att_w"), ("att_wcum", o.att_wcum, "f_att_wcum"), ("ctx", o.ctx, "f_ctx"),
                          ("att_c", o.att_c, "f_att_c"), ("dec_c", o.dec_c, "f_dec_c"),
                          ("att_h (current)", o.att_h0 if last_odd else o.att_h1, "f_att_h"),
                          ("dec_h (current)", o.dec_h0 if last_odd else o.dec_h1, "f_dec_h")):
        cmp(name, gd.t, key)
    for name, gd in vars(o).items():
        gd.assert_guards("%s %s" % (tag, name))
    if xbuf is not None:
        ck.ok(int(xbuf[B * T_in].item()) == 0, tag + ": the error word of att_xbuf was raised")
    if pace is not None:
        ck.ok(int(pace[1].item()) == 0, tag + ": the error word of pace_flag was raised")
    ck.done()
    return seen


_AR_SMALL = [
    # B, attention_dim, filters, kernel, q_part, adjacent, denseT, plan
    (1, 128, 32, 31, True, True, True, dict(FUSED_ATT=True, Q_PARTS=True, PROJ_FUSED=True, UNITS_2=False, SPLIT=False)),
    (1, 64, 16, 33, False, False, False, dict(FUSED_ATT=False, Q_PARTS=False, PROJ_FUSED=False)),
    (3, 128, 32, 31, True, True, True, dict(FUSED_ATT=True, Q_PARTS=True, PROJ_FUSED=True)),
    (3, 128, 32, 31, False, False, True, dict(FUSED_ATT=True, Q_PARTS=False, PROJ_FUSED=False)),
    (3, 64, 16, 33, True, False, True, dict(FUSED_ATT=True, Q_PARTS=True, PROJ_FUSED=False)),
    (3, 64, 16, 33, False, True, True, dict(FUSED_ATT=True, Q_PARTS=False, PROJ_FUSED=True)),
    (3, 128, 32, 31, True, True, False, dict(FUSED_ATT=False, Q_PARTS=False, Q_BIG=False, PROJ_FUSED=True)),
    (3, 64, 16, 33, False, False, False, dict(FUSED_ATT=False, Q_PARTS=False, PROJ_FUSED=False)),
    (9, 128, 32, 31, True, True, True, dict(FUSED_ATT=False, Q_PARTS=False, Q_BIG=False, ONE=False, PROJ_FUSED=True)),
    (9, 64, 16, 33, False, False, False, dict(FUSED_ATT=False, Q_PARTS=False, PROJ_FUSED=False)),
    (33, 128, 32, 31, False, False, True, dict(FUSED_ATT=False, Q_PARTS=False, PROJ_FUSED=False)),
    (33, 64, 16, 33, True, True, True, dict(FUSED_ATT=False, Q_PARTS=False, PROJ_FUSED=True)),
]


@pytest.mark.parametrize("B,ad,F_,KS,q_part,adjacent,denseT,plan", _AR_SMALL)
def test_decode_autoregressive_small(lib, B, ad, F_, KS, q_part, adjacent, denseT, plan):
    """P 32, E 64, A = D 128, 20 mels (21 projection rows: no multiple of 4), T_in 40 with ragged lengths; 18 steps as calls of 7 and
    11: the second call starts on the odd ping-pong parity."""
    c = _decode_case(_DSMALL, _CALLS_SMALL, B, False, ad, F_, KS, q_part, adjacent, denseT, plan=plan)
    _run_decode(lib, c, "decode[AR B=%d ad=%d F=%d KS=%d q_part=%d adjacent=%d denseT=%d]" % (B, ad, F_, KS, q_part, adjacent, denseT))


@pytest.mark.parametrize("B", [9, 65])
def test_decode_autoregressive_prenet_36(lib, B):
    """prenet_dim 36: n1 % 16 != 0, so t2s_sbgemm_lstm_ok refuses the attention cell and it stays on lstm_cell_kernel past 8 items;
    65 items: a second 64-item chunk of its item loop."""
    c = _decode_case(dict(_DSMALL, P=36), _CALLS_SMALL, B, False, plan=dict(FUSED_ATT=False, PROJ_FUSED=True, UNITS_2=False))
    _run_decode(lib, c, "decode[AR B=%d P=36]" % B)


def test_decode_teacher_forced_serial(lib):
    c = _decode_case(_DSMALL, _CALLS_SMALL, 3, True, plan=dict(SPLIT=False, FUSED_ATT=True, Q_PARTS=True, UNITS_2=False, PROJ_FUSED=False))
    _run_decode(lib, c, "decode[TF B=3 no saves]")


@pytest.mark.parametrize("calls", [_CALLS_SMALL, ((0, 1), (1, 17))])
def test_decode_teacher_forced_split_chunks(lib, calls):
    """All saves and both dropout masks at B = 3: the decoder cells on the helper stream in chunks of 16 steps; as calls of 1 and 17
    steps the second call spans two chunks and starts on the odd parity."""
    c = _decode_case(_DSMALL, calls, 3, True, saves=True, drops=True, plan=dict(SPLIT=True, PACED=False, UNITS_2=True, FUSED_ATT=True))
    _run_decode(lib, c, "decode[TF B=3 saves drops calls=%s]" % (calls,))


def test_decode_teacher_forced_paced(lib):
    c = _decode_case(_DSMALL, _CALLS_SMALL, 9, True, saves=True, pace=True, plan=dict(SPLIT=True, PACED=True, FUSED_ATT=False, ONE=False))
    _run_decode(lib, c, "decode[TF B=9 saves pace_flag]")


def test_decode_teacher_forced_one_launch_attention(lib):
    c = _decode_case(_DSMALL, _CALLS_SMALL, 9, True, saves=True, xbuf=True, plan=dict(SPLIT=True, PACED=False, ONE=True, FUSED_ATT=False))
    _run_decode(lib, c, "decode[TF B=9 saves att_xbuf]")


def test_decode_reference_sizes_streamed(lib):
    """1024 / 1024 / 512 / 256 / 128 / 32 / 31, 80 mels, B = 2 with gate_part, w_pre2T, ploc and q_part; mask_steps = 4 of 6 steps:
    steps 4 and 5 leave the folded prenet and read pre2."""
    c = _decode_case(_DREF, _CALLS_REF, 2, False, stream=True, mask_steps=4,
                     plan=dict(STREAM_GATES=True, FOLD_PRE2=True, USE_PLOC=True, FUSED_ATT=True, Q_PARTS=True, PROJ_FUSED=True))
    _run_decode(lib, c, "decode[ref AR B=2 streamed]")


def test_decode_reference_sizes_big_batch(lib):
    c = _decode_case(_DREF, _CALLS_REF, 9, True, saves=True, xbuf=True, plan=dict(SPLIT=True, Q_BIG=True, ONE=True, FUSED_ATT=False))
    _run_decode(lib, c, "decode[ref TF B=9 saves q_part att_xbuf]")
