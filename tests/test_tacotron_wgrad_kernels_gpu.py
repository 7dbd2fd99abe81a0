"""t2s_wgrad_gemm - every weight gradient of the Tacotron train step - through the C ABI (run with -m gpu on an MI355X): alone on
time-major planes built here (section 1), then behind its feeders and in front of t2s_wn_backward with the argument pattern of each
of its call sites (section 2).  The conventions follow tests/test_tacotron_bwd_kernels_gpu.py and
tests/test_waveglow_bwd_kernels_gpu.py: f32 outputs live in wg_bwd_util.Guarded buffers (NaN sentinel inside, guard words either
side, checked after every launch), every compared output goes through wg_bwd_util.check (norm-relative error AND the maximum error
relative to the expectation's largest element, after a `PARITY ...` line), and the float64 expectation is built from the operands
only, never from a library output.

The branch of conv_gemm_kernel these calls take is `a.ksplit > 1 || a.k0 > 0` (or the plain one, for ksplit = 1 from chunk 0), with
a_bstride != 0 for B > 1; t2s_wgrad_gemm_flat (test_waveglow_bwd_kernels_gpu.py section 7) takes `a.kflat > 0` instead.

Section 1 holds the planes' own values (hi + lo joined) in float64, so input rounding is not in its error; operand rows [M, Mpad)
and [N, Npad) hold a finite 5.0 that must reach no stored element.  Every slab is compared with the sum over its own K range
(slab b * ksplit + s: chunks [k0 + s * kchunk, min(k0 + (s + 1) * kchunk, k1)), kchunk = ceil((k1 - k0) / ksplit)), then the slab
sum with the whole window.  Slabs whose range is empty must be zeros, exactly: t2s_wn_backward adds all ksplit slabs of a buffer
nobody cleared.  Section 2 starts from f32 tensors, so the feeders' split into hi + lo is in its error; its planes are pre-filled
with 5.0 as well, so a feeder that left a row or a position of the valid region to the buffer's earlier contents would show.

Bars: wg_bwd_util.GEMM_NORM / GEMM_MAX (2e-5 / 1e-4), the bars t2s_wgrad_gemm_flat is held to - the same kernel, the same
three-product split-bf16 arithmetic and f32 accumulation.  The arithmetic's own floor (wg_bwd_util.split3_floor of each case's
operands) is printed; a case whose floor exceeded a quarter of a bar would take 4 x its floor (the rule of
tests/test_waveglow_fwd_kernels_gpu.py) - none does at these K.  Empty slabs and refused calls are exact.
profiles/tacotron_wgrad_kernel_tests.md has the measured figures, the floors and what four hand-made library changes do to these
tests and to the whole-model gradient test."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import taco_ref_util as R
import wg_bwd_util as U
from text2speech_amd import _lib, planes
from text2speech_amd.tacotron.autograd import _IW_WGS
from wg_bwd_util import DEV, GEMM_MAX, GEMM_NORM, Guarded, check, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
ptr = _lib.ptr
FILL = 5.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _sync():
    torch.cuda.synchronize()


def _ru(a, b):
    return -(-a // b) * b


def _bars(label, a, b, eq):
    """Prints the arithmetic's floor for operands a, b contracted by `eq` and returns the (norm, max) bars of the case."""
    fn, fm = U.split3_floor(a, b, eq)
    print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e" % (label, fn, fm))
    return (4 * fn if fn > GEMM_NORM / 4 else GEMM_NORM), (4 * fm if fm > GEMM_MAX / 4 else GEMM_MAX)


def _filled(*shape):
    """bf16 device planes holding FILL everywhere"""
    return torch.full(shape, FILL, dtype=torch.bfloat16, device=DEV)


def _untouched(out):
    return bool(out.untouched(out.t).all())


# ================================================================================================== 1. the GEMM alone
_OPS = {}


class _Operands:
    """Seeded time-major planes [B][n_tchunks][rows_pad][32] (hi, lo) of an M x K and an N x K operand per batch entry, K =
    32 n_tchunks, and the float64 values they hold (a [B, M, K], x [B, N, K]); rows past M / N hold FILL."""

    def __init__(self, B, M, N, nt):
        self.B, self.M, self.N, self.nt = B, M, N, nt
        self.Mpad, self.Npad = _lib.padded_rows(M), _lib.plane_rows(N, 0)
        gen = torch.Generator().manual_seed(7000 + 1000 * B + 10 * M + N + nt)

        def side(rows, rows_pad):
            # every batch entry at its own scale: one read in another's place shows in the norm as well
            v = torch.randn(B, rows, nt * 32, generator=gen) * (1.0 + torch.arange(B, dtype=torch.float32)).view(B, 1, 1)
            hi, lo = planes.split_bf16(v)
            pair = []
            for p in (hi, lo):
                t = torch.full((B, nt, rows_pad, 32), FILL, dtype=torch.bfloat16)
                t[:, :, :rows] = p.view(B, rows, nt, 32).permute(0, 2, 1, 3)           # tm[b][k / 32][row][k % 32] = v[b][row][k]
                pair.append(dev(t))
            return pair, hi.double() + lo.double()

        self.A, self.a = side(M, self.Mpad)
        self.X, self.x = side(N, self.Npad)
        self.zb = torch.zeros(self.Mpad, device=DEV)

    def args(self, out, k0, k1, ksplit, over=None):
        """The argument list of t2s_wgrad_gemm for these operands; `over` replaces single arguments by name."""
        a = dict(A_hi=ptr(self.A[0]), A_lo=ptr(self.A[1]), X_hi=ptr(self.X[0]), X_lo=ptr(self.X[1]), zero_bias=ptr(self.zb),
                 out=ptr(out), B=self.B, M=self.M, N=self.N, Mpad=self.Mpad, Npad=self.Npad, n_tchunks=self.nt, k0=k0, k1=k1,
                 ksplit=ksplit, stream=_lib.current_stream())
        assert all(k in a for k in over or {}), over
        a.update(over or {})
        return list(a.values())

    def want(self, k0, k1, ksplit):
        """float64 [B * ksplit, M, N] slabs over their own K ranges, and which slabs have an empty range"""
        kchunk = -(-(k1 - k0) // ksplit)
        out = torch.zeros(self.B, ksplit, self.M, self.N, dtype=torch.float64)
        empty = []
        for s in range(ksplit):
            lo, hi = k0 + s * kchunk, min(k0 + (s + 1) * kchunk, k1)
            empty.append(lo >= hi)
            if lo < hi:
                out[:, s] = torch.einsum("bmt,bnt->bmn", self.a[:, :, 32 * lo:32 * hi], self.x[:, :, 32 * lo:32 * hi])
        return out.view(self.B * ksplit, self.M, self.N), empty * self.B


def _operands(B, M, N, nt):
    key = (B, M, N, nt)
    if key not in _OPS:
        _OPS[key] = _Operands(B, M, N, nt)
    return _OPS[key]


def _gemm_case(o, k0, k1, ksplit):
    """One launch: guards, every slab against its own K range (empty ones exactly zero), the slab sum against the window."""
    tag = "B=%d M=%d N=%d nt=%d k=[%d,%d) ksplit=%d" % (o.B, o.M, o.N, o.nt, k0, k1, ksplit)
    norm_bar, max_bar = _bars("wgrad_gemm " + tag, o.a[:, :, 32 * k0:32 * k1], o.x[:, :, 32 * k0:32 * k1], "bmt,bnt->bmn")
    want, empty = o.want(k0, k1, ksplit)
    out = Guarded(o.B * ksplit, o.M, o.N)
    _lib.call("t2s_wgrad_gemm", *o.args(out.t, k0, k1, ksplit))
    _sync()
    out.assert_guards("wgrad_gemm " + tag)
    got = out.t.cpu()
    assert bool(torch.isfinite(got).all()), "%s: %d elements were never written" % (tag, int((~torch.isfinite(got)).sum()))
    failed = []
    for i in range(o.B * ksplit):
        if empty[i]:
            if not torch.equal(got[i], torch.zeros(o.M, o.N)):
                failed.append("%s: slab %d has an empty K range and is not all zeros" % (tag, i))
            continue
        try:
            check("wgrad_gemm %s slab %d" % (tag, i), got[i], want[i], norm_bar, max_bar)
        except AssertionError as e:
            failed.append(str(e))
    try:
        check("wgrad_gemm %s slab sum" % tag, got.double().view(o.B, ksplit, o.M, o.N).sum(1),
              torch.einsum("bmt,bnt->bmn", o.a[:, :, 32 * k0:32 * k1], o.x[:, :, 32 * k0:32 * k1]), norm_bar, max_bar)
    except AssertionError as e:
        failed.append(str(e))
    assert not failed, "\n".join(failed)


def test_gemm_minimal_launch(lib):
    """B = 1, M = 4, N = 2, one K-step, one slab: the smallest call the entry point accepts."""
    _gemm_case(_operands(1, 4, 2, 1), 0, 1, 1)


@pytest.mark.parametrize("ksplit", [1, 2, 3, 4, 5])
def test_gemm_ragged_tiles(lib, ksplit):
    """M = 260 (the second 256-row tile holds 4 rows), N = 257 (the second column tile holds one column), five K-steps.  ksplit 3
    gives a short last slab (2, 2, 1), 4 gives kchunk = 2 and an empty fourth slab, 5 one step per slab."""
    _gemm_case(_operands(1, 260, 257, 5), 0, 5, ksplit)


def test_gemm_tacotron_split_rule(lib):
    """items_wgrad's rule at 17 chunks: ks = min(16, nch) = 16, kchunk = 2, nine slabs own K-steps and seven must come back zero."""
    o = _operands(1, 32, 33, 17)
    assert sum(o.want(0, 17, 16)[1]) == 7
    _gemm_case(o, 0, 17, 16)


@pytest.mark.parametrize("ksplit", [1, 2])
def test_gemm_batch_stride(lib, ksplit):
    """B = 3 with different values (and scales) per entry: ksplit 1 is the per-batch form of the convolution, encoder and d_memory
    calls (slab b reads entry b), 2 pins the slab index b * ksplit + s."""
    _gemm_case(_operands(3, 80, 161, 3), 0, 3, ksplit)


@pytest.mark.parametrize("k0,k1,ksplit", [(1, 4, 1), (1, 4, 2), (2, 5, 1), (2, 5, 2), (0, 3, 2), (0, 3, 1)])
def test_gemm_k_window(lib, k0, k1, ksplit):
    """Chunks [k0, k1) of five, the chunks outside holding values like those inside: include/t2s_hip.h promises the sum over the
    window alone.  (0, 3) unsplit is the form that used to run all five chunks."""
    _gemm_case(_operands(1, 260, 257, 5), k0, k1, ksplit)


@pytest.mark.parametrize("k0,k1", [(0, 2), (1, 3)])
def test_gemm_k_window_per_batch(lib, k0, k1):
    """The window with B = 3, unsplit: every entry starts at its own chunk k0 and stops at its own k1."""
    _gemm_case(_operands(3, 80, 161, 3), k0, k1, 1)


_OFF = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)       # a pointer n bytes into a tensor


def _refusals():
    o = lambda: _operands(1, 260, 257, 5)
    r = [("M % 4 != 0", lambda: dict(M=258)), ("ksplit 0", lambda: dict(ksplit=0)), ("ksplit 17", lambda: dict(ksplit=17)),
         ("k1 > n_tchunks", lambda: dict(k1=6)), ("k0 == k1", lambda: dict(k0=3, k1=3)), ("k0 > k1", lambda: dict(k0=4, k1=2)),
         ("k0 < 0", lambda: dict(k0=-1)), ("Npad != t2s_plane_rows(N, 0)", lambda: dict(Npad=768)),
         ("Mpad < M", lambda: dict(Mpad=256)), ("Mpad % 256 != 0", lambda: dict(Mpad=384))]
    r += [("%s NULL" % n, (lambda n=n: {n: None})) for n in ("A_hi", "A_lo", "X_hi", "X_lo", "zero_bias", "out")]
    r += [("A_hi not 16-byte aligned", lambda: dict(A_hi=_OFF(o().A[0], 2))), ("A_lo not 16-byte aligned", lambda: dict(A_lo=_OFF(o().A[1], 8))),
          ("X_hi not 16-byte aligned", lambda: dict(X_hi=_OFF(o().X[0], 2))), ("X_lo not 16-byte aligned", lambda: dict(X_lo=_OFF(o().X[1], 4)))]
    return r


@pytest.mark.parametrize("what,over", _refusals(), ids=[w for w, _ in _refusals()])
def test_gemm_refusals(lib, what, over):
    """One bad argument at a time on the ragged-tile operands (otherwise k = [0, 5), ksplit = 2): T2S_EINVAL, and nothing written."""
    o = _operands(1, 260, 257, 5)
    out = Guarded(2, o.M, o.N)
    assert lib.t2s_wgrad_gemm(*o.args(out.t, 0, 5, 2, over())) == EINVAL, what
    _sync()
    out.assert_guards(what)
    assert _untouched(out), "%s: the refused call wrote to its output" % what


# ================================================================================================== 2. the four call-site chains

def _wn_backward(P, ks, Prows, Pcols, row_off, col_off, tap_stride, w, O, Cin, Kt, dW, db):
    """t2s_wn_backward as _Bwd.slab_to_grad calls it (autograd.py:174-183): plain weight, the bias from the ones column Pcols - 1"""
    _lib.call("t2s_wn_backward", ptr(P), ks, Prows, Pcols, row_off, col_off, tap_stride, Pcols - 1, 1, ptr(w), None, O, Cin, Kt,
              ptr(dW), None, ptr(db), 0, _lib.current_stream())


def _wide(t, extra):
    """[rows, C] -> device [rows, C + extra], the extra columns holding 77: a row stride that differs from the row length"""
    return dev(torch.cat([t, torch.full((t.size(0), extra), 77.0)], 1))


@pytest.mark.parametrize("items", [33, 17 * 32])
def test_items_wgrad_chain(lib, items):
    """_Bwd.items_wgrad + slab_to_grad (text2speech_amd/tacotron/autograd.py:145-183) for y = [x | h_prev] W^T + b over (step, batch)
    items, B = 3: t2s_rows_to_tm for two A sources (the gate gradients of two layers side by side, row_off 0 and 20) and two X
    sources, the second with shift = B (the recurrent input: item i reads h of item i - B, zero for the first step);
    t2s_tm_ones_row(.., 1, items_pad, 0, items, Npad, N_cols); t2s_wgrad_gemm(B = 1, .., ksplit) with ksplit from the rule of line
    167; t2s_wn_backward for W_ih (with the bias) and W_hh (col_off = 24).  items = 33: the second chunk holds one item, ksplit 2;
    items = 544: 17 chunks, ksplit 16, seven empty slabs.  dW / db against float64 autograd of F.linear on the f32 inputs, and every
    slab against the same sum over its own items."""
    B, M, N_cols, C1, C2, M1 = 3, 36, 40, 24, 16, 20
    gen = torch.Generator().manual_seed(100 + items)
    dy1, dy2 = torch.randn(items, M1, generator=gen), torch.randn(items, M - M1, generator=gen) * 0.5
    x1, h = torch.randn(items, C1, generator=gen), torch.randn(items, C2, generator=gen)
    w_ih, w_hh = torch.randn(M, C1, generator=gen), torch.randn(M, C2, generator=gen)
    d_dy1, d_dy2, d_x1, d_h = _wide(dy1, 4), _wide(dy2, 0), _wide(x1, 8), _wide(h, 4)
    st = _lib.current_stream()
    # ---- float64: autograd of the layer, and the slabs ----
    dy = torch.cat([dy1, dy2], 1).double()
    xin = torch.cat([x1.double(), R.shift_items(h.double(), B)], 1)
    W = torch.cat([w_ih, w_hh], 1).double().requires_grad_(True)
    b = torch.zeros(M, dtype=torch.float64, requires_grad=True)
    dW_want, db_want = torch.autograd.grad((F.linear(xin, W, b) * dy).sum(), [W, b])
    norm_bar, max_bar = _bars("items_wgrad items=%d" % items, dy.t().contiguous(), R.with_ones(xin).t().contiguous(), "mt,nt->mn")
    # ---- the chain ----
    items_pad = _ru(items, 32)
    nch = items_pad // 32
    M4 = _ru(M, 4)
    Mpad = _lib.padded_rows(M4)
    N = N_cols + 1
    Npad = _ru(N, 256)
    A, X = (_filled(nch, Mpad, 32), _filled(nch, Mpad, 32)), (_filled(nch, Npad, 32), _filled(nch, Npad, 32))
    for (t, C, off, shift) in ((d_dy1, M1, 0, 0), (d_dy2, M - M1, M1, 0)):
        _lib.call("t2s_rows_to_tm", ptr(t), t.size(1), items, items_pad, shift, C, ptr(A[0]), ptr(A[1]), Mpad, off, st)
    for (t, C, off, shift) in ((d_x1, C1, 0, 0), (d_h, C2, C1, B)):
        _lib.call("t2s_rows_to_tm", ptr(t), t.size(1), items, items_pad, shift, C, ptr(X[0]), ptr(X[1]), Npad, off, st)
    _lib.call("t2s_tm_ones_row", ptr(X[0]), ptr(X[1]), 1, items_pad, 0, items, Npad, N_cols, st)
    tiles = -(-M4 // 256) * -(-N // 256)
    ks = max(1, min(16, nch, -(-_IW_WGS // tiles)))
    assert ks == {33: 2, 544: 16}[items]
    P = Guarded(ks, M4, N)
    zb = torch.zeros(Mpad, device=DEV)
    _lib.call("t2s_wgrad_gemm", ptr(A[0]), ptr(A[1]), ptr(X[0]), ptr(X[1]), ptr(zb), ptr(P.t), 1, M4, N, Mpad, Npad, nch, 0, nch, ks, st)
    dW_ih, dW_hh, db = Guarded(M, C1), Guarded(M, C2), Guarded(M)
    d_wih, d_whh = dev(w_ih), dev(w_hh)
    _wn_backward(P.t, ks, M4, N, 0, 0, 0, d_wih, M, C1, 1, dW_ih.t, db.t)
    _wn_backward(P.t, ks, M4, N, 0, C1, 0, d_whh, M, C2, 1, dW_hh.t, None)
    _sync()
    for o_, name in ((P, "P"), (dW_ih, "dW_ih"), (dW_hh, "dW_hh"), (db, "db")):
        o_.assert_guards("items_wgrad %s" % name)
    # rows [M, Mpad) / [N, Npad) belong to nobody: still the filler, bit for bit
    for pl_, n in ((A, M), (X, N)):
        for p in pl_:
            assert bool((p[:, n:].float() == FILL).all()), "a feeder wrote past its rows"
    got = P.t.cpu()
    assert bool(torch.isfinite(got).all())
    kchunk = -(-nch // ks)
    n_empty = 0
    for s in range(ks):
        lo, hi = min(32 * s * kchunk, items), min(32 * (s + 1) * kchunk, items)
        if s * kchunk >= nch:
            n_empty += 1
            assert torch.equal(got[s], torch.zeros(M4, N)), "slab %d has no K-step and is not all zeros" % s
        else:
            check("items_wgrad items=%d slab %d" % (items, s), got[s], R.items_wgrad(dy, xin, lo, hi), norm_bar, max_bar)
    assert n_empty == {33: 0, 544: 7}[items]
    check("items_wgrad items=%d dW_ih" % items, dW_ih.t, dW_want[:, :C1], norm_bar, max_bar)
    check("items_wgrad items=%d dW_hh" % items, dW_hh.t, dW_want[:, C1:], norm_bar, max_bar)
    check("items_wgrad items=%d db" % items, db.t, db_want, norm_bar, max_bar)


def test_conv_wgrad_chain(lib):
    """_Bwd.conv_bn_stack_backward's weight gradient (text2speech_amd/tacotron/autograd.py:214-234), B = 2, Cin = 80 (Cin_pad 96),
    Cout = 36, Kt = 5, T = 70, halo 2 (Lp 260, nt = 9 chunks, the last one four rows): t2s_plane_transpose of d_conv and of the
    saved input once per tap (shift = tap - Kt // 2, n_off = tap * Cin_pad); t2s_tm_ones_row(B, Lp, halo, T, ..); the per-batch
    GEMM over all nt chunks (k0 = 0, k1 = nt, ksplit 1: the halo rows and the rows past halo + T are zeros in the planes);
    t2s_wn_backward with Kt and tap_stride = Cin_pad.  Against float64 autograd of F.conv1d on the values the planes hold."""
    B, Cin, Cout, Kt, T, halo = 2, 80, 36, 5, 70, 2
    gen = torch.Generator().manual_seed(200)
    d_conv, d_vals = U.rand_planes(gen, B, Cout, T, halo, scale=0.5)
    x_pl, x_vals = U.rand_planes(gen, B, Cin, T, halo)
    w = torch.randn(Cout, Cin, Kt, generator=gen)
    st = _lib.current_stream()
    W = w.double().requires_grad_(True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    dW_want, db_want = torch.autograd.grad((F.conv1d(x_vals, W, b, padding=Kt // 2) * d_vals).sum(), [W, b])
    assert U.rel(R.conv1d_wgrad(d_vals, x_vals, Kt)[0], dW_want) < 1e-12            # the plain sum says the same
    xp = F.pad(R.with_ones(x_vals.transpose(1, 2)).transpose(1, 2), (Kt // 2, Kt // 2))
    cols = torch.cat([xp[:, :Cin, k:k + T] for k in range(Kt)] + [xp[:, Cin:, Kt // 2:Kt // 2 + T]], 1)
    norm_bar, max_bar = _bars("conv wgrad", d_vals, cols, "bmt,bnt->mn")
    Lp = _lib.plane_rows(T, halo)
    assert d_conv[0].size(2) == Lp and x_pl[0].size(2) == Lp
    occ, icc = -(-Cout // 32), -(-Cin // 32)
    nt = -(-Lp // 32)
    Cin_pad = _ru(Cin, 32)
    Mpad = _lib.padded_rows(Cout)
    Ncols = Kt * Cin_pad
    N = Ncols + 1
    Npad = _ru(N, 256)
    A, X = (_filled(B, nt, Mpad, 32), _filled(B, nt, Mpad, 32)), (_filled(B, nt, Npad, 32), _filled(B, nt, Npad, 32))
    _lib.call("t2s_plane_transpose", ptr(d_conv[0]), ptr(d_conv[1]), B, occ, occ, Lp, 0, ptr(A[0]), ptr(A[1]), Mpad, 0, st)
    for tap in range(Kt):
        _lib.call("t2s_plane_transpose", ptr(x_pl[0]), ptr(x_pl[1]), B, icc, icc, Lp, tap - Kt // 2, ptr(X[0]), ptr(X[1]), Npad,
                  tap * Cin_pad, st)
    _lib.call("t2s_tm_ones_row", ptr(X[0]), ptr(X[1]), B, Lp, halo, T, Npad, Ncols, st)
    M4 = _ru(Cout, 4)
    P = Guarded(B, M4, N)
    zb = torch.zeros(Mpad, device=DEV)
    _lib.call("t2s_wgrad_gemm", ptr(A[0]), ptr(A[1]), ptr(X[0]), ptr(X[1]), ptr(zb), ptr(P.t), B, M4, N, Mpad, Npad, nt, 0, nt, 1, st)
    dW, db = Guarded(Cout, Cin, Kt), Guarded(Cout)
    d_w = dev(w)
    _wn_backward(P.t, B, M4, N, 0, 0, Cin_pad, d_w, Cout, Cin, Kt, dW.t, db.t)
    _sync()
    for o_, name in ((P, "P"), (dW, "dW"), (db, "db")):
        o_.assert_guards("conv wgrad %s" % name)
    assert bool(torch.isfinite(P.t).all())
    # slab b is batch entry b's own sum, in the column order tap * Cin_pad + c, the ones column last
    got = P.t.double().cpu()
    for bi in range(B):
        want = torch.einsum("mt,nt->mn", d_vals[bi], cols[bi])
        g = torch.cat([got[bi][:, k * Cin_pad:k * Cin_pad + Cin] for k in range(Kt)] + [got[bi][:, N - 1:]], 1)
        check("conv wgrad slab %d" % bi, g, want, norm_bar, max_bar)
    check("conv wgrad dW [Cout][Cin][Kt]", dW.t, dW_want, norm_bar, max_bar)
    check("conv wgrad db", db.t, db_want, norm_bar, max_bar)


def test_encoder_projection_wgrad_chain(lib):
    """encoder_backward's input projection (text2speech_amd/tacotron/autograd_encoder.py:65-83), B = 2, T = 37, H = 8, Cin = 40,
    halo 2: t2s_rows_to_tm_batched of dgx [B][T][8H] with shift = halo (position halo + t, the plane row of step t), one set of
    planes per batch entry; t2s_plane_transpose of the saved input planes; the ones row at column Cin; the per-batch GEMM over all
    chunks; t2s_wn_backward once per direction (row_off 0 and 4H).  Against float64 autograd of F.linear per direction."""
    B, T, H, Cin, halo = 2, 37, 8, 40, 2
    gen = torch.Generator().manual_seed(300)
    dgx = torch.randn(B, T, 8 * H, generator=gen) * 0.5
    x_pl, x_vals = U.rand_planes(gen, B, Cin, T, halo)
    w = [torch.randn(4 * H, Cin, generator=gen) for _ in range(2)]
    st = _lib.current_stream()
    want = []
    for d in range(2):
        W = w[d].double().requires_grad_(True)
        b = torch.zeros(4 * H, dtype=torch.float64, requires_grad=True)
        want.append(torch.autograd.grad((F.linear(x_vals.transpose(1, 2), W, b) * dgx[:, :, 4 * H * d:4 * H * (d + 1)].double()).sum(), [W, b]))
    norm_bar, max_bar = _bars("encoder projection wgrad", dgx.double().transpose(1, 2).contiguous(),
                              R.with_ones(x_vals.transpose(1, 2)).transpose(1, 2).contiguous(), "bmt,bnt->mn")
    Lp = _lib.plane_rows(T, halo)
    nt = -(-Lp // 32)
    items_pad = nt * 32
    M = 8 * H
    Mpad = _lib.padded_rows(M)
    icc = _ru(Cin, 32) // 32
    N = Cin + 1
    Npad = _ru(N, 256)
    A, X = (_filled(B, nt, Mpad, 32), _filled(B, nt, Mpad, 32)), (_filled(B, nt, Npad, 32), _filled(B, nt, Npad, 32))
    d_dgx = dev(dgx)
    _lib.call("t2s_rows_to_tm_batched", ptr(d_dgx), M, T * M, T, items_pad, halo, M, ptr(A[0]), ptr(A[1]), nt * Mpad * 32, Mpad, 0, B, st)
    _lib.call("t2s_plane_transpose", ptr(x_pl[0]), ptr(x_pl[1]), B, icc, icc, Lp, 0, ptr(X[0]), ptr(X[1]), Npad, 0, st)
    _lib.call("t2s_tm_ones_row", ptr(X[0]), ptr(X[1]), B, Lp, halo, T, Npad, Cin, st)
    P = Guarded(B, M, N)
    zb = torch.zeros(Mpad, device=DEV)
    _lib.call("t2s_wgrad_gemm", ptr(A[0]), ptr(A[1]), ptr(X[0]), ptr(X[1]), ptr(zb), ptr(P.t), B, M, N, Mpad, Npad, nt, 0, nt, 1, st)
    outs, keep = [], []
    for d in range(2):
        dW, db = Guarded(4 * H, Cin), Guarded(4 * H)
        keep.append(dev(w[d]))
        _wn_backward(P.t, B, M, N, 4 * H * d, 0, 0, keep[-1], 4 * H, Cin, 1, dW.t, db.t)
        outs.append((dW, db))
    _sync()
    P.assert_guards("encoder projection P")
    assert bool(torch.isfinite(P.t).all())
    for d, (dW, db) in enumerate(outs):
        dW.assert_guards("encoder projection dW")
        db.assert_guards("encoder projection db")
        check("encoder projection dW direction %d" % d, dW.t, want[d][0], norm_bar, max_bar)
        check("encoder projection db direction %d" % d, db.t, want[d][1], norm_bar, max_bar)


def test_d_memory_chain(lib):
    """The deferred d_memory (text2speech_amd/tacotron/autograd.py:358-373), B = 3, T = 45 decoder steps of T_cap = 48, T_in = 20,
    E = 24: t2s_rows_to_tm_batched of the alignments [B][T_cap][T_in] (ld T_in, batch stride T_cap T_in; rows T .. T_cap - 1 hold
    77 and must not be read) and of d_ctx [T][B][E] (ld B E, batch stride E); the ones row; the per-batch GEMM with M = T_in whose
    slabs ARE the result; t2s_wn_backward in the mode of line 372 (one slab of B T_in rows, no bias).  Against einsum in float64."""
    B, T, T_cap, T_in, E = 3, 45, 48, 20, 24
    gen = torch.Generator().manual_seed(400)
    align = torch.full((B, T_cap, T_in), 77.0)
    align[:, :T] = torch.softmax(torch.randn(B, T, T_in, generator=gen) * 2, 2)
    dctx = torch.randn(T, B, E, generator=gen) * 0.3
    memory = torch.randn(B, T_in, E, generator=gen)
    st = _lib.current_stream()
    a64, d64 = align[:, :T].double(), dctx.double()
    want = torch.einsum("bti,tbe->bie", a64, d64)
    assert U.rel(R.context_wgrad(a64, d64), want) == 0.0
    norm_bar, max_bar = _bars("d_memory", a64.transpose(1, 2).contiguous(), R.with_ones(d64.transpose(0, 1)).transpose(1, 2).contiguous(),
                              "bmt,bnt->bmn")
    items_pad = _ru(T, 32)
    nch = items_pad // 32
    Mpad, N = _lib.padded_rows(T_in), E + 1
    Npad = _ru(N, 256)
    A, X = (_filled(B, nch, Mpad, 32), _filled(B, nch, Mpad, 32)), (_filled(B, nch, Npad, 32), _filled(B, nch, Npad, 32))
    d_align, d_dctx, d_memory_in = dev(align), dev(dctx), dev(memory)
    _lib.call("t2s_rows_to_tm_batched", ptr(d_align), T_in, T_cap * T_in, T, items_pad, 0, T_in, ptr(A[0]), ptr(A[1]), nch * Mpad * 32,
              Mpad, 0, B, st)
    _lib.call("t2s_rows_to_tm_batched", ptr(d_dctx), B * E, E, T, items_pad, 0, E, ptr(X[0]), ptr(X[1]), nch * Npad * 32, Npad, 0, B, st)
    _lib.call("t2s_tm_ones_row", ptr(X[0]), ptr(X[1]), B, items_pad, 0, T, Npad, E, st)
    P = Guarded(B, T_in, N)
    zb = torch.zeros(Mpad, device=DEV)
    _lib.call("t2s_wgrad_gemm", ptr(A[0]), ptr(A[1]), ptr(X[0]), ptr(X[1]), ptr(zb), ptr(P.t), B, T_in, N, Mpad, Npad, nch, 0, nch, 1, st)
    d_mem = Guarded(B, T_in, E)
    _lib.call("t2s_wn_backward", ptr(P.t), 1, B * T_in, N, 0, 0, 0, N - 1, 1, ptr(d_memory_in), None, B * T_in, E, 1, ptr(d_mem.t),
              None, None, 0, st)
    _sync()
    P.assert_guards("d_memory P")
    d_mem.assert_guards("d_memory")
    assert bool(torch.isfinite(P.t).all())
    check("d_memory [B][T_in][E]", d_mem.t, want, norm_bar, max_bar)
    check("d_memory ones column = sum_t align", P.t[:, :, N - 1], a64.sum(1), norm_bar, max_bar)
