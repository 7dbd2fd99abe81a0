"""The three _h16_ragged entry points behind WaveGlow.infer_batch on the fp16 chain (include/t2s_hip.h), one by one through _lib.call
in the manner of tests/test_waveglow_ragged_kernels_gpu.py, on the operands tests/test_waveglow_h16_kernels_gpu.py builds:
t2s_wg_start_h16_ragged, t2s_wg_res_only_h16_ragged (both row orders) and t2s_wg_in_cond_gate_fold_h16_ragged (both tile heights).

Every case is B = 5 entries of lengths 1, L, and one below, at and one above the kernel's own column-tile edge E, with L = E + 2:
E = 64 x START_TT = 512 for start_kernel, T2S_TILE_N = 256 for the two GEMMs.  Output planes and fold_acc are pre-filled with a
nonzero pattern, guards either side included - a workspace an earlier, longer call has used - and the same inputs go through the
unmasked _h16 partner on buffers of their own.  At E = 256 the lengths 1, 255 and 256 leave the second column tile pure padding:
that is the tile the GEMMs skip (no load, no matrix instruction); 257 and 258 cut it, and a cut tile is computed whole.  Asserted:

  start, residual   rows t < len[b] bit for bit the partner's and, joined, the float64 value of the decoded operands at the bars
                    of tests/test_waveglow_h16_kernels_gpu.py; rows len[b] <= t < L exactly zero in both planes - stored by the
                    epilogue in a cut tile, by the skip path in a skipped one; halo, rows [L, Lp), channels past C and the guards
                    still the pattern;
  gate              every tile with t0 < len[b]: acts (hi, lo) and fold_acc bit for bit the partner's over the WHOLE tile, the
                    columns at and past len[b] included, and float64 at the bars; every tile with t0 >= len[b]: acts still the
                    pattern, fold_acc exactly zero under fold_init = 1 and still the pattern under fold_init = 0."""
import math

import pytest
import torch

import test_waveglow_h16_kernels_gpu as H
import wg_bwd_util as U
import wg_fwd_util as W
from text2speech_amd import _lib

pytestmark = pytest.mark.gpu

DEV = U.DEV
HALO = H.HALO
G8 = 8
PAD = 1024              # elements in front of and behind every output buffer
FILL = 0.75             # what an output plane holds beforehand, guards included
FOLD_FILL = 0.375       # ... and fold_acc
START_EDGE = 64 * 8     # 64 x START_TT (csrc/waveglow_ops.hip)
TILE = 256              # T2S_TILE_N = T2S_RAG_SKIP_COLS (csrc/t2s_kernels.h)
H16 = H.H16


def _lengths(edge):
    L = edge + 2
    return L, [1, L, edge - 1, edge, edge + 1]


def _len_dev(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device=DEV)


class _Planes:
    """a (hi, lo) pair of fp16 plane buffers [B, nc, Lp, 32] holding FILL everywhere, PAD guard elements either side included"""

    def __init__(self, B, nc, Lp):
        self.shape = (B, nc, Lp, 32)
        n = math.prod(self.shape)
        self.raw = [torch.full((n + 2 * PAD,), FILL, **H16) for _ in range(2)]
        self.hi, self.lo = (r[PAD:PAD + n].view(*self.shape) for r in self.raw)

    def set_rows(self, pair, L, C):
        """channels < C of the data rows [HALO, HALO + L) from another plane pair; the channel slots past C keep FILL"""
        for dst, src in zip((self.hi, self.lo), pair):
            v = dst[:, :, HALO:HALO + L].permute(0, 2, 1, 3).reshape(dst.size(0), L, -1)
            v[:, :, :C] = src[:, :, HALO:HALO + L].permute(0, 2, 1, 3).reshape(dst.size(0), L, -1)[:, :, :C]
            dst[:, :, HALO:HALO + L] = v.view(dst.size(0), L, -1, 32).permute(0, 2, 1, 3)

    def ptrs(self):
        return _lib.ptr(self.hi), _lib.ptr(self.lo)

    def assert_frame(self, L, C, label):
        n = math.prod(self.shape)
        for r, p in zip(self.raw, (self.hi, self.lo)):
            assert bool((r[:PAD] == FILL).all()) and bool((r[PAD + n:] == FILL).all()), label + ": wrote outside the buffer"
            assert bool((p[:, :, :HALO] == FILL).all()), label + ": the halo in front was written"
            assert bool((p[:, :, HALO + L:] == FILL).all()), label + ": rows [L, Lp) were written"
            if C % 32:
                assert bool((p[:, -1, :, C % 32:] == FILL).all()), label + ": channels past C were written"


class _Fold:
    """fold_acc [nslots, B, 8, L] f32 holding FOLD_FILL, PAD guard floats either side included"""

    def __init__(self, *shape):
        self.n = math.prod(shape)
        self.raw = torch.full((self.n + 2 * PAD,), FOLD_FILL, device=DEV)
        self.t = self.raw[PAD:PAD + self.n].view(*shape)

    def assert_guards(self, label):
        assert bool((self.raw[:PAD] == FOLD_FILL).all()) and bool((self.raw[PAD + self.n:] == FOLD_FILL).all()), \
            label + ": wrote outside fold_acc"


def _bits(t):
    return t.view(torch.int16)


def _chan(p, b, C, r0, r1):
    """[r1 - r0, C] of entry b: channels < C of data rows [r0, r1) of one plane"""
    return p[b, :, HALO + r0:HALO + r1].permute(1, 0, 2).reshape(r1 - r0, 32 * p.size(1))[:, :C]


def _assert_x(label, got, ref, lengths, L, C, want64, bars, Cw=None):
    """got, ref: _Planes of the ragged call and of the partner; want64: float64 [B, C, L]; Cw: the channel slots the kernel writes
    (default C; start_kernel stores whole 32-channel rows, zeros past C)"""
    Cw = C if Cw is None else Cw
    got.assert_frame(L, Cw, label)
    ref.assert_frame(L, Cw, label + " (partner)")
    for b, n in enumerate(lengths):
        n = min(max(n, 0), L)
        for g, r in ((got.hi, ref.hi), (got.lo, ref.lo)):
            assert torch.equal(_bits(_chan(g, b, Cw, 0, n)), _bits(_chan(r, b, Cw, 0, n))), \
                "%s: entry %d differs from the partner below its length" % (label, b)
            assert bool((_bits(_chan(g, b, Cw, n, L)) == 0).all()), "%s: entry %d has rows past its length that are not zero" % (label, b)
        if n:
            U.check("%s entry %d" % (label, b), U.plane_values((got.hi[b:b + 1], got.lo[b:b + 1]), C, n, HALO), want64[b:b + 1, :, :n], *bars)


# ---------------------------------------------------------------------------------------------- t2s_wg_start_h16_ragged
@pytest.mark.parametrize("c_off,nh", [(0, 4), (6, 1)])
def test_start_h16_ragged(c_off, nh):
    _lib.load()
    L, lengths = _lengths(START_EDGE)
    B, C = len(lengths), 36
    wn = H._WN(C, 2, 3, nh, 32, seed=5 + nh)
    Lp = _lib.plane_rows(L, HALO)
    z = U.dev(torch.randn(B, G8, L, generator=torch.Generator().manual_seed(L + c_off)))
    lens = _len_dev(lengths)
    st = _lib.current_stream()
    X, Xr = _Planes(B, 2, Lp), _Planes(B, 2, Lp)
    head = (_lib.ptr(z), _lib.ptr(wn.w_start()), _lib.ptr(wn.p("start.bias")), B, G8, c_off, nh, C, L, Lp, HALO)
    _lib.call("t2s_wg_start_h16_ragged", *head, *X.ptrs(), _lib.ptr(lens), st)
    _lib.call("t2s_wg_start_h16", *head, *Xr.ptrs(), st)
    torch.cuda.synchronize()
    want = torch.einsum("cj,bjt->bct", wn.w_start().double().cpu(), z.double().cpu()[:, c_off:c_off + nh]) + \
        wn.p("start.bias").double().cpu()[None, :, None]
    label = "start_h16_ragged off%d nh%d" % (c_off, nh)
    _assert_x(label, X, Xr, lengths, L, C, want, (U.GEMM_NORM, U.GEMM_MAX), Cw=64)


# ---------------------------------------------------------------------------------------------- t2s_wg_res_only_h16_ragged
def _res_launch(C, pair8, lengths, L):
    """-> (label, X, Xr, want64, bars) after t2s_wg_res_only_h16_ragged on X and its partner on Xr, in place on the oracle's x_0"""
    B, xc = 5, -(-C // 32)
    wn, _, _, layers, _ = H._case(C, 8, 3, 4, 40, B, L)
    ly = layers[0]
    Lp = _lib.plane_rows(L, HALO)
    A2h, b2, Mpad2, _ = wn.res(0, bool(pair8))
    Ap, X0 = H._to_h16(ly["acts"], Lp), H._to_h16(ly["x"], Lp)
    X, Xr = _Planes(B, xc, Lp), _Planes(B, xc, Lp)
    X.set_rows(X0, L, C)
    Xr.set_rows(X0, L, C)
    assert len(lengths) == B
    lens = _len_dev(lengths)
    st = _lib.current_stream()
    head = (_lib.ptr(A2h), None, _lib.ptr(b2), _lib.ptr(Ap[0]), _lib.ptr(Ap[1]))
    _lib.call("t2s_wg_res_only_h16_ragged", *head, *X.ptrs(), B, C, L, Lp, HALO, Mpad2, pair8, _lib.ptr(lens), st)
    _lib.call("t2s_wg_res_only_h16", *head, *Xr.ptrs(), B, C, L, Lp, HALO, Mpad2, pair8, st)
    torch.cuda.synchronize()
    w_res, b_res = wn.res_decoded(0, bool(pair8))
    av, xv = U.plane_values(Ap, C, L, HALO), U.plane_values(X0, C, L, HALO)
    mm = lambda a, b: torch.einsum("oc,bct->bot", a, b)
    want = xv + mm(w_res, av) + b_res[None, :, None]
    floor = H._two_product_floor(w_res, av, mm)
    label = "res_only_h16_ragged C%d pair8=%d lengths %s" % (C, pair8, lengths)
    print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e (of W_res . acts alone)" % (label, floor[0], floor[1]))
    return label, X, Xr, want, H._bars(floor)


@pytest.mark.parametrize("C,pair8", [(64, 0), (64, 1), (48, 0)])
def test_res_only_h16_ragged(C, pair8):
    """lengths 1, 255 and 256 skip the second tile (its rows 256, 257 must still come out as zeros); 257 and 258 cut it"""
    _lib.load()
    L, lengths = _lengths(TILE)
    label, X, Xr, want, bars = _res_launch(C, pair8, lengths, L)
    _assert_x(label, X, Xr, lengths, L, C, want, bars)


def test_res_only_h16_ragged_clamped_lengths():
    """straight through the ABI: a length of 0 skips every tile of its entry, a negative one is clamped to 0 and one above L to L"""
    _lib.load()
    L, _ = _lengths(TILE)
    label, X, Xr, want, bars = _res_launch(64, 1, [0, -3, L + 5, 2, L], L)
    _assert_x(label, X, Xr, [0, 0, L, 2, L], L, 64, want, bars)


# ---------------------------------------------------------------------------------------------- t2s_wg_in_cond_gate_fold_h16_ragged
@pytest.mark.parametrize("fold_init", [1, 0])
@pytest.mark.parametrize("dil", [1, 128])
@pytest.mark.parametrize("C,tile", [(64, 128), (48, 256)])
def test_in_cond_gate_fold_h16_ragged(C, tile, dil, fold_init):
    lib = _lib.load()
    L, lengths = _lengths(TILE)
    B, n_cond, ks, nslots = len(lengths), 40, 3, 2
    assert lib.t2s_wg_gate_tile_rows(B, C, L) == tile, "the tile-height rule moved this case off the %d-row kernel" % tile
    assert lib.t2s_wg_gate_fold_slots(B, C, L) == nslots
    i = int(math.log2(dil))
    wn, _, spect, layers, _ = H._case(C, 8, ks, 4, n_cond, B, L)
    Lp = _lib.plane_rows(L, HALO)
    xc = -(-C // 32)
    Sp, Xp = H._to_h16(spect, Lp), H._to_h16(layers[i]["x"], Lp)
    Ah, b1 = wn.gate(i)
    lens = _len_dev(lengths)
    st = _lib.current_stream()
    acts, acts_r = _Planes(B, xc, Lp), _Planes(B, xc, Lp)
    fold, fold_r = _Fold(nslots, B, 8, L), _Fold(nslots, B, 8, L)
    label = "gate_h16_ragged C%d (%d rows) d%d fold_init=%d" % (C, tile, dil, fold_init)

    def args(a, f):
        return (_lib.ptr(Ah), None, _lib.ptr(b1), _lib.ptr(Xp[0]), _lib.ptr(Xp[1]), _lib.ptr(Sp[0]), _lib.ptr(Sp[1]), *a.ptrs(),
                _lib.ptr(wn.fold(i)[0]), _lib.ptr(f.t), fold_init, B, C, n_cond, ks, dil, L, Lp, HALO, wn.Mpad1)
    _lib.call("t2s_wg_in_cond_gate_fold_h16_ragged", *args(acts, fold), _lib.ptr(lens), st)
    _lib.call("t2s_wg_in_cond_gate_fold_h16", *args(acts_r, fold_r), st)
    torch.cuda.synchronize()
    # nothing outside the buffers, the data rows, the channels
    acts.assert_frame(L, C, label)
    acts_r.assert_frame(L, C, label + " (partner)")
    fold.assert_guards(label)
    # float64 of the decoded operands, as tests/test_waveglow_h16_kernels_gpu.py::_check_gate builds it
    w_in, w_cond, bias = wn.gate_decoded(i)
    xv, sv = U.plane_values(Xp, C, L, HALO), U.plane_values(Sp, n_cond, L, HALO)
    pre = H._gate_pre(w_in, w_cond, bias, xv, sv, dil, ks)
    want = torch.tanh(pre[:, :C]) * torch.sigmoid(pre[:, C:])
    xh, sh = xv.to(torch.float16).double(), sv.to(torch.float16).double()
    pre32 = H._gate_pre(w_in, w_cond, bias, xh.float(), sh.float(), dil, ks).double() + \
        H._gate_pre(w_in, w_cond, torch.zeros_like(bias), (xv - xh).float(), (sv - sh).float(), dil, ks).double()
    emu = torch.tanh(pre32[:, :C]) * torch.sigmoid(pre32[:, C:])
    bars = H._bars((U.rel(emu, want), U.maxrel(emu, want)))
    Fd = W._endfold_decode(wn.fold(i)[0], C)[:8, :C]
    fbars = H._bars(H._split3_floor_f16(Fd, want.float().double(), "jc,bct->bjt"))
    print("BARS   %-60s acts %.1e / %.1e  fold %.1e / %.1e" % (label, *bars, *fbars))
    n_skipped = 0
    for b, n in enumerate(lengths):
        for t0 in range(0, L, TILE):
            t1 = min(t0 + TILE, L)
            where = "%s: entry %d (length %d) tile [%d, %d)" % (label, b, n, t0, t1)
            rows = slice(HALO + t0, HALO + t1)
            if t0 < n:      # computed whole, the columns at and past the entry's end included
                for g, r in ((acts.hi, acts_r.hi), (acts.lo, acts_r.lo)):
                    assert torch.equal(_bits(g[b, :, rows]), _bits(r[b, :, rows])), where + ": acts differ from the partner's"
                assert torch.equal(fold.t[:, b, :, t0:t1].view(torch.int32), fold_r.t[:, b, :, t0:t1].view(torch.int32)), \
                    where + ": fold_acc differs from the partner's"
                got = U.plane_values((acts.hi[b:b + 1], acts.lo[b:b + 1]), C, t1, HALO)[:, :, t0:]
                U.check(where + " acts", got, want[b:b + 1, :, t0:t1], *bars)
                wantf = torch.einsum("jc,bct->bjt", Fd, got) + (0.0 if fold_init else nslots * FOLD_FILL)
                U.check(where + " fold", fold.t[:, b, :, t0:t1].double().sum(0)[None], wantf, *fbars)
            else:           # skipped
                n_skipped += 1
                for g in (acts.hi, acts.lo):
                    assert bool((g[b, :, rows] == FILL).all()), where + ": a skipped tile wrote acts"
                if fold_init:
                    assert bool((fold.t[:, b, :, t0:t1].view(torch.int32) == 0).all()), where + ": fold_acc is not exactly zero"
                else:
                    assert bool((fold.t[:, b, :, t0:t1] == FOLD_FILL).all()), where + ": fold_acc was touched under fold_init = 0"
    assert n_skipped == 3


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_validation_without_launching():
    """lengths = NULL, a misaligned plane and the partner's own shape refusals, each alone, return T2S_EINVAL with nothing
    enqueued: the outputs keep their sentinel.  The tuples the broken ones are made from are themselves accepted."""
    lib = _lib.load()
    P = _lib.ptr
    B, C, n_cond, L, taps = 2, 64, 32, 40, 3
    Lp = _lib.plane_rows(L, HALO)
    A = torch.zeros(taps * 2 + 1, 256, 32, **H16)
    bias = torch.zeros(256, device=DEV)
    Xp, Sp = torch.zeros(B, 2, Lp, 32, **H16), torch.zeros(B, 1, Lp, 32, **H16)
    fold_A = torch.zeros(8192, **H16)
    outs = [torch.full((B, 2, Lp, 32), FILL, **H16) for _ in range(2)]
    acc = _Fold(2, B, 8, L)
    lens = _len_dev([L, 3])
    st = _lib.current_stream()
    off2 = lambda t: _lib.c_vp(t.data_ptr() + 2)          # two bytes past a 16-byte boundary

    def unchanged():
        torch.cuda.synchronize()
        return all(bool((o == FILL).all()) for o in outs) and bool((acc.raw == FOLD_FILL).all())

    def gate(**ch):
        a = dict(A_hi=P(A), A_lo=None, bias=P(bias), X_hi=P(Xp), X_lo=P(Xp), S_hi=P(Sp), S_lo=P(Sp), acts_hi=P(outs[0]), acts_lo=P(outs[1]),
                 fold_A=P(fold_A), fold_acc=P(acc.t), fold_init=1, B=B, C=C, n_cond=n_cond, taps=taps, dilation=1, L=L, Lp=Lp, halo=HALO,
                 Mpad=256, lengths=P(lens), stream=st)
        a.update(ch)
        return lib.t2s_wg_in_cond_gate_fold_h16_ragged(*a.values())

    def res(**ch):
        a = dict(A_hi=P(A), A_lo=None, bias=P(bias), acts_hi=P(Xp), acts_lo=P(Xp), X_hi=P(outs[0]), X_lo=P(outs[1]), B=B, C=C, L=L, Lp=Lp,
                 halo=HALO, Mpad=256, pair8=1, lengths=P(lens), stream=st)
        a.update(ch)
        return lib.t2s_wg_res_only_h16_ragged(*a.values())

    z, ws, bs = torch.zeros(B, G8, L, device=DEV), torch.zeros(C, 4, device=DEV), torch.zeros(C, device=DEV)

    def start(**ch):
        a = dict(z=P(z), w=P(ws), bias=P(bs), B=B, n_group=G8, c_off=0, n_half=4, C=C, L=L, Lp=Lp, halo=HALO, X_hi=P(outs[0]), X_lo=P(outs[1]),
                 lengths=P(lens), stream=st)
        a.update(ch)
        return lib.t2s_wg_start_h16_ragged(*a.values())

    bad = [(gate, dict(lengths=None)), (res, dict(lengths=None)), (start, dict(lengths=None)),
           (gate, dict(A_hi=off2(A))), (gate, dict(X_lo=off2(Xp))), (gate, dict(acts_hi=off2(outs[0]))), (gate, dict(fold_A=off2(fold_A))),
           (res, dict(A_hi=off2(A))), (res, dict(X_hi=off2(outs[0]))), (start, dict(X_lo=off2(outs[1]))),
           (gate, dict(A_hi=None)), (gate, dict(acts_lo=None)), (gate, dict(fold_acc=None)), (gate, dict(C=24)), (gate, dict(C=40)),
           (gate, dict(Lp=Lp + 1)), (gate, dict(dilation=HALO + 1)),
           (res, dict(acts_lo=None)), (res, dict(X_lo=None)), (res, dict(C=48, pair8=1)), (res, dict(C=30, pair8=0)), (res, dict(Lp=Lp - 1)),
           (start, dict(X_hi=None)), (start, dict(z=None)), (start, dict(Lp=Lp - 1)), (start, dict(n_half=9))]
    for fn, ch in bad:
        assert fn(**ch) == -1, "%s accepted %r" % (fn.__name__, ch)
        assert unchanged(), "%s wrote something with %r" % (fn.__name__, ch)
    # the tuples themselves are accepted (zero operands: the launches are harmless)
    for fn in (gate, res, start):
        assert fn() == 0, fn.__name__
    torch.cuda.synchronize()
