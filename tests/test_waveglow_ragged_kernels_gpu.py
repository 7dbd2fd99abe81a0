"""The four _ragged entry points of WaveGlow.infer_batch (include/t2s_hip.h), one by one through _lib.call in the manner of
tests/test_waveglow_fwd_kernels_gpu.py: t2s_wg_start_ragged (both forms), t2s_wg_res_only_ragged (both row orders),
t2s_wg_res_only_start_ragged and t2s_wg_flow_boundary_ragged (both forms).

Every case is B = 5 entries of lengths 1, L, and one below, at and one above the kernel's own column-tile edge E, with L = E + 2 the
smallest size that has all three inside the range: E = 64 x START_TT = 512 columns per workgroup for start_kernel, T2S_TILE_N = 256
for the residual GEMM, FB_TC = 64 for flow_boundary_kernel.  The output planes are pre-filled with a nonzero pattern - a workspace
that an earlier, longer call has used - and the same inputs go through the unmasked partner on planes of their own.  Asserted:
  rows t < len[b]         bit for bit the partner's (and, joined, the float64 value built from the same inputs at the GEMM bars);
  X rows len[b] <= t < L  exactly zero in both planes - written, not skipped;
  rows [L, Lp), the halo  still the pattern, and nothing in front of or behind the buffer;
  window rows t < len[b]  bit for bit planes.start_window of the entry truncated to len[b], ones-column included, as
                          tests/test_start_fold_gpu.py holds the unmasked writer to its definition."""
import math

import pytest
import torch

import wg_bwd_util as U
import wg_fwd_util as W
from text2speech_amd import _lib, planes

pytestmark = pytest.mark.gpu

DEV = U.DEV
HALO = 128
G8 = 8
PAD = 1024              # bf16 elements in front of and behind every plane buffer
FILL = 0.75             # what an output plane holds beforehand, guards included
START_EDGE = 64 * 8     # 64 x START_TT (csrc/waveglow_ops.hip)
RES_EDGE = 256          # T2S_TILE_N (csrc/conv_gemm.hip)
FB_EDGE = 64            # FB_TC (csrc/waveglow_ops.hip)


def _lengths(edge):
    L = edge + 2
    return L, [1, L, edge - 1, edge, edge + 1]


class _Planes:
    """a (hi, lo) pair of plane buffers [B, nc, Lp, 32] holding FILL everywhere, PAD guard elements either side included"""

    def __init__(self, B, nc, Lp):
        self.shape = (B, nc, Lp, 32)
        n = math.prod(self.shape)
        self.raw = [torch.full((n + 2 * PAD,), FILL, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        self.hi, self.lo = (r[PAD:PAD + n].view(*self.shape) for r in self.raw)

    def set_rows(self, pair, L):
        """data rows [HALO, HALO + L) from another plane pair"""
        for dst, src in zip((self.hi, self.lo), pair):
            dst[:, :, HALO:HALO + L] = src[:, :, HALO:HALO + L]

    def ptrs(self):
        return _lib.ptr(self.hi), _lib.ptr(self.lo)

    def assert_frame(self, L, label):
        n = math.prod(self.shape)
        for r, p in zip(self.raw, (self.hi, self.lo)):
            assert bool((r[:PAD] == FILL).all()) and bool((r[PAD + n:] == FILL).all()), label + ": wrote outside the buffer"
            assert bool((p[:, :, :HALO] == FILL).all()), label + ": the halo in front was written"
            assert bool((p[:, :, HALO + L:] == FILL).all()), label + ": rows [L, Lp) were written"


def _assert_x(label, got, ref, lengths, L, C, want64=None):
    """got, ref: _Planes of the ragged call and of the partner; want64: float64 [B, C, L] or None"""
    got.assert_frame(L, label)
    for b, n in enumerate(lengths):
        for g, r in ((got.hi, ref.hi), (got.lo, ref.lo)):
            assert torch.equal(g[b, :, HALO:HALO + n], r[b, :, HALO:HALO + n]), "%s: entry %d differs from the partner below its length" % (label, b)
            assert bool((g[b, :, HALO + n:HALO + L] == 0).all()), "%s: entry %d has rows past its length that are not zero" % (label, b)
        if want64 is not None:
            U.check("%s entry %d" % (label, b), U.plane_values((got.hi[b:b + 1], got.lo[b:b + 1]), C, n, HALO), want64[b:b + 1, :, :n],
                    U.GEMM_NORM, U.GEMM_MAX)


def _window_rows(z, c_off, nh, taps, nwc, n):
    """the window rows [n, nwc, 32] (hi, lo) of ONE entry z [G, L] truncated to its first n columns, by their definition"""
    win = planes.start_window(z[None, c_off:c_off + nh, :n], taps)
    hi, lo = planes.start_fold_sets(win, False, nwc, 1)
    return hi.view(nwc, 32, n).permute(2, 0, 1), lo.view(nwc, 32, n).permute(2, 0, 1)


def _assert_window(label, got, z, lengths, L, c_off, nh, taps, nwc):
    got.assert_frame(L, label)
    hw = taps // 2
    ncol = taps * (nh + 1)
    for b, n in enumerate(lengths):
        wh, wl = _window_rows(z[b], c_off, nh, taps, nwc, n)
        assert torch.equal(got.hi[b, :, HALO:HALO + n].permute(1, 0, 2), wh), "%s: entry %d hi" % (label, b)
        assert torch.equal(got.lo[b, :, HALO:HALO + n].permute(1, 0, 2), wl), "%s: entry %d lo" % (label, b)
        # spelled out for set 0: the ones-column of the last tap is 0 in the entry's last hw rows - its end, not the batch's
        v = got.hi[b, 0, HALO:HALO + n, :ncol].float() + got.lo[b, 0, HALO:HALO + n, :ncol].float()
        assert bool((v[n - hw:, (taps - 1) * (nh + 1) + nh] == 0).all()) and bool((v[:, hw * (nh + 1) + nh] == 1).all())
        # rows past the entry: every tap at or behind lengths[b] is outside, so from lengths[b] + hw on the rows are zero
        for p in (got.hi, got.lo):
            assert bool((p[b, :, HALO + min(n + hw, L):HALO + L] == 0).all()), "%s: entry %d rows past its end" % (label, b)


def _z(B, L, seed):
    return U.dev(torch.randn(B, G8, L, generator=torch.Generator().manual_seed(seed)))


def _len_dev(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------- t2s_wg_start_ragged
@pytest.mark.parametrize("window", [False, True], ids=["plain", "window"])
@pytest.mark.parametrize("c_off,nh,taps", [(0, 4, 3), (6, 1, 3), (0, 4, 5)])
def test_start_ragged(c_off, nh, taps, window):
    _lib.load()
    L, lengths = _lengths(START_EDGE)
    B, C = len(lengths), 160
    xc = C // 32
    nwc = 2 if 2 * taps * (nh + 1) <= 32 else 4
    Lp = _lib.plane_rows(L, HALO)
    gen = torch.Generator().manual_seed(L + 10 * nh + taps)
    z = _z(B, L, seed=L + nh)
    ws, bs = U.dev(torch.randn(C, nh, generator=gen)), U.dev(torch.randn(C, generator=gen))
    lens = _len_dev(lengths)
    st = _lib.current_stream()
    X, Xr = _Planes(B, xc, Lp), _Planes(B, xc, Lp)
    head = (_lib.ptr(z), _lib.ptr(ws), _lib.ptr(bs), B, G8, c_off, nh, C, L, Lp, HALO)
    if window:
        Wp, Wr = _Planes(B, nwc, Lp), _Planes(B, nwc, Lp)
        _lib.call("t2s_wg_start_ragged", *head, *X.ptrs(), taps, nwc, *Wp.ptrs(), _lib.ptr(lens), st)
        _lib.call("t2s_wg_start_window", *head, *Xr.ptrs(), taps, nwc, *Wr.ptrs(), st)
    else:
        _lib.call("t2s_wg_start_ragged", *head, *X.ptrs(), 0, 0, None, None, _lib.ptr(lens), st)
        _lib.call("t2s_wg_start", *head, *Xr.ptrs(), st)
    torch.cuda.synchronize()
    label = "start_ragged %s off%d nh%d taps%d" % ("window" if window else "plain", c_off, nh, taps)
    want = torch.einsum("cj,bjt->bct", ws.double().cpu(), z[:, c_off:c_off + nh].double().cpu()) + bs.double().cpu()[None, :, None]
    _assert_x(label, X, Xr, lengths, L, C, want)
    if window:
        _assert_window(label, Wp, z, lengths, L, c_off, nh, taps, nwc)
        # the full-length entry is the partner's, every row
        assert torch.equal(Wp.hi[1], Wr.hi[1]) and torch.equal(Wp.lo[1], Wr.lo[1])


# ---------------------------------------------------------------------------------------------- the residual GEMMs
def _pack_res(wn_sd, C, pair8):
    """res_skip_layers[0] of a two-layer WN (2C rows) through t2s_pack_conv_weight_table as text2speech_amd/glow.py lays the job out"""
    Cpad = -(-C // 32) * 32
    Mpad2 = _lib.padded_rows(2 * C)
    f32 = lambda k: U.dev(wn_sd["WN.0.res_skip_layers.0." + k].to(torch.float32))
    v, g, b = f32("weight_v"), f32("weight_g").flatten(), f32("bias")
    Ah = torch.zeros(Cpad // 32, Mpad2, 32, dtype=torch.bfloat16, device=DEV)
    Al, b2, s_rs = torch.zeros_like(Ah), torch.zeros(Mpad2, device=DEV), torch.empty(2 * C, device=DEV)
    row = [v.data_ptr(), g.data_ptr(), b.data_ptr(), 0, Ah.data_ptr(), Al.data_ptr(), b2.data_ptr(), 0, 2 * C, C, 1, 2 if pair8 else 0,
           C if pair8 else 0, Mpad2, 0, Cpad, 0, 0, s_rs.data_ptr()]
    table = torch.tensor([row], dtype=torch.int64).to(DEV)
    _lib.call("t2s_pack_conv_weight_table", _lib.ptr(table), 1, -(-2 * C // 16), _lib.current_stream())
    torch.cuda.synchronize()
    return Ah, Al, b2, Mpad2


_RES = {}


def _res_case(C, nh):
    """the seeded two-layer WN of a width, its inputs at the residual GEMM's shape and the oracle's layer 0: once per (C, nh)"""
    if (C, nh) not in _RES:
        L, lengths = _lengths(RES_EDGE)
        sd = W.wn_state(C, 2, 3, nh, 32, seed=1000 * C + nh)
        audio, spect = W.wn_inputs(len(lengths), nh, 32, L, seed=L + C)
        layers, _ = W.layer_expect(sd, W.wn_cfg(C, 2, 3), audio, spect)
        _RES.clear()
        _RES[(C, nh)] = (sd, audio, layers[0])
    return _RES[(C, nh)]


@pytest.mark.parametrize("C,pair8", [(160, 1), (160, 0), (36, 0)])
def test_res_only_ragged(C, pair8):
    """in place on the oracle's x_0 and acts_0: x_1 = x_0 + W_res . acts_0 + b below each entry's length, zeros from there to L"""
    _lib.load()
    L, lengths = _lengths(RES_EDGE)
    B, xc = len(lengths), -(-C // 32)
    sd, _, ly = _res_case(C, 4)
    Lp = _lib.plane_rows(L, HALO)
    A2h, A2l, b2, Mpad2 = _pack_res(sd, C, bool(pair8))
    Ap = planes.to_planes(U.dev(ly["acts"].float()), HALO, Lp)
    x0 = planes.to_planes(U.dev(ly["x"].float()), HALO, Lp)
    X, Xr = _Planes(B, xc, Lp), _Planes(B, xc, Lp)
    X.set_rows(x0, L)
    Xr.set_rows(x0, L)
    lens = _len_dev(lengths)
    st = _lib.current_stream()
    head = (_lib.ptr(A2h), _lib.ptr(A2l), _lib.ptr(b2), _lib.ptr(Ap[0]), _lib.ptr(Ap[1]))
    _lib.call("t2s_wg_res_only_ragged", *head, *X.ptrs(), B, C, L, Lp, HALO, Mpad2, pair8, _lib.ptr(lens), st)
    _lib.call("t2s_wg_res_only", *head, *Xr.ptrs(), B, C, L, Lp, HALO, Mpad2, pair8, st)
    torch.cuda.synchronize()
    label = "res_only_ragged C%d pair8=%d" % (C, pair8)
    _assert_x(label, X, Xr, lengths, L, C, ly["x_next"])
    if C % 32:
        for p in (X.hi, X.lo):          # channels past C: what they held (x_0's planes have zeros there)
            assert float(p[:, -1, HALO:HALO + L, C % 32:].float().abs().max()) == 0.0, label + ": channels past C were written"


@pytest.mark.parametrize("C,c_off,nh", [(160, 0, 4), (128, 2, 3), (32, 6, 1)])
def test_res_only_start_ragged(C, c_off, nh):
    """x_0 rebuilt from z in the epilogue; the X planes' data rows hold NaN beforehand (they are only written)"""
    _lib.load()
    L, lengths = _lengths(RES_EDGE)
    B, xc = len(lengths), C // 32
    sd, audio, ly = _res_case(C, nh)
    Lp = _lib.plane_rows(L, HALO)
    A2h, A2l, b2, Mpad2 = _pack_res(sd, C, True)
    Ap = planes.to_planes(U.dev(ly["acts"].float()), HALO, Lp)
    z = _z(B, L, seed=C + L)
    z[:, c_off:c_off + nh] = U.dev(audio.float())
    f32 = lambda k: U.dev(sd["WN.0.start." + k].to(torch.float32))
    w_start = torch.empty(C, nh, device=DEV)
    st = _lib.current_stream()
    v, g, b_start = f32("weight_v"), f32("weight_g").flatten(), f32("bias")
    _lib.call("t2s_weightnorm_small", _lib.ptr(v), _lib.ptr(g), C, nh, _lib.ptr(w_start), st)
    X, Xr = _Planes(B, xc, Lp), _Planes(B, xc, Lp)
    for p in (X, Xr):
        p.hi[:, :, HALO:HALO + L] = float("nan")
        p.lo[:, :, HALO:HALO + L] = float("nan")
    lens = _len_dev(lengths)
    head = (_lib.ptr(A2h), _lib.ptr(A2l), _lib.ptr(b2), _lib.ptr(Ap[0]), _lib.ptr(Ap[1]), _lib.ptr(z), _lib.ptr(w_start),
            _lib.ptr(b_start), G8, c_off, nh)
    _lib.call("t2s_wg_res_only_start_ragged", *head, *X.ptrs(), B, C, L, Lp, HALO, Mpad2, _lib.ptr(lens), st)
    _lib.call("t2s_wg_res_only_start", *head, *Xr.ptrs(), B, C, L, Lp, HALO, Mpad2, st)
    torch.cuda.synchronize()
    _assert_x("res_only_start_ragged C%d off%d nh%d" % (C, c_off, nh), X, Xr, lengths, L, C, ly["x_next"])


# ---------------------------------------------------------------------------------------------- t2s_wg_flow_boundary_ragged
@pytest.mark.parametrize("full", [False, True], ids=["window-only", "coupling+conv"])
@pytest.mark.parametrize("c_off,nh,taps", [(0, 4, 3), (2, 3, 3), (0, 4, 5)])
def test_flow_boundary_ragged(c_off, nh, taps, full):
    """the window planes from the finished columns, each entry's taps ending at its own length; with the coupling of the flow before
    and the 1x1 convolution (per column: over all L columns, as the partner) z_out and log_s bit for bit the partner's"""
    _lib.load()
    L, lengths = _lengths(FB_EDGE)
    B, nslots, nl = len(lengths), 4, 3
    n_rem = G8 - c_off
    nwc = 2 if 2 * taps * (nh + 1) <= 32 else 4
    Lp = _lib.plane_rows(L, HALO)
    gen = torch.Generator().manual_seed(100 * taps + 10 * c_off + nh)
    z = _z(B, L, seed=L + c_off)
    z_keep = z.clone()
    lens = _len_dev(lengths)
    st = _lib.current_stream()
    Wp, Wr = _Planes(B, nwc, Lp), _Planes(B, nwc, Lp)
    label = "flow_boundary_ragged %s off%d nh%d taps%d" % ("full" if full else "window-only", c_off, nh, taps)
    if full:
        fold_acc = U.dev(0.1 * torch.randn(nslots, B, 8, L, generator=gen))
        bes, b_end = U.dev(0.1 * torch.randn(nl, 8, generator=gen)), U.dev(0.1 * torch.randn(8, generator=gen))
        Wm = U.dev(torch.randn(8, 8, generator=gen)[:n_rem, :n_rem])
        outs = []
        for name, planes_, tail in (("t2s_wg_flow_boundary_ragged", Wp, (_lib.ptr(lens), st)), ("t2s_wg_flow_boundary", Wr, (st,))):
            z_out = torch.full((B, G8, L), float("nan"), device=DEV)
            ls = torch.full((B, 4, L), float("nan"), device=DEV)
            _lib.call(name, _lib.ptr(z), _lib.ptr(z_out), _lib.ptr(fold_acc), nslots, _lib.ptr(bes), nl, _lib.ptr(b_end), _lib.ptr(ls),
                      0, 4, _lib.ptr(Wm), c_off, n_rem, nh, B, G8, L, Lp, HALO, taps, nwc, *planes_.ptrs(), *tail)
            outs.append((z_out, ls))
        torch.cuda.synchronize()
        (z_out, ls), (z_ref, ls_ref) = outs
        assert bool(torch.isfinite(z_out).all()) and bool(torch.isfinite(ls).all())
        assert torch.equal(z_out, z_ref) and torch.equal(ls, ls_ref), label + ": z_out / log_s differ from the partner"
        # float64 from the same inputs: the coupling of the flow before (c_off 0, n_half 4), then the convolution
        zd, fa = z.double().cpu(), fold_acc.double().cpu().sum(0)
        sums = fa + bes.double().cpu().sum(0)[None, :, None] + b_end.double().cpu()[None, :, None]
        zd[:, 4:8] = torch.exp(sums[:, 4:]) * zd[:, 4:8] + sums[:, :4]
        zd[:, c_off:] = torch.einsum("ij,bjt->bit", Wm.double().cpu(), zd[:, c_off:])
        U.check(label + " z_out", z_out, zd, U.F32_NORM, U.F32_MAX)
        U.check(label + " log_s", ls, sums[:, 4:], U.F32_NORM, U.F32_MAX)
        src = z_out
    else:
        _lib.call("t2s_wg_flow_boundary_ragged", _lib.ptr(z), None, None, 0, None, 0, None, None, 0, 0, None, c_off, n_rem, nh, B, G8, L,
                  Lp, HALO, taps, nwc, *Wp.ptrs(), _lib.ptr(lens), st)
        _lib.call("t2s_wg_flow_boundary", _lib.ptr(z), None, None, 0, None, 0, None, None, 0, 0, None, c_off, n_rem, nh, B, G8, L,
                  Lp, HALO, taps, nwc, *Wr.ptrs(), st)
        torch.cuda.synchronize()
        src = z
    assert torch.equal(z, z_keep), label + ": the input buffer changed"
    _assert_window(label, Wp, src, lengths, L, c_off, nh, taps, nwc)
    Wr.assert_frame(L, label + " (partner)")
    assert torch.equal(Wp.hi[1], Wr.hi[1]) and torch.equal(Wp.lo[1], Wr.lo[1])         # the full-length entry: the partner's rows
    for b, n in enumerate(lengths):             # and every row whose taps all lie below the entry's length
        m = max(n - taps // 2, 0)
        assert torch.equal(Wp.hi[b, :, HALO:HALO + m], Wr.hi[b, :, HALO:HALO + m]) and torch.equal(Wp.lo[b, :, HALO:HALO + m], Wr.lo[b, :, HALO:HALO + m])
