"""The WaveGlow backward kernels one by one through the C ABI (run with -m gpu on an MI355X), each against a float64 restatement
on the CPU at its tile edges.  Every case asserts the norm-relative error, the MAXIMUM error relative to the expectation's largest
element (one wrong row, column or tile edge moves no norm), untouched halo rows and untouched memory around the output.

The expectations are evaluated on the values the operand planes actually hold (hi + lo read back), so input rounding is not
counted; what remains is the arithmetic of the kernels (split-bf16: hi.hi + hi.lo + lo.hi, f32 accumulate), whose floor
wg_bwd_util.split3_floor computes on the CPU.  Bars: the GEMM kernels and plane outputs take test_wn_layer's (2e-5 / 1e-4), the
f32 small ops test_small_stages' (1e-5 / 1e-4).  profiles/waveglow_bwd_kernel_parity.md has that floor and what the
max-relative assertion adds; every check prints its two figures (`PARITY ...`) before it asserts."""
import types

import pytest
import torch
import torch.nn.functional as F

import wg_bwd_util as U
from text2speech_amd import _lib, planes
from text2speech_amd.glow_autograd import _chunk_rows, _chunk_table
from wg_bwd_util import DEV, F32_MAX, F32_NORM, GEMM_MAX, GEMM_NORM, Guarded, check, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
ptr = _lib.ptr


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _sync():
    torch.cuda.synchronize()


def _bf_full(shape, value):
    return torch.full(shape, value, dtype=torch.bfloat16, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. t2s_wgrad_cl
# An operand side is a list of pieces (pair, first chunk, chunks, row shift); a pair of rank 2 is a constant chunk (batch stride 0).

def _table(pieces, consts):
    rows = []
    for pair, first, n, shift in pieces:
        if pair[0].dim() == 2:
            rows.append([pair[0].data_ptr(), pair[1].data_ptr(), 0])
        else:
            rows += _chunk_rows(pair, n, shift, first)
    return _chunk_table(consts, rows, DEV)


def _side_values(pieces, B, r0, r1):
    out = []
    for pair, first, n, shift in pieces:
        v = U.plane_rows(pair, first, n, shift, r0, r1)
        out.append(v.expand(B, -1, -1) if v.size(0) == 1 else v)
    return torch.cat(out, 1)


_WGRAD = {}


def _wgrad_case(name):
    """Operand planes, chunk tables and the float64 expectation of one t2s_wgrad_cl shape (built once per module)."""
    if name in _WGRAD:
        return _WGRAD[name]
    gen = torch.Generator().manual_seed(100 + ord(name))
    B, L, halo = dict(a=(1, 1, 32), b=(3, 130, 128), c=(2, 300, 32), d=(1, 33, 32))[name]
    Lp = _lib.plane_rows(L, halo)
    c = types.SimpleNamespace(name=name, B=B, L=L, halo=halo, Lp=Lp, k0=halo // 32, k1=-(-(halo + L) // 32))
    c.zero_plane = torch.zeros(Lp, 32, dtype=torch.bfloat16, device=DEV)
    c.ones_plane = torch.zeros(Lp, 32, dtype=torch.bfloat16, device=DEV)
    c.ones_plane[halo:halo + L, 0] = 1.0              # 1 on [halo, halo + L) only
    ones = ((c.ones_plane, c.zero_plane), 0, 1, 0)
    rp = lambda C: U.rand_planes(gen, B, C, L, halo)[0]
    if name == "a":        # one chunk either side, one time step
        c.a_pieces = [(rp(32), 0, 1, 0)]
        c.b_pieces = [(rp(32), 0, 1, 0), ones]
        c.M, c.N = 32, 33
    elif name == "b":      # M rows from two plane sets; N: three dilated taps of x, a slice of a wider set, ones
        x, s_wide = rp(64), rp(160)
        c.a_pieces = [(rp(64), 0, 2, 0), (rp(64), 0, 2, 0)]
        c.b_pieces = [(x, 0, 2, -128), (x, 0, 2, 0), (x, 0, 2, 128), (s_wide, 1, 3, 0), ones]
        c.M, c.N = 128, 289
    elif name == "c":      # ten M chunks (8 + 2), N exactly one tile: the bias gradient as row sums (bias_cols)
        c.a_pieces = [(rp(320), 0, 10, 0)]
        c.b_pieces = [(rp(256), 0, 8, 0)]
        c.M, c.N = 320, 256
    else:                  # the second N tile holds the ones column only
        c.a_pieces = [(rp(512), 0, 16, 0)]
        c.b_pieces = [(rp(256), 0, 8, 0), ones]
        c.M, c.N = 512, 257
    c.ta, c.tb = _table(c.a_pieces, c), _table(c.b_pieces, c)
    r0, r1 = 32 * c.k0, 32 * c.k1
    c.a_val = _side_values(c.a_pieces, B, r0, r1)[:, :c.M]
    c.b_val = _side_values(c.b_pieces, B, r0, r1)[:, :c.N]
    c.want = torch.einsum("bmt,bnt->mn", c.a_val, c.b_val)
    c.floor = U.split3_floor(c.a_val, c.b_val, "bmt,bnt->mn")
    print("FLOOR  wgrad_cl case %s: split-bf16 emulation norm-rel %.3e max-rel %.3e" % ((name,) + c.floor))
    _WGRAD[name] = c
    return c


def _run_wgrad_cl(c, nsplit, ldp, bias_cols=0):
    out = Guarded(nsplit, c.M, ldp)
    _lib.call("t2s_wgrad_cl", ptr(c.ta), c.ta.size(0), ptr(c.tb), c.tb.size(0), ptr(out.t), c.B, c.M, c.N, ldp, c.k0, c.k1,
              nsplit, bias_cols, _lib.current_stream())
    _sync()
    label = "wgrad_cl[%s nsplit=%d ldp=%d]" % (c.name, nsplit, ldp)
    out.assert_guards(label)
    check(label, out.t[:, :, :c.N].double().sum(0), c.want, GEMM_NORM, GEMM_MAX)     # (columns N .. ldp-1 are scratch)
    return out


@pytest.mark.parametrize("ldp", [36, 33])        # ping-pong kernel / lockstep kernel
def test_wgrad_cl_one_step(lib, ldp):
    """1a: B = 1, one chunk of M, 32 channels + ones, L = 1."""
    _run_wgrad_cl(_wgrad_case("a"), 1, ldp)


@pytest.mark.parametrize("ldp", [292, 289])
@pytest.mark.parametrize("nsplit", [1, 2, 4, 15])    # 2: a slab crosses a batch boundary; 4: the last slab is shorter; 15 = B (k1 - k0)
def test_wgrad_cl_taps_slices_and_splits(lib, nsplit, ldp):
    """1b: two M plane sets, dilated taps at -128 / 0 / +128, a slice of a wider plane set, ones; second N tile ragged."""
    c = _wgrad_case("b")
    assert c.B * (c.k1 - c.k0) == 15
    _run_wgrad_cl(c, nsplit, ldp)


def test_wgrad_cl_bias_cols(lib):
    """1c: M = 320 (8 + 2 chunks), N = 256, bias_cols: columns N .. N+3 of the slabs sum to the row sums of the M operand."""
    c = _wgrad_case("c")
    out = _run_wgrad_cl(c, 3, 260, bias_cols=1)
    check("wgrad_cl[c bias columns]", out.t[:, :, 256:260].double().sum((0, 2)), c.a_val.sum((0, 2)), GEMM_NORM, GEMM_MAX)


@pytest.mark.parametrize("nsplit,ldp", [(1, 260), (2, 260), (1, 257)])
def test_wgrad_cl_one_column_tile(lib, nsplit, ldp):
    """1d: M = 512, N = 257: the second N tile holds one column."""
    _run_wgrad_cl(_wgrad_case("d"), nsplit, ldp)


def test_wgrad_cl_argument_checks(lib):
    """1e: T2S_EINVAL without a launch (the output keeps its sentinel)."""
    c, cc = _wgrad_case("b"), _wgrad_case("c")
    out = Guarded(15, cc.M, 292)
    st = _lib.current_stream()

    def rc(c=c, n_a=None, n_b=None, ldp=292, nsplit=1, bias_cols=0, N=None):
        return lib.t2s_wgrad_cl(ptr(c.ta), c.ta.size(0) if n_a is None else n_a, ptr(c.tb), c.tb.size(0) if n_b is None else n_b,
                                ptr(out.t), c.B, c.M, c.N if N is None else N, ldp, c.k0, c.k1, nsplit, bias_cols, st)
    assert rc(nsplit=7) == EINVAL            # ceil(15 / 7) = 3 K-blocks per slab: slabs 5 and 6 would own none
    assert rc(nsplit=16) == EINVAL
    assert rc(n_a=16) == EINVAL and rc(n_b=8) == EINVAL and rc(n_b=15) == EINVAL     # table length is 8 x tiles
    assert rc(ldp=288) == EINVAL             # ldp < N
    # bias_cols on case c (N = 256, a whole tile: nothing else to object to)
    assert rc(cc, bias_cols=1, ldp=256) == EINVAL        # ldp < N + 4
    assert rc(cc, bias_cols=1, ldp=261) == EINVAL        # the lockstep kernel (ldp % 4 != 0) has no bias columns
    # ... and on a ragged last N tile, where columns N .. N+3 are columns the tile's own epilogue stores scratch to: refused, not raced
    assert rc(bias_cols=1, N=64, n_b=8, ldp=68) == EINVAL
    _sync()
    assert bool(out.untouched(out.t).all())


# -------------------------------------------------------------------------------------------------------------- 2. t2s_wn_backward

def _wn_backward(lib, label, nsplit, Prows, Pcols, row_off, col_off, tap_stride, col_bias, nb, O, Cin, Kt, with_g=True, db_accum=0,
                 seed=0):
    gen = torch.Generator().manual_seed(seed + 7 * O + Cin)
    P = torch.randn(nsplit, Prows, Pcols, generator=gen)
    v = torch.randn(O, Cin, Kt, generator=gen)
    g = torch.rand(O, generator=gen) + 0.5 if with_g else None
    db0 = torch.randn(O, generator=gen)
    P_d, v_d, g_d = dev(P), dev(v), None if g is None else dev(g)
    dv, dg, db = Guarded(O, Cin, Kt), Guarded(O), Guarded(O, fill=dev(db0))
    _lib.call("t2s_wn_backward", ptr(P_d), nsplit, Prows, Pcols, row_off, col_off, tap_stride, col_bias, nb, ptr(v_d), ptr(g_d), O, Cin,
              Kt, ptr(dv.t), ptr(dg.t) if with_g else None, ptr(db.t), db_accum, _lib.current_stream())
    _sync()
    Ps = P.double().sum(0)
    dW = torch.stack([Ps[row_off:row_off + O, col_off + tap * tap_stride:col_off + tap * tap_stride + Cin] for tap in range(Kt)], 2)
    v64 = v.double().requires_grad_(True)
    g64 = None if g is None else g.double().requires_grad_(True)
    loss = (U.wn_eff(v64, g64) * dW).sum()
    grads = torch.autograd.grad(loss, [v64] + ([] if g is None else [g64]))
    check(label + " dv", dv.t, grads[0], F32_NORM, F32_MAX)
    if with_g:
        check(label + " dg", dg.t, grads[1], F32_NORM, F32_MAX)
    else:
        assert bool(dg.untouched(dg.t).all())
    want_db = Ps[row_off:row_off + O, col_bias:col_bias + nb].sum(1) + (db0.double() if db_accum else 0.0)
    check(label + " db", db.t, want_db, F32_NORM, F32_MAX)
    for o in (dv, dg, db):
        o.assert_guards(label)


@pytest.mark.parametrize("nsplit", [1, 7])
def test_wn_backward_in_layer_call(lib, nsplit):
    """The slabs of the gate convolution's weight gradient at C = 64, n_cond = 96: in_layers (Kt = 3, tap_stride = C) and cond_layers
    (col_off = 3 C) read the same slabs; 16-byte path of the kernel."""
    C, S = 64, 96
    N2 = 3 * C + S + 1
    ld2 = -(-N2 // 4) * 4
    _wn_backward(lib, "wn_backward[in nsplit=%d]" % nsplit, nsplit, 2 * C, ld2, 0, 0, C, N2 - 1, 1, 2 * C, C, 3, seed=nsplit)
    _wn_backward(lib, "wn_backward[cond nsplit=%d]" % nsplit, nsplit, 2 * C, ld2, 0, 3 * C, 0, N2 - 1, 1, 2 * C, S, 1, seed=nsplit,
                 db_accum=1)


def test_wn_backward_rows_1024_four_bias_columns(lib):
    """O = 1024 rows of the res/skip weight gradient with the bias gradient in four partial-sum columns (n_bias_cols = 4)."""
    _wn_backward(lib, "wn_backward[O=1024 nb=4]", 7, 1024, 516, 0, 0, 0, 512, 4, 1024, 512, 1)


@pytest.mark.parametrize("col_off", [4, 5])      # 16-byte path / scalar path
def test_wn_backward_offsets_plain_weight(lib, col_off):
    """g = NULL (plain weight: dv = dW), non-zero row_off and col_off, O = 2."""
    Pcols = 40 if col_off == 4 else 39
    _wn_backward(lib, "wn_backward[g=NULL col_off=%d]" % col_off, 3, 8, Pcols, 3, col_off, 12, 36, 2, 2, 8, 3, with_g=False,
                 db_accum=1)
    _wn_backward(lib, "wn_backward[O=2 col_off=%d]" % col_off, 1, 8, Pcols, 5, col_off, 12, 37, 1, 2, 8, 3)


def test_wn_backward_lds_limit(lib):
    """Cin * Kt = 12288 floats is the 48 KB the kernel keeps of a row; one more is refused."""
    _wn_backward(lib, "wn_backward[12288]", 1, 2, 12292, 0, 0, 4096, 12288, 4, 2, 4096, 3)
    buf = torch.zeros(2 * 12292, device=DEV)
    assert lib.t2s_wn_backward(ptr(buf), 1, 1, 12292, 0, 0, 0, 12290, 1, ptr(buf), None, 1, 12289, 1, ptr(buf), None, None, 0,
                               _lib.current_stream()) == EINVAL
    _sync()


# ---------------------------------------------------------------------------------------------------------- 3. t2s_pack_transposed

@pytest.mark.parametrize("Cin,pair8,flip,with_scale", [(64, 0, 0, True), (64, 0, 1, True), (64, 1, 1, True), (64, 1, 0, False),
                                                       (40, 0, 1, True)])
def test_pack_transposed(lib, Cin, pair8, flip, with_scale):
    """A[c][koff + tap' O_pad + o] = scale[o] v[o][c][flip ? Kt-1-tap' : tap'] as (hi, lo) [k / 32][Mpad][32], koff != 0, O_pad > O;
    pair8: packed row 16 m + 4 q + e of every 32 = channel 8 q + 4 m + e."""
    O, Kt, O_pad, Mpad, koff = 40, 3, 64, 256, 32
    gen = torch.Generator().manual_seed(Cin + pair8)
    v = torch.randn(O, Cin, Kt, generator=gen)
    scale = torch.rand(O, generator=gen) + 0.5 if with_scale else None
    nk = (koff + Kt * O_pad) // 32 + 1                   # one K chunk behind the packed range
    A_hi, A_lo = _bf_full((nk, Mpad, 32), 7.0), _bf_full((nk, Mpad, 32), 7.0)
    v_d, s_d = dev(v), None if scale is None else dev(scale)
    _lib.call("t2s_pack_transposed", ptr(v_d), ptr(s_d), O, Cin, Kt, flip, O_pad, Mpad, koff, ptr(A_hi), ptr(A_lo), pair8,
              _lib.current_stream())
    _sync()
    rows = 64            # whole 32-row groups (the PERM_PAIR8 order is defined on them)
    got = U.packed_values(A_hi, A_lo, rows, nk * 32, pair8=bool(pair8))
    prod = v if scale is None else v * scale.view(-1, 1, 1)          # the f32 product the kernel splits
    want = torch.full((rows, nk * 32), 14.0, dtype=torch.float64)    # 7 + 7: never written
    for tp in range(Kt):
        k0 = koff + tp * O_pad
        want[:Cin, k0:k0 + O_pad] = 0.0                              # columns O .. O_pad-1 of every tap: zeros
        want[:Cin, k0:k0 + O] = prod[:, :, Kt - 1 - tp if flip else tp].t().double()
    err = (got - want).abs()
    assert bool((err <= 2.0 ** -15 * want.abs()).all()), float((err / want.abs().clamp_min(1e-30)).max())
    # rows that hold no channel: as they were
    tail = (A_hi.double() + A_lo.double())[:, rows:]
    assert bool((tail == 14.0).all())


# ------------------------------------------------------------------------------------------------------ 4. t2s_wg_bwd_gate_dgrad

def _pack_T(v, g, flip, Mpad, pair8, A=None, koff=0, nk=None):
    """t2s_weightnorm_scale + t2s_pack_transposed of one conv weight v [O][Cin][Kt]; returns (A_hi, A_lo) and what must stay alive."""
    O, Cin, Kt = v.shape
    st = _lib.current_stream()
    v_d, g_d = dev(v), None if g is None else dev(g)
    scale = torch.empty(O, device=DEV)
    _lib.call("t2s_weightnorm_scale", ptr(v_d), ptr(g_d), O, Cin * Kt, ptr(scale), st)
    if A is None:
        nk = Kt * O // 32 if nk is None else nk
        A = (torch.zeros(nk, Mpad, 32, dtype=torch.bfloat16, device=DEV), torch.zeros(nk, Mpad, 32, dtype=torch.bfloat16, device=DEV))
    _lib.call("t2s_pack_transposed", ptr(v_d), ptr(scale), O, Cin, Kt, flip, O, Mpad, koff, ptr(A[0]), ptr(A[1]), pair8, st)
    return A, (v_d, g_d, scale)


def _slice_ptrs(pair, first):
    """(hi, lo) pointers of chunk `first` of batch entry 0 of a plane pair [B, chunks, Lp, 32]."""
    off = 2 * first * pair[0].size(2) * 32
    return _lib.c_vp(pair[0].data_ptr() + off), _lib.c_vp(pair[1].data_ptr() + off)


def _widen(pair, chunks, first, fill):
    """The plane pair as chunks [first, first + own) of a wider set whose other chunks hold `fill`."""
    B, own, Lp, _ = pair[0].shape
    out = []
    for p in pair:
        w = _bf_full((B, chunks, Lp, 32), fill)
        w[:, first:first + own] = p
        out.append(w)
    return tuple(out)


@pytest.mark.parametrize("B,C,L,last,pair8,sliced", [
    (2, 64, 300, False, 0, False),       # 128-row lockstep
    (1, 160, 257, True, 0, True),        # 128-row lockstep, DX = NULL, acts / G / DP slices of wider plane sets
    (10, 64, 2500, False, 1, False),     # ping-pong: 1 x 10 x 10 = exactly 100 tiles
    (10, 64, 2500, False, 0, False),
    (4, 512, 3300, False, 1, False),     # ping-pong, two M tiles
])
def test_bwd_gate_dgrad(lib, B, C, L, last, pair8, sliced):
    """d_pre = gate'(acts, G) * (W_rs^T [d_x ; d_skip]) against float64 autograd through tanh * sigmoid and the res/skip 1x1 conv."""
    halo = 32
    Lp = _lib.plane_rows(L, halo)
    cc = C // 32
    pp = L > 2000
    assert lib.t2s_wg_bwd_pair8_ok(B, C, L) == (1 if pp else 0)
    if pair8:
        assert lib.t2s_wg_bwd_pair8_ok(B, C, L) == 1
    gen = torch.Generator().manual_seed(C + L + pair8)
    rows2 = C if last else 2 * C
    v = torch.randn(rows2, C, 1, generator=gen) / C ** 0.5
    g = torch.rand(rows2, generator=gen) + 0.5
    Mc = _lib.padded_rows(C)
    A, keep = _pack_T(v, g, 0, Mc, pair8)
    W = U.packed_values(A[0], A[1], C, rows2, pair8=bool(pair8)).t().contiguous()         # [rows2, C] as the planes hold it
    assert U.maxrel(W, U.wn_eff(v.double(), g.double())[:, :, 0]) < 2.0 ** -15
    DS, DSv = U.rand_planes(gen, B, C, L, halo)
    DX, DXv = (None, None) if last else U.rand_planes(gen, B, C, L, halo)
    # G = sigmoid of random values, acts = tanh * G: acts / G is well conditioned (|pre-activation| <= 4: the quotient of the two
    # rounded planes stays inside (-1, 1), where the expectation's atanh is defined)
    gate = torch.sigmoid(torch.randn(B, C, L, generator=gen).clamp_(-4.0, 4.0))
    acts = torch.tanh(torch.randn(B, C, L, generator=gen).clamp_(-4.0, 4.0)) * gate
    Gp, Ap = planes.to_planes(dev(gate), halo), planes.to_planes(dev(acts), halo)
    tg_bchunks, dp_bchunks, tfirst, dfirst = 0, 0, 0, 0
    DP = (torch.zeros(B, 2 * cc, Lp, 32, dtype=torch.bfloat16, device=DEV), torch.zeros(B, 2 * cc, Lp, 32, dtype=torch.bfloat16, device=DEV))
    if sliced:          # layer 1 of 3
        tg_bchunks, dp_bchunks, tfirst, dfirst = 3 * cc, 3 * 2 * cc, cc, 2 * cc
        Gp, Ap = _widen(Gp, tg_bchunks, tfirst, float("nan")), _widen(Ap, tg_bchunks, tfirst, float("nan"))
        DP = _widen(DP, dp_bchunks, dfirst, 3.0)
    zb = torch.zeros(Mc, device=DEV)
    a_h, a_l = _slice_ptrs(Ap, tfirst)
    g_h, g_l = _slice_ptrs(Gp, tfirst)
    d_h, d_l = _slice_ptrs(DP, dfirst)
    _lib.call("t2s_wg_bwd_gate_dgrad", ptr(A[0]), ptr(A[1]), ptr(zb), None if last else ptr(DX[0]), None if last else ptr(DX[1]),
              ptr(DS[0]), ptr(DS[1]), a_h, a_l, g_h, g_l, tg_bchunks, d_h, d_l, dp_bchunks, B, C, L, Lp, halo, Mc, pair8,
              _lib.current_stream())
    _sync()
    Gv, Av = U.plane_values(Gp, C, L, halo, tfirst), U.plane_values(Ap, C, L, halo, tfirst)
    a_t = torch.atanh(Av / Gv).requires_grad_(True)
    a_s = torch.logit(Gv).requires_grad_(True)
    rs = F.conv1d(torch.tanh(a_t) * torch.sigmoid(a_s), W.unsqueeze(-1))
    d_rs = DSv if last else torch.cat([DXv, DSv], 1)
    want = torch.cat(torch.autograd.grad((rs * d_rs).sum(), [a_t, a_s]), 1)
    label = "bwd_gate_dgrad[B=%d C=%d L=%d %s pair8=%d]" % (B, C, L, "ping-pong" if pp else "lockstep", pair8)
    check(label, U.plane_values(DP, 2 * C, L, halo, dfirst), want, GEMM_NORM, GEMM_MAX)
    own = tuple(p[:, dfirst:dfirst + 2 * cc] for p in DP)
    U.assert_halo_zero(own, L, halo, label)
    if sliced:
        for p in DP:
            assert bool((p[:, :dfirst] == 3.0).all()) and bool((p[:, dfirst + 2 * cc:] == 3.0).all()), "a neighbouring slice was written"


# -------------------------------------------------------------------------------------------------------- 5. t2s_conv_accumulate

@pytest.mark.parametrize("B,Cin,Cout,taps,dil,init,L,pair8,n_w", [
    (2, 128, 64, 3, 1, 1, 300, 0, 1),        # lockstep
    (1, 128, 64, 3, 128, 0, 257, 0, 1),      # accumulates into non-zero O; halo = 128
    (1, 128, 64, 5, 32, 1, 97, 0, 1),        # halo = 64
    (10, 128, 64, 3, 64, 0, 2500, 1, 1),     # ping-pong (100 tiles)
    (2, 1024, 640, 1, 1, 1, 4352, 1, 4),     # the conditioning GEMM: 3 x 17 x 2 = 102 tiles, four weights side by side along K, X a slice
])
def test_conv_accumulate(lib, B, Cin, Cout, taps, dil, init, L, pair8, n_w):
    """O (+)= W^T (*) X against float64 autograd of the dilated convolution's input gradient."""
    halo = max(32, -(-(taps // 2) * dil // 32) * 32)
    Lp = _lib.plane_rows(L, halo)
    pp = L > 2000
    assert lib.t2s_wg_bwd_pair8_ok(B, Cout, L) == (1 if pp else 0)
    if pair8:
        assert lib.t2s_wg_bwd_pair8_ok(B, Cout, L) == 1
    gen = torch.Generator().manual_seed(Cin + L + taps)
    Mpad = _lib.padded_rows(Cout)
    Ow = Cin // n_w                           # output channels of each of the n_w forward convolutions
    A, keep = None, []
    for i in range(n_w):
        v = torch.randn(Ow, Cout, taps, generator=gen) / (Cout * taps) ** 0.5
        g = torch.rand(Ow, generator=gen) + 0.5
        A, k = _pack_T(v, g, 1, Mpad, pair8, A=A, koff=i * Ow, nk=taps * Cin // 32)
        keep.append((k, v, g))
    WT = U.packed_values(A[0], A[1], Cout, taps * Cin, pair8=bool(pair8))         # [Cout, tap' Cin + o], taps mirrored
    W = WT.view(Cout, taps, Cin).flip(1).permute(2, 0, 1).contiguous()            # the forward weight [Cin, Cout, taps]
    for i, (_, v, g) in enumerate(keep):          # flip = 1, koff = i * Ow, O_pad = O: each packed weight is the forward weight
        assert U.maxrel(W[i * Ow:(i + 1) * Ow], U.wn_eff(v.double(), g.double())) < 2.0 ** -15
    X, Xv = U.rand_planes(gen, B, Cin, L, halo)
    x_bchunks, xfirst = 0, 0
    if n_w > 1:         # X = chunks [4, 4 + Cin / 32) of a wider plane set
        x_bchunks, xfirst = Cin // 32 + 8, 4
        X = _widen(X, x_bchunks, xfirst, float("nan"))
    O0 = torch.randn(B, Cout, L, generator=gen)
    O = planes.to_planes(dev(O0), halo)
    O0v = U.plane_values(O, Cout, L, halo)
    zb = torch.zeros(Mpad, device=DEV)
    x_h, x_l = _slice_ptrs(X, xfirst)
    _lib.call("t2s_conv_accumulate", ptr(A[0]), ptr(A[1]), ptr(zb), x_h, x_l, x_bchunks, ptr(O[0]), ptr(O[1]), B, Cin, Cout, taps, dil,
              init, L, Lp, halo, Mpad, pair8, _lib.current_stream())
    _sync()
    x = torch.zeros(B, Cout, L, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(x, W, dilation=dil, padding=dil * (taps // 2))
    want = torch.autograd.grad((y * Xv).sum(), x)[0]
    if not init:
        want = want + O0v
    label = "conv_accumulate[B=%d %d->%d taps=%d dil=%d init=%d L=%d %s pair8=%d]" % (
        B, Cin, Cout, taps, dil, init, L, "ping-pong" if pp else "lockstep", pair8)
    check(label, U.plane_values(O, Cout, L, halo), want, GEMM_NORM, GEMM_MAX)
    U.assert_halo_zero(O, L, halo, label)


# ------------------------------------------------------------------------------------------------------------ 6. t2s_wg_skip_sum

def test_skip_sum(lib):
    """skip = sum_i (W_skip,i acts_i + b_skip,i) over a flow's layers packed along K as the backward does (koff = i * Cpad; the last
    layer's res/skip convolution has skip rows only)."""
    B, C, L, nl, halo = 2, 64, 300, 3, 32
    xc = C // 32
    Lp = _lib.plane_rows(L, halo)
    Mskip = _lib.padded_rows(C)
    gen = torch.Generator().manual_seed(6)
    st = _lib.current_stream()
    A = (torch.zeros(nl * xc, Mskip, 32, dtype=torch.bfloat16, device=DEV), torch.zeros(nl * xc, Mskip, 32, dtype=torch.bfloat16, device=DEV))
    bias = torch.zeros(Mskip, device=DEV)
    acts, actv = U.rand_planes(gen, B, nl * C, L, halo)
    keep, want = [], 0.0
    for i in range(nl):
        rows2 = 2 * C if i < nl - 1 else C
        r0 = rows2 - C
        v = torch.randn(rows2, C, 1, generator=gen) / C ** 0.5
        g = torch.rand(rows2, generator=gen) + 0.5
        b = torch.randn(rows2, generator=gen) * 0.1
        v_d, g_d, b_d = dev(v), dev(g), dev(b)
        keep += [v_d, g_d, b_d]
        _lib.call("t2s_pack_conv_weight", _lib.c_vp(v_d.data_ptr() + 4 * r0 * C), _lib.c_vp(g_d.data_ptr() + 4 * r0), 0,
                  _lib.c_vp(b_d.data_ptr() + 4 * r0), C, C, 1, 0, 0, 0, Mskip, i * C, C, ptr(A[0]), ptr(A[1]), ptr(bias), 1 if i else 0, st)
        _sync()
        Wi = U.packed_values(A[0], A[1], C, nl * C)[:, i * C:(i + 1) * C]                       # what the planes hold
        assert U.maxrel(Wi, U.wn_eff(v.double(), g.double())[r0:, :, 0]) < 2.0 ** -15
        want = want + F.conv1d(actv[:, i * C:(i + 1) * C], Wi.unsqueeze(-1), b[r0:].double())
    skip = Guarded(B, xc, Lp, 32)
    _lib.call("t2s_wg_skip_sum", ptr(A[0]), ptr(A[1]), ptr(bias), ptr(acts[0]), ptr(acts[1]), nl * xc, nl * xc, ptr(skip.t), B, C, L, Lp,
              halo, Mskip, st)
    _sync()
    skip.assert_guards("skip_sum")
    check("skip_sum[B=2 C=64 nl=3 L=300]", planes.from_f32_planes(skip.t, C, L, halo), want, GEMM_NORM, GEMM_MAX)
    assert bool(skip.untouched(skip.t[:, :, :halo]).all()) and bool(skip.untouched(skip.t[:, :, halo + L:]).all())


# ------------------------------------------------------------- 7. the time-major fallback: plane_transpose, tm_ones_row, wgrad_gemm_flat

def _tm_expect(pair, first, n, shift, n_tch):
    """[B, n_tch, 32 n, 32] bf16 (hi, lo): tm[b][r / 32][c][r % 32] = plane[b][first + c / 32][r + shift][c % 32], zero outside."""
    out = []
    for p in pair:
        B, _, Lp, _ = p.shape
        src = torch.zeros(B, n, n_tch * 32 + 2 * abs(shift), 32, dtype=torch.bfloat16, device=DEV)
        src[:, :, abs(shift):abs(shift) + Lp] = p[:, first:first + n]
        src = src[:, :, abs(shift) + shift:abs(shift) + shift + n_tch * 32]                          # row r holds plane row r + shift
        out.append(src.reshape(B, n, n_tch, 32, 32).permute(0, 2, 1, 4, 3).reshape(B, n_tch, n * 32, 32))
    return out


@pytest.mark.parametrize("nsplit", [1, 2, 4, 15])
def test_time_major_fallback(lib, nsplit):
    """The weight-gradient path taken when n_mel_channels * n_group is no multiple of 32: plane_transpose (shifts 0 / -128 / +128,
    n_off != 0, a slice of a wider set), tm_ones_row and wgrad_gemm_flat at the operands of case 1b, against the same float64 result."""
    c = _wgrad_case("b")
    B, Lp = c.B, c.Lp
    n_tch = Lp // 32
    Mpad, Npad = 256, 512
    st = _lib.current_stream()
    tm = lambda rows: (_bf_full((B, n_tch, rows, 32), 5.0), _bf_full((B, n_tch, rows, 32), 5.0))
    TA, TX = tm(Mpad), tm(Npad)
    want_A = [t.clone() for t in TA]
    want_X = [t.clone() for t in TX]
    for T, want, pieces in ((TA, want_A, c.a_pieces), (TX, want_X, c.b_pieces[:-1])):
        n_off = 0
        for pair, first, n, shift in pieces:
            s_h, s_l = _slice_ptrs(pair, first)
            _lib.call("t2s_plane_transpose", s_h, s_l, B, pair[0].size(1), n, Lp, shift, ptr(T[0]), ptr(T[1]), T[0].size(2), n_off, st)
            for w, e in zip(want, _tm_expect(pair, first, n, shift, n_tch)):
                w[:, :, n_off:n_off + 32 * n] = e
            n_off += 32 * n
    _lib.call("t2s_tm_ones_row", ptr(TX[0]), ptr(TX[1]), B, Lp, c.halo, c.L, Npad, c.N - 1, st)
    _sync()
    ones = torch.zeros(Lp, dtype=torch.bfloat16, device=DEV)
    ones[c.halo:c.halo + c.L] = 1.0
    want_X[0][:, :, c.N - 1] = ones.view(n_tch, 32)
    want_X[1][:, :, c.N - 1] = 0.0
    for got, want in zip(TA + TX, want_A + want_X):          # bit for bit, the rows nobody owns (still 5.0) included
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the GEMM reads whole 256-row tiles: rows past M / N must not hold the filler
    for T, n in ((TA, c.M), (TX, c.N)):
        for p in T:
            p[:, :, n:] = 0.0
    out = Guarded(nsplit, c.M, c.N)
    zb = torch.zeros(Mpad, device=DEV)
    _lib.call("t2s_wgrad_gemm_flat", ptr(TA[0]), ptr(TA[1]), ptr(TX[0]), ptr(TX[1]), ptr(zb), ptr(out.t), B, c.M, c.N, Mpad, Npad, n_tch,
              c.k0, c.k1, nsplit, st)
    _sync()
    out.assert_guards("wgrad_gemm_flat")
    check("wgrad_gemm_flat[b nsplit=%d]" % nsplit, out.t.double().sum(0), c.want, GEMM_NORM, GEMM_MAX)
    if nsplit == 1:
        assert lib.t2s_wgrad_gemm_flat(ptr(TA[0]), ptr(TA[1]), ptr(TX[0]), ptr(TX[1]), ptr(zb), ptr(out.t), B, c.M, c.N, Mpad, Npad,
                                       n_tch, c.k0, c.k1, 7, st) == EINVAL


# ------------------------------------------------------------------------------------------------------------- 8. small f32 ops
SHAPES = [(1, 1), (3, 97), (2, 2000)]


@pytest.mark.parametrize("B,L", SHAPES)
def test_small_wgrad_and_rows_sum(lib, B, L):
    """out[r][j] = sum_{b,t} P[b][r][t] Q[b][q_off + j][t] with P from (hi, lo) planes or f32 planes, either output order, with and
    without the row sums, J = 1 and 16, q_off != 0; and t2s_rows_sum."""
    halo, chunks, R = 32, 2, 40
    Lp = _lib.plane_rows(L, halo)
    gen = torch.Generator().manual_seed(B + L)
    st = _lib.current_stream()
    Pp, Pv = U.rand_planes(gen, B, R, L, halo)
    Pf32 = torch.zeros(B, chunks, Lp, 32, device=DEV)
    Pf32[:, :, halo:halo + L] = (Pp[0].float() + Pp[1].float())[:, :, halo:halo + L]     # the same values as f32 planes
    scratch = torch.empty(lib.t2s_small_wgrad_scratch(B, chunks), device=DEV)
    for J in (1, 16):
        Jtot, q_off = J + 3, 2
        Q = torch.randn(B, Jtot, L, generator=gen)
        Q_d = dev(Q)
        want = torch.einsum("brt,bjt->rj", Pv, Q[:, q_off:q_off + J].double())
        want_rs = Pv.sum((0, 2))
        for f32 in (0, 1):
            for tr in (0, 1):
                for with_rs in (0, 1):
                    out, rs = Guarded(J, R) if tr else Guarded(R, J), Guarded(R)
                    _lib.call("t2s_small_wgrad", None if f32 else ptr(Pp[0]), None if f32 else ptr(Pp[1]), ptr(Pf32) if f32 else None,
                              ptr(Q_d), ptr(out.t), ptr(rs.t) if with_rs else None, ptr(scratch), B, chunks, Lp, halo, L, R, J, Jtot,
                              q_off, tr, st)
                    _sync()
                    label = "small_wgrad[B=%d L=%d J=%d f32=%d tr=%d rs=%d]" % (B, L, J, f32, tr, with_rs)
                    check(label, out.t.t() if tr else out.t, want, F32_NORM, F32_MAX)
                    if with_rs:
                        check(label + " rowsum", rs.t, want_rs, F32_NORM, F32_MAX)
                    else:
                        assert bool(rs.untouched(rs.t).all())
                    out.assert_guards(label)
                    rs.assert_guards(label)
        o = Guarded(J)
        _lib.call("t2s_rows_sum", ptr(Q_d), B, Jtot, q_off, J, L, ptr(o.t), st)
        _sync()
        check("rows_sum[B=%d L=%d J=%d]" % (B, L, J), o.t, Q[:, q_off:q_off + J].double().sum((0, 2)), F32_NORM, F32_MAX)
        o.assert_guards("rows_sum")


@pytest.mark.parametrize("B,L", SHAPES)
def test_start_dgrad(lib, B, L):
    """d_z[:, c_off : c_off + n_half] += W_start^T d_x, the other channels of d_z as they were."""
    halo, C, G = 32, 72, 8
    Lp = _lib.plane_rows(L, halo)
    gen = torch.Generator().manual_seed(3 * B + L)
    X, Xv = U.rand_planes(gen, B, C, L, halo)
    for c_off, nh in ((0, 4), (2, 3), (6, 1)):
        w = torch.randn(C, nh, generator=gen)
        dz0 = torch.randn(B, G, L, generator=gen)
        w_d = dev(w)
        dz = Guarded(B, G, L, fill=dev(dz0))
        _lib.call("t2s_wg_start_dgrad", ptr(X[0]), ptr(X[1]), ptr(w_d), ptr(dz.t), B, G, c_off, nh, C, L, Lp, halo, _lib.current_stream())
        _sync()
        x = torch.zeros(B, nh, L, dtype=torch.float64, requires_grad=True)
        add = torch.autograd.grad((F.conv1d(x, w.double().unsqueeze(-1)) * Xv).sum(), x)[0]
        want = dz0.double()
        want[:, c_off:c_off + nh] += add
        label = "start_dgrad[B=%d L=%d c_off=%d]" % (B, L, c_off)
        check(label, dz.t, want, F32_NORM, F32_MAX)
        keep = [j for j in range(G) if not c_off <= j < c_off + nh]
        assert torch.equal(dz.t[:, keep].cpu(), dz0[:, keep])
        dz.assert_guards(label)


@pytest.mark.parametrize("B,L", SHAPES)
def test_convinv_wgrad(lib, B, L):
    """dW = d_out . z_in^T + (*gscale_ptr * gmul) W^-T against float64 autograd of the 1x1 convolution and gmul * logdet(W)."""
    G = 8
    gen = torch.Generator().manual_seed(5 * B + L)
    for n in (4, 6, 8):
        c_off = G - n
        Winv = torch.linalg.qr(torch.randn(n, n, generator=gen))[0] @ torch.diag(torch.rand(n, generator=gen) + 0.5)
        if torch.det(Winv) < 0:
            Winv[:, 0] = -Winv[:, 0]
        dz, zin = torch.randn(B, G, L, generator=gen), torch.randn(B, G, L, generator=gen)
        gs = torch.randn(1, generator=gen)
        gmul = float(B * L)
        dz_d, zin_d, Winv_d, gs_d = dev(dz), dev(zin), dev(Winv), dev(gs)
        for with_gs in (0, 1):
            dW = Guarded(n, n)
            _lib.call("t2s_wg_convinv_wgrad", ptr(dz_d), ptr(zin_d), ptr(Winv_d), ptr(gs_d) if with_gs else None, gmul, B, G, c_off, n, L,
                      ptr(dW.t), _lib.current_stream())
            _sync()
            W = torch.linalg.inv(Winv.double()).requires_grad_(True)         # the matrix whose inverse the kernel was handed
            loss = (F.conv1d(zin[:, c_off:].double(), W.unsqueeze(-1)) * dz[:, c_off:].double()).sum()
            if with_gs:
                loss = loss + float(gs) * gmul * torch.logdet(W)
            label = "convinv_wgrad[B=%d L=%d n=%d gscale=%d]" % (B, L, n, with_gs)
            check(label, dW.t, torch.autograd.grad(loss, W)[0], F32_NORM, F32_MAX)
            dW.assert_guards(label)


@pytest.mark.parametrize("n_mel", [80, 10])
@pytest.mark.parametrize("B,L", SHAPES)
def test_upsample_wgrad(lib, B, L, n_mel):
    """ConvTranspose1d(n_mel, n_mel, 1024, stride 256) weight / bias gradient from the conditioning-plane gradient, against float64
    autograd through conv_transpose1d, the trim to the audio length and the squeeze."""
    halo, G, ksize, stride = 32, 8, 1024, 256
    T = L * G
    frames = T // stride + 1
    Lp = _lib.plane_rows(L, halo)
    gen = torch.Generator().manual_seed(n_mel + L)
    D, Dv = U.rand_planes(gen, B, n_mel * G, L, halo)
    mel = torch.randn(B, n_mel, frames, generator=gen)
    mel_d = dev(mel)
    dW, db = Guarded(n_mel, n_mel, ksize), Guarded(n_mel)
    _lib.call("t2s_wg_upsample_wgrad", ptr(D[0]), ptr(D[1]), ptr(mel_d), B, n_mel, frames, ksize, stride, G, L, Lp, halo, ptr(dW.t),
              ptr(db.t), _lib.current_stream())
    _sync()
    W = torch.zeros(n_mel, n_mel, ksize, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(n_mel, dtype=torch.float64, requires_grad=True)
    up = F.conv_transpose1d(mel.double(), W, b, stride=stride)[:, :, :T]
    spect = up.reshape(B, n_mel, L, G).permute(0, 1, 3, 2).reshape(B, n_mel * G, L)
    gW, gb = torch.autograd.grad((spect * Dv).sum(), [W, b])
    label = "upsample_wgrad[B=%d L=%d n_mel=%d]" % (B, L, n_mel)
    check(label + " dW", dW.t, gW, F32_NORM, F32_MAX)
    check(label + " db", db.t, gb, F32_NORM, F32_MAX)
    dW.assert_guards(label)
    db.assert_guards(label)


@pytest.mark.parametrize("mode", ["null", "scalar", "full"])
@pytest.mark.parametrize("B,L", SHAPES)
def test_affine_backward(lib, B, L, mode):
    """Affine coupling backward + un-apply against float64 autograd of a1' = exp(log_s) a1 + b; the un-applied z is the forward's
    input; g_log_s NULL, one broadcast float, or element-wise."""
    G, c_off, nh = 8, 2, 3
    gen = torch.Generator().manual_seed(11 * B + L)
    z_in = torch.randn(B, G, L, generator=gen)
    wn_out = torch.randn(B, 2 * nh, L, generator=gen) * 0.5             # (b ; log_s)
    dz0 = torch.randn(B, G, L, generator=gen)
    g_ls = None if mode == "null" else torch.randn(1 if mode == "scalar" else B * nh * L, generator=gen)
    lo, hi = c_off + nh, c_off + 2 * nh
    a1 = z_in[:, lo:hi].double().requires_grad_(True)
    bb = wn_out[:, :nh].double().requires_grad_(True)
    ls = wn_out[:, nh:].double().requires_grad_(True)
    a1p = torch.exp(ls) * a1 + bb
    z_out = z_in.clone()
    z_out[:, lo:hi] = a1p.detach().float()                              # what the forward left in z
    loss = (a1p * dz0[:, lo:hi].double()).sum()
    if g_ls is not None:
        loss = loss + (ls * (g_ls.double() if mode == "scalar" else g_ls.double().view(B, nh, L))).sum()
    d_a1, d_b, d_ls = torch.autograd.grad(loss, [a1, bb, ls])
    z, dz, d_out = Guarded(B, G, L, fill=dev(z_out)), Guarded(B, G, L, fill=dev(dz0)), Guarded(B, 2 * nh, L)
    wn_d, g_d = dev(wn_out), None if g_ls is None else dev(g_ls)
    _lib.call("t2s_wg_affine_backward", ptr(z.t), ptr(dz.t), ptr(wn_d), ptr(g_d), 1 if mode == "scalar" else 0, ptr(d_out.t), B, G, c_off,
              nh, L, _lib.current_stream())
    _sync()
    label = "affine_backward[B=%d L=%d g_log_s=%s]" % (B, L, mode)
    check(label + " d_out", d_out.t, torch.cat([d_b, d_ls], 1), F32_NORM, F32_MAX)
    check(label + " dz", dz.t[:, lo:hi], d_a1, F32_NORM, F32_MAX)
    check(label + " z", z.t[:, lo:hi], z_in[:, lo:hi], F32_NORM, F32_MAX)
    keep = [j for j in range(G) if not lo <= j < hi]
    assert torch.equal(z.t[:, keep].cpu(), z_in[:, keep]) and torch.equal(dz.t[:, keep].cpu(), dz0[:, keep])
    for o in (z, dz, d_out):
        o.assert_guards(label)
