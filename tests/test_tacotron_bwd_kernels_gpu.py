"""The Tacotron backward kernels one by one through the C ABI (run with -m gpu on an MI355X), each against a plain float64
restatement of the same operation on the CPU (torch in float64, autograd where that states the math best; never another kernel
of this library), at the shapes where the launchers change kernels and at the kernels' tile edges.  Every compared output goes
through wg_bwd_util.check: norm-relative error AND the maximum error relative to the expectation's largest element (one wrong
row, chunk edge or halo position moves no norm), after a `PARITY ...` line with both figures.  f32 outputs live in Guarded
buffers (NaN sentinel inside, guard words either side); accumulated outputs start from known non-zero values of the size of what
is added to them, so the `+=` is seen; the start is taken off again in float64 before the comparison, so the bars are relative to
the gradient alone and the start leaves only its own rounding in the kernel's f32 `+=`.

Which kernel a case launches (dispatch: t2s_launch_att_bwd_front / _conv, t2s_launch_lstm_cell_bwd, t2s_launch_att_energy,
run_attention, t2s_taco_bptt_steps):
  att_bwd_dw_kernel               every three-launch case of section 1 (f32x4 loads at enc_dim 68: the attention_dim 64 / 72 rows)
  att_bwd_energy_mfma_kernel      section 1, attention_dim 128 / 32 filters / kernel 31 and 5
  att_bwd_energy_kernel (VALU)    section 1, attention_dim 64, 72, 96, and 128 with 8 filters
  att_bwd_conv_mfma_kernel        section 1, 32 filters and kernel <= 31 (attention_dim 128 and 96)
  att_bwd_conv_kernel (VALU)      section 1, 16 filters / kernel 33, kernel 63, 8 filters / kernel 7
  att_bwd_fused_kernel            section 1 one-launch cases (no folded cell); section 2 "fold" (folded cell) and "q_kernel"
  lstm_cell_bwd_kernel            section 4 (no wq); section 2 attention_dim 64 (q_dim % 16 == 0) and 72 (tail loop) with wq
  lstm_cell_bwd_q_kernel          section 2 "q_kernel" and "three" at attention_dim 128
  att_energy_kernel               section 3 with w_loc_denseT = NULL, more than 8 items, or T = 513
  att_fused_kernel                section 3, attention_dim 64 / 72 / 96 with w_loc_denseT (its matrix-core twin
                                  att_fused_mfma_kernel: the reference-shape case)

Bars: these kernels are f32 end to end (VALU, or the exact-f32 matrix-core instruction), so the project's f32 bars apply -
wg_bwd_util.F32_NORM = 1e-5, F32_MAX = 1e-4 - also to plane outputs read back as hi + lo.  The softmax backward and the
location-convolution gradients cancel, so for every section 1 / 2 output the same float64 restatement is also evaluated in float32
on the CPU and its error against float64 printed (`FLOOR ...`): what any f32 evaluation costs before the kernels' own summation
order.  No output needed a bar derived from that floor: all of them meet 1e-5 / 1e-4 (profiles/tacotron_bwd_kernel_parity.md has
the measured figures, the floors, and what four hand-made kernel changes do to these tests and to the whole-model one)."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

import wg_bwd_util as U
from text2speech_amd import _lib
from taco_ref_util import LEN as _LEN, att_step as _att_step, lstm as _lstm
from text2speech_amd.tacotron.autograd import _AttBwd, _Bptt, _BnBwd, _p
from wg_bwd_util import DEV, F32_MAX, F32_NORM, Guarded, check, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
ptr = _lib.ptr


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _sync():
    torch.cuda.synchronize()


class _Checks:
    """Every check of a case runs (and prints its figures); done() then fails with all that missed."""

    def __init__(self):
        self.failed = []

    def __call__(self, label, got, want):
        try:
            check(label, got, want, F32_NORM, F32_MAX)
        except AssertionError as e:
            self.failed.append(str(e))

    def ok(self, cond, msg):
        if not bool(cond):
            self.failed.append(msg)

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def _start_like(gen, want, parts=1):
    """f32 CPU start value of an accumulated output [parts, *want.shape]: non-zero everywhere, of the size of the largest element
    that is added to it (1 where nothing is), so its rounding in the kernel's `+=` stays far below the bars."""
    s = float(want.abs().max()) or 1.0
    return ((0.5 + torch.rand(parts, *want.shape, generator=gen)) * (s / parts)).float()


def _added(o, name, t, shape=None):
    """What a call added to an accumulated output: read back minus its start value, in float64 (shape given: one slot per row of
    `t`, the slots' differences summed).  The start's own rounding in the kernel's f32 `+=` is the only trace it leaves."""
    d = t.double().cpu() - o.start[name].double().reshape(t.shape)
    return d if shape is None else d.sum(0).view(*shape)


def _print_floors(ref64, ref32, tag):
    for k, v in ref64.items():
        print("FLOOR  %-60s norm-rel %.3e  max-rel %.3e" % ("%s %s" % (tag, k), U.rel(ref32[k], v), U.maxrel(ref32[k], v)))


# ================================================================================ 1. t2s_taco_att_bwd against float64 autograd
_ATT = {}


def _att_case(AD, F_, KS, T, B, E, step0=False, only1=False):
    """Inputs (f32 values on the CPU), the float64 forward / autograd gradients and the float32 floors of one attention step."""
    key = (AD, F_, KS, T, B, E, step0, only1)
    if key in _ATT:
        return _ATT[key]
    g = torch.Generator().manual_seed(1000 + AD * 7 + F_ * 5 + KS * 3 + T * 11 + B + E + 2 * step0 + only1)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x = types.SimpleNamespace(AD=AD, F=F_, KS=KS, T=T, B=B, E=E, step0=step0, only1=only1, gen=g)
    x.lengths = torch.tensor(_LEN[B](T), dtype=torch.int32)
    x.q, x.pmem, x.memory = r(B, AD, sc=0.5), r(B, T, AD, sc=0.5), r(B, T, E)
    x.w_prev, x.wc_prev = torch.softmax(r(B, T), 1), torch.rand(B, T, generator=g) * 2
    if step0:
        x.w_prev, x.wc_prev = torch.zeros(B, T), torch.zeros(B, T)
    x.K, x.D, x.v = r(F_, 2, KS, sc=0.2), r(AD, F_, sc=0.2), r(AD, sc=0.3)
    x.dctx = [r(B, E, sc=0.1), None if only1 else r(B, E, sc=0.1), None if only1 else r(B, E, sc=0.1)]
    x.cw, x.cwc = r(B, T, sc=0.05), r(B, T, sc=0.05)          # dL/dw, dL/dwc of this step coming from step t + 1

    def ref(dtype):
        leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
        q, pmem, memory, wp, wcp, K, D, v = map(leaf, (x.q, x.pmem, x.memory, x.w_prev, x.wc_prev, x.K, x.D, x.v))
        w, ctx, wc = _att_step(q, pmem, memory, wp, wcp, K, D, v, x.lengths)
        dctx = sum(d.to(dtype) for d in x.dctx if d is not None)
        L = (dctx * ctx).sum() + (x.cw.to(dtype) * w).sum() + (x.cwc.to(dtype) * wc).sum()
        gr = torch.autograd.grad(L, [q, pmem, memory, K, D, v, wp, wcp])
        names = ("d_q", "d_pmem", "d_memory", "dK", "dD", "dv", "dw_carry", "dwc_carry")
        out = dict(zip(names, gr))
        out["dctx"] = dctx
        return w.detach(), ctx.detach(), out

    x.w, x.ctx, x.ref = ref(torch.float64)
    _print_floors(x.ref, ref(torch.float32)[2], "att_bwd AD=%d F=%d KS=%d T=%d B=%d E=%d" % (AD, F_, KS, T, B, E))
    # device operands, with row strides that differ from the row lengths where the struct has a stride
    x.d = dd = types.SimpleNamespace()
    wide = lambda t, extra: dev(torch.cat([t, torch.full((t.size(0), extra), 77.0)], 1))
    dd.dctx = [None if t is None else wide(t, e) for t, e in zip(x.dctx, (8, 0, 4))]
    dd.w_cur, dd.ctx = wide(x.w.float(), 5), wide(x.ctx.float(), 12)
    dd.w_prev, dd.wc_prev = (None, None) if step0 else (wide(x.w_prev, 5), dev(x.wc_prev))
    dd.q, dd.pmem, dd.memory, dd.lengths = dev(x.q), dev(x.pmem), dev(x.memory), dev(x.lengths)
    dd.K, dd.D, dd.v = dev(x.K), dev(x.D), dev(x.v)
    _ATT[key] = x
    return x


def _att_struct(x):
    a, dd, E, T = _AttBwd(), x.d, x.E, x.T
    for i, (t, e) in enumerate(zip(dd.dctx, (8, 0, 4))):
        setattr(a, "dctx%d" % (i + 1), _p(t))
        setattr(a, "sc%d" % (i + 1), E + e)
    a.w_cur, a.s_wcur = _p(dd.w_cur), T + 5
    a.w_prev, a.wc_prev, a.s_wprev, a.s_wcprev = _p(dd.w_prev), _p(dd.wc_prev), T + 5, T
    a.q, a.pmem, a.memory, a.lengths = _p(dd.q), _p(dd.pmem), _p(dd.memory), _p(dd.lengths)
    a.w_loc_conv, a.w_loc_dense, a.w_v = _p(dd.K), _p(dd.D), _p(dd.v)
    a.B, a.T, a.att_dim, a.enc_dim, a.loc_f, a.loc_ks = x.B, T, x.AD, E, x.F, x.KS
    return a


def _att_outputs(x, a, with_dmem):
    """Guarded outputs and scratch of one call; accumulated ones start from known values (o.start: f32 CPU copies)."""
    B, T, AD, E, F_, KS, g, ref = x.B, x.T, x.AD, x.E, x.F, x.KS, x.gen, x.ref
    nch = (T + 31) // 32
    o = types.SimpleNamespace(nch=nch, start={})

    def acc(name, want, parts=1, shape=None):
        s = _start_like(g, want, parts)
        o.start[name] = s
        return Guarded(*(shape or s.shape[1:]), fill=dev(s.reshape(shape or s.shape[1:])))

    o.d_q = Guarded(B, AD)
    o.d_pmem = acc("d_pmem", ref["d_pmem"])
    o.d_memory = acc("d_memory", ref["d_memory"]) if with_dmem else None
    # one slot per (batch element, 32-position chunk); dD slots hold the transposed gradient [loc_f][att_dim]
    o.dD = acc("dD", ref["dD"].t().contiguous(), B * nch, (B * nch, F_ * AD))
    o.dK = acc("dK", ref["dK"], B * nch, (B * nch, F_ * 2 * KS))
    o.dv = acc("dv", ref["dv"], B * nch, (B * nch, AD))
    o.dw_buf, o.df_buf, o.dq_part, o.dctx_out = Guarded(B, T), Guarded(B, T, 32), Guarded(B, nch, AD), Guarded(B, E)
    a.d_q, a.d_pmem, a.d_memory = _p(o.d_q.t), _p(o.d_pmem.t), None if o.d_memory is None else _p(o.d_memory.t)
    a.dD_part, a.dK_part, a.dv_part = _p(o.dD.t), _p(o.dK.t), _p(o.dv.t)
    a.dw_buf, a.df_buf, a.dq_part = _p(o.dw_buf.t), _p(o.df_buf.t), _p(o.dq_part.t)
    a.dctx_out = None if with_dmem else _p(o.dctx_out.t)
    return o


def _att_compare(x, o, tag, d_q, cw, cwc):
    ref, B, T, AD, F_, KS = x.ref, x.B, x.T, x.AD, x.F, x.KS
    ck = _Checks()
    ck(tag + " d_q", d_q, ref["d_q"])
    ck(tag + " d_pmem", _added(o, "d_pmem", o.d_pmem.t), ref["d_pmem"])
    for b in range(B):      # positions from `length` on keep their start value, bit for bit
        ln = int(x.lengths[b])
        ck.ok(torch.equal(o.d_pmem.t[b, ln:].cpu(), o.start["d_pmem"][0, b, ln:]), tag + ": d_pmem written past the length")
    if o.d_memory is not None:
        ck(tag + " d_memory", _added(o, "d_memory", o.d_memory.t), ref["d_memory"])
    else:
        ck(tag + " dctx_out", o.dctx_out.t, ref["dctx"])
    ck(tag + " dD (slot sum)", _added(o, "dD", o.dD.t, (F_, AD)), ref["dD"].t())
    ck(tag + " dK (slot sum)", _added(o, "dK", o.dK.t, (F_, 2, KS)), ref["dK"])
    ck(tag + " dv (slot sum)", _added(o, "dv", o.dv.t, (AD,)), ref["dv"])
    ck(tag + " dw_carry", cw, ref["dw_carry"])
    ck(tag + " dwc_carry", cwc, ref["dwc_carry"])
    for name in ("d_q", "d_pmem", "d_memory", "dD", "dK", "dv", "dw_buf", "df_buf", "dq_part", "dctx_out"):
        if getattr(o, name) is not None:
            getattr(o, name).assert_guards(tag + " " + name)
    ck.done()


def _three_launch(AD, F_, KS, T, B, E, step0=False, only1=False):
    """Both forms of d_memory: accumulated in the call (onto a known start), and deferred (dctx_out, d_memory NULL)."""
    x = _att_case(AD, F_, KS, T, B, E, step0, only1)
    for with_dmem in (True, False):
        a = _att_struct(x)
        o = _att_outputs(x, a, with_dmem)
        cw, cwc = Guarded(B, T, fill=dev(x.cw)), Guarded(B, T, fill=dev(x.cwc))         # in / out
        a.dw_carry, a.dwc_carry = _p(cw.t), _p(cwc.t)
        _lib.call("t2s_taco_att_bwd", ctypes.byref(a), _lib.current_stream())
        _sync()
        tag = "att_bwd3[AD=%d F=%d KS=%d T=%d B=%d E=%d%s%s %s]" % (AD, F_, KS, T, B, E, " step0" if step0 else "",
                                                                    " dctx1" if only1 else "", "d_memory" if with_dmem else "dctx_out")
        cw.assert_guards(tag + " dw_carry")
        cwc.assert_guards(tag + " dwc_carry")
        _att_compare(x, o, tag, o.d_q.t, cw.t, cwc.t)


@pytest.mark.parametrize("T", [1, 31, 32, 33, 70])
def test_att_bwd_three_launch_matrix_core(lib, T):
    """att_bwd_dw_kernel + att_bwd_energy_mfma_kernel + att_bwd_conv_mfma_kernel; ragged lengths, one of them 1."""
    _three_launch(128, 32, 31, T, 3, 512, step0=(T == 70))


def test_att_bwd_three_launch_matrix_core_kernel5(lib):
    _three_launch(128, 32, 5, 96, 2, 512, only1=True)


@pytest.mark.parametrize("T", [33, 70])
def test_att_bwd_three_launch_valu_dim64(lib, T):
    """att_bwd_energy_kernel + att_bwd_conv_kernel at 64 attention channels, 16 filters, kernel 33; enc_dim 68: a multiple of 4,
    not of 256 (att_bwd_dw_kernel's 16-byte loads)."""
    _three_launch(64, 16, 33, T, 3, 68, step0=(T == 33))


def test_att_bwd_three_launch_valu_widest_kernel(lib):
    """attention_dim 72 (no multiple of 64), kernel 63: the widest the C ABI accepts (s_cat / s_df hold 32 + 62 positions)."""
    _three_launch(72, 32, 63, 40, 2, 68, only1=True)


def test_att_bwd_three_launch_valu_energies_matrix_core_conv(lib):
    _three_launch(96, 32, 31, 65, 2, 512)


def test_att_bwd_three_launch_few_filters(lib):
    """attention_dim 128 but 8 filters: both matrix-core gates fail on the filter count alone."""
    _three_launch(128, 8, 7, 64, 1, 512)


@pytest.mark.parametrize("KS", [31, 5])
@pytest.mark.parametrize("T", [33, 70, 256])
def test_att_bwd_one_launch(lib, T, KS):
    """att_bwd_fused_kernel without the folded cell: sdot from the saved context, carries read from and scattered into three
    slots per position ([0] own chunk, [1] from the chunk to the right, [2] from the left) - totals split over the slots that exist
    for a position as tests/test_att_bwd_fused_gpu.py does, garbage in those that do not."""
    B, AD, F_, E = 3, 128, 32, 512
    x = _att_case(AD, F_, KS, T, B, E)
    a = _att_struct(x)
    o = _att_outputs(x, a, False)
    g, pad = x.gen, KS // 2
    t = torch.arange(T)
    l, t0 = t % 32, t - t % 32
    has1, has2 = (l >= 32 - pad) & (t0 + 32 < T), (l < pad) & (t0 > 0)
    ins = []
    for tot in (x.cw, x.cwc):
        s1, s2 = torch.randn(B, T, generator=g) * 0.05, torch.randn(B, T, generator=g) * 0.05
        s0 = tot - torch.where(has1, s1, torch.zeros(())) - torch.where(has2, s2, torch.zeros(()))
        ins.append(dev(torch.stack([s0, torch.where(has1, s1, torch.full((), 123.0)), torch.where(has2, s2, torch.full((), -77.0))])))
    # (s0 + s1 + s2 re-read in float64 is the total it was made from up to one f32 rounding, far below the bars)
    tot64 = [i[0].double().cpu() + torch.where(has1, i[1].double().cpu(), torch.zeros((), dtype=torch.float64)) +
             torch.where(has2, i[2].double().cpu(), torch.zeros((), dtype=torch.float64)) for i in ins]
    for tt, src in zip(tot64, (x.cw, x.cwc)):
        assert float((tt - src.double()).abs().max()) < 1e-7
    outs = [Guarded(3, B, T), Guarded(3, B, T)]
    a.dw_carry, a.dwc_carry = _p(ins[0]), _p(ins[1])
    a.ctx, a.s_ctx, a.dw_carry_out, a.dwc_carry_out = _p(x.d.ctx), E + 12, _p(outs[0].t), _p(outs[1].t)
    _lib.call("t2s_taco_att_bwd", ctypes.byref(a), _lib.current_stream())
    _sync()
    tag = "att_bwd1[KS=%d T=%d B=%d]" % (KS, T, B)
    tot = []
    for og in outs:
        og.assert_guards(tag + " carries")
        v = og.t.double().cpu()
        assert bool(torch.isfinite(v[0]).all()), "an own-chunk carry slot was not written"
        assert bool(torch.isfinite(v[1][:, has1]).all()) and bool(torch.isfinite(v[2][:, has2]).all()), \
            "a carry slot that exists for a position was not written"
        tot.append(v[0] + torch.where(has1, v[1], torch.zeros_like(v[1])) + torch.where(has2, v[2], torch.zeros_like(v[2])))
    _att_compare(x, o, tag, o.dq_part.t.double().cpu().sum(1), tot[0], tot[1])


# ======================================================================== 2. t2s_taco_bptt_steps on a small float64 decoder loop
_BPTT = {}
_BP = dict(P=32, E=64, A=128, D=128, T_in=40, T_out=18, T_cap=20, p_att=0.1, p_dec=0.1)


def _bptt_case(ad, F_, KS, B, masks):
    """The loop of tacotron.py:355-393 with random weights at small sizes (18 steps: one past BPTT_CHUNK = 16), what t2s_taco_bptt
    documents as saved, and autograd of <d_hc, [h_dec | ctx]> for the references."""
    key = (ad, F_, KS, B, masks)
    if key in _BPTT:
        return _BPTT[key]
    g = torch.Generator().manual_seed(7000 + ad + F_ + KS + B)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    P, E, A, D, T_in, T_out = (_BP[k] for k in ("P", "E", "A", "D", "T_in", "T_out"))
    c = types.SimpleNamespace(ad=ad, F=F_, KS=KS, B=B, masks=masks, gen=g)
    c.lengths = torch.tensor(_LEN[B](T_in), dtype=torch.int32)
    c.Wa, c.ba = r(4 * A, P + E + A, sc=0.08), r(4 * A, sc=0.1)           # attention_rnn: [W_ih | W_hh] over [prenet | ctx | h]
    c.Wd, c.bd = r(4 * D, A + E + D, sc=0.08), r(4 * D, sc=0.1)           # decoder_rnn:   [W_ih | W_hh] over [h_att | ctx | h]
    c.Wq, c.K, c.Dl, c.v = r(ad, A, sc=0.1), r(F_, 2, KS, sc=0.2), r(ad, F_, sc=0.2), r(ad, sc=0.3)
    c.pmem, c.memory, c.pre = r(B, T_in, ad, sc=0.5), r(B, T_in, E), r(T_out, B, P)
    c.d_hc = r(T_out, B, D + E, sc=0.1)
    c.m_att = (torch.rand(T_out, B, A, generator=g) >= _BP["p_att"]).to(torch.uint8)
    c.m_dec = (torch.rand(T_out, B, D, generator=g) >= _BP["p_dec"]).to(torch.uint8)
    c.s_att, c.s_dec = 1.0 / (1.0 - _BP["p_att"]), 1.0 / (1.0 - _BP["p_dec"])

    def run(dtype):
        cv = lambda t: t.to(dtype)
        leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
        Wa, ba, Wd, bd, Wq = map(cv, (c.Wa, c.ba, c.Wd, c.bd, c.Wq))
        pmem, memory, K, Dl, v = map(leaf, (c.pmem, c.memory, c.K, c.Dl, c.v))
        z = lambda *s: torch.zeros(*s, dtype=dtype)
        h_a, c_a, h_d, c_d, ctx, w, wc = z(B, A), z(B, A), z(B, D), z(B, D), z(B, E), z(B, T_in), z(B, T_in)
        sv = {k: [] for k in ("za", "ga", "ca", "zd", "gd", "cd", "q", "w", "wc", "ctx", "xa", "xd", "hc")}
        L = 0
        for t in range(T_out):
            xa = torch.cat([cv(c.pre[t]), ctx, h_a], 1)
            if not xa.requires_grad:            # (step 0: nothing upstream of the first cell's input)
                xa.requires_grad_(True)
            za, ga, c_a, h = _lstm(xa, Wa, ba, c_a)
            h_a = h * cv(c.m_att[t]) * c.s_att if masks else h
            q = h_a @ Wq.t()
            w, ctx, wc = _att_step(q, pmem, memory, w, wc, K, Dl, v, c.lengths)
            xd = torch.cat([h_a, ctx, h_d], 1)
            zd, gd, c_d, h = _lstm(xd, Wd, bd, c_d)
            h_d = h * cv(c.m_dec[t]) * c.s_dec if masks else h
            hc = torch.cat([h_d, ctx], 1)
            L = L + (cv(c.d_hc[t]) * hc).sum()
            for k, val in zip(sv, (za, ga, c_a, zd, gd, c_d, q, w, wc, ctx, xa, xd, hc)):
                sv[k].append(val)
        n = T_out
        gr = torch.autograd.grad(L, sv["za"] + sv["zd"] + sv["q"] + sv["ctx"] + sv["xa"] + sv["xd"] + [pmem, memory, K, Dl, v])
        st = lambda i: torch.stack(gr[i * n:(i + 1) * n])
        ref = dict(dg_a=st(0), dg_d=st(1), dq_all=st(2), dctx_all=st(3), out_a=st(4), out_d=st(5), d_pmem=gr[6 * n],
                   d_memory=gr[6 * n + 1], dK=gr[6 * n + 2], dD=gr[6 * n + 3], dv=gr[6 * n + 4])
        return {k: torch.stack(val).detach() for k, val in sv.items()}, ref

    c.sv, c.ref = run(torch.float64)
    _print_floors(c.ref, run(torch.float32)[1], "bptt ad=%d F=%d KS=%d B=%d%s" % (ad, F_, KS, B, "" if masks else " no masks"))
    sv, f = c.sv, lambda t: dev(t.float())
    c.d = dd = types.SimpleNamespace()
    dd.W_dT, dd.W_aT, dd.Wq, dd.K, dd.Dl, dd.v = dev(c.Wd.t()), dev(c.Wa.t()), dev(c.Wq), dev(c.K), dev(c.Dl), dev(c.v)
    dd.dec_gates, dd.dec_c, dd.att_gates, dd.att_c = f(sv["gd"]), f(sv["cd"]), f(sv["ga"]), f(sv["ca"])
    dd.q_all, dd.wcum_all, dd.hc_all = f(sv["q"]), f(sv["wc"]), f(sv["hc"])
    align = torch.full((B, _BP["T_cap"], T_in), 0.125)                    # rows past T_out are never read
    align[:, :T_out] = sv["w"].float().permute(1, 0, 2)
    dd.align, dd.pmem, dd.memory, dd.lengths = dev(align), dev(c.pmem), dev(c.memory), dev(c.lengths)
    dd.m_att, dd.m_dec, dd.d_hc = dev(c.m_att), dev(c.m_dec), dev(c.d_hc)
    _BPTT[key] = c
    return c


def _bptt_struct(c, form):
    """The t2s_taco_bptt of one call with its Guarded outputs `o` and the exchange buffer.  form: "fold" (ctx_all, second carry
    pair, att_xbuf), "q_kernel" (the same without att_xbuf), "three" (none of them and no dctx_all: three launches, carries in
    place, d_memory accumulated in the loop)."""
    P, E, A, D, T_in, T_out, T_cap = (_BP[k] for k in ("P", "E", "A", "D", "T_in", "T_out", "T_cap"))
    B, ad, F_, KS, dd, ref, g = c.B, c.ad, c.F, c.KS, c.d, c.ref, c.gen
    nch = (T_in + 31) // 32
    KD, KA = A + E + D, P + E + A
    deferred = form != "three"
    o = types.SimpleNamespace(start={})

    def acc(name, want, parts=1, shape=None):
        s = _start_like(g, want, parts)
        o.start[name] = s
        return Guarded(*(shape or s.shape[1:]), fill=dev(s.reshape(shape or s.shape[1:])))

    o.out_d, o.out_a = Guarded(T_out, B, KD), Guarded(T_out, B, KA)
    o.dg_d, o.dg_a, o.dq_all = Guarded(T_out, B, 4 * D), Guarded(T_out, B, 4 * A), Guarded(T_out, B, ad)
    o.dctx_all = Guarded(T_out, B, E)
    zg = lambda *s: Guarded(*s, fill=torch.zeros(*s, device=DEV))
    o.dc_d, o.dc_a = zg(B, D), zg(B, A)
    o.dw_c, o.dwc_c, o.dw_c2, o.dwc_c2 = zg(3, B, T_in), zg(3, B, T_in), zg(3, B, T_in), zg(3, B, T_in)
    o.d_pmem = acc("d_pmem", ref["d_pmem"])
    o.d_memory = Guarded(B, T_in, E) if deferred else acc("d_memory", ref["d_memory"])
    o.dD = acc("dD", ref["dD"].t().contiguous(), B * nch, (B * nch, F_ * ad))
    o.dK = acc("dK", ref["dK"], B * nch, (B * nch, F_ * 2 * KS))
    o.dv = acc("dv", ref["dv"], B * nch, (B * nch, ad))
    o.dw_buf, o.df_buf, o.dq_part = Guarded(B, T_in), Guarded(B, T_in, 32), Guarded(B, nch, ad)
    xbuf = torch.zeros(2 * (B * nch * 128 + 3), device=DEV)
    bp = _Bptt(B=B, T_in=T_in, T_out=T_out, T_cap=T_cap, prenet_dim=P, enc_dim=E, att_rnn_dim=A, dec_rnn_dim=D, att_dim=ad,
               loc_filters=F_, loc_kernel=KS, W_dT=_p(dd.W_dT), W_aT=_p(dd.W_aT), w_query=_p(dd.Wq), w_loc_conv=_p(dd.K),
               w_loc_dense=_p(dd.Dl), w_v=_p(dd.v), dec_gates_all=_p(dd.dec_gates), dec_c_all=_p(dd.dec_c),
               att_gates_all=_p(dd.att_gates), att_c_all=_p(dd.att_c), q_all=_p(dd.q_all), wcum_all=_p(dd.wcum_all),
               align=_p(dd.align), pmem=_p(dd.pmem), memory=_p(dd.memory), lengths=_p(dd.lengths),
               att_drop=_p(dd.m_att) if c.masks else None, dec_drop=_p(dd.m_dec) if c.masks else None,
               att_drop_scale=c.s_att, dec_drop_scale=c.s_dec, d_hc=_p(dd.d_hc), out_d=_p(o.out_d.t), out_a=_p(o.out_a.t),
               dg_d=_p(o.dg_d.t), dg_a=_p(o.dg_a.t), dq_all=_p(o.dq_all.t), dc_d=_p(o.dc_d.t), dc_a=_p(o.dc_a.t),
               dw_c=_p(o.dw_c.t), dwc_c=_p(o.dwc_c.t), d_pmem=_p(o.d_pmem.t), d_memory=_p(o.d_memory.t), dD_part=_p(o.dD.t),
               dK_part=_p(o.dK.t), dv_part=_p(o.dv.t), dw_buf=_p(o.dw_buf.t), df_buf=_p(o.df_buf.t), dq_part=_p(o.dq_part.t),
               dctx_all=_p(o.dctx_all.t) if deferred else None)
    if deferred:                # the forward's contexts: hc_all[t][b] = [h_dec | ctx]
        bp.ctx_all, bp.s_ctx_step, bp.s_ctx_item = _p(dd.hc_all, D), B * (D + E), D + E
        bp.dw_c2, bp.dwc_c2 = _p(o.dw_c2.t), _p(o.dwc_c2.t)
        if form == "fold":
            bp.att_xbuf = _p(xbuf)
    return bp, o, xbuf


def _run_bptt(c, form):
    P, E, A, D, T_in, T_out = (_BP[k] for k in ("P", "E", "A", "D", "T_in", "T_out"))
    B, ad, F_, KS, ref = c.B, c.ad, c.F, c.KS, c.ref
    nch, deferred = (T_in + 31) // 32, form != "three"
    bp, o, xbuf = _bptt_struct(c, form)
    _lib.call("t2s_taco_bptt_steps", ctypes.byref(bp), T_out, 0, _lib.current_stream())
    _sync()
    tag = "bptt[ad=%d F=%d KS=%d B=%d %s%s]" % (ad, F_, KS, B, form, "" if c.masks else " no masks")
    ck = _Checks()
    ck.ok(int(xbuf.view(torch.int64)[B * nch * 128].item()) == 0, tag + ": the error word of att_xbuf was raised")
    for name in ("dg_d", "dg_a", "dq_all", "out_d", "out_a"):
        ck("%s %s" % (tag, name), getattr(o, name).t, ref[name])
    if deferred:
        ck(tag + " dctx_all", o.dctx_all.t, ref["dctx_all"])
        ck.ok(o.d_memory.untouched(o.d_memory.t).all(), tag + ": d_memory touched although dctx_all defers it")
    else:
        ck(tag + " d_memory", _added(o, "d_memory", o.d_memory.t), ref["d_memory"])
        ck.ok(o.dctx_all.untouched(o.dctx_all.t).all(), tag + ": dctx_all written although it was not handed over")
    ck(tag + " d_pmem", _added(o, "d_pmem", o.d_pmem.t), ref["d_pmem"])
    for name, shape, want in (("dD", (F_, ad), ref["dD"].t()), ("dK", (F_, 2, KS), ref["dK"]), ("dv", (ad,), ref["dv"])):
        ck("%s %s (slot sum)" % (tag, name), _added(o, name, getattr(o, name).t, shape), want)
    for name, gd in vars(o).items():
        if isinstance(gd, Guarded):
            gd.assert_guards(tag + " " + name)
    ck.done()


@pytest.mark.parametrize("form", ["fold", "q_kernel", "three"])
def test_bptt_reference_attention_dims(lib, form):
    """attention_dim 128, 32 filters, kernel 31, B = 3.  "fold": att_bwd_fused_kernel with the attention cell folded in (the error
    word of att_xbuf stays 0); "q_kernel": the cell in its own launch (lstm_cell_bwd_q_kernel); "three": att_bwd_dw / energy_mfma /
    conv_mfma kernels with carries in place and d_memory accumulated in the loop.  Sizes as the issue gives them (P 32, E 64,
    A = D = 128, T_in 40, T_out 18): every launcher accepts them."""
    _run_bptt(_bptt_case(128, 32, 31, 3, True), form)


def test_bptt_reference_attention_dims_no_masks(lib):
    _run_bptt(_bptt_case(128, 32, 31, 3, False), "fold")


@pytest.mark.parametrize("ad", [64, 72])
@pytest.mark.parametrize("masks", [True, False])
def test_bptt_off_reference_attention_dims(lib, ad, masks):
    """16 filters, kernel 33: with ctx_all offered t2s_att_bwd_fused_ok says no and the loop falls back to three launches (VALU
    energies and convolution); the attention cell goes through lstm_cell_bwd_kernel with wq - q_dim 64 is whole blocks of 16 query
    rows, 72 leaves 8 to the tail loop."""
    _run_bptt(_bptt_case(ad, 16, 33, 3, masks), "fold")


@pytest.mark.parametrize("masks", [True, False])
def test_bptt_nine_items(lib, masks):
    """B = 9: split_rows - the A + E rows of the transposed decoder GEMM as one launch per chunk of steps."""
    _run_bptt(_bptt_case(128, 32, 31, 9, masks), "fold")


# ================================================================================= 3. t2s_taco_attention off the reference shape
def _att_forward(AD, F_, KS, T, B, E, denseT, A=128):
    g = torch.Generator().manual_seed(3000 + AD + F_ + KS + T * 13 + B + E + denseT)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    lengths = torch.tensor(_LEN[B](T), dtype=torch.int32)
    h, Wq = r(B, A, sc=0.5), r(AD, A, sc=0.1)
    pmem, memory = r(B, T, AD, sc=0.5), r(B, T, E)
    w0, wc0 = torch.softmax(r(B, T), 1), torch.rand(B, T, generator=g) * 2
    K, D, v = r(F_, 2, KS, sc=0.2), r(AD, F_, sc=0.2), r(AD, sc=0.3)
    d64 = lambda t: t.double()
    w, ctx, wc = _att_step(d64(h) @ d64(Wq).t(), d64(pmem), d64(memory), d64(w0), d64(wc0), d64(K), d64(D), d64(v), lengths)
    gw, gwc, gctx = Guarded(B, T, fill=dev(w0)), Guarded(B, T, fill=dev(wc0)), Guarded(B, E)
    qs, es = Guarded(B, AD), Guarded(B, T)
    ins = [dev(t) for t in (h, memory, pmem, lengths, Wq, K, D, D.t().contiguous(), v)]
    _lib.call("t2s_taco_attention", ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), ptr(gw.t), ptr(gwc.t), ptr(gctx.t),
              ptr(qs.t), ptr(es.t), ptr(ins[4]), ptr(ins[5]), ptr(ins[6]), ptr(ins[7]) if denseT else None, ptr(ins[8]), B, T, A,
              AD, E, F_, KS, _lib.current_stream())
    _sync()
    tag = "attention[AD=%d F=%d KS=%d T=%d B=%d E=%d denseT=%d]" % (AD, F_, KS, T, B, E, denseT)
    ck = _Checks()
    ck(tag + " w", gw.t, w)
    ck(tag + " w_cum", gwc.t, wc)
    ck(tag + " ctx", gctx.t, ctx)
    for b in range(B):
        ck.ok(float(gw.t[b, int(lengths[b]):].abs().sum()) == 0.0, tag + ": a weight past the length is not exactly 0")
    for name, gd in (("w", gw), ("w_cum", gwc), ("ctx", gctx), ("q_scratch", qs), ("e_scratch", es)):
        gd.assert_guards(tag + " " + name)
    ck.done()


_OFF_ROWS = [(64, 16, 33, 68), (72, 32, 63, 68), (96, 32, 31, 512)]          # (attention_dim, filters, kernel, enc_dim)


@pytest.mark.parametrize("AD,F_,KS,E", _OFF_ROWS)
@pytest.mark.parametrize("T", [33, 70])
def test_attention_one_launch_off_reference(lib, AD, F_, KS, E, T):
    """att_fused_kernel (the form without matrix cores): up to 8 items, T <= 512, w_loc_denseT given."""
    _att_forward(AD, F_, KS, T, 3, E, True)


@pytest.mark.parametrize("AD,F_,KS,E", _OFF_ROWS)
@pytest.mark.parametrize("T", [15, 16, 17])
def test_attention_three_launches_off_reference(lib, AD, F_, KS, E, T):
    """w_loc_denseT = NULL: query GEMV + att_energy_kernel + softmax / context; T around ATT_TQ = 16."""
    _att_forward(AD, F_, KS, T, 3, E, False)


@pytest.mark.parametrize("AD,F_,KS,T,B,E,denseT", [
    (64, 16, 33, 40, 9, 68, True),          # more than ATT_FUSED_MAX_B = 8 items: three launches, att_energy_kernel
    (128, 32, 31, 40, 9, 512, True),        # ... and the matrix-core energies at the reference dims
    (64, 16, 33, 513, 2, 68, True),         # one position past the one-launch form's 512
    (128, 32, 31, 70, 3, 512, False),       # the reference shape without the transposed weight: att_energy_kernel
    (128, 32, 31, 70, 3, 512, True),        # the reference shape: att_fused_mfma_kernel
])
def test_attention_other_paths(lib, AD, F_, KS, T, B, E, denseT):
    _att_forward(AD, F_, KS, T, B, E, denseT)


# ================================================================================================== 4. the small entry points
@pytest.mark.parametrize("H,n_src,mask,cprev", [(1024, 3, True, True), (100, 1, False, False), (257, 2, True, True),
                                                (257, 3, False, False), (100, 2, True, True)])
def test_lstm_cell_bwd(lib, H, n_src, mask, cprev):
    """lstm_cell_bwd_kernel without wq.  float64: z -> (i, f, g, o), c' = f c + i g, h = o tanh(c') * mask * scale;
    L = <dh1 + dh2 + dh3, h> + <dc_carry, c'>; dgates = dL/dz, the new carry = dL/dc."""
    B, scale = 3, 1.0 / 0.9
    g = torch.Generator().manual_seed(4000 + H + n_src)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    z, c_prev = r(B, 4 * H), (r(B, H) if cprev else torch.zeros(B, H))
    strides = (H + 8, 2 * H, H)[:n_src]
    srcs = [r(B, s, sc=0.3) for s in strides]
    m = (torch.rand(B, H, generator=g) >= 0.1).to(torch.uint8)
    carry = r(B, H, sc=0.3)
    z64, c64 = z.double().requires_grad_(True), c_prev.double().requires_grad_(True)
    i, f, gg, o = z64.chunk(4, 1)
    gates = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], 1)
    i, f, gg, o = gates.chunk(4, 1)
    c_new = f * c64 + i * gg
    h = o * torch.tanh(c_new)
    if mask:
        h = h * m.double() * scale
    dh = sum(s[:, :H].double() for s in srcs)
    want_dg, want_dc = torch.autograd.grad((dh * h).sum() + (carry.double() * c_new).sum(), [z64, c64])
    d_srcs = [dev(s) for s in srcs] + [None] * (3 - n_src)
    d_gates, d_cnew, d_cprev, d_m = dev(gates.detach().float()), dev(c_new.detach().float()), dev(c_prev), dev(m)
    dc, dg = Guarded(B, H, fill=dev(carry)), Guarded(B, 4 * H)
    _lib.call("t2s_lstm_cell_bwd", ptr(d_srcs[0]), strides[0], ptr(d_srcs[1]), strides[1] if n_src > 1 else 0, ptr(d_srcs[2]),
              strides[2] if n_src > 2 else 0, ptr(d_m) if mask else None, scale, ptr(d_gates), ptr(d_cnew),
              ptr(d_cprev) if cprev else None, ptr(dc.t), ptr(dg.t), B, H, _lib.current_stream())
    _sync()
    tag = "lstm_cell_bwd[H=%d sources=%d mask=%d c_prev=%d]" % (H, n_src, mask, cprev)
    ck = _Checks()
    ck(tag + " dgates", dg.t, want_dg)
    ck(tag + " dc_carry", dc.t, want_dc)
    dg.assert_guards(tag + " dgates")
    dc.assert_guards(tag + " dc_carry")
    ck.done()


_BN_SHAPES = [(2, 80, 130), (1, 33, 1), (3, 512, 63), (2, 64, 64), (2, 64, 65)]
_PLANE_MARK = 7.0           # what plane outputs hold before a call: a written halo row or an unwritten data row shows


def _marked_planes(B, C, Lp):
    mk = lambda: torch.full((B, -(-C // 32), Lp, 32), _PLANE_MARK, dtype=torch.bfloat16, device=DEV)
    return mk(), mk()


def _planes_ok(ck, pair, C, L, halo, tag):
    """Halo rows still hold the mark; channels C .. 32 ceil(C / 32) of the data rows are zero."""
    for p in pair:
        ck.ok(bool((p[:, :, :halo].float() == _PLANE_MARK).all()) and bool((p[:, :, halo + L:].float() == _PLANE_MARK).all()),
              tag + ": halo rows were written")
        if C % 32:
            ck.ok(float(p[:, -1, halo:halo + L, C % 32:].float().abs().max()) == 0.0, tag + ": channels past C are not zero")


@pytest.mark.parametrize("B,C,T", _BN_SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("mask", [False, True])
def test_bn_train_and_bwd(lib, B, C, T, act, mask):
    """t2s_bn_train (bn_stats_kernel, bn_apply_kernel) then t2s_bn_bwd on the forward's mean and variance (bn_bwd_reduce / _final /
    _apply kernels; tiles of 64 steps x 32 channels), the gradient of the output as f32 and as planes.  float64:
    y = act(F.batch_norm(x, training=True)) * mask * 2 and autograd of <dout, y>.  With B T = 1 the variance is 0 and dx = 0."""
    halo, eps = 32, 1e-5
    Lp = _lib.plane_rows(T, halo)
    g = torch.Generator().manual_seed(5000 + B + C + T + act)
    x = torch.randn(B, C, T, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3
    m = (torch.rand(B, C, T, generator=g) >= 0.5).to(torch.uint8)

    def fwd(xx, ga, be):
        if B * T > 1:
            return F.batch_norm(xx, None, None, ga, be, True, 0.0, eps)
        # (F.batch_norm refuses one value per channel in training mode: the same formula written out)
        mu, va = xx.mean((0, 2), keepdim=True), xx.var((0, 2), unbiased=False, keepdim=True)
        return (xx - mu) / torch.sqrt(va + eps) * ga[None, :, None] + be[None, :, None]

    if act == 1 and B * T > 1:          # relu: keep every pre-activation away from 0, where the gradient is not defined
        for _ in range(4):
            near = fwd(x.double(), gamma.double(), beta.double()).abs() < 1e-3
            x[near] += 0.05
        assert not bool((fwd(x.double(), gamma.double(), beta.double()).abs() < 1e-4).any())
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    ybn = fwd(x64, g64, b64)
    y = (ybn, torch.relu(ybn), torch.tanh(ybn))[act]
    if mask:
        y = y * m.double() * 2.0
    tag = "bn[B=%d C=%d T=%d act=%d mask=%d]" % (B, C, T, act, mask)
    ck = _Checks()
    # ---- forward ----
    dx_, dg_, db_, dm_ = dev(x), dev(gamma), dev(beta), dev(m)
    mean, var, out = Guarded(C), Guarded(C), Guarded(B, C, T)
    O = _marked_planes(B, C, Lp)
    _lib.call("t2s_bn_train", ptr(dx_), ptr(dg_), ptr(db_), eps, act, ptr(dm_) if mask else None, 2.0, B, C, T, Lp, halo,
              ptr(mean.t), ptr(var.t), ptr(O[0]), ptr(O[1]), ptr(out.t), _lib.current_stream())
    _sync()
    ck(tag + " mean", mean.t, x.double().mean((0, 2)))
    ck(tag + " var", var.t, x.double().var((0, 2), unbiased=False))
    ck(tag + " out f32", out.t, y.detach())
    ck(tag + " out planes", U.plane_values(O, C, T, halo), y.detach())
    _planes_ok(ck, O, C, T, halo, tag + " out planes")
    for name, gd in (("mean", mean), ("var", var), ("out", out)):
        gd.assert_guards(tag + " " + name)
    # ---- backward, from the forward's statistics ----
    for as_planes in (False, True):
        if as_planes:
            dpair, dout = U.rand_planes(g, B, C, T, halo, 0.3)
        else:
            dout32 = torch.randn(B, C, T, generator=g) * 0.3
            d_dout, dout = dev(dout32), dout32.double()
        want_dx, want_dg, want_db = torch.autograd.grad((dout * y).sum(), [x64, g64, b64], retain_graph=True)
        dgam, dbet = Guarded(C), Guarded(C)
        DX = _marked_planes(B, C, Lp)
        part = torch.empty(B * C * 2, dtype=torch.float64, device=DEV)
        a = _BnBwd(x=dx_.data_ptr(), mean=mean.t.data_ptr(), var=var.t.data_ptr(), gamma=dg_.data_ptr(), beta=db_.data_ptr(), eps=eps,
                   dout_f32=None if as_planes else d_dout.data_ptr(), dout_hi=dpair[0].data_ptr() if as_planes else None,
                   dout_lo=dpair[1].data_ptr() if as_planes else None, mask=dm_.data_ptr() if mask else None, mask_scale=2.0,
                   act=act, dgamma=dgam.t.data_ptr(), dbeta=dbet.t.data_ptr(), dx_hi=DX[0].data_ptr(), dx_lo=DX[1].data_ptr(),
                   B=B, C=C, T=T, Lp=Lp, halo=halo)
        _lib.call("t2s_bn_bwd", ctypes.byref(a), ptr(part), _lib.current_stream())
        _sync()
        t2 = "%s bwd dout=%s" % (tag, "planes" if as_planes else "f32")
        ck(t2 + " dgamma", dgam.t, want_dg)
        ck(t2 + " dbeta", dbet.t, want_db)
        got_dx = U.plane_values(DX, C, T, halo)
        if B * T == 1:
            ck.ok(bool(torch.isfinite(got_dx).all()) and float(got_dx.abs().max()) == 0.0, t2 + ": dx of a single sample is not 0")
        else:
            ck(t2 + " dx", got_dx, want_dx)
        _planes_ok(ck, DX, C, T, halo, t2 + " dx")
        dgam.assert_guards(t2 + " dgamma")
        dbet.assert_guards(t2 + " dbeta")
    ck.done()


@pytest.mark.parametrize("B,T", [(23, 89), (4, 512), (3, 683), (41, 100)])         # B T = 2047, 2048, 2049, 4100
@pytest.mark.parametrize("E", [512, 40])
def test_embedding_grad(lib, B, T, E):
    """embedding_grad_kernel: the ids pass through LDS EMBG_CHUNK = 2048 at a time (T = 100 does not divide it); ids 70 .. 79 never
    occur and their rows must come out as zeros (the output starts as NaN)."""
    V, halo = 80, 32
    g = torch.Generator().manual_seed(6000 + B * T + E)
    ids = torch.randint(0, 70, (B, T), generator=g)
    pair, vals = U.rand_planes(g, B, E, T, halo)
    want = torch.zeros(V, E, dtype=torch.float64).index_add_(0, ids.flatten(), vals.permute(0, 2, 1).reshape(-1, E))
    out = Guarded(V, E)
    d_ids = dev(ids)
    _lib.call("t2s_embedding_grad", ptr(d_ids), ptr(pair[0]), ptr(pair[1]), B, T, E, V, pair[0].size(2), halo, ptr(out.t),
              _lib.current_stream())
    _sync()
    check("embedding_grad[B=%d T=%d E=%d]" % (B, T, E), out.t, want, F32_NORM, F32_MAX)
    assert float(out.t[70:].abs().max()) == 0.0
    out.assert_guards("embedding_grad")


def test_embedding_grad_one_symbol_everywhere(lib):
    B, T, E, V, halo = 41, 100, 40, 80, 32
    g = torch.Generator().manual_seed(6100)
    ids = torch.full((B, T), 5, dtype=torch.int64)
    pair, vals = U.rand_planes(g, B, E, T, halo)
    want = torch.zeros(V, E, dtype=torch.float64)
    want[5] = vals.sum((0, 2))
    out = Guarded(V, E)
    d_ids = dev(ids)
    _lib.call("t2s_embedding_grad", ptr(d_ids), ptr(pair[0]), ptr(pair[1]), B, T, E, V, pair[0].size(2), halo, ptr(out.t),
              _lib.current_stream())
    _sync()
    check("embedding_grad[one symbol in all 4100 positions]", out.t, want, F32_NORM, F32_MAX)
    out.assert_guards("embedding_grad")


def _tm_expect(x, items, items_pad, shift, C):
    """float64 [items_pad / 32, C, 32]: slot (chunk, c, r) holds x[32 chunk + r - shift][c], zero outside [0, items)."""
    src = torch.arange(items_pad) - shift
    ok = (src >= 0) & (src < items)
    v = torch.zeros(items_pad, C, dtype=torch.float64)
    v[ok] = x[src[ok], :C].double()
    return v.view(items_pad // 32, 32, C).permute(0, 2, 1)


@pytest.mark.parametrize("C", [33, 64])
def test_rows_to_tm(lib, C):
    """rows_to_tm_kernel: f32 rows (stride ld > C) -> time-major planes tm[item / 32][n_off + c][item % 32] at n_off = 32 of a wider
    Npad; items 1, 31, 33, 70, shifts 0, +3, -2.  Rows outside [n_off, n_off + C) keep what they held."""
    Npad, n_off, ld = 128, 32, C + 5
    g = torch.Generator().manual_seed(6200 + C)
    ck = _Checks()
    for items in (1, 31, 33, 70):
        for shift in (0, 3, -2):
            items_pad = -(-items // 32) * 32 + (32 if items == 33 else 0)
            x = torch.randn(items, ld, generator=g)
            d_x = dev(x)
            hi, lo = (torch.full((items_pad // 32, Npad, 32), _PLANE_MARK, dtype=torch.bfloat16, device=DEV) for _ in range(2))
            _lib.call("t2s_rows_to_tm", ptr(d_x), ld, items, items_pad, shift, C, ptr(hi), ptr(lo), Npad, n_off, _lib.current_stream())
            _sync()
            tag = "rows_to_tm[C=%d items=%d shift=%d]" % (C, items, shift)
            got = (hi.double() + lo.double()).cpu()
            want = _tm_expect(x, items, items_pad, shift, C)
            ck(tag, got[:, n_off:n_off + C], want)
            src = torch.arange(items_pad) - shift
            empty = ((src < 0) | (src >= items)).view(-1, 1, 32).expand(-1, C, -1)
            ck.ok(float(got[:, n_off:n_off + C][empty].abs().sum()) == 0.0 if bool(empty.any()) else True,
                  tag + ": a slot of an item outside [0, items) is not zero")
            for p in (hi, lo):
                ck.ok(bool((p[:, :n_off].float() == _PLANE_MARK).all()) and bool((p[:, n_off + C:].float() == _PLANE_MARK).all()),
                      tag + ": rows outside [n_off, n_off + C) were written")
    ck.done()


def test_rows_to_tm_batched(lib):
    """Three sets at once, with batch strides on both sides (the source sets overlap nothing, the planes have a gap between sets)."""
    nb, items, items_pad, C, ld, Npad, n_off, shift = 3, 70, 96, 33, 40, 128, 32, 3
    g = torch.Generator().manual_seed(6300)
    x_bstride, dst_bstride = items * ld + 24, (items_pad // 32) * Npad * 32 + 64
    xs = torch.randn(nb, x_bstride, generator=g)
    d_x = dev(xs)
    hi, lo = (torch.full((nb, dst_bstride), _PLANE_MARK, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    _lib.call("t2s_rows_to_tm_batched", ptr(d_x), ld, x_bstride, items, items_pad, shift, C, ptr(hi), ptr(lo), dst_bstride, Npad,
              n_off, nb, _lib.current_stream())
    _sync()
    ck = _Checks()
    for z in range(nb):
        tm = lambda p: p[z, :dst_bstride - 64].double().cpu().view(items_pad // 32, Npad, 32)
        want = _tm_expect(xs[z, :items * ld].view(items, ld), items, items_pad, shift, C)
        ck("rows_to_tm_batched[set %d]" % z, (tm(hi) + tm(lo))[:, n_off:n_off + C], want)
        for p in (hi, lo):
            ck.ok(bool((tm(p)[:, :n_off] == _PLANE_MARK).all()) and bool((tm(p)[:, n_off + C:] == _PLANE_MARK).all()) and
                  bool((p[z, dst_bstride - 64:].float() == _PLANE_MARK).all()), "rows_to_tm_batched[set %d]: wrote outside its rows" % z)
    ck.done()


@pytest.mark.parametrize("C", [80, 33])
@pytest.mark.parametrize("L", [1, 63, 64, 65])
def test_rows_to_planes_and_back(lib, C, L):
    """rows_to_planes_kernel ([B][L][C] channel-last rows -> planes) and planes_to_f32_kernel (planes -> [B][C][L], written or
    added onto a non-zero start), and the round trip."""
    B, halo = 2, 32
    Lp = _lib.plane_rows(L, halo)
    g = torch.Generator().manual_seed(6400 + C + L)
    x = torch.randn(B, L, C, generator=g)
    d_x = dev(x)
    pair = _marked_planes(B, C, Lp)
    _lib.call("t2s_rows_to_planes", ptr(d_x), B, L, C, Lp, halo, ptr(pair[0]), ptr(pair[1]), _lib.current_stream())
    _sync()
    tag = "[C=%d L=%d]" % (C, L)
    ck = _Checks()
    held = U.plane_values(pair, C, L, halo)
    ck("rows_to_planes" + tag, held, x.double().permute(0, 2, 1))
    _planes_ok(ck, pair, C, L, halo, "rows_to_planes" + tag)
    start = torch.randn(B, C, L, generator=g)
    for accumulate in (0, 1):
        out = Guarded(B, C, L, fill=dev(start))
        _lib.call("t2s_planes_to_f32", ptr(pair[0]), ptr(pair[1]), B, C, L, Lp, halo, ptr(out.t), accumulate, _lib.current_stream())
        _sync()
        ck("planes_to_f32%s accumulate=%d" % (tag, accumulate), out.t, held + (start.double() if accumulate else 0.0))
        if not accumulate:
            ck("rows_to_planes -> planes_to_f32" + tag, out.t, x.double().permute(0, 2, 1))
        out.assert_guards("planes_to_f32" + tag)
    ck.done()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_small_f32_ops(lib, n):
    """relu_drop_bwd_kernel, sum_axis0_kernel, add3_kernel (b and / or c NULL), scale_by_scalar_kernel (in NULL)."""
    g = torch.Generator().manual_seed(6500 + n)
    r = lambda *s: torch.randn(*s, generator=g)
    st = _lib.current_stream()
    ck = _Checks()

    def run(label, want, fn):
        out = Guarded(n)
        fn(out)
        _sync()
        ck("%s[n=%d]" % (label, n), out.t, want)
        out.assert_guards(label)

    dy, y = r(n), torch.relu(r(n)) * (torch.rand(n, generator=g) >= 0.5)
    d_dy, d_y = dev(dy), dev(y)
    run("relu_drop_bwd", torch.where(y > 0, dy.double() * 2.0, torch.zeros((), dtype=torch.float64)),
        lambda o: _lib.call("t2s_relu_drop_bwd", ptr(d_dy), ptr(d_y), 2.0, n, ptr(o.t), st))
    m = r(7, n)
    d_m = dev(m)
    run("sum_axis0", m.double().sum(0), lambda o: _lib.call("t2s_sum_axis0", ptr(d_m), 7, n, ptr(o.t), st))
    a, b, c = r(n), r(n), r(n)
    d_a, d_b, d_c = dev(a), dev(b), dev(c)
    for label, bb, cc in (("add3 a+b+c", b, c), ("add3 a+b", b, None), ("add3 a+c", None, c), ("add3 a", None, None)):
        want = a.double() + (0 if bb is None else bb.double()) + (0 if cc is None else cc.double())
        run(label, want, lambda o, bb=bb, cc=cc: _lib.call("t2s_add3", ptr(d_a), ptr(d_b) if bb is not None else None,
                                                           ptr(d_c) if cc is not None else None, n, ptr(o.t), st))
    s = torch.tensor([0.37])
    d_s = dev(s)
    run("scale_by_scalar", a.double() * float(s.double()) * float(torch.tensor(-1.5)),
        lambda o: _lib.call("t2s_scale_by_scalar", ptr(d_a), n, ptr(d_s), -1.5, ptr(o.t), st))
    run("scale_by_scalar in=NULL", torch.full((n,), float(s.double()) * 0.25, dtype=torch.float64),
        lambda o: _lib.call("t2s_scale_by_scalar", None, n, ptr(d_s), 0.25, ptr(o.t), st))
    ck.done()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(lib):
    """T2S_EINVAL, and nothing written, for what the wrappers document: NULL required pointers, items_pad % 32, n_off + C > Npad,
    an even location kernel, 129 attention channels, 33 filters, the one-launch attention backward with d_memory set."""
    st = _lib.current_stream()
    out = Guarded(4096)
    o, buf = ptr(out.t), torch.zeros(4096, device=DEV)
    bp = ptr(buf)
    # rows_to_tm
    assert lib.t2s_rows_to_tm(None, 8, 4, 32, 0, 4, o, o, 32, 0, st) == EINVAL
    assert lib.t2s_rows_to_tm(bp, 8, 4, 32, 0, 4, None, o, 32, 0, st) == EINVAL
    assert lib.t2s_rows_to_tm(bp, 8, 4, 33, 0, 4, o, o, 32, 0, st) == EINVAL            # items_pad % 32
    assert lib.t2s_rows_to_tm(bp, 8, 40, 32, 0, 4, o, o, 32, 0, st) == EINVAL           # items_pad < items
    assert lib.t2s_rows_to_tm(bp, 8, 4, 32, 0, 4, o, o, 32, 29, st) == EINVAL           # n_off + C > Npad
    assert lib.t2s_rows_to_tm_batched(bp, 8, 64, 4, 32, 0, 4, o, o, 1024, 32, 29, 2, st) == EINVAL
    assert lib.t2s_rows_to_tm_batched(bp, 8, 64, 4, 48, 0, 4, o, o, 1024, 32, 0, 2, st) == EINVAL
    assert lib.t2s_rows_to_tm_batched(bp, 8, 64, 4, 32, 0, 4, o, o, 1024, 32, 0, 0, st) == EINVAL
    # the small ops
    assert lib.t2s_lstm_cell_bwd(bp, 8, None, 0, None, 0, None, 1.0, None, bp, bp, o, o, 1, 8, st) == EINVAL
    assert lib.t2s_lstm_cell_bwd(bp, 8, None, 0, None, 0, None, 1.0, bp, bp, bp, None, o, 1, 8, st) == EINVAL
    assert lib.t2s_lstm_cell_bwd(bp, 8, None, 0, None, 0, None, 1.0, bp, bp, bp, o, o, 1, 0, st) == EINVAL
    assert lib.t2s_relu_drop_bwd(None, bp, 2.0, 8, o, st) == EINVAL and lib.t2s_relu_drop_bwd(bp, bp, 2.0, 0, o, st) == EINVAL
    assert lib.t2s_sum_axis0(None, 2, 8, o, st) == EINVAL and lib.t2s_sum_axis0(bp, 0, 8, o, st) == EINVAL
    assert lib.t2s_add3(None, bp, bp, 8, o, st) == EINVAL and lib.t2s_add3(bp, bp, bp, 0, o, st) == EINVAL
    assert lib.t2s_scale_by_scalar(bp, 8, None, 1.0, o, st) == EINVAL and lib.t2s_scale_by_scalar(bp, 0, bp, 1.0, o, st) == EINVAL
    assert lib.t2s_planes_to_f32(None, bp, 1, 4, 4, 320, 32, o, 0, st) == EINVAL
    assert lib.t2s_rows_to_planes(bp, 1, 4, 4, 100, 32, o, o, st) == EINVAL              # Lp below t2s_plane_rows(T, halo)
    assert lib.t2s_rows_to_planes(None, 1, 4, 4, 320, 32, o, o, st) == EINVAL
    assert lib.t2s_embedding_grad(None, bp, bp, 1, 4, 4, 8, 320, 32, o, st) == EINVAL
    assert lib.t2s_embedding_grad(bp, bp, bp, 1, 4, 4, 0, 320, 32, o, st) == EINVAL
    assert lib.t2s_bn_train(bp, bp, bp, 1e-5, 3, None, 2.0, 1, 4, 4, 320, 32, o, o, None, None, o, st) == EINVAL      # act
    assert lib.t2s_bn_train(bp, bp, bp, 1e-5, 0, None, 2.0, 1, 4, 4, 320, 32, o, o, None, None, None, st) == EINVAL   # no output
    assert lib.t2s_bn_train(bp, bp, bp, 1e-5, 0, None, 2.0, 1, 4, 4, 100, 32, o, o, o, o, None, st) == EINVAL         # Lp
    part = torch.zeros(64, dtype=torch.float64, device=DEV)
    bn = _BnBwd(x=buf.data_ptr(), mean=buf.data_ptr(), var=buf.data_ptr(), gamma=buf.data_ptr(), beta=buf.data_ptr(), eps=1e-5,
                dout_f32=None, dout_hi=None, dout_lo=None, mask=None, mask_scale=2.0, act=0, dgamma=out.t.data_ptr(),
                dbeta=out.t.data_ptr(), dx_hi=out.t.data_ptr(), dx_lo=out.t.data_ptr(), B=1, C=4, T=4, Lp=320, halo=32)
    assert lib.t2s_bn_bwd(ctypes.byref(bn), ptr(part), st) == EINVAL                     # neither form of dout
    bn.dout_f32 = buf.data_ptr()
    assert lib.t2s_bn_bwd(ctypes.byref(bn), None, st) == EINVAL
    # the attention step, backward: the struct of a small valid call, one field wrong at a time
    x = _att_case(128, 32, 31, 33, 3, 512)

    def att(**kw):
        a = _att_struct(x)
        for name in ("d_q", "d_pmem", "dD_part", "dK_part", "dv_part", "dw_buf", "df_buf", "dq_part", "dctx_out", "dw_carry",
                     "dwc_carry"):
            setattr(a, name, out.t.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.t2s_taco_att_bwd(ctypes.byref(a), st)

    assert att(loc_ks=30) == EINVAL and att(loc_ks=65) == EINVAL
    assert att(att_dim=129) == EINVAL and att(loc_f=33) == EINVAL
    assert att(enc_dim=510) == EINVAL
    assert att(w_cur=None) == EINVAL and att(d_pmem=None) == EINVAL and att(dctx_out=None) == EINVAL      # (no d_memory either)
    one = dict(ctx=buf.data_ptr(), s_ctx=512, dw_carry_out=buf.data_ptr(), dwc_carry_out=buf.data_ptr())
    assert att(d_memory=out.t.data_ptr(), **one) == EINVAL                                # the one-launch form defers d_memory
    assert att(loc_ks=33, **one) == EINVAL and att(att_dim=64, **one) == EINVAL           # ... and has the reference dims only
    assert lib.t2s_taco_att_bwd(None, st) == EINVAL
    # the attention step, forward
    def fwd(att_dim=128, loc_f=32, loc_ks=31, h=bp):
        return lib.t2s_taco_attention(h, bp, bp, None, o, o, o, o, o, bp, bp, bp, bp, bp, 1, 4, 8, att_dim, 8, loc_f, loc_ks, st)

    assert fwd(loc_ks=30) == EINVAL and fwd(att_dim=129) == EINVAL and fwd(loc_f=33) == EINVAL and fwd(h=None) == EINVAL
    # the reversed loop
    c = _Bptt(B=1, T_in=4, T_out=2, T_cap=2)
    assert lib.t2s_taco_bptt_steps(None, 2, 0, st) == EINVAL
    assert lib.t2s_taco_bptt_steps(ctypes.byref(c), 3, 0, st) == EINVAL                   # t_hi > T_out
    assert lib.t2s_taco_bptt_steps(ctypes.byref(c), 2, 0, st) == EINVAL                   # NULL buffers
    # ... and a struct that is valid but for one dimension: refused before the decoder-cell chain of the first chunk is enqueued
    bp, o, _ = _bptt_struct(_bptt_case(128, 32, 31, 3, True), "fold")
    assert lib.t2s_taco_bptt_steps(ctypes.byref(bp), _BP["T_out"] + 1, 0, st) == EINVAL
    for field, bad in (("loc_kernel", 30), ("loc_kernel", 65), ("att_dim", 129), ("loc_filters", 33), ("enc_dim", 62)):
        good = getattr(bp, field)
        setattr(bp, field, bad)
        assert lib.t2s_taco_bptt_steps(ctypes.byref(bp), _BP["T_out"], 0, st) == EINVAL, field
        setattr(bp, field, good)
    _sync()
    for name in ("out_d", "out_a", "dg_d", "dg_a", "dq_all", "dctx_all", "d_memory", "dw_buf", "df_buf", "dq_part"):
        gd = getattr(o, name)
        assert bool(gd.untouched(gd.t).all()), "a refused t2s_taco_bptt_steps wrote to " + name
    for name in ("d_pmem", "dD", "dK", "dv"):
        assert torch.equal(getattr(o, name).t.cpu().reshape(-1), o.start[name].reshape(-1)), "a refused t2s_taco_bptt_steps wrote to " + name
    assert float(o.dc_d.t.abs().max()) == 0.0 and float(o.dc_a.t.abs().max()) == 0.0
    _sync()
    assert bool(out.untouched(out.t).all()), "a refused call wrote to its output"
    out.assert_guards("refusals")
