"""``t2s_taco_decode_steps_w16``: the autoregressive decode of up to 8 items with the four LSTM matrices streamed as IEEE binary16.

The weights are the seeded f32 decoder weights of tests/test_tacotron_fwd_kernels_gpu.py with the four LSTM matrices rounded through
``.half()``; the fp16 tensors go into ``t2s_taco_w16``, their widened f32 copies into ``t2s_taco_decoder``.  Two checks per case:
 (a) every output, state and scratch buffer of the fp16 run equals, bit for bit, the buffer ``t2s_taco_decode_steps`` leaves from the
     same struct - the fp16 kernels keep the f32 kernels' lane-to-k mapping and summation order, and widening a half is exact;
 (b) every output is within the F32 bars (wg_bwd_util) of the float64 decoder loop on the rounded weights.
Kernels by case:
   small sizes (A = 128, K = 224 / 320 per cell)     lstm_cell_kernel<1, 4, false, false, W16>: masked slots past K, and the
                                                      W_ih | W_hh seam inside a wave's slot range
   reference sizes, B <= 4, the streamed chain       lstm_cell_p2_kernel<W16>, gate_stream_role<W16> in att_fused_mfma_kernel<true, true, W16>,
                                                      lstm_cell_kernel<., 4, false, true, W16>; steps 4 and 5 (past mask_steps) read pre2
   reference sizes, B = 5, 8                          lstm_cell_kernel<3, 4, false, false, W16> (the full rows)
Then the engine: a .half() model takes the path by itself and returns what it returns with the switch off."""
import ctypes
import types

import pytest
import torch

import test_tacotron_fwd_kernels_gpu as K
from taco_ref_util import ragged
from text2speech_amd import _lib, synth
from text2speech_amd.tacotron.tacotron import _DecoderStruct
from wg_bwd_util import DEV, Guarded, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
LSTM = ("att_w_ih", "att_w_hh", "dec_w_ih", "dec_w_hh")
_CASES = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rounded_weights(dims):
    """The seeded decoder weights with the four LSTM matrices rounded through .half(): `w` holds the widened f32 copies, `w.h16` the
    fp16 tensors themselves."""
    src = K._dec_weights(dims, 128, 32, 31)
    w = types.SimpleNamespace(**vars(src))
    w.h16 = {name: getattr(src, name).half() for name in LSTM}
    for name in LSTM:
        setattr(w, name, w.h16[name].float())
    return w


def _case(dims, calls, B, stream, mask_steps=None):
    """K._decode_case for the autoregressive decode on the rounded weights; the float64 reference is computed once per case."""
    key = (tuple(sorted(dims.items())), calls, B, stream, mask_steps)
    if key in _CASES:
        return _CASES[key]
    P, E, A, T_in, T_cap = (dims[k] for k in ("P", "E", "A", "T_in", "T_cap"))
    c = types.SimpleNamespace(dims=dims, calls=calls, B=B, teacher=False, ad=128, F=32, KS=31, stream=stream, fold=stream, drops=False)
    c.n_steps = calls[-1][0] + calls[-1][1]
    c.mask_steps = T_cap if mask_steps is None else mask_steps
    c.w = _rounded_weights(dims)
    g = torch.Generator().manual_seed(52000 + B + P)
    c.lengths = torch.tensor(ragged(B, T_in), dtype=torch.int32)
    c.pmem, c.memory = torch.randn(B, T_in, 128, generator=g) * 0.5, torch.randn(B, T_in, E, generator=g)
    c.mk = (torch.rand(c.mask_steps, B, 2, P, generator=g) >= 0.5).to(torch.uint8)
    c.ref = K._decoder_loop(c, torch.float64)
    _CASES[key] = c
    return c


def _build(c, B=None, teacher=False):
    """A decoder struct for case `c` with fresh state: (struct, w16 struct, guarded buffers by name, tensors to keep alive)."""
    w, B = c.w, c.B if B is None else B
    P, E, A, n_mel, T_in, T_cap = (c.dims[k] for k in ("P", "E", "A", "n_mel", "T_in", "T_cap"))
    D, ad = A, c.ad
    keep = []

    def dv(t):
        keep.append(dev(t))
        return keep[-1]

    d = _DecoderStruct()
    for k, val in dict(B=B, T_in=T_in, n_mel=n_mel, prenet_dim=P, enc_dim=E, att_rnn_dim=A, dec_rnn_dim=D, att_dim=ad, loc_filters=c.F,
                       loc_kernel=c.KS, T_cap=T_cap, teacher_forced=int(teacher), mask_steps=0 if teacher else c.mask_steps).items():
        setattr(d, k, val)
    for name in LSTM + ("att_b_ih", "att_b_hh", "dec_b_ih", "dec_b_hh", "w_query", "w_loc_conv", "w_loc_dense", "w_v", "w_pre2"):
        setattr(d, name, dv(getattr(w, name)).data_ptr())
    w16 = _lib.TacoW16()
    for name in LSTM:
        setattr(w16, name, dv(w.h16[name]).data_ptr())
    w_all, b_all = dv(torch.cat([w.w_proj, w.w_projpre], 0)), dv(torch.cat([w.b_proj, w.b_projpre], 0))
    d.w_proj, d.b_proj = w_all.data_ptr(), b_all.data_ptr()
    d.w_projpre, d.b_projpre = w_all.data_ptr() + (n_mel + 1) * (D + E) * 4, b_all.data_ptr() + (n_mel + 1) * 4
    d.w_loc_denseT = dv(w.w_loc_dense.t()).data_ptr()
    rep = lambda t: t if t.size(0) == B else t[:1].expand(B, *t.shape[1:])        # (the refusal structs: more items than the case)
    d.memory, d.pmem, d.mem_lengths = dv(rep(c.memory)).data_ptr(), dv(rep(c.pmem)).data_ptr(), dv(rep(c.lengths)).data_ptr()
    d.prenet_masks = dv(c.mk if c.mk.size(1) == B else c.mk[:, :1].expand(-1, B, -1, -1)).data_ptr()
    if teacher:
        d.pre_all = dv(torch.zeros(T_cap + 1, B, P)).data_ptr()
    d.att_drop_scale = d.dec_drop_scale = 1.0
    o = {}
    zg = lambda *s: Guarded(*s, fill=torch.zeros(*s, device=DEV))
    for name, sh in dict(att_h0=(B, A), att_h1=(B, A), att_c=(B, A), dec_h0=(B, D), dec_h1=(B, D), dec_c=(B, D), att_w=(B, T_in),
                         att_wcum=(B, T_in), ctx=(B, E), q=(B, ad), energies=(B, T_in), pre1=(B, P), pre2=(B, P),
                         q_part=(A // 2, B, ad)).items():
        o[name] = zg(*sh)
    o["align_out"], o["mel_gate_out"] = Guarded(B, T_cap, T_in), Guarded(B, n_mel + 1, T_cap)
    if teacher:
        o["hc_all"] = Guarded(T_cap, B, D + E)
    if c.stream:
        o["gate_part"], o["ploc"] = zg(3, B, 4 * A), zg(B, T_in, ad)
        d.w_pre2T = dv(w.w_pre2.t()).data_ptr()
    for name, gd in o.items():
        setattr(d, name, gd.t.data_ptr())
    return d, w16, o, keep


def _plan_bits(lib, c, d, w16, step0, n, tag):
    bits, bits16, nbytes = ctypes.c_uint(0), ctypes.c_uint(0), ctypes.c_longlong(0)
    assert lib.t2s_taco_decode_plan(ctypes.byref(d), step0, n, ctypes.byref(bits)) == 0, tag
    assert lib.t2s_taco_decode_plan_w16(ctypes.byref(d), ctypes.byref(w16), step0, n, ctypes.byref(bits16), ctypes.byref(nbytes)) == 0, tag
    assert bits16.value == bits.value, tag
    A, P, E = (c.dims[k] for k in ("A", "P", "E"))
    assert nbytes.value == 2 * (4 * A * (P + E + A) + 4 * A * (A + E + A)), tag
    for name in ("STREAM_GATES", "FOLD_PRE2", "USE_PLOC"):
        assert bool(bits.value & K._PLAN_BITS[name]) == c.stream, "%s: plan bit %s (plan 0x%x)" % (tag, name, bits.value)
    for name in ("FUSED_ATT", "Q_PARTS", "PROJ_FUSED"):
        assert bits.value & K._PLAN_BITS[name], "%s: plan bit %s is clear (plan 0x%x)" % (tag, name, bits.value)
    assert not bits.value & (K._PLAN_BITS["SPLIT"] | K._PLAN_BITS["UNITS_2"] | K._PLAN_BITS["Q_BIG"]), tag


def _run_both(lib, c, tag):
    runs = {}
    for form in ("f32", "w16"):
        d, w16, o, keep = _build(c)
        for step0, n in c.calls:
            _plan_bits(lib, c, d, w16, step0, n, tag)
            if form == "f32":
                _lib.call("t2s_taco_decode_steps", ctypes.byref(d), step0, n, K._st())
            else:
                _lib.call("t2s_taco_decode_steps_w16", ctypes.byref(d), ctypes.byref(w16), step0, n, K._st())
        K._sync()
        runs[form] = o
    ck = K._Checks()
    # (a) bit for bit, scratch and unwritten sentinels included
    for name, gd in runs["w16"].items():
        a, b = gd.t.view(torch.int32), runs["f32"][name].t.view(torch.int32)
        n_diff = int((a != b).sum().item())
        print("EQUAL  %-60s %d of %d words differ" % ("%s %s" % (tag, name), n_diff, a.numel()))
        ck.ok(n_diff == 0, "%s: %s differs from the f32 entry point in %d of %d words" % (tag, name, n_diff, a.numel()))
        gd.assert_guards("%s %s" % (tag, name))
    # (b) the float64 decoder loop on the rounded weights
    o, ref, n = runs["w16"], c.ref, c.n_steps
    ck("%s align_out" % tag, o["align_out"].t[:, :n].permute(1, 0, 2), ref["w"])
    ck("%s mel_gate_out" % tag, o["mel_gate_out"].t[:, :, :n].permute(2, 0, 1), ref["mel_gate"])
    ck.ok(bool(o["align_out"].untouched(o["align_out"].t[:, n:]).all()), tag + ": align_out written past the last step")
    ck.ok(bool(o["mel_gate_out"].untouched(o["mel_gate_out"].t[:, :, n:]).all()), tag + ": mel_gate_out written past the last step")
    last_odd = (n - 1) & 1
    for name, key in (("att_w", "f_att_w"), ("att_wcum", "f_att_wcum"), ("ctx", "f_ctx"), ("att_c", "f_att_c"), ("dec_c", "f_dec_c"),
                      ("att_h0" if last_odd else "att_h1", "f_att_h"), ("dec_h0" if last_odd else "dec_h1", "f_dec_h")):
        ck("%s %s" % (tag, name), o[name].t, ref[key])
    ck.done()


@pytest.mark.parametrize("B", [1, 3, 8])
def test_small_sizes_equal_the_f32_entry_point(lib, B):
    """P 32, E 64, A = D 128, T_in 40 ragged, 18 steps as calls of 7 and 11 (the second starts on the odd ping-pong parity).  The
    attention cell has K = 224: one slot per wave with lanes past K masked, and the W_ih | W_hh seam at k = 96 inside wave 0's slot."""
    _run_both(lib, _case(K._DSMALL, K._CALLS_SMALL, B, False), "w16[small B=%d]" % B)


@pytest.mark.parametrize("B", [1, 2, 4])
def test_reference_sizes_streamed_chain(lib, B):
    """gate_part, w_pre2T, ploc and q_part given; mask_steps = 4 of 6 steps: steps 4 and 5 leave the folded prenet and read pre2."""
    _run_both(lib, _case(K._DREF, K._CALLS_REF, B, True, mask_steps=4), "w16[ref streamed B=%d]" % B)


@pytest.mark.parametrize("B", [5, 8])
def test_reference_sizes_full_rows(lib, B):
    """5 to 8 items: every cell streams its full [W_ih | W_hh] rows, three slots per wave."""
    _run_both(lib, _case(K._DREF, K._CALLS_REF, B, False, mask_steps=4), "w16[ref full rows B=%d]" % B)


def test_the_rounded_matrices_hold_subnormals():
    """A flush-to-zero conversion would show in the equality tests above only if the weights hold fp16 subnormals: they do."""
    w = _rounded_weights(K._DREF)
    for name in LSTM:
        a = w.h16[name].float().abs()
        n = int(((a > 0) & (a < 2.0 ** -14)).sum())
        print("%s: %d nonzero values below 2^-14 of %d" % (name, n, a.numel()))
        assert n > 0, name


def test_refusals_leave_the_outputs_untouched(lib):
    c = _case(K._DSMALL, K._CALLS_SMALL, 3, False)

    def refused(label, B=3, teacher=False, save=None, member=None, value=None, offset=0, null_w=False):
        d, w16, o, keep = _build(c, B=B, teacher=teacher)
        if save:
            keep.append(torch.zeros(c.dims["T_cap"] * B * 4 * c.dims["A"], device=DEV))
            setattr(d, save, keep[-1].data_ptr())
        if member:
            setattr(w16, member, value if offset == 0 else getattr(w16, member) + offset)
        before = {name: gd.raw.clone() for name, gd in o.items()}
        wp = None if null_w else ctypes.byref(w16)
        assert lib.t2s_taco_decode_plan_w16(ctypes.byref(d), wp, 0, 4, None, None) == (0 if null_w else EINVAL), label
        assert lib.t2s_taco_decode_steps_w16(ctypes.byref(d), wp, 0, 4, K._st()) == EINVAL, label
        K._sync()
        for name, gd in o.items():
            assert torch.equal(gd.raw, before[name]), "%s: %s was written" % (label, name)

    refused("teacher forced", teacher=True)
    refused("B = 9", B=9)
    for save in ("att_gates_all", "att_c_all", "dec_gates_all", "dec_c_all", "att_h_all", "q_all", "wcum_all"):
        refused(save, save=save)
    for name in LSTM:
        refused(name + " NULL", member=name, value=None)
        refused(name + " + 4 bytes", member=name, offset=4)
    refused("w NULL", null_w=True)


# ------------------------------------------------------------------------------------------------ engine
HP = synth.TACOTRON_HPARAMS
N_STEPS = 6


@pytest.fixture(scope="module")
def half_model():
    assert torch.cuda.is_available()
    _lib.load()
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    m = m.cuda().eval().half()
    m.decoder.gate_threshold, m.decoder.max_decoder_steps = 2.0, N_STEPS
    return m


def _inputs(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, 80, (B, T), generator=gen)
    masks = (torch.rand(N_STEPS, B, 2, 256, generator=gen) < 0.5).to(torch.uint8)
    return ids, masks


def _equal_outputs(a, b, label):
    for name, x, y in zip(("mel", "mel_post", "gate", "alignments"), a, b):
        assert x.dtype == y.dtype == torch.float16 and torch.equal(x, y), "%s: %s differs with decode_w16 off" % (label, name)


def test_engine_inference_takes_the_path_by_itself(half_model):
    from oracle import tacotron_oracle as TO
    eng = half_model._eng()
    ids, masks = _inputs(1, 16, 61)
    try:
        eng.decode_w16 = None
        auto = half_model.inference(ids.to(DEV), None, prenet_masks=masks)
        assert eng.last_decode_w16 is True
        plan, offer, nbytes = eng.last_decode_plan, eng.last_decode_offer, eng.last_decode_lstm_bytes
        eng.decode_w16 = False
        off = half_model.inference(ids.to(DEV), None, prenet_masks=masks)
        assert eng.last_decode_w16 is False
        assert (eng.last_decode_plan, eng.last_decode_offer) == (plan, offer)
        assert nbytes == 35_651_584 and eng.last_decode_lstm_bytes == 2 * nbytes
    finally:
        eng.decode_w16 = None
    assert plan.stream_gates and plan.fold_pre2 and plan.use_ploc
    assert tuple(auto[0].shape) == (1, 80, N_STEPS)
    _equal_outputs(auto, off, "inference B=1")
    sd = {k: (v.half().float() if v.is_floating_point() else v) for k, v in synth.tacotron_state().items()}
    with torch.no_grad():
        o = TO.tacotron_inference(sd, HP, ids, N_STEPS, masks.float())
    for name, got, want in (("mel", auto[0], o[0]), ("mel_post", auto[1], o[1])):
        r = _rel(got.float(), want)
        print("ORACLE %s norm-rel %.3e" % (name, r))
        assert r < 1e-3, name


def test_engine_inference_batch(half_model):
    eng = half_model._eng()
    lengths = (16, 9, 5)
    ids, masks = _inputs(3, 16, 62)
    try:
        eng.decode_w16 = None
        *auto, olen_a = half_model.inference_batch(ids.to(DEV), torch.tensor(lengths), prenet_masks=masks)
        assert eng.last_decode_w16 is True and eng.last_decode_lstm_bytes == 35_651_584
        eng.decode_w16 = False
        *off, olen_b = half_model.inference_batch(ids.to(DEV), torch.tensor(lengths), prenet_masks=masks)
        assert eng.last_decode_w16 is False and eng.last_decode_lstm_bytes == 71_303_168
    finally:
        eng.decode_w16 = None
    _equal_outputs(auto, off, "inference_batch B=3")
    assert olen_a.cpu().tolist() == olen_b.cpu().tolist() == [N_STEPS] * 3


def test_engine_f32_model_never_takes_the_path():
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    m = m.cuda().eval()
    m.decoder.gate_threshold, m.decoder.max_decoder_steps = 2.0, N_STEPS
    eng = m._eng()
    ids, masks = _inputs(1, 16, 63)
    m.inference(ids.to(DEV), None, prenet_masks=masks)
    assert eng.last_decode_w16 is False
    assert list(eng.last_decode_offer) == ["q_part", "gate_part", "ploc", "w_pre2T"]
    assert eng.last_decode_lstm_bytes == 71_303_168
    eng.decode_w16 = True
    with pytest.raises(_lib.T2SError):
        m.inference(ids.to(DEV), None, prenet_masks=masks)
