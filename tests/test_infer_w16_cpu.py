"""Host side of WaveGlow.infer's fp16 chain for .half() models (engine switch infer_w16): the fp16 plane helpers, which calls are
eligible, the overflow refusal and the ctypes table of the _h16 entry points.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from text2speech_amd import _lib, glow, planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(C=32, n_layers=2):
    return glow.WaveGlow(n_mel_channels=4, n_flows=2, n_group=8, n_early_every=4, n_early_size=2,
                         WN_config=dict(n_layers=n_layers, n_channels=C, kernel_size=3))


def test_split_f16_against_float64():
    """hi = the fp16 nearest to x, lo = the fp16 nearest to x - hi, restated in float64 (x is an f32 number, so x - hi is exact
    there as it is in f32); values across fp16's range, subnormals and an overflow included."""
    gen = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=gen) * s for s in (1e-6, 1e-4, 1.0, 300.0, 3e4)] +
                  [torch.tensor([0.0, -0.0, 65504.0, 65519.9, 65520.0, -7e4, 2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11])])
    hi, lo = planes.split_f16(x)
    assert hi.dtype == lo.dtype == torch.float16
    x64 = x.double().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        hi64 = x64.astype(np.float16)
        lo64 = (x64 - hi64.astype(np.float64)).astype(np.float16)
    assert np.array_equal(hi.numpy().view(np.uint16), hi64.view(np.uint16))
    fin = np.isfinite(hi64)
    assert np.array_equal(lo.numpy().view(np.uint16)[fin], lo64.view(np.uint16)[fin])
    assert not fin.all() and bool(torch.isinf(hi[~torch.from_numpy(fin)]).all())       # |x| >= 65520 overflows: the engine's guard
    # hi + lo carries x to 22 bits (|lo| <= 2^-11 |x|, rounded to 11 bits) down to half a subnormal step, 2^-25, of the lo plane
    ok = torch.from_numpy(fin)
    err = ((hi.double() + lo.double()) - x.double()).abs()[ok]
    assert bool((err <= 2.0 ** -22 * x.double().abs()[ok] + 2.0 ** -25).all())


def test_to_planes_formats():
    """fmt = "f16": the same layout with split_f16's pair; the default arguments give what they gave (split-bf16)."""
    x = torch.randn(2, 36, 7, generator=torch.Generator().manual_seed(1))
    hb, lb = planes.to_planes(x, 2, Lp=12)
    assert hb.dtype == torch.bfloat16 and tuple(hb.shape) == (2, 2, 12, 32)
    h0, l0 = planes.split_bf16(x)
    assert torch.equal(planes.from_planes(hb, lb, 36, 7, 2), h0.float() + l0.float())
    hf, lf = planes.to_planes(x, 2, Lp=12, fmt="f16")
    assert hf.dtype == lf.dtype == torch.float16 and tuple(hf.shape) == (2, 2, 12, 32)
    h1, l1 = planes.split_f16(x)
    assert torch.equal(planes.from_planes(hf, lf, 36, 7, 2), h1.float() + l1.float())
    assert float(hf[:, :, :2].abs().max()) == 0.0 and float(hf[:, :, 9:].abs().max()) == 0.0 and float(hf[:, 1, :, 4:].abs().max()) == 0.0
    with pytest.raises(ValueError):
        planes.to_planes(x, 2, Lp=12, fmt="fp8")


def test_eligibility():
    """infer only, every WN parameter fp16, n_channels % 16 == 0, the shipped library; True on an ineligible call raises before
    anything is launched (no GPU here), None and False never do."""
    _lib.load()
    assert _lib.operand_format() == 0
    m = _model()
    eng = m._eng()
    assert eng.infer_w16 is None and eng.last_infer_w16 is False
    ok, why = eng.w16_eligible()
    assert not ok and "float16" in why                      # a float model
    assert eng.use_w16() is False
    eng.infer_w16 = True
    with pytest.raises(_lib.T2SError, match="infer_w16 = True"):
        eng.use_w16()
    m.half()
    for c in m.convinv:                                     # the reference script's call order: only the WN parameters count
        c.float()
    assert eng.w16_eligible() == (True, "")
    assert eng.use_w16() is True
    ok, why = eng.w16_eligible(batch=True)
    assert not ok and "infer_batch" in why
    with pytest.raises(_lib.T2SError, match="infer_batch"):
        eng.use_w16(batch=True)
    eng.infer_w16 = False
    assert eng.use_w16() is False and eng.use_w16(batch=True) is False
    eng.infer_w16 = None
    assert eng.use_w16() is glow._INFER_W16_AUTO and eng.use_w16(batch=True) is False
    m.WN[1].res_skip_layers[0].float()                      # mixed dtypes
    assert eng.w16_eligible()[0] is False and eng.use_w16() is False
    m16 = _model(C=24).half()
    ok, why = m16._eng().w16_eligible()
    assert not ok and "16" in why
    m16._eng().infer_w16 = True
    with pytest.raises(_lib.T2SError):
        m16._eng().use_w16()
    # after remove_weightnorm the plain weights are what counts
    m2 = glow.WaveGlow.remove_weightnorm(_model().half())
    assert m2._eng().w16_eligible() == (True, "")


def test_refuse_overflow(monkeypatch):
    monkeypatch.delenv("T2S_F16_GUARD", raising=False)
    t = torch.zeros(2, 8)
    glow.WaveGlow._refuse_overflow(t, w16=True)
    t[1, 3] = float("inf")
    with pytest.raises(_lib.T2SError, match="infer_w16 = False"):
        glow.WaveGlow._refuse_overflow(t, w16=True)
    with pytest.raises(_lib.T2SError, match="split-bf16 library"):
        glow.WaveGlow._refuse_overflow(t)
    t[1, 3] = float("nan")
    with pytest.raises(_lib.T2SError):
        glow.WaveGlow._refuse_overflow(t, w16=True)
    monkeypatch.setenv("T2S_F16_GUARD", "0")                # timing runs: no read-back
    glow.WaveGlow._refuse_overflow(t, w16=True)


def test_h16_symbols_mirror_their_partners():
    """Every _h16 function declared in include/t2s_hip.h is in the ctypes table with its partner's argtypes, and the header gives
    both the same parameter list."""
    src = open(os.path.join(ROOT, "include", "t2s_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {name: re.sub(r"\s+", " ", args).strip() for name, args in re.findall(r"\bint\s+(t2s_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src)}
    h16 = sorted(n for n in decl if n.endswith("_h16"))
    assert h16 == sorted(["t2s_pack_conv_weight_table_h16", "t2s_wg_endfold_weights_h16", "t2s_wg_upsample_squeeze_h16",
                          "t2s_wg_start_h16", "t2s_wg_in_cond_gate_fold_h16", "t2s_wg_res_only_h16"])
    lib = _lib.load()
    for n in h16:
        partner = n[:-4]
        assert partner in decl and decl[n] == decl[partner], n
        assert n in _lib.SIGNATURES and _lib.SIGNATURES[n] == _lib.SIGNATURES[partner], n
        assert getattr(lib, n).argtypes == getattr(lib, partner).argtypes
    assert lib.t2s_abi_version() == 4
