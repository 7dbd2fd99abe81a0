"""WaveGlow.infer of a .half() model on fp16 planes with one-plane weights (engine switch infer_w16, the _h16 entry points) against
the float64 oracle, next to the split-bf16 path it leaves unchanged.

Models: the 12-flow, 8-layer small configuration at C = 64 (128-row gate tiles at these lengths) and C = 80 (256-row ping-pong
tiles), .half() with the 1x1 convolutions put back to float as the reference's inference script does.  Shapes: 12 frames at
B = 1 and 5 frames at B = 2, seeded noise, sigma 0.666.  The mels are f32 tensors, so the audio comes back in f32.

Yardsticks:
  infer_w16 = True    the oracle on the fp16-ROUNDED EFFECTIVE weights of every in / cond / res_skip convolution (computed in f32
                      from the half-rounded weight_v / weight_g, rounded to fp16, handed to the oracle as plain `.weight` keys),
                      at the project's audio bars (tests/test_e2e_gpu.py): < 1e-3 norm-relative, < 2e-3 max-relative
  infer_w16 = False   the oracle on the half-rounded parameters, < 2e-3: the existing yardstick of a .half() model
  True against False  < 2e-3.  On the CPU, in exact arithmetic, rounding the effective weights moves the audio by 1.2e-4 norm /
                      1.0e-4 max (C = 64, 40 frames) and 2.2e-4 / 2.8e-4 (C = 256, 24 frames); the figure measured here is
                      printed next to those."""
import functools

import pytest
import torch

from oracle import waveglow_oracle as WO
from text2speech_amd import _lib, glow, synth
from text2speech_amd.glow import WaveGlow

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA = 0.666
SHAPES = [(1, 12), (2, 5)]          # (B, frames)


def _cfg(C):
    return dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2,
                WN_config=dict(n_layers=8, n_channels=C, kernel_size=3))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _half_rounded(sd):
    """what .half() leaves of the parameters, as f32; the 1x1 convolutions stay float (reference inference.py:73-74)"""
    return {k: (v if "convinv" in k else v.half().float()) for k, v in sd.items()}


def _w16_state(sd_h):
    """sd_h with every in / cond / res_skip convolution as a plain `.weight`: the f32 effective weight rounded to fp16"""
    out = {}
    for k, v in sd_h.items():
        layer = any(s in k for s in ("in_layers", "cond_layers", "res_skip_layers"))
        if layer and k.endswith(".weight_g"):
            continue
        if layer and k.endswith(".weight_v"):
            prefix = k[:-len(".weight_v")]
            out[prefix + ".weight"] = WO.effective_weight(sd_h, prefix).half().float()
        else:
            out[k] = v
    return out


@functools.lru_cache(maxsize=None)
def _inputs(B, frames):
    gen = torch.Generator().manual_seed(100 * B + frames)
    L = frames * 256 // 8
    mel = torch.randn(B, 80, frames, generator=gen)
    nf = torch.randn(B, 4, L, generator=gen)
    ne = tuple(torch.randn(B, 2, L, generator=gen) for _ in range(2))
    return mel, nf, ne


@functools.lru_cache(maxsize=None)
def _oracles(C, B, frames):
    """(audio of the oracle on the fp16-rounded effective weights, on the half-rounded parameters): float64, computed once"""
    cfg = _cfg(C)
    sd_h = _half_rounded(synth.waveglow_state(cfg))
    mel, nf, ne = _inputs(B, frames)
    d = lambda sd: {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        a16 = WO.waveglow_infer(d(_w16_state(sd_h)), cfg, mel.double(), nf.double(), [t.double() for t in ne], sigma=SIGMA)
        ah = WO.waveglow_infer(d(sd_h), cfg, mel.double(), nf.double(), [t.double() for t in ne], sigma=SIGMA)
    return a16, ah


def _model(C, half=True):
    cfg = _cfg(C)
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg))
    m = m.to(DEV).eval()
    if half:
        m.half()
        for c in m.convinv:
            c.float()
    return m


@functools.lru_cache(maxsize=None)
def _half_model(C):
    return _model(C)


def _infer(m, B, frames, w16):
    mel, nf, ne = _inputs(B, frames)
    m._eng().infer_w16 = w16
    try:
        out = m.infer(mel.to(DEV), sigma=SIGMA, noise=(nf, list(ne)))
    finally:
        m._eng().infer_w16 = None
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,frames", SHAPES)
@pytest.mark.parametrize("C,tile", [(64, 128), (80, 256)])
def test_half_model_parity_and_the_two_paths(C, tile, B, frames):
    _lib.load()
    L = frames * 256 // 8
    assert _lib.load().t2s_wg_gate_tile_rows(B, C, L) == tile
    m = _half_model(C)
    eng = m._eng()
    a16_o, ah_o = _oracles(C, B, frames)
    # the fp16 chain against the oracle on the fp16-rounded effective weights
    a16 = _infer(m, B, frames, True)
    assert eng.last_infer_w16 is True and eng.last_path == (False, False, None)
    assert a16.dtype == torch.float32 and tuple(a16.shape) == (B, frames * 256) and bool(torch.isfinite(a16).all())
    n, mx = _rel(a16, a16_o), _maxrel(a16, a16_o)
    print("PARITY infer_w16=True  C%d B%d %d frames vs oracle(fp16 effective weights)  norm-rel %.3e  max-rel %.3e" % (C, B, frames, n, mx))
    # the split-bf16 path of the same model against the existing yardstick
    abf = _infer(m, B, frames, False)
    assert eng.last_infer_w16 is False
    nb = _rel(abf, ah_o)
    print("PARITY infer_w16=False C%d B%d %d frames vs oracle(half parameters)         norm-rel %.3e  max-rel %.3e" % (C, B, frames, nb, _maxrel(abf, ah_o)))
    # None: what the measured default selects (text2speech_amd/glow.py, _INFER_W16_AUTO), bit for bit that path's result
    a_none = _infer(m, B, frames, None)
    assert eng.last_infer_w16 is glow._INFER_W16_AUTO and torch.equal(a_none, a16 if glow._INFER_W16_AUTO else abf)
    # the two paths against each other
    nd, md = _rel(a16, abf), _maxrel(a16, abf)
    print("PATHS  infer_w16 True vs False C%d B%d %d frames  norm-rel %.3e  max-rel %.3e   (oracle, fp16-rounded vs unrounded effective "
          "weights: %.3e / %.3e here; 1.2e-4 / 1.0e-4 at C = 64, 40 frames; 2.2e-4 / 2.8e-4 at C = 256, 24 frames)"
          % (C, B, frames, nd, md, _rel(a16_o, ah_o), _maxrel(a16_o, ah_o)))
    assert n < 1e-3, "fp16 chain: norm-relative %.3e >= 1e-3" % n
    assert mx < 2e-3, "fp16 chain: max-relative %.3e >= 2e-3" % mx
    assert nb < 2e-3, "split-bf16 path of the half model: %.3e >= 2e-3" % nb
    assert nd < 2e-3, "the two paths differ by %.3e >= 2e-3" % nd


def test_float_model_untouched():
    """A float model: None takes today's path and gives the bits False gives; True raises before anything is launched."""
    _lib.load()
    m = _model(64, half=False)
    B, frames = SHAPES[0]
    a_none = _infer(m, B, frames, None)
    assert m._eng().last_infer_w16 is False
    path_none = m._eng().last_path
    a_off = _infer(m, B, frames, False)
    assert m._eng().last_infer_w16 is False and m._eng().last_path == path_none
    assert torch.equal(a_none, a_off)
    with pytest.raises(_lib.T2SError, match="infer_w16 = True"):
        _infer(m, B, frames, True)
    assert m._eng().packed16 is None


def test_infer_batch_excluded():
    """infer_batch of a half model stays on split-bf16: True raises, None equals False bit for bit."""
    _lib.load()
    m = _half_model(64)
    B, frames = 2, 5
    mel, nf, ne = _inputs(B, frames)
    lengths = torch.tensor([5, 3])
    eng = m._eng()

    def run(w16):
        eng.infer_w16 = w16
        try:
            out, lens = m.infer_batch(mel.to(DEV), lengths, sigma=SIGMA, noise=(nf, list(ne)))
        finally:
            eng.infer_w16 = None
        torch.cuda.synchronize()
        return out, lens

    with pytest.raises(_lib.T2SError, match="infer_batch"):
        run(True)
    a_none, l_none = run(None)
    assert eng.last_infer_w16 is False
    a_off, l_off = run(False)
    assert torch.equal(a_none, a_off) and torch.equal(l_none, l_off)


def test_repeated_calls_and_parameter_update():
    """The fp16 operands are packed once per parameter version: a second call gives the same bits, an in-place update of one
    gain changes the result (and the split-bf16 pack cached beside them follows the same key)."""
    _lib.load()
    m = _model(64)
    B, frames = SHAPES[0]
    a1 = _infer(m, B, frames, True)
    pk = m._eng().packed16
    key = m._eng().packed16_key
    a2 = _infer(m, B, frames, True)
    assert torch.equal(a1, a2) and m._eng().packed16 is pk and m._eng().packed16_key == key
    b1 = _infer(m, B, frames, False)              # the other path in between: its own cache, the shared workspace
    a3 = _infer(m, B, frames, True)
    assert torch.equal(a1, a3)
    with torch.no_grad():
        m.WN[3].in_layers[2].weight_g.mul_(1.25)
    a4 = _infer(m, B, frames, True)
    assert m._eng().packed16_key != key
    assert not torch.equal(a1, a4) and bool(torch.isfinite(a4).all())
    b2 = _infer(m, B, frames, False)
    assert not torch.equal(b1, b2)
    assert _rel(a4, b2) < 2e-3
