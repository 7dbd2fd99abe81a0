"""tests/wg_fwd_util.py's expectations against the oracle, in float64 on the CPU: the per-layer pieces the GPU file
(tests/test_waveglow_fwd_kernels_gpu.py) compares kernels with must add up to what oracle.waveglow_oracle.wn_forward returns."""
import pytest
import torch

import wg_fwd_util as W
from oracle import waveglow_oracle as O

# (B, C, n_layers, kernel size, n_half, n_cond, L)
CONFIGS = [(2, 16, 3, 3, 4, 32, 37), (1, 48, 4, 5, 3, 40, 70)]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module", params=CONFIGS, ids=["C16-k3", "C48-k5"])
def case(request):
    B, C, nl, ks, nh, n_cond, L = request.param
    sd = W.wn_state(C, nl, ks, nh, n_cond, seed=C + ks)
    cfg = W.wn_cfg(C, nl, ks)
    audio, spect = W.wn_inputs(B, nh, n_cond, L, seed=L)
    assert audio.dtype == torch.float64 and all(v.dtype == torch.float64 for v in sd.values())
    layers, out = W.layer_expect(sd, cfg, audio, spect)
    return sd, cfg, audio, spect, layers, out


def test_fold_terms_sum_to_wn_end(case):
    """sum_i (F_i . acts_i + bes_i) + b_end is wn_forward's output, to 1e-12 relative"""
    sd, cfg, audio, spect, layers, out = case
    got = sum(ly["fold"] + ly["bes"][None, :, None] for ly in layers) + sd["WN.0.end.bias"][None, :, None]
    assert torch.equal(out, O.wn_forward(sd, cfg, 0, audio, spect))
    assert float(out.abs().max()) > 0.0
    assert _rel(got, out) < 1e-12, _rel(got, out)


def test_residual_chain_is_the_oracles_taps(case):
    """x_{i+1} = x_i + W_res,i . acts_i + b_res,i, chained from x_0 = WN.start's output, is the oracle's tap of every layer but the
    last (which has no residual half: its tap repeats x), to 1e-12 relative; layer_expect's x_i is that chain's input"""
    sd, cfg, audio, spect, layers, out = case
    C, nl = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    taps = []
    O.wn_forward(sd, cfg, 0, audio, spect, taps=taps)
    x = torch.einsum("cj,bjt->bct", W.eff(sd, "start")[:, :, 0], audio) + sd["WN.0.start.bias"][None, :, None]
    for i in range(nl):
        assert _rel(layers[i]["x"], x) < 1e-12, i
        assert torch.equal(layers[i]["acts"], taps[i][0]) and torch.equal(layers[i]["x_next"], taps[i][1])
        if i < nl - 1:
            w = W.eff(sd, "res_skip_layers.%d" % i)[:C, :, 0]
            x = x + torch.einsum("oc,bct->bot", w, layers[i]["acts"]) + sd["WN.0.res_skip_layers.%d.bias" % i][:C][None, :, None]
        assert _rel(x, taps[i][1]) < 1e-12, i


def test_layouts_and_rounding():
    """_gate_row is a permutation of the 2C rows into the padded tile rows; plane_round is what planes.to_planes stores"""
    from text2speech_amd import planes
    for C in (16, 80, 144, 512):
        rows = W._gate_row(torch.arange(2 * C), C)
        assert rows.unique().numel() == 2 * C and int(rows.max()) < -(-C // 128) * 256
    x = torch.randn(2, 40, 7, generator=torch.Generator().manual_seed(1)).double()
    hi, lo = planes.to_planes(x.float(), 4, 16)
    got = planes.from_planes(hi, lo, 40, 7, 4).double()
    assert torch.equal(got, W.plane_round(x))
    assert float((got - x).abs().max()) < 2.0 ** -15 * float(x.abs().max())


def test_n_cond_zero_adds_nothing():
    """the stand-in conditioning of an n_cond = 0 state (one zero-fed channel, zero bias) contributes exactly zero"""
    sd = W.wn_state(16, 2, 1, 4, 0, seed=5)
    audio, spect = W.wn_inputs(2, 4, 0, 9, seed=6)
    assert float(spect.abs().max()) == 0.0 and spect.size(1) == 1
    for i in range(2):
        assert float(sd["WN.0.cond_layers.%d.bias" % i].abs().max()) == 0.0
    layers, _ = W.layer_expect(sd, W.wn_cfg(16, 2, 1), audio, spect)
    s = torch.einsum("oc,bct->bot", W.eff(sd, "in_layers.0")[:, :, 0], layers[0]["x"]) + sd["WN.0.in_layers.0.bias"][None, :, None]
    want = torch.tanh(s[:, :16]) * torch.sigmoid(s[:, 16:])
    assert _rel(layers[0]["acts"], want) < 1e-12
