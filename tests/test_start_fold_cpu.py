"""WN.start folded into the first gate GEMM of a flow, the algebra on the CPU in f64: the composed weight
applied to the window (audio taps + the ones-channel) against the oracle's layer-0 pre-activation in_layers[0](start(a)), on the
seeded small-model weights the golden vectors were made with.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import waveglow_oracle as O
from text2speech_amd import _lib, planes, synth


def _layer0_preact_oracle(sd, cfg, k, a):
    """oracle.waveglow_oracle.wn_forward's first two statements (reference glow.py:156,159) in the dtype of `a`"""
    ks = cfg["WN_config"]["kernel_size"]
    p = "WN.%d." % k
    x = F.conv1d(a, O.effective_weight(sd, p + "start"), sd[p + "start.bias"])
    return F.conv1d(x, O.effective_weight(sd, p + "in_layers.0"), sd[p + "in_layers.0.bias"], dilation=1, padding=(ks - 1) // 2)


@pytest.mark.parametrize("k,n_half", [(0, 4), (5, 3), (11, 2)])
@pytest.mark.parametrize("L", [1, 2, 257])
def test_composed_layer0_is_exact_in_f64(k, n_half, L):
    """Every time step, t = 0 and t = L - 1 included (where a tap of the ones-channel falls into the zero padding and b_start must
    NOT be counted for it), for flows with n_half = 4, 3 and 2.  Bar: both sides are f64 sums of the same ks * C * (n_half + 1) <= 960
    products in different association orders; each is within n * eps * sum |terms| of the exact value (eps = 1.1e-16, n <= 960,
    sum |terms| < 50 for these weights and |a| < 5), i.e. 5e-12 - asserted at 1e-11."""
    cfg = synth.WAVEGLOW_SMALL
    assert O._flow_sizes(cfg)[k][1] == n_half
    sd = {n: t.double() for n, t in synth.waveglow_state(cfg).items()}
    gen = torch.Generator().manual_seed(100 * k + L)
    a = torch.randn(2, n_half, L, generator=gen, dtype=torch.float64)
    want = _layer0_preact_oracle(sd, cfg, k, a)
    p = "WN.%d." % k
    ks = cfg["WN_config"]["kernel_size"]
    M = planes.start_fold_matrix(O.effective_weight(sd, p + "in_layers.0"), O.effective_weight(sd, p + "start"), sd[p + "start.bias"])
    win = planes.start_window(a, ks)
    assert M.shape == (2 * cfg["WN_config"]["n_channels"], ks * (n_half + 1)) and win.shape == (2, ks * (n_half + 1), L)
    got = torch.einsum("mk,bkt->bmt", M, win) + sd[p + "in_layers.0.bias"].view(1, -1, 1)
    err = float((got - want).abs().max())
    print("flow %d (n_half %d), L %d: max abs error %.2e (pre-activation max %.2f)" % (k, n_half, L, err, float(want.abs().max())))
    assert err < 1e-11
    # the edges really differ from the interior: without the ones-channel's zero taps t = 0 would be off by W_in0[tap 0] . b_start
    if L > 2:
        all_ones = win.clone()
        all_ones[:, [tap * (n_half + 1) + n_half for tap in range(ks)]] = 1.0
        naive = torch.einsum("mk,bkt->bmt", M, all_ones) + sd[p + "in_layers.0.bias"].view(1, -1, 1)
        assert float((naive - want)[:, :, 1:-1].abs().max()) < 1e-11 and float((naive - want)[:, :, 0].abs().max()) > 1e-4


def test_window_definition():
    a = torch.arange(1.0, 11.0).view(1, 2, 5)
    w = planes.start_window(a, 3)
    assert w.shape == (1, 9, 5)
    assert w[0, 0].tolist() == [0, 1, 2, 3, 4] and w[0, 3].tolist() == [1, 2, 3, 4, 5] and w[0, 6].tolist() == [2, 3, 4, 5, 0]
    assert w[0, 2].tolist() == [0, 1, 1, 1, 1] and w[0, 5].tolist() == [1, 1, 1, 1, 1] and w[0, 8].tolist() == [1, 1, 1, 1, 0]
    assert w[0, 1].tolist() == [0, 6, 7, 8, 9]


def test_start_fold_switch_and_fallback(monkeypatch):
    """Host logic: on by default for the no-grad path, T2S_START_FOLD=0 and the composed-conditioning opt-in select the unfolded
    layer 0, and a geometry whose taps do not fit a 32-wide K-step (kernel_size 7: 7 * 5 = 35 columns) falls back.  path() is the
    one decision all of it comes from: the same cases on the whole record, the one-launch flow boundary included."""
    from text2speech_amd.glow import WaveGlow
    monkeypatch.delenv("T2S_START_FOLD", raising=False)
    monkeypatch.delenv("T2S_FLOW_BOUNDARY", raising=False)
    monkeypatch.delenv("T2S_COND_COMPOSE", raising=False)
    eng = WaveGlow(**synth.WAVEGLOW_SMALL)._eng()
    assert eng.start_fold_on()
    assert eng.path() == (True, True, None)
    monkeypatch.setenv("T2S_FLOW_BOUNDARY", "0")
    assert eng.path() == (True, False, None)
    monkeypatch.delenv("T2S_FLOW_BOUNDARY")
    monkeypatch.setenv("T2S_START_FOLD", "0")
    assert not eng.start_fold_on()
    assert eng.path() == (False, False, None)
    monkeypatch.setenv("T2S_START_FOLD", "1")
    assert eng.start_fold_on()
    assert eng.path() == (True, True, None)
    monkeypatch.setenv("T2S_COND_COMPOSE", "1")
    assert not eng.start_fold_on()
    assert eng.path() == (False, False, (32, 4, 320))
    monkeypatch.delenv("T2S_COND_COMPOSE")
    cfg7 = dict(synth.WAVEGLOW_SMALL, n_flows=4, WN_config=dict(n_layers=4, n_channels=64, kernel_size=7))
    assert not WaveGlow(**cfg7)._eng().start_fold_on()
    assert WaveGlow(**cfg7)._eng().path() == (False, False, None)
    cfg5 = dict(synth.WAVEGLOW_SMALL, n_flows=4, WN_config=dict(n_layers=4, n_channels=128, kernel_size=5))
    e5 = WaveGlow(**cfg5)._eng()
    assert e5.start_fold_on() and e5.geom()["nwc"] == 4     # 5 * 5 = 25 columns: one column set per window chunk
    assert e5.path() == (True, True, None)
    cfg5["WN_config"]["n_channels"] = 64
    assert not WaveGlow(**cfg5)._eng().start_fold_on()      # ... which needs four channel chunks of start_kernel workgroups
    assert WaveGlow(**cfg5)._eng().path() == (False, False, None)
    assert eng.geom()["nwc"] == 2
    # the one-launch boundary wants the residual rows in the PAIR8 order: C % 32 == 0
    cfg48 = dict(synth.WAVEGLOW_SMALL, n_flows=4, WN_config=dict(n_layers=4, n_channels=48, kernel_size=3))
    assert WaveGlow(**cfg48)._eng().path() == (True, False, None)
    # every no-grad gate GEMM carries the folded WN.end (C % 16 == 0): refused here, by name, not by the first launch
    cfg48["WN_config"]["n_channels"] = 40
    with pytest.raises(_lib.T2SError, match="n_channels % 16"):
        WaveGlow(**cfg48)._eng().path()


@pytest.mark.parametrize("nwc,ncol", [(2, 15), (2, 9), (4, 25)])
def test_four_column_sets_carry_both_factors_to_f32(nwc, ncol):
    """The kernels' arithmetic emulated: per column set the three products hi.hi + hi.lo + lo.hi of the (weight, window) planes,
    summed over the four sets (planes.start_fold_sets), against the exact product of the f32 factors.  Set 0 alone leaves the
    16-bit rounding of both factors (about 2^-17 each); the four sets leave only terms of relative size 2^-24 and below (residual
    times residual or lo, lo times residual) - asserted at 2^-22 of |w||a| per column."""
    gen = torch.Generator().manual_seed(nwc * 100 + ncol)
    w = torch.randn(64, ncol, generator=gen)
    a = torch.randn(ncol, 50, generator=gen)
    wh, wl = planes.start_fold_sets(w, True, nwc, 1)
    ah, al = planes.start_fold_sets(a, False, nwc, 0)
    d = lambda t: t.double()
    got = d(wh) @ d(ah) + d(wh) @ d(al) + d(wl) @ d(ah)
    want = d(w) @ d(a)
    scale = d(w).abs() @ d(a).abs()
    h0, l0 = planes.split_bf16(w)
    b0, c0 = planes.split_bf16(a)
    plain = d(h0) @ d(b0) + d(h0) @ d(c0) + d(l0) @ d(b0)
    e_four, e_plain = float(((got - want).abs() / scale).max()), float(((plain - want).abs() / scale).max())
    print("nwc %d, %d columns: error / sum|w||a|: four sets %.1e, plain split %.1e" % (nwc, ncol, e_four, e_plain))
    assert e_four < 2.0 ** -22 and e_plain > 8 * e_four
