"""Streaming synthesis, the host side (text2speech_amd/streaming.py): the halo formula, the fact it rests on - on the float64 oracle a
window with the exact halo IS the whole call's audio, one with a 2-frame halo is not - and the window schedule.  No GPU."""
import pytest
import torch

import streaming_ref as R
from text2speech_amd import _lib, streaming, synth


def test_vocoder_halo():
    assert streaming.vocoder_halo(synth.WAVEGLOW_SMALL) == (99, 96)
    assert streaming.vocoder_halo(synth.WAVEGLOW_DEFAULT) == (99, 96)
    small = dict(synth.WAVEGLOW_SMALL, n_flows=4, WN_config=dict(n_layers=4, n_channels=64, kernel_size=3))
    assert streaming.vocoder_halo(small) == (5, 2)       # 4 x 15 = 60 columns of 32 per frame -> 2, and 3 frames of the upsampler
    from text2speech_amd.glow import WaveGlow
    assert streaming.vocoder_halo(WaveGlow(**small)) == (5, 2)
    with pytest.raises(_lib.T2SError):
        streaming.vocoder_halo(dict(synth.WAVEGLOW_SMALL, n_group=6))       # 256 % 6


@pytest.fixture(scope="module")
def whole():
    """the stress weights in float64, a mel of 260 frames, one [1, 8, 8320] draw, the oracle's whole run: computed once"""
    torch.set_num_threads(max(1, min(8, torch.get_num_threads())))
    sd = R.double_state(synth.waveglow_state(R.CFG, **R.STRESS))
    gen = torch.Generator().manual_seed(97)
    mel = torch.randn(1, 80, R.F, generator=gen)
    z = torch.randn(1, R.CFG["n_group"], R.cols(R.CFG, R.F), generator=gen)
    return dict(sd=sd, mel=mel, z=z, audio=R.oracle(sd, R.CFG, mel, z))


@pytest.mark.parametrize("f0,f1", R.WINDOWS)
def test_oracle_window_is_the_whole_call(whole, f0, f1):
    """Exact halo: rel-L2 <= 1e-12 against the whole run's slice (measured 0.0 on every window).  Halo (2, 2): > 10 ORACLE_BAR
    (measured >= 3.5e-2), so the project's bar tells a wrong window from a right one."""
    want = whole["audio"][256 * f0:256 * f1]
    exact = R.oracle_window(whole["sd"], R.CFG, whole["mel"], whole["z"], f0, f1, streaming.vocoder_halo(R.CFG))
    short = R.oracle_window(whole["sd"], R.CFG, whole["mel"], whole["z"], f0, f1, (2, 2))
    e_exact, e_short = R.rel(exact, want), R.rel(short, want)
    print("oracle window [%d, %d): exact halo rel %.3e (bit-equal %s), halo (2, 2) rel %.3e max-rel %.3e"
          % (f0, f1, e_exact, bool(torch.equal(exact, want)), e_short, R.maxrel(short, want)))
    assert tuple(exact.shape) == (256 * (f1 - f0),)
    assert e_exact <= 1e-12
    assert e_short > 10 * R.ORACLE_BAR


def _run_plan(F, first, window, halo, step=64):
    """the windows a stream issues while the known frames grow by `step` up to F: [(f0, f1, lo, hi, n_known, end)]"""
    out, start, n = [], 0, 0
    while True:
        n = min(F, n + step)
        end = n == F
        while True:
            w = streaming.plan_windows(first, window, halo, n, end, start)
            if w is None:
                break
            out.append(w + (n, end))
            start = w[1]
        if end:
            return out


@pytest.mark.parametrize("F", [1, 31, 32, 33, 127, 128, 129, 260])
@pytest.mark.parametrize("first,window,halo", [(32, 128, (99, 96)), (16, 64, (99, 96)), (64, 256, (103, 100)), (32, 128, (5, 2)),
                                               (32, 128, (0, 0))])
def test_plan_windows(F, first, window, halo):
    wins = _run_plan(F, first, window, halo)
    assert wins, "no window at all"
    pos = 0
    for f0, f1, lo, hi, n, end in wins:
        assert f0 == pos and f1 > f0, "not in order, or an empty window"          # a partition of [0, F), in order
        pos = f1
        assert 0 <= lo <= max(0, f0 - halo[0]) and lo <= f0             # at least the halo on the left, or the utterance's start
        assert hi <= n, "issued before its last frame was known"
        assert hi >= f1 + halo[1] or (end and hi == F)                  # at least the halo on the right, or the utterance's end
        assert f1 - f0 == (first if f0 == 0 else window) or (end and f1 == F)
    assert pos == F
    lengths = {hi - lo for _, _, lo, hi, _, _ in wins}
    assert len(lengths) <= 3, lengths
    regular = {hi - lo for f0, _, lo, hi, _, end in wins if f0 > 0 and not end}
    assert len(regular) <= 1, regular                                   # the regular windows all have one length
    # nothing is issued twice, and nothing more is issued once the end has been delivered
    assert streaming.plan_windows(first, window, halo, F, True, F) is None


def test_plan_windows_waits_and_refuses():
    assert streaming.plan_windows(32, 128, (99, 96), 127) is None               # 32 + 96 = 128 frames decide the first window
    assert streaming.plan_windows(32, 128, (99, 96), 128) == (0, 32, 0, 128)
    assert streaming.plan_windows(32, 128, (99, 96), 300, False, 32) is None    # a regular region is 323 frames long
    assert streaming.plan_windows(32, 128, (99, 96), 323, False, 32) == (32, 160, 0, 323)
    assert streaming.plan_windows(32, 128, (99, 96), 1000, False, 160) == (160, 288, 61, 384)
    assert streaming.plan_windows(32, 128, (99, 96), 300, True, 160) == (160, 288, 0, 300)
    assert streaming.plan_windows(32, 128, (99, 96), 1000, True, 928) == (928, 1000, 677, 1000)
    with pytest.raises(ValueError):
        streaming.plan_windows(0, 128, (99, 96), 10)
    with pytest.raises(ValueError):
        streaming.plan_windows(32, 128, (-1, 96), 10)
