"""audio.Limiter without a device: every constructor argument it refuses and every audio / lengths / gain shape or type that
limit_batch and true_peak_batch refuse, with their messages; what it derives from its arguments; and that nothing on this path
falls back to a CPU computation."""
import numpy as np
import pytest
import torch

from text2speech_amd import _lib, audio, longform
from text2speech_amd.data import PcmPool

T2SError = _lib.T2SError


def test_derived_attributes():
    lim = audio.Limiter(44800)
    assert (lim.sampling_rate, lim.lookahead, lim.oversample, lim.half_width, lim.reach, lim.n_taps) == (44800, 67, 4, 10, 144, 81)
    assert lim.ceiling == float(np.float32(10.0 ** (-1.0 / 20.0))) and lim.ceiling_db == -1.0
    assert audio.Limiter(48000, -2.0, 0.0, 1, 3).reach == 3 and audio.Limiter(48000, lookahead_ms=0).lookahead == 0
    assert audio.Limiter(8000, lookahead_ms=1.5).lookahead == 12 and audio.Limiter(48000, lookahead_ms=21.3).lookahead == 1022
    assert audio.Limiter(44100, ceiling_db=0).ceiling == 1.0
    assert (audio.LIMIT_FLAG_LIMITED, audio.LIMIT_FLAG_NONFINITE, audio.LIMIT_MAX_LOOKAHEAD) == (1, 8, 1024)
    assert audio.LimiterReport._fields == ("true_peak", "sample_peak", "min_gain", "limited", "flags")
    for name in ("Limiter", "LimiterReport", "LIMIT_FLAG_LIMITED", "LIMIT_FLAG_NONFINITE", "LIMIT_MAX_LOOKAHEAD"):
        assert name in audio.__all__


@pytest.mark.parametrize("kw,message", [
    (dict(sampling_rate=0), "sampling_rate must be a positive integer"),
    (dict(sampling_rate=-8000), "sampling_rate must be a positive integer"),
    (dict(sampling_rate=44100.5), "sampling_rate must be a positive integer"),
    (dict(sampling_rate=True), "sampling_rate must be a positive integer"),
    (dict(sampling_rate="48k"), "sampling_rate must be a positive integer"),
    (dict(sampling_rate=None), "sampling_rate must be a positive integer"),
    (dict(ceiling_db=0.5), "ceiling_db must be finite and at most 0"),
    (dict(ceiling_db=float("nan")), "ceiling_db must be finite and at most 0"),
    (dict(ceiling_db=-float("inf")), "ceiling_db must be finite and at most 0"),
    (dict(ceiling_db="-1"), "ceiling_db must be finite and at most 0"),
    (dict(ceiling_db=None), "ceiling_db must be finite and at most 0"),
    (dict(ceiling_db=-2000.0), "gives a ceiling of 0 in float32"),
    (dict(lookahead_ms=-0.1), "lookahead_ms must be finite and not negative"),
    (dict(lookahead_ms=float("inf")), "lookahead_ms must be finite and not negative"),
    (dict(lookahead_ms=float("nan")), "lookahead_ms must be finite and not negative"),
    (dict(lookahead_ms=None), "lookahead_ms must be finite and not negative"),
    (dict(lookahead_ms=23.0), "is 1030 samples at 44800 Hz, the most is 1024"),
    (dict(oversample=0), "oversample must be 1, 2 or 4"),
    (dict(oversample=3), "oversample must be 1, 2 or 4"),
    (dict(oversample=8), "oversample must be 1, 2 or 4"),
    (dict(oversample=True), "oversample must be 1, 2 or 4"),
    (dict(oversample="4"), "oversample must be 1, 2 or 4"),
    (dict(half_width=0), "half_width must be an integer in \\[1, 32\\]"),
    (dict(half_width=33), "half_width must be an integer in \\[1, 32\\]"),
    (dict(half_width=10.0), "half_width must be an integer in \\[1, 32\\]"),
    (dict(half_width=True), "half_width must be an integer in \\[1, 32\\]"),
    (dict(beta=-1.0), "beta must be finite and not negative"),
    (dict(beta=float("nan")), "beta must be finite and not negative"),
    (dict(beta=None), "beta must be finite and not negative"),
    (dict(device="cpu"), "there is no CPU path"),
])
def test_refused_constructor_arguments(kw, message):
    args = dict(sampling_rate=44800)
    args.update(kw)
    with pytest.raises(T2SError, match=message):
        audio.Limiter(**args)


X = torch.zeros(3, 100)


@pytest.mark.parametrize("args,message", [
    ((np.zeros((3, 100), np.float32),), "audio must be a tensor, got a ndarray"),
    (([0.0, 0.1],), "audio must be a tensor, got a list"),
    ((torch.zeros(()),), "audio must be \\[N\\], \\[B, N\\] or \\[B, 1, N\\] and hold samples, got \\(\\)"),
    ((torch.zeros(2, 2, 100),), "audio must be \\[N\\], \\[B, N\\] or \\[B, 1, N\\] and hold samples, got \\(2, 2, 100\\)"),
    ((torch.zeros(2, 1, 1, 100),), "audio must be \\[N\\], \\[B, N\\] or \\[B, 1, N\\]"),
    ((torch.zeros(3, 0),), "audio must be \\[N\\], \\[B, N\\] or \\[B, 1, N\\] and hold samples, got \\(3, 0\\)"),
    ((torch.zeros(3, 100, dtype=torch.float64),), "expected float32 or float16, got torch.float64"),
    ((torch.zeros(3, 100, dtype=torch.int16),), "expected float32 or float16, got torch.int16 \\(int16 pools go through PcmPool.limit\\)"),
    ((torch.zeros(3, 100, dtype=torch.bfloat16),), "expected float32 or float16, got torch.bfloat16"),
    ((torch.zeros(65536, 1),), "65536 rows, the most is 65535"),
    ((X, [100, 100]), "lengths has shape \\(2,\\), the batch holds 3 entries"),
    ((X, torch.tensor([[100, 100, 100]])), "lengths has shape \\(1, 3\\), the batch holds 3 entries"),
    ((X, 100), "lengths has shape \\(\\), the batch holds 3 entries"),
    ((X, [100.0, 50.0, 3.0]), "lengths must be integers, got torch.float32"),
    ((X, torch.tensor([True, False, True])), "lengths must be integers, got torch.bool"),
    ((X, ["a", "b", "c"]), "lengths must be a tensor or a sequence of integers"),
    ((X, None, [1.0, 1.0, 1.0]), "gain must be None or a float64 tensor in HBM .* got a list"),
    ((X, None, 2.0), "gain must be None or a float64 tensor in HBM .* got a float"),
    ((X, None, torch.ones(3)), "gain must be None or a float64 tensor in HBM .* got torch.float32"),
    ((X, None, torch.ones(2, dtype=torch.float64)), "gain has shape \\(2,\\), the batch holds 3 entries"),
    ((X, None, torch.ones(3, 1, dtype=torch.float64)), "gain has shape \\(3, 1\\), the batch holds 3 entries"),
    ((torch.zeros(100), None, torch.ones(2, dtype=torch.float64)), "gain has shape \\(2,\\), the batch holds 1 entries"),
])
def test_refused_batches(args, message):
    lim = audio.Limiter(44800)
    with pytest.raises(T2SError, match="Limiter.limit_batch: " + message):
        lim.limit_batch(*args)
    with pytest.raises(T2SError, match="Limiter.true_peak_batch: " + message):
        lim.true_peak_batch(*args)


def test_there_is_no_cpu_path():
    lim = audio.Limiter(44800)
    for call in (lambda: lim.limit_batch(X), lambda: lim.true_peak_batch(X, [100, 50, 3]), lambda: lim(X), lambda: lim.forward(X[0]),
                 lambda: lim.limit_batch(X, None, torch.ones(3, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="expected a tensor in HBM \\(cuda\\); there is no CPU path"):
            call()
    assert lim._tables is None, "nothing was uploaded"


def test_the_stages_around_it_refuse_what_is_not_a_limiter():
    ld = audio.Loudness(44800)
    with pytest.raises(T2SError, match="Loudness.normalize_limit_batch: limiter must be an audio.Limiter, got a Loudness"):
        ld.normalize_limit_batch(X, None, ld)
    with pytest.raises(T2SError, match="the limiter is built for 48000 Hz, this Loudness for 44800"):
        ld.normalize_limit_batch(X, None, audio.Limiter(48000))
    with pytest.raises(T2SError, match="limit_long: expected a LongForm result"):
        longform.limit_long((X, 3), audio.Limiter(44800))
    r = longform.LongForm(torch.zeros(1, 100, dtype=torch.int16), None, None, ["a"], None)
    with pytest.raises(T2SError, match="limit_long: the audio is torch.int16; synthesize with pcm16=False, limit, then audio.to_pcm16"):
        longform.limit_long(r, audio.Limiter(44800))
    assert callable(PcmPool.limit) and callable(PcmPool.true_peak)


def test_the_window_is_a_normalised_hann_whose_running_sum_reaches_one():
    for L in (0, 1, 2, 12, 67, 72, 1024):
        w = audio.limiter_window(L)
        acc = 0.0
        for v in w:
            acc += float(v)
        assert w.dtype == np.float64 and w.size == 2 * L + 1 and 1.0 <= acc <= 1.0 + 2.0 ** -50
        assert np.array_equal(w[:L], w[:L:-1][:L]) and (w > 0).all() and w.argmax() == L
