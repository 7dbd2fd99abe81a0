"""tests/warp_ref.py (the numpy restatement of the time warp and the symbol spans, include/t2s_hip.h) against np.interp in float64 and
on hand-built cases; text2speech_amd/rate.py's host integers against it.  No device."""
import numpy as np
import pytest

import warp_ref as W
from text2speech_amd import rate as RT

Q = W.Q


def _warp(x, stretch, length=None, cap=None):
    x = np.atleast_2d(np.asarray(x))
    F = x.shape[1]
    length = F if length is None else length
    c, n = W.cum_map(stretch, F, length, cap)
    out, exact, _ = W.warp_entry(x, c, min(max(length, 0), F), n, cap or max(n, 1))
    return c, n, out, exact


@pytest.mark.parametrize("seed", range(4))
def test_it_is_np_interp_at_the_frame_centres(seed):
    rng = np.random.RandomState(seed)
    F = int(rng.randint(2, 400))
    x = rng.uniform(-1, 1, (3, F)).astype(np.float32)
    s = np.rint(Q / rng.uniform(1 / 8, 8, F)).astype(np.int64)
    c, n, out, exact = _warp(x, s)
    centres = (c[:-1] + c[1:]).astype(np.float64) / (2.0 * Q)
    j = np.arange(n) + 0.5
    worst = 0.0
    for ch in range(3):
        want = np.interp(j, centres, x[ch].astype(np.float64))
        worst = max(worst, float(np.abs(exact[ch] - want).max()))
        assert np.abs(out[ch, :n].astype(np.float64) - want).max() <= 2.0 ** -24 + 1e-12
    print("restatement vs np.interp, F = %d, %d output frames: worst %.3g in float64" % (F, n, worst))
    assert worst <= 1e-12
    assert n == max(1, (int(s.sum()) + Q // 2) >> 20)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_rate_one_is_the_identity_bit_for_bit(dtype):
    x = np.random.RandomState(1).uniform(-4, 4, (2, 57)).astype(dtype)
    x[0, 3], x[1, 9] = np.nan, -0.0
    c, n, out, _ = _warp(x, W.stretch_q(1.0))
    assert W.stretch_q(1.0) == Q and n == 57 and c.tolist() == [f * Q for f in range(58)]
    assert out.tobytes() == x.tobytes()


def test_half_rate_on_a_ramp():
    x = np.arange(10, dtype=np.float32)
    c, n, out, _ = _warp(x, W.stretch_q(0.5))
    assert n == 20 and W.stretch_q(0.5) == 2 * Q
    # output centre j + 0.5 lies at source coordinate (j + 0.5) 0.5 - 0.5, clamped to the ramp's ends
    want = np.clip((np.arange(20) + 0.5) * 0.5 - 0.5, 0, 9).astype(np.float32)
    assert out[0].tolist() == want.tolist()


@pytest.mark.parametrize("rate", [0.5, 0.8, 1.25, 2.0])
def test_uniform_rate_gives_the_linear_coordinate(rate):
    F = 200
    c, n = W.cum_map(W.stretch_q(rate), F, F)
    f, a = W.coords(c, F, n)
    r = Q / W.stretch_q(rate)
    want = np.clip((np.arange(n) + 0.5) * r - 0.5, 0, F - 1)
    assert np.abs(f + a - want).max() < 1e-9


def test_a_single_frame_and_a_zero_length_entry():
    x = np.array([[2.5, np.nan, 1e4]], dtype=np.float32)
    c, n, out, _ = _warp(x, W.stretch_q(0.5), length=1, cap=4)
    assert n == 2 and out[0].tolist() == [2.5, 2.5, 0.0, 0.0]
    c, n, out, _ = _warp(x, W.stretch_q(2.0), length=1, cap=4)
    assert n == 1 and out[0].tolist() == [2.5, 0.0, 0.0, 0.0]                  # never below one frame
    c, n, out, _ = _warp(x, W.stretch_q(0.5), length=0, cap=4)
    assert n == 0 and c.tolist() == [0, 0, 0, 0] and out[0].tolist() == [0.0] * 4
    c, n, out, _ = _warp(x, W.stretch_q(0.5), length=-3, cap=4)
    assert n == 0


def test_cap_cuts_the_length_and_the_map_repeats_behind_the_entry():
    c, n = W.cum_map(2 * Q, 6, 4, cap=5)
    assert n == 5 and c.tolist() == [0, 2 * Q, 4 * Q, 6 * Q, 8 * Q, 8 * Q, 8 * Q]
    assert W.cum_map(2 * Q, 6, 4, cap=100)[1] == 8 and W.cum_map(2 * Q, 6, 9)[1] == 12


def test_p_exactly_on_a_centre_copies_the_frame():
    """stretches 1, 3, 1 (units of Q): the doubled centres are 1, 5, 9 Q, the output's 1, 3, 5, 7, 9 Q - frames 0, 2 and 4 fall on a
    centre (a = 0: the right neighbour, a NaN here for the last, is not read), 1 and 3 lie half-way"""
    x = np.array([[1.0, 3.0, 7.0, np.nan]], dtype=np.float32)
    s = [Q, 3 * Q, Q, Q]
    c, n, out, _ = _warp(x, s, length=3)
    assert n == 5
    f, a = W.coords(c, 3, n)
    assert f.tolist() == [0, 0, 1, 1, 2] and a.tolist() == [0.0, 0.5, 0.0, 0.5, 0.0]
    assert out[0].tolist() == [1.0, 2.0, 3.0, 5.0, 7.0]


def test_symbol_stretches_clamp_and_fall_back_to_rate_one():
    table = np.array([1.0, 0.25, 4.0, np.nan, np.inf, -np.inf, 0.0, -3.0, 1.25, 0.8], dtype=np.float32)
    path = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1, 10, 2 ** 31 - 1]
    s = W.symbol_stretches(path, table, in_len=9)
    half, twice = W.stretch_q(2.0), W.stretch_q(0.5)
    assert s.tolist() == [Q, twice, half, Q, half, twice, twice, twice, W.stretch_q(np.float32(1.25)), Q, Q, Q, Q]
    assert W.symbol_stretches([0, 1], table, in_len=0).tolist() == [Q, Q]           # S = clamp(0, 1, T_in) = 1: symbol 1 is outside


def test_spans_on_a_monotone_path_abut():
    path = [0, 0, 1, 1, 1, 2, 3, 3, -1, -1]
    s = W.symbol_stretches(path, np.array([1.0, 0.5, 2.0, 0.8], dtype=np.float32), 4)
    c, n = W.cum_map(s, 10, 8)
    fl = W.first_last(path, 8, 4, 5)
    assert fl.tolist() == [[0, 1], [2, 4], [5, 5], [6, 7], [-1, -1]]
    sp = W.spans(c, fl, 8, 4, 256)
    assert sp[0, 0] == 0 and sp[3, 1] == (int(c[8]) * 256) >> 20
    assert all(sp[k, 1] == sp[k + 1, 0] for k in range(3)) and sp[4].tolist() == [-1, -1]
    assert sp[:, 1].tolist()[:4] == [512, 512 + 3 * 512, 2048 + 128, 2176 + 2 * 320]
    # trimming, the join's offset and the resampler's ratio, in that order
    sp2 = W.spans(c, fl, 8, 4, 256, trim=(600, 1500), offset=1000, ratio=(15, 14), total=2600)
    want = [[(min(max(u - 600, 0), 1500) + 1000) * 15 // 14 for u in row] for row in sp[:4].tolist()]
    assert sp2[:4].tolist() == [[min(u, 2600) for u in row] for row in want] and sp2[4].tolist() == [-1, -1]
    assert sp2[3, 1] == 2600 and sp2[0, 0] == 1000 * 15 // 14


def test_a_revisited_and_an_uncovered_symbol():
    path = [0, 1, 0, 3, 3, 1]
    fl = W.first_last(path, 6, 4, 4)
    assert fl.tolist() == [[0, 2], [1, 5], [-1, -1], [3, 4]]
    c, _ = W.cum_map(Q, 6, 6)
    sp = W.spans(c, fl, 6, 4, 100)
    assert sp.tolist() == [[0, 300], [100, 600], [-1, -1], [300, 500]]
    assert W.spans(c, fl, 0, 4, 100).tolist() == [[-1, -1]] * 4                # no frame: no span
    assert W.spans(c, fl, 6, 2, 100).tolist() == [[0, 300], [100, 600], [-1, -1], [-1, -1]]    # symbols at or behind S_b


def test_host_integers_of_the_package_are_the_maps():
    assert RT.Q == Q
    for rate in (0.125, 0.5, 0.8, 1.0, 1.1, 1.25, 1.9999, 2.0, 3.3, 8.0):
        assert RT.stretch_q(rate) == W.stretch_q(rate)
        for frames in list(range(0, 40)) + [255, 256, 257, 999, 1000, 65536]:
            c, n = W.cum_map(W.stretch_q(rate), max(frames, 1), frames)
            assert RT.warped_length(frames, rate) == n == W.warped_length(frames, rate), (frames, rate)
    assert RT.warped_length(10, 1.0) == 10 and RT.warped_length(1, 8.0) == 1 and RT.warped_length(0, 0.5) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf"), 0.1, 8.5, "fast", None, True):
        with pytest.raises(ValueError):
            RT.stretch_q(bad)
    with pytest.raises(ValueError):
        RT.warped_length(-1, 1.0)


def test_synthesize_long_refuses_a_bad_speed_before_it_touches_a_model():
    import torch
    from text2speech_amd import longform as L
    t, w = torch.nn.Identity().eval(), torch.nn.Identity().eval()
    for bad in (0.05, 9.0, float("nan"), "fast", [1.0], [1.0, 0.0]):
        with pytest.raises(ValueError, match="speed|rate"):
            L.synthesize_long_timed(t, w, "가. 나.", seed=1, speed=bad)
    import inspect
    plain, timed = inspect.signature(L.synthesize_long).parameters, inspect.signature(L.synthesize_long_timed).parameters
    assert list(timed) == list(plain) + ["speed", "timestamps"]         # one implementation: the same arguments, the same defaults
    assert all(timed[n].default == plain[n].default and timed[n].kind == plain[n].kind for n in plain)
    assert timed["speed"].default is None and timed["timestamps"].default is False
    assert L._check_speed(None, 3) is None and L._check_speed(0.8, 2) == [0.8, 0.8] and L._check_speed([1, 2.0], 2) == [1.0, 2.0]
    assert L.LongFormTimed._fields == L.LongForm._fields + ("spans",)
    assert L.LongFormCheckedTimed._fields == L.LongFormChecked._fields + ("spans",)
