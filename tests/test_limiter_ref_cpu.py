"""tests/limiter_ref.py - the float64 restatement the GPU tests compare csrc/limiter.hip with - pinned without a device: its
envelope against scipy.signal.resample_poly, hand-built cases in closed form, the two guarantees (s <= r, no stored sample over
the ceiling), the preconditions on the seeded inputs that let the GPU tests ask for EQUAL counts, flags and int16 samples, the
window-with-reach property that prepares streaming, and the output's true-peak overshoot (recorded in profiles/limiter_tests.md)."""
import numpy as np
import pytest
from scipy.signal import resample_poly

import limiter_ref as R
from text2speech_amd import audio

C = R.ceiling(R.CEILING_DB)
GAINS = (1.0, 3.0, 8.0)


def test_the_ceiling_is_a_float32_value():
    assert C == float(np.float32(C)) and abs(C - 10.0 ** (-1.0 / 20.0)) < 2.0 ** -24


@pytest.mark.parametrize("os", (2, 4))
def test_the_envelope_sum_is_resample_poly(os):
    gen = np.random.RandomState(os)
    for n in (1, 2, 19, 20, 21, 500):
        u = gen.standard_normal(n)
        p, y = R.envelope(u, os)
        assert np.abs(y - resample_poly(u, os, 1)).max() <= 1e-12
        assert (p >= np.abs(u)).all() and np.array_equal(p, np.maximum(np.abs(u), np.abs(y.reshape(n, os)).max(1)))
    p, y = R.envelope(u, 1)
    assert np.array_equal(p, np.abs(u)) and np.array_equal(y, u)


def test_the_package_uploads_the_same_filter_and_window():
    for os in R.OVERSAMPLES:
        assert np.array_equal(audio.resample_filter(1, os, R.HALF_WIDTH, 5.0)[2], R.interp_filter(os, R.HALF_WIDTH, 5.0))
    for L in R.LOOKAHEADS + (5, 200):
        w = audio.limiter_window(L)
        assert np.array_equal(w, R.window(L)) and w.size == 2 * L + 1
        assert 1.0 <= R.asc_sum(w) <= 1.0 + 2.0 ** -50 and abs(w.sum() - 1.0) < 2.0 ** -50
        k = np.arange(-L, L + 1)
        hann = 0.5 + 0.5 * np.cos(np.pi * k / (L + 1))
        assert np.abs(w - hann / hann.sum()).max() <= 2.0 ** -50


@pytest.mark.parametrize("L", (1, 16, 67))
def test_one_impulse_of_twice_the_ceiling_gives_the_hann_dip(L):
    n, i0 = 6 * L + 40, 3 * L + 17
    x = np.zeros(n)
    x[i0] = 2.0 * C
    ref = R.limit(x, C, L, os=1)
    w = R.window(L)
    want = np.ones(n)
    for d in range(-2 * L, 2 * L + 1):                          # m = 1/2 over i0 +- L: s = 1 - 1/2 (the window's weight inside)
        inside = [k for k in range(-L, L + 1) if abs(d + k) <= L]
        want[i0 + d] = 1.0 - 0.5 * sum(w[k + L] for k in inside)
    assert np.abs(ref.s - want).max() <= 1e-12
    assert ref.s[i0] == 0.5 and ref.s.min() == 0.5 and ref.o[i0] == C
    assert (ref.s[:i0 - 2 * L] == 1.0).all() and (ref.s[i0 + 2 * L + 1:] == 1.0).all()
    assert ref.counts == (1, R.FLAG_LIMITED) and ref.stats[:3] == (2.0 * C, 2.0 * C, 0.5)


@pytest.mark.parametrize("os", R.OVERSAMPLES)
def test_a_row_at_or_below_the_ceiling_comes_back_unchanged(os):
    gen = np.random.RandomState(5)
    x = (0.05 * gen.standard_normal(700)).astype(np.float32)
    if os == 1:
        x[100], x[101] = np.float32(C), -np.float32(C)          # AT the ceiling is not over it
    ref = R.limit(x, C, 67, os)
    assert ref.counts == (0, 0) and ref.stats[2] == 1.0 and (ref.s == 1.0).all()
    assert ref.out.tobytes() == x.tobytes()
    x16 = R.clip(700, 3, "int16", 16) // 4
    ref = R.limit(x16, C, 16, os)
    assert ref.counts == (0, 0) and ref.out.tobytes() == x16.tobytes()


def test_without_look_ahead_the_gain_is_the_required_gain():
    x = R.clip(2049, 11, "float32", 0)
    for os in R.OVERSAMPLES:
        ref = R.limit(x, C, 0, os, g=3.0)
        assert ref.counts[0] > 100 and np.array_equal(ref.s, ref.r)


def test_rows_that_are_empty_or_not_finite():
    ref = R.limit(np.zeros(0, np.float32), C, 16)
    assert ref.stats == (0.0, 0.0, 1.0, 0.0) and ref.counts == (0, 0) and ref.out.size == 0
    x = R.clip(300, 1, "float32", 16)
    x[7] = np.inf
    ref = R.limit(x, C, 16, g=3.0)
    assert ref.stats == (np.inf, np.inf, 1.0, 0.0) and ref.counts == (0, R.FLAG_NONFINITE) and ref.out.tobytes() == x.tobytes()


def _inputs():
    for L in R.LOOKAHEADS:
        for os in R.OVERSAMPLES:
            for kind in R.KINDS:
                for n in R.lengths_for(L):
                    yield L, os, kind, n, R.clip(n, R.seed_of(n, L, os, kind), kind, L)


def test_guarantees_and_preconditions_on_the_seeded_inputs():
    """s <= r and no stored sample over the ceiling, everywhere; and what lets the GPU tests compare for equality: no p within
    1e-9 relative of the ceiling (the count and the flags cannot flip on a rounding) and no int16 reference output within 1e-6
    of a half-integer (rint cannot flip)."""
    closest_p, closest_half, limited = 1.0, 1.0, 0
    top16 = np.rint(32768.0 * C)
    for L, os, kind, n, x in _inputs():
        for g in GAINS:
            ref = R.reference(x, C, L, os, g)
            if n == 0:
                continue
            assert (ref.s <= ref.r).all() and (ref.s > 0).all()
            closest_p = min(closest_p, float(np.abs(ref.p / C - 1.0).min()))
            limited += ref.counts[0]
            if kind == "int16":
                assert np.abs(ref.out.astype(np.int64)).max() <= top16
                v = 32768.0 * ref.o
                closest_half = min(closest_half, float(np.abs(v - np.floor(v) - 0.5).min()))
            else:
                assert ref.out.dtype == np.float32 and np.abs(ref.out).max() <= np.float32(C)
    print("LIMITER inputs: closest p to the ceiling %.3e relative, closest int16 output to a half-integer %.3e, %d limited samples"
          % (closest_p, closest_half, limited))
    assert closest_p > 1e-9 and closest_half > 1e-6 and limited > 100000


def test_the_true_peak_of_the_output_is_recorded_not_promised():
    """max p(o) / c, p metered at 4 x whatever the limiter oversampled by.  Nothing bounds it by construction; what the float64
    restatement gives on the 2 T + 1 rows is printed for profiles/limiter_tests.md.  What IS asserted is the two facts around it:
    the sample peak never exceeds the ceiling, and a limiter that does not oversample leaves a true peak far above it."""
    worst = {}
    for L in R.LOOKAHEADS:
        for os in R.OVERSAMPLES:
            n = 2 * R.TILE + 1
            x = R.clip(n, R.seed_of(n, L, os, "float32"), "float32", L)
            for g in GAINS:
                ref = R.reference(x, C, L, os, g)
                out = ref.out.astype(np.float64)
                assert np.abs(out).max() <= C
                worst[(os, L)] = max(worst.get((os, L), 0.0), float(R.envelope(out, 4)[0].max()) / C)
    for (os, L), v in sorted(worst.items()):
        print("LIMITER overshoot os %d L %4d: true peak of the output / ceiling = %.6f" % (os, L, v))
    assert min(worst[(1, L)] for L in R.LOOKAHEADS) > 1.05
    assert all(worst[(4, L)] < worst[(1, L)] for L in R.LOOKAHEADS if L >= 16)   # (an instant gain change, L <= 1, is a clipper)


@pytest.mark.parametrize("os", R.OVERSAMPLES)
@pytest.mark.parametrize("L", (0, 1, 16, 67))
def test_a_window_with_reach_gives_the_rows_own_samples(L, os):
    """o[i] depends on x over [i - R, i + R], R = 2 L + half_width: limiting x[a - R : b + R] with the same explicit gain gives
    limit(x)[a : b] exactly - and with R - 1 it does not, on this input (the sample at b + R - 1 carries the row's largest value and
    enters the row's largest inter-sample peak, which sets m over its reach)."""
    reach = 2 * L + R.HALF_WIDTH
    n, a, b = 3000, 1100, 1500
    x = R.clip(n, 77 + L, "float32", L).astype(np.float64)
    x[b + reach - 1] = 0.999
    i = b - 1 + 2 * L                                           # the last sample whose r reaches o[b - 1]: two equal samples, so that
    x[i] = x[i + 1] = 0.99                                      # p[i] is the value BETWEEN them, which the filter forms from i +- hw
    g = 3.0
    whole = R.limit(x, C, L, os, g=g)
    part = R.limit(x[a - reach:b + reach], C, L, os, g=g)
    assert np.array_equal(part.o[reach:reach + b - a], whole.o[a:b]) and np.array_equal(part.s[reach:reach + b - a], whole.s[a:b])
    short = R.limit(x[a - reach + 1:b + reach - 1], C, L, os, g=g)
    if os > 1:
        assert not np.array_equal(short.o[reach - 1:reach - 1 + b - a], whole.o[a:b]), "R - 1 was enough"
