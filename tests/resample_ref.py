"""Restatement of the sample-rate conversion the library computes (include/t2s_hip.h, t2s_resample_table), vectorised numpy, nothing
from scipy: scipy.signal.resample_poly(x, up, down) at its defaults (window=('kaiser', 5.0), padtype='constant').

    g = gcd(up, down); up //= g; down //= g;  R = max(up, down);  half = 10 R;  n_taps = 2 half + 1
    h[j] = up w[j] sinc((j - half) / R) / R / sum(w sinc / R),   w = numpy.kaiser(n_taps, 5.0)
    n_out = ceil(n_in up / down)
    y[m] = sum_k x[k] h[half + m down - k up]     over 0 <= k < n_in with the tap index inside [0, n_taps)

Products and sums are formed in numpy.longdouble (64-bit mantissa on x86, so its own error is far below one float64 rounding) and
rounded to float64 once.  tests/test_resample_ref_cpu.py compares it with scipy; the GPU tests compare the kernels with it.

The seeded inputs of the GPU tests are defined here (`int16_cases`), so that the CPU test can assert on exactly those inputs that no
reference sample lies within 1e-6 of a half-integer - the int16 comparison on the GPU then needs no exemption."""
import math

import numpy as np

HALF_WIDTH = 10
RATIOS = ((2, 1), (1, 2), (3, 7), (64, 63), (5, 14))        # the ratios of the kernel tests


def filter_ref(up, down, half_width=HALF_WIDTH, beta=5.0):
    """(up, down, h): the reduced ratio and the float64 filter"""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    R = max(up, down)
    half = half_width * R
    j = np.arange(2 * half + 1)
    h = np.kaiser(2 * half + 1, beta) * (1.0 / R) * np.sinc((j - half) / R)
    return up, down, up * h / h.sum()


def out_length(n_in, up, down):
    return -(-n_in * up // down)


def taps_per_output(n_taps, up):
    return -(-n_taps // up)


def resample_ref(x, up, down, h=None, with_magnitude=False):
    """x: 1-D array (any real dtype; its values are taken exactly) -> float64 [ceil(n up / down)]; with_magnitude also returns
    sum_k |x[k]| |h[...]| per output, the scale of the rounding-error bound."""
    if h is None:
        up, down, h = filter_ref(up, down)
    x = np.asarray(x)
    n_in, n_taps = x.size, h.size
    half = n_taps // 2
    n_out = out_length(n_in, up, down)
    c = half + np.arange(n_out, dtype=np.int64) * down           # h's index under sample 0
    p, kc = c % up, c // up                                      # tap p + i up lies under sample kc - i
    i = np.arange(taps_per_output(n_taps, up), dtype=np.int64)[::-1]          # descending i: ascending k
    j = p[:, None] + i[None, :] * up
    k = kc[:, None] - i[None, :]
    ok = (j < n_taps) & (k >= 0) & (k < n_in)
    xs = x.astype(np.longdouble)[np.clip(k, 0, n_in - 1)]
    hs = h.astype(np.longdouble)[np.clip(j, 0, n_taps - 1)]
    prod = np.where(ok, xs * hs, np.longdouble(0))
    y = prod.sum(axis=1).astype(np.float64)
    if with_magnitude:
        return y, np.abs(prod).sum(axis=1).astype(np.float64)
    return y


def to_int16(y):
    """rint (ties to even), saturated, NaN -> 0: what an int16 destination stores"""
    r = np.rint(np.where(np.isnan(y), 0.0, y))
    return np.clip(r, -32768, 32767).astype(np.int16)


def near_half_integer(y, eps=1e-6):
    """count of samples within eps of k + 1/2"""
    f = np.abs(y - np.floor(y) - 0.5)
    return int((f < eps).sum())


def n_in_for(n_out, up, down):
    """the smallest n_in whose output has at least n_out samples (exactly n_out wherever the ratio can give it)"""
    n = max(1, n_out * down // up)
    while out_length(n, up, down) < n_out:
        n += 1
    while n > 1 and out_length(n - 1, up, down) >= n_out:
        n -= 1
    return n


def kernel_lengths(up, down, tile):
    """the input lengths of the kernel tests: 1, 2, one more than the filter's reach, and the tile's edges"""
    up, down, h = filter_ref(up, down)
    half = h.size // 2
    ns = [1, 2, half // up + 1] + [n_in_for(t, up, down) for t in (tile - 1, tile, tile + 1, 2 * tile + 1)]
    return sorted(set(ns))


def clip_int16(seed, n, amplitude=20000):
    """seeded noise, int16 [n]; amplitude 32768 reaches both ends of the range"""
    gen = np.random.RandomState(seed)
    return gen.randint(-amplitude, amplitude, n).astype(np.int16)


def square_wave(n, period=64):
    return np.where((np.arange(n) // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)


POOL_CLIP_LENGTHS = (1, 2, 77, 300, 1501, 33)               # the clips of the pool tests (1501 -> more than one tile at 64 / 63)

# tests/test_resample_gpu.py: a pool at 44100 Hz brought to 44800 (64 / 63) and 16000 (160 / 441); wav files (rate, samples) in path
# order, read into a pool at 44800 Hz (22400 -> 44800 is 2 / 1)
SURFACE_RATE, SURFACE_TARGETS = 44100, (44800, 16000)
SURFACE_CLIP_LENGTHS = (3000, 1, 700, 2049)
WAV_TARGET = 44800
WAV_FILES = ((44100, 1800), (44800, 900), (22400, 1000), (44100, 1), (44800, 1300), (44800, 40), (22400, 333))


def surface_clips():
    return [clip_int16(700 + q, n, 32768 if q == 0 else 20000) for q, n in enumerate(SURFACE_CLIP_LENGTHS)]


def wav_clips():
    return [clip_int16(800 + q, n) for q, (_, n) in enumerate(WAV_FILES)]


def int16_cases(tile):
    """(label, up, down, int16 clip) of every int16 -> int16 comparison of the GPU tests"""
    cases = []
    for r, (up, down) in enumerate(RATIOS):
        for n in kernel_lengths(up, down, tile):
            cases.append(("single %d/%d n %d" % (up, down, n), up, down, clip_int16(1000 * r + n % 997, n)))
        cases.append(("full scale %d/%d" % (up, down), up, down, clip_int16(77 + r, 700, 32768)))
    for up, down in ((64, 63), (5, 14)):
        for q, n in enumerate(POOL_CLIP_LENGTHS):
            cases.append(("pool %d/%d clip %d" % (up, down, q), up, down, clip_int16(500 + q, n)))
    for up, down in ((64, 63), (1, 2)):
        cases.append(("square %d/%d" % (up, down), up, down, square_wave(900)))
    for up, down in ((64, 63), (5, 14)):
        for amp in (20000, 2048):
            cases.append(("float source %d/%d amplitude %d" % (up, down, amp), up, down, clip_int16(31, 1501, amp)))
    cases.append(("dst_cap", 64, 63, clip_int16(9, 1501)))
    safe = clip_int16(12, 400)
    for first, last in ((0, 400), (370, 400), (399, 400), (0, 100)):
        cases.append(("table values %d:%d" % (first, last), 3, 7, safe[first:last]))
    for target in SURFACE_TARGETS:
        for q, c in enumerate(surface_clips()):
            cases.append(("PcmPool.resample %d clip %d" % (target, q), target, SURFACE_RATE, c))
    for q, ((rate, _), c) in enumerate(zip(WAV_FILES, wav_clips())):
        if rate != WAV_TARGET:
            cases.append(("wav file %d" % q, WAV_TARGET, rate, c))
    return cases
