"""The float64 numpy restatement of the true-peak meter and look-ahead limiter (include/t2s_hip.h states the arithmetic;
text2speech_amd/csrc/limiter.hip is the device form).  Written from the definitions, independently of the package: its own
filter, its own window, `sliding_window_view` for the minimum and explicit ascending sums for the rest (a product, then an add:
the device fuses the two, which is part of the tests' rounding bound)."""
import collections

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

FLAG_LIMITED, FLAG_NONFINITE = 1, 8

Limited = collections.namedtuple("Limited", "out o s r p u stats counts")


def ceiling(ceiling_db):
    """the ceiling as a float32 value, held in a float"""
    return float(np.float32(10.0 ** (ceiling_db / 20.0)))


def interp_filter(os, half_width=10, beta=5.0):
    """scipy.signal.resample_poly(x, os, 1)'s default filter: os * firwin(2 half_width os + 1, 1 / os, window=('kaiser', beta))"""
    half = half_width * os
    t = np.arange(-half, half + 1, dtype=np.float64) / os
    h = np.kaiser(2 * half + 1, beta) * (np.sinc(t) / os)
    return os * (h / h.sum())


def asc_sum(v):
    acc = 0.0
    for t in v:
        acc = acc + float(t)
    return acc


def window(L):
    """w[k] = 1/2 + 1/2 cos(pi k / (L + 1)), k = -L .. L, normalised; the centre tap is raised by the last few ulps it takes for
    the sum in ascending order to be no less than 1 (so that s is exactly 1 wherever every m in reach is 1)"""
    k = np.arange(-L, L + 1, dtype=np.float64)
    w = 0.5 + 0.5 * np.cos(np.pi * k / (L + 1))
    w = w / w.sum()
    while asc_sum(w) < 1.0:
        w[L] += max(1.0 - asc_sum(w), np.spacing(w[L]))
    return w


def envelope(u, os, half_width=10, beta=5.0):
    """(p [n], y [os n]): y the row oversampled with zero extension, every sum in ascending source index; p[i] the largest of
    |u[i]| and |y[os i + q]|"""
    u = np.asarray(u, np.float64)
    n = u.size
    p = np.abs(u)
    y = np.zeros((n, os))
    if os == 1:
        y[:, 0] = u
        return p, y.reshape(-1)
    h = interp_filter(os, half_width, beta)
    up = np.concatenate([np.zeros(half_width), u, np.zeros(half_width)])
    for q in range(os):
        acc = np.zeros(n)
        for d in range(0 if q == 0 else 1, 2 * half_width + 1):          # sample i - half_width + d meets tap q + os (2 hw - d)
            acc = acc + up[d:d + n] * h[q + os * (2 * half_width - d)]
        y[:, q] = acc
        p = np.maximum(p, np.abs(acc))
    return p, y.reshape(-1)


def limit(x, c, L, os=4, half_width=10, beta=5.0, g=1.0):
    """x int16 / float32 / float16 / float64 [n] -> Limited.  `out` is what the device stores (int16 for int16, else float32), `o`
    the float64 product, `stats` (true_peak, sample_peak, s_min, 0), `counts` (limited samples, flags)."""
    x = np.asarray(x)
    n = x.size
    is16 = x.dtype == np.int16
    u = x.astype(np.float64) / 32768.0 * g if is16 else x.astype(np.float64) * g
    if n == 0:
        e = np.zeros(0)
        return Limited(x.copy() if is16 else x.astype(np.float32), e, e, e, e, u, (0.0, 0.0, 1.0, 0.0), (0, 0))
    if not np.all(np.isfinite(u)):
        out = x.copy() if is16 else x.astype(np.float32)
        one = np.ones(n)
        return Limited(out, None, one, one, None, u, (np.inf, np.inf, 1.0, 0.0), (0, FLAG_NONFINITE))
    p, _ = envelope(u, os, half_width, beta)
    over = p > c
    r = np.ones(n)
    r[over] = c / p[over]
    rp = np.concatenate([np.ones(2 * L), r, np.ones(2 * L)])
    m = sliding_window_view(rp, 2 * L + 1).min(axis=-1)                  # m over [-L, n + L)
    w = window(L)
    acc = np.zeros(n)
    for k in range(2 * L + 1):
        acc = acc + w[k] * m[k:k + n]
    s = np.minimum(r, acc)
    o = u * s
    if is16:
        out = np.clip(np.rint(32768.0 * o), -32768, 32767).astype(np.int16)
    else:
        out = o.astype(np.float32)
    cnt = int(over.sum())
    stats = (float(p.max()) if n else 0.0, float(np.abs(u).max()) if n else 0.0, float(s.min()) if n else 1.0, 0.0)
    return Limited(out, o, s, r, p, u, stats, (cnt, FLAG_LIMITED if cnt else 0))


def env_bound(u, os, half_width=10, beta=5.0):
    """the rounding bound on the device's p against this file's: both are sums of T = 2 half_width + 1 products in the same order,
    one fused (T roundings) and one not (2 T): |dp[i]| <= (3 T) 2^-53 sum_j |h||u|, taken as the worst phase"""
    u = np.abs(np.asarray(u, np.float64))
    if os == 1:
        return np.zeros(u.size)
    h = np.abs(interp_filter(os, half_width, beta))
    up = np.concatenate([np.zeros(half_width), u, np.zeros(half_width)])
    worst = np.zeros(u.size)
    for q in range(os):
        acc = np.zeros(u.size)
        for d in range(0 if q == 0 else 1, 2 * half_width + 1):
            acc = acc + up[d:d + u.size] * h[q + os * (2 * half_width - d)]
        worst = np.maximum(worst, acc)
    return 3 * (2 * half_width + 1) * 2.0 ** -53 * worst


# ---- the seeded inputs the CPU and GPU tests share --------------------------------------------------------------------------------
TILE = 1024                     # t2s_limit_tile(), asserted by the GPU tests
CEILING_DB = -1.0
LOOKAHEADS = (0, 1, 16, 67, 1024)
OVERSAMPLES = (1, 2, 4)
KINDS = ("int16", "float32", "float16")
HALF_WIDTH = 10


def lengths_for(L):
    """n in {1, 2, 2 L, 2 L + 1, T - 1, T, T + 1, 2 T + 1} (2 L = 0 is the empty row)"""
    return sorted({1, 2, 2 * L, 2 * L + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1})


def peaks_for(n, L):
    """where the placed peaks go: within half_width of each end, at T - 1 and T, so that a +-2 L dip straddles a tile edge, two
    closer than L, and a run of five equal samples over the ceiling (ties in the minimum) - those that fit the row"""
    spots = [0, 3, HALF_WIDTH, n - 1, n - 1 - 4, n - 1 - HALF_WIDTH, TILE - 1, TILE, TILE - L, TILE + L, TILE - 2 * L - 1, TILE + 2 * L,
             300, 300 + max(1, L // 2)]
    spots = sorted({s for s in spots if 0 <= s < n})
    run = (600, 5) if n >= 700 else None
    return spots, run


def clip(n, seed, kind, L, level=0.2):
    """a seeded row: Gaussian noise of `level` (so that gains of 3 and 8 push much of it over the ceiling), the placed peaks of
    peaks_for at 0.93 .. 1.0 with alternating signs, the run at 0.95"""
    gen = np.random.RandomState(seed)
    x = np.clip(level * gen.standard_normal(n), -0.85, 0.85)
    spots, run = peaks_for(n, L)
    for q, s in enumerate(spots):
        x[s] = (0.93 + 0.07 * gen.random_sample()) * (1 if q % 2 else -1)
    if run:
        x[run[0]:run[0] + run[1]] = 0.95
    if kind == "int16":
        return np.rint(x * 32767.0).astype(np.int16)
    return x.astype(np.float32 if kind == "float32" else np.float16)


def seed_of(n, L, os, kind):
    return 1000 * L + 7 * n + 3 * os + KINDS.index(kind)


_CACHE = {}


def reference(x, c, L, os, g=1.0):
    """limit(...) of a row, computed once and shared"""
    key = (x.dtype.str, x.tobytes(), c, L, os, g)
    if key not in _CACHE:
        _CACHE[key] = limit(x, c, L, os, HALF_WIDTH, 5.0, g)
    return _CACHE[key]


def bounds(ref, L, os):
    """(b_p [n], b_s): the rounding bounds on the device's p and s against this file's (profiles/limiter_tests.md derives them).
    p: env_bound.  r = c / p: one more rounding on each side and the error of p passed on, |dr| <= r (b_p / p + 2^-52).  m is a
    minimum of r: no new error.  The window sum: 2 L + 1 products in the same order, fused on the device (W roundings) and not
    here (2 W), of terms that sum to 1: 3 W 2^-53, plus sum w |dm| <= max |dr|.  s is the smaller of the two: the larger bound."""
    b_p = env_bound(ref.u, os, HALF_WIDTH)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_r = np.where(ref.p > 0, ref.r * (b_p / np.where(ref.p > 0, ref.p, 1.0) + 2.0 ** -52), 0.0)
    b_s = (float(d_r.max()) if d_r.size else 0.0) * (1 + 2.0 ** -40) + 3 * (2 * L + 1) * 2.0 ** -53
    return b_p, b_s
