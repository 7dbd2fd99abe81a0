"""ITU-R BS.1770-4 / EBU R128 gated loudness restated in float64 (numpy + scipy.signal.lfilter, run sequentially over the row): the
reference of csrc/loudness.hip, and the cases its GPU tests use.  tests/test_loudness_ref_cpu.py checks this file against the
standard's table and a per-sample loop, and asserts the conditions that let the GPU tests demand equal counts and equal int16."""
import math

import numpy as np
from scipy.signal import lfilter

SEGMENT, TILE = 32, 8192        # t2s_loud_segment(), t2s_loud_tile(): the GPU tests assert that the library says the same
GATE_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)
RATES = (8000, 44100, 44800)
KINDS = ("int16", "float32", "float16")
LEVELS = (0.3, 1e-5, 0.004, 0.1)
SHORT, SILENT, PEAK, NONFINITE = 1, 2, 4, 8


def coefficients(fs):
    """((b, a) shelf, (b, a) high-pass) of the K-weighting at the rate fs"""
    def den(f0, Q):
        K = math.tan(math.pi * f0 / fs)
        a0 = 1.0 + K / Q + K * K
        return K, a0, np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K, a0, a1 = den(f0, Q)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    _, _, a2 = den(38.13547087602444, 0.5003270373238773)
    return (b1, a1), (np.array([1.0, -2.0, 1.0]), a2)


def hop(fs):
    return int(math.floor(fs / 10.0 + 0.5))


def as_float64(x):
    """the samples as the measure counts them: int16 / 32768, floats widened"""
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


def kweight(x64, fs):
    (b1, a1), (b2, a2) = coefficients(fs)
    return lfilter(b2, a2, lfilter(b1, a1, x64))


def kweight_loop(x64, fs):
    """the same filter as an explicit per-sample loop (direct form I), for the CPU test"""
    out = np.asarray(x64, dtype=np.float64)
    for b, a in coefficients(fs):
        y = np.zeros(out.size)
        for i in range(out.size):
            acc = b[0] * out[i]
            if i >= 1:
                acc += b[1] * out[i - 1] - a[1] * y[i - 1]
            if i >= 2:
                acc += b[2] * out[i - 2] - a[2] * y[i - 2]
            y[i] = acc
        out = y
    return out


def hop_energies(x64, fs):
    h = hop(fs)
    nh = x64.size // h
    if nh == 0:
        return np.zeros(0)
    y = kweight(x64, fs)[:nh * h]
    return np.array([math.fsum((y[k * h:(k + 1) * h] ** 2).tolist()) for k in range(nh)])


def block_ms(z, h):
    J = max(0, z.size - 3)
    return np.array([(((z[j] + z[j + 1]) + z[j + 2]) + z[j + 3]) / (4.0 * h) for j in range(J)])


def _mean(v):
    s = 0.0
    for t in v:
        s += float(t)
    return s / len(v)


def measure(x, fs, target_lufs=-23.0, peak_limit=None):
    """x: int16 / float32 / float16 / float64 row -> dict(J, nA, nR, flags, ms, lufs, peak, g, blocks (ms_j), margin: the smallest
    relative distance of any block to a gate it is compared with)"""
    x64 = as_float64(x)
    h = hop(fs)
    finite = bool(np.isfinite(x64).all())
    peak = float(np.abs(x64).max()) if x64.size and finite else (math.inf if not finite else 0.0)
    J = max(0, x64.size // h - 3)
    out = dict(J=J, nA=0, nR=0, flags=0, ms=0.0, lufs=-math.inf, peak=peak, g=1.0, blocks=np.zeros(0), margin=math.inf)
    if J == 0:
        out["flags"] |= SHORT
    if not finite:
        out["flags"] |= NONFINITE
        out["lufs"] = math.nan
        return out
    if J == 0:
        return out
    ms_j = block_ms(hop_energies(x64, fs), h)
    out["blocks"] = ms_j
    out["margin"] = float(np.min(np.abs(ms_j - GATE_ABS) / GATE_ABS))
    A = ms_j[ms_j > GATE_ABS]
    out["nA"] = int(A.size)
    if A.size == 0:
        out["flags"] |= SILENT
        return out
    thr = 0.1 * _mean(A)
    out["margin"] = min(out["margin"], float(np.min(np.abs(A - thr) / thr)))
    Rset = A[A > thr]
    out["nR"] = int(Rset.size)
    ms = _mean(Rset)
    g = math.sqrt(10.0 ** ((target_lufs + 0.691) / 10.0) / ms)
    if peak_limit is not None and peak * g > peak_limit:
        g = peak_limit / peak
        out["flags"] |= PEAK
    out.update(ms=ms, lufs=-0.691 + 10.0 * math.log10(ms), g=g)
    return out


def apply_float(x, g):
    """float32 / float16 row -> float32: (float)((double)x g); g = 1 copies"""
    x = np.asarray(x)
    return x.astype(np.float32) if g == 1.0 else (x.astype(np.float64) * g).astype(np.float32)


def apply_int16(x, g):
    """int16 -> int16: rint((double)x g), ties to even, saturated"""
    return np.clip(np.rint(np.asarray(x).astype(np.float64) * g), -32768, 32767).astype(np.int16)


def half_integer_margin(x, g):
    """the smallest distance of any x g from a half-integer (where rint would depend on the last bit of g)"""
    v = np.asarray(x).astype(np.float64) * g
    return float(np.min(np.abs(np.abs(v - np.floor(v)) - 0.5))) if v.size else math.inf


def recipe(seed, fs, n):
    """Gaussian noise whose level is constant over stretches of 6 h samples and cycles through LEVELS from index seed % 4, clipped
    to +-1: float64 [n]"""
    h = hop(fs)
    x = np.random.default_rng(seed).standard_normal(n)
    level = np.array(LEVELS)[(seed % 4 + np.arange(n) // (6 * h)) % 4] if n else np.zeros(0)
    return np.clip(x * level, -1.0, 1.0)


def steady(seed, fs, n):
    """noise at 0.3 and 0.05 in turns of 6 h samples: the relative gate rejects the quiet turns and every block lies far above the
    absolute gate at any gain a test applies, so the gated set does not change when the row is scaled"""
    h = hop(fs)
    x = np.random.default_rng(seed).standard_normal(n)
    return np.clip(x * np.array([0.3, 0.05])[(seed + np.arange(n) // (6 * h)) % 2], -1.0, 1.0)


def steady_rows(fs):
    """(n, seed) of the padded batches of tests/test_loudness_gpu.py: three rows that are measured, one too short"""
    h = hop(fs)
    return [(25 * h + 5, 0), (13 * h + 17, 1), (3 * h + 9, 2), (TILE + 4 * h, 3)]


def as_kind(sig, kind):
    if kind == "int16":
        return np.clip(np.rint(sig * 32767.0), -32768, 32767).astype(np.int16)
    return sig.astype(np.float32 if kind == "float32" else np.float16)


def lengths_for(fs):
    """(n, seed) of the kernel cases at one rate: the row's ends, the segment's and the tile's edges, the first blocks, the recipe's
    25 h + 5.  4 h gets seed 1 (nothing above the absolute gate), the long rows seeds whose levels make both gates reject."""
    h = hop(fs)
    ns = [0, 1, SEGMENT - 1, SEGMENT, SEGMENT + 1, 4 * h - 1, 4 * h, 4 * h + 1, 5 * h - 1, 5 * h, TILE - 1, TILE, TILE + 1,
          2 * TILE + 17, 25 * h + 5]
    seeds = {4 * h: 1, 25 * h + 5: 0}
    return [(n, seeds.get(n, i % 8)) for i, n in enumerate(ns)]


def clip(fs, n, seed, kind):
    return as_kind(recipe(seed, fs, n), kind)


def kernel_cases():
    """every (fs, kind, n, seed) of tests/test_loudness_kernels_gpu.py's sweep"""
    return [(fs, kind, n, seed) for fs in RATES for kind in KINDS for n, seed in lengths_for(fs)]


# the five rows of the batch-position test and the pool of the int16 test: (n in hops and samples, seed)
def batch_rows(fs):
    h = hop(fs)
    return [(25 * h + 5, 0), (4 * h, 1), (13 * h + 17, 2), (TILE + 1, 3), (31 * h - 3, 5)]


def pool_rows(fs):
    h = hop(fs)
    return [(13 * h + 17, 4), (2 * h + 3, 6), (25 * h + 5, 0), (4 * h, 1), (31 * h - 3, 7), (5 * h, 2)]


POOL_TARGET, POOL_PEAK_LIMIT = -23.0, 32767.0 / 32768.0


def click_row(fs, kind="float32"):
    """a quiet row with one full-scale click: a high target makes the peak limit set the gain"""
    h = hop(fs)
    sig = recipe(2, fs, 9 * h) * 0.02
    sig[4 * h + 7] = 1.0
    return as_kind(sig, kind)


# ---- the refused argument tuples: one rule broken each.  A pointer argument takes "null" or "mis" (4 bytes past an aligned one) ----
_NAN, _INF = float("nan"), float("inf")
REFUSED_MEASURE = [dict(src="null"), dict(table="null"), dict(coef="null"), dict(scratch="null"), dict(stats="null"), dict(counts="null"),
                   dict(table="mis"), dict(coef="mis"), dict(scratch="mis"), dict(stats="mis"), dict(src_len=0), dict(src_len=-3),
                   dict(rows=0), dict(rows=-1), dict(rows=65536), dict(max_count=0), dict(max_count=-1), dict(max_count=1 << 31),
                   dict(h=399), dict(h=38401), dict(h=0), dict(h=SEGMENT - 1), dict(kind=3), dict(kind=-1), dict(gate=_NAN),
                   dict(gate=_INF), dict(gate=-1.0), dict(T=_NAN), dict(T=_INF), dict(T=0.0), dict(T=-1.0), dict(limit=_NAN),
                   dict(scratch_len="short"), dict(scratch_len=0)]
REFUSED_APPLY = [dict(src="null"), dict(table="null"), dict(stats="null"), dict(dst="null"), dict(table="mis"), dict(stats="mis"),
                 dict(src_len=0), dict(dst_len=0), dict(rows=0), dict(rows=65536), dict(max_out=0), dict(max_out=(1 << 40) + 1),
                 dict(kind=3), dict(kind=-1), dict(dkind=1), dict(dkind=2), dict(dkind=-1), dict(dst="src"), dict(dst="inside src")]


def refused_pointer(value, good):
    return None if value == "null" else good + 4 if value == "mis" else good
