"""The time warp of a mel and the symbol spans read from its cumulative map, restated in numpy: include/t2s_hip.h's definition of
t2s_warp_map / t2s_warp_gather / t2s_warp_spans (csrc/warp.hip; text2speech_amd/rate.py).  Integers are Python ints or int64, the one
floating-point expression of an output value is formed in float64 and rounded once.  tests/test_warp_ref_cpu.py pins it against
np.interp."""
import math

import numpy as np

Q = 1 << 20
MIN_RATE, MAX_RATE = 0.5, 2.0


def stretch_q(rate):
    """rint(Q / rate) in double, ties to even: the output frames per source frame in units of 1 / Q"""
    return int(np.rint(np.float64(Q) / np.float64(rate)))


def warped_length(frames, rate, cap=None):
    """F' of `frames` source frames at one rate"""
    frames = int(frames)
    if frames <= 0:
        return 0
    n = max(1, (frames * stretch_q(rate) + Q // 2) >> 20)
    return n if cap is None else min(n, cap)


def symbol_stretches(path, symbol_rates, in_len, min_rate=MIN_RATE, max_rate=MAX_RATE):
    """s[f] of one entry from its path [N] and its table [T_in] float32: rate 1 for a path value outside [0, S) and for a NaN"""
    table = np.asarray(symbol_rates, dtype=np.float32)
    S = min(max(int(in_len), 1), table.size)
    s = np.full(len(path), Q, dtype=np.int64)
    for f, k in enumerate(path):
        k = int(k)
        if k < 0 or k >= S:
            continue
        v = np.float64(table[k])
        if math.isnan(v):
            continue
        v = min(max(v, np.float64(min_rate)), np.float64(max_rate))
        s[f] = int(np.rint(np.float64(Q) / v))
    return s


def cum_map(stretch, F, length, cap=None):
    """(c int64 [F + 1], F') of one entry: `stretch` an int (every frame) or F values; entries behind F_b repeat c[F_b]"""
    Fb = min(max(int(length), 0), F)
    s = np.full(F, int(stretch), dtype=np.int64) if np.ndim(stretch) == 0 else np.asarray(stretch, dtype=np.int64)[:F].copy()
    s[Fb:] = 0
    c = np.zeros(F + 1, dtype=np.int64)
    c[1:] = np.cumsum(s)
    if Fb == 0:
        return c, 0
    n = max(1, int((int(c[Fb]) + Q // 2) >> 20))
    return c, (n if cap is None else max(1, min(n, cap)))


def coords(c, length, n_out):
    """(f, a) of the output frames 0 .. n_out - 1 of one entry: the source frame and the weight of its right neighbour (float64);
    a = 0 with f clamped where the definition copies a frame"""
    Fb = int(length)
    m = (c[:Fb] + c[1:Fb + 1]).astype(np.int64)
    p = (2 * np.arange(n_out, dtype=np.int64) + 1) * Q
    f = np.searchsorted(m, p, side="right").astype(np.int64) - 1         # the largest f with m[f] <= p, -1 for none
    inner = (f >= 0) & (f < Fb - 1)
    fs = np.clip(f, 0, max(Fb - 1, 0))
    ws = np.zeros(n_out, dtype=np.float64)
    fi = fs[inner]
    ws[inner] = (p[inner] - m[fi]).astype(np.float64) / (m[fi + 1] - m[fi]).astype(np.float64)      # integers below 2^53: exact
    return fs, ws


def warp_entry(x, c, length, n_out, cap):
    """One entry: x [C, >= F_b] float32 or float16 -> (out [C, cap] of x's dtype, exact [C, n_out] float64 before the one rounding,
    bound_small [C, n_out] = |x[f]| + |x[f + 1]| in float64).  Columns n_out .. cap - 1 are +0.  x[f + 1] is not read where a = 0."""
    C = x.shape[0]
    out = np.zeros((C, cap), dtype=x.dtype)
    exact = np.zeros((C, n_out), dtype=np.float64)
    small = np.zeros((C, n_out), dtype=np.float64)
    if n_out == 0:
        return out, exact, small
    f, a = coords(c, length, n_out)
    left = x[:, f]
    right = x[:, np.where(a == 0.0, f, f + 1)]
    exact[:] = (1.0 - a) * left.astype(np.float64) + a * right.astype(np.float64)
    copy = a == 0.0
    out[:, :n_out] = exact.astype(x.dtype)
    out[:, :n_out][:, copy] = left[:, copy]                   # bit for bit (a NaN's payload, a -0)
    small[:] = np.abs(left.astype(np.float64)) + np.where(copy, 0.0, np.abs(right.astype(np.float64)))
    return out, exact, small


def first_last(path, length, in_len, T_in):
    """int32 [T_in, 2]: the smallest and the largest f < F_b with path[f] == k for k < S, (-1, -1) where there is none"""
    Fb = min(max(int(length), 0), len(path))
    S = min(max(int(in_len), 1), T_in)
    fl = np.full((T_in, 2), -1, dtype=np.int32)
    for f in range(Fb):
        k = int(path[f])
        if 0 <= k < S:
            if fl[k, 0] < 0:
                fl[k, 0] = f
            fl[k, 1] = f
    return fl


def spans(c, fl, length, in_len, hop, trim=None, offset=None, ratio=(1, 1), total=None):
    """int64 [T_in, 2] of one entry: [start, end) of every symbol in samples; trim = (start, kept) or None, offset an int or None"""
    T_in = fl.shape[0]
    Fb = min(max(int(length), 0), len(c) - 1)
    S = min(max(int(in_len), 1), T_in)
    up, down = ratio
    out = np.full((T_in, 2), -1, dtype=np.int64)
    if Fb == 0:
        return out
    for k in range(S):
        first, last = int(fl[k, 0]), int(fl[k, 1])
        if first < 0 or last < first or last >= Fb:
            continue
        for e, t in enumerate((int(c[first]), int(c[last + 1]))):
            u = (t * hop) >> 20
            if trim is not None:
                u = min(max(u - int(trim[0]), 0), int(trim[1]))
            if offset is not None:
                u += int(offset)
            u = (u * up) // down
            if total is not None:
                u = min(u, int(total))
            out[k, e] = u
    return out
