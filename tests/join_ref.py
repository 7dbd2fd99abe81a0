"""A numpy restatement of the join's definition (include/t2s_hip.h, "joining the rows of padded batches"): int64 offsets, the ramp built
in float64 and rounded once to float32, float32 multiplies.  tests/test_join_ref_cpu.py pins it; the GPU tests compare the kernels
with it bit for bit."""
import numpy as np


def ramp(F):
    """r(k) = (float)((double)(2k + 1) / (double)(2F)), 0 <= k < F, as float32 [F]"""
    if F <= 0:
        return np.zeros(0, dtype=np.float32)
    return ((2.0 * np.arange(F, dtype=np.float64) + 1.0) / np.float64(2 * F)).astype(np.float32)


def offsets(lengths, caps, order=None, gaps=None, gap=0):
    """lengths, caps by row; order position -> row; gaps [n - 1] by position or None (`gap` everywhere)
    -> (int64 [n + 1] with offsets[n] = total, the clamped length of every position)"""
    n = len(lengths)
    order = list(range(n)) if order is None else list(order)
    off = np.zeros(n + 1, dtype=np.int64)
    lens = np.zeros(n, dtype=np.int64)
    for p in range(n):
        row = order[p]
        ln = min(max(int(lengths[row]), 0), int(caps[row])) if 0 <= row < n else 0
        lens[p] = ln
        g = 0
        if p < n - 1:
            g = max(int(gaps[p]), 0) if gaps is not None else int(gap)
        off[p + 1] = off[p] + ln + g
    return off, lens


def fade_segment(x, F, lead, trail):
    """one segment's samples (f32 or f16 [len]) with the ramps -> float32 [len]"""
    y = np.asarray(x).astype(np.float32)
    ln = y.size
    if F <= 0 or ln == 0:
        return y.copy()
    r = ramp(F)
    i = np.arange(ln, dtype=np.int64)
    y = y.copy()
    if lead:
        m = i < F
        y[m] = y[m] * r[i[m]]
    if trail:
        k = ln - 1 - i
        m = k < F
        y[m] = y[m] * r[k[m]]
    return y


def join(rows, lengths, order=None, gaps=None, gap=0, fade=0, fade_ends=False, dst_cap=None, fill=0.0):
    """rows: a list of 1-D arrays (row r holds caps[r] = rows[r].size samples), lengths by row.
    -> (dst float32 [dst_cap], length = min(total, dst_cap), offsets int64 [n + 1] unclipped).  `fill` stands where the definition
    says +0 (a test passes NaN to see which elements the definition leaves to the zeros)."""
    n = len(rows)
    caps = [np.asarray(r).size for r in rows]
    off, lens = offsets(lengths, caps, order, gaps, gap)
    total = int(off[n])
    if dst_cap is None:
        dst_cap = total
    dst = np.full(dst_cap, fill, dtype=np.float32)
    order = list(range(n)) if order is None else list(order)
    for p in range(n):
        ln = int(lens[p])
        if ln == 0:
            continue
        y = fade_segment(np.asarray(rows[order[p]])[:ln], fade, p > 0 or fade_ends, p < n - 1 or fade_ends)
        lo = int(off[p])
        hi = min(lo + ln, dst_cap)
        if hi > lo:
            dst[lo:hi] = y[:hi - lo]
    return dst, min(total, dst_cap), off
