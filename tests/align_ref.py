"""The alignment check of include/t2s_hip.h (t2s_align_rows / t2s_align_stats) restated in numpy and Python floats, written from the
definition and not from the kernels; tests/test_align_ref_cpu.py pins it on hand-built matrices.  Loops over rows: it is for tests."""
import collections
import math

import numpy as np

TRUNCATED, SKIP, BACK, STALL, UNFINISHED, DIFFUSE, NONFINITE, EMPTY = 1, 2, 4, 8, 16, 32, 64, 128
OFF = dict(max_frames=0, skip_max=-1, back_max=-1, stall_max=-1, end_slack=-1, min_focus=0.0)       # every threshold switched off

Report = collections.namedtuple("Report", "pos peak bad stats focus dur flags")


def clamp(v, lo, hi):
    return max(lo, min(int(v), hi))


def rows(A, in_len=None, out_len=None):
    """A [B, N, T_in] float32 or float16 -> (pos int32 [B, N], peak float32 [B, N], bad uint8 [B, N])"""
    A = np.asarray(A)
    B, N, T = A.shape
    pos = np.full((B, N), -1, dtype=np.int32)
    peak = np.zeros((B, N), dtype=np.float32)
    bad = np.zeros((B, N), dtype=np.uint8)
    for b in range(B):
        S = clamp(T if in_len is None else in_len[b], 1, T)
        F = clamp(N if out_len is None else out_len[b], 0, N)
        for t in range(F):
            v = A[b, t, :S].astype(np.float64)                  # (exact: every f16 and f32 is a double)
            # "start at best = -inf, j = 0, update on v > best": a NaN never wins, the first of equal maxima does, and a row
            # with nothing above -inf stays at j = 0 - numpy's argmax of the row with its NaNs put to -inf
            seen = np.where(np.isnan(v), -math.inf, v)
            at = int(np.argmax(seen))
            pos[b, t] = at
            peak[b, t] = np.float32(seen[at])
            bad[b, t] = 0 if np.isfinite(v).all() else 1
    return pos, peak, bad


def stats(pos, peak, bad, T_in, in_len=None, out_len=None, max_frames=0, skip_max=-1, back_max=-1, stall_max=-1, end_slack=-1,
          min_focus=0.0):
    """the entry pass -> (stats int32 [B, 8], focus float64 [B], dur int32 [B, T_in], flags int32 [B]); focus is the correctly
    rounded sum (math.fsum) divided by F: the value an error bound of the device's sum is stated against"""
    B, N = pos.shape
    st = np.zeros((B, 8), dtype=np.int32)
    focus = np.zeros(B, dtype=np.float64)
    dur = np.zeros((B, T_in), dtype=np.int32)
    flags = np.zeros(B, dtype=np.int32)
    for b in range(B):
        S = clamp(T_in if in_len is None else in_len[b], 1, T_in)
        F = clamp(N if out_len is None else out_len[b], 0, N)
        p = [int(v) for v in pos[b, :F]]
        steps = [y - x for x, y in zip(p, p[1:])]
        max_skip = max([0] + steps)
        max_back = max([0] + [-d for d in steps])
        longest, run = 0, 0
        for t in range(F):
            run = run + 1 if t > 0 and p[t] == p[t - 1] else 1
            longest = max(longest, run)
        last = p[-1] if F else -1
        for v in p:
            if 0 <= v < S:
                dur[b, v] += 1
        covered = int((dur[b, :S] > 0).sum())
        bad_rows = int(bad[b, :F].astype(np.int64).sum())
        with np.errstate(all="ignore"):
            try:
                total = math.fsum(float(v) for v in peak[b, :F])
            except (OverflowError, ValueError):                 # an infinity or a NaN among the peaks: what IEEE gives
                total = float(np.sum(peak[b, :F].astype(np.float64)))
            f = total / F if F else 0.0
        st[b] = [F, S, max_skip, max_back, longest, last, covered, bad_rows]
        focus[b] = f
        bits = 0
        if max_frames > 0 and F >= max_frames:
            bits |= TRUNCATED
        if skip_max >= 0 and max_skip > skip_max:
            bits |= SKIP
        if back_max >= 0 and max_back > back_max:
            bits |= BACK
        if stall_max >= 0 and longest > stall_max:
            bits |= STALL
        if end_slack >= 0 and last < S - 1 - end_slack:
            bits |= UNFINISHED
        if min_focus > 0 and not f >= min_focus:
            bits |= DIFFUSE
        if bad_rows > 0:
            bits |= NONFINITE
        if F == 0:
            bits |= EMPTY
        flags[b] = bits
    return st, focus, dur, flags


def report(A, in_len=None, out_len=None, **thresholds):
    pos, peak, bad = rows(A, in_len, out_len)
    st, focus, dur, flags = stats(pos, peak, bad, np.asarray(A).shape[2], in_len, out_len, **thresholds)
    return Report(pos, peak, bad, st, focus, dur, flags)


def focus_bound(peak_row, F):
    """2^-53 (F + 1) mean|peak|: a double sum of F terms in any order, plus one division, against the correctly rounded sum"""
    if F == 0:
        return 0.0
    return 2.0 ** -53 * (F + 1) * float(np.abs(peak_row[:F].astype(np.float64)).mean())


def random_alignments(B, N, T_in, dtype, seed, in_len=None, path=None):
    """Seeded alignments for the GPU tests: every row a softmax over T_in columns of logits with a ridge, rounded to `dtype`.  The
    ridge of entry b moves by 0, 1 or 2 columns a frame and wraps at S_b (in_len clamped; T_in without it) - or follows `path`
    ([B, N] columns) where one is given.  tests/test_align_ref_cpu.py asserts that no row's two largest values among its first S_b
    columns are closer than MARGIN, for the shapes and lengths the GPU tests use - so that an argmax cannot hang on a rounding."""
    rng = np.random.RandomState(seed)
    logits = rng.uniform(-4.0, 0.0, (B, N, T_in))
    S = np.array([clamp(T_in if in_len is None else in_len[b], 1, T_in) for b in range(B)])
    centre = np.cumsum(rng.randint(0, 3, (B, N)), axis=1) % S[:, None] if path is None else np.asarray(path).reshape(B, N)
    np.put_along_axis(logits, centre[:, :, None], 3.0, axis=2)
    e = np.exp(logits)
    return (e / e.sum(axis=2, keepdims=True)).astype(dtype)


MARGIN = 2.0 ** -9          # relative to the row's largest value: eight f16 roundings (2^-11 each) apart at the least


def top2_gap(A, in_len=None, out_len=None):
    """the smallest (largest - second largest) / largest over every row t < F_b, among its first S_b columns (S_b = 1: no second)"""
    A = np.asarray(A).astype(np.float64)
    B, N, T = A.shape
    worst = math.inf
    for b in range(B):
        S = clamp(T if in_len is None else in_len[b], 1, T)
        F = clamp(N if out_len is None else out_len[b], 0, N)
        if S < 2 or F == 0:
            continue
        part = np.sort(A[b, :F, :S], axis=1)
        worst = min(worst, float(((part[:, -1] - part[:, -2]) / part[:, -1]).min()))
    return worst
