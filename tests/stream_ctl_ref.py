"""The control inside a stream (include/t2s_hip.h: t2s_align_window / t2s_warp_window_map / t2s_warp_window_gather) restated in numpy,
piece by piece, on top of tests/align_ref.py and tests/warp_ref.py: what a push carries is written out here from the definition -
running maxima, integer counts, the run-start frame, 256 double partial sums; a cumulative integer map - and
tests/test_stream_ctl_ref_cpu.py shows that for any cuts the pieces are the whole-row restatement's result.  Loops: it is for tests."""
import numpy as np

import align_ref as R
import warp_ref as W

Q = W.Q
LIVE = R.SKIP | R.BACK | R.STALL | R.NONFINITE
BLOCK = 256


def tree_sum(part):
    """the fixed 256-way tree of the entry pass over the partial sums (float64): 128 pairs i, i + 128, then 64, ..."""
    s = np.array(part, dtype=np.float64)
    w = BLOCK // 2
    with np.errstate(all="ignore"):
        while w:
            s[:w] = s[:w] + s[w:2 * w]
            w //= 2
    return float(s[0])


def device_focus(peak_row, F):
    """the whole-row kernel's focus, in its own order: thread i adds frames i, i + 256, ... in double, the tree joins the 256 sums,
    one division"""
    if F == 0:
        return 0.0
    part = np.zeros(BLOCK, dtype=np.float64)
    with np.errstate(all="ignore"):
        for t in range(F):
            part[t % BLOCK] = part[t % BLOCK] + np.float64(peak_row[t])
        return tree_sum(part) / F


def cuts_of(total, family, seed=0):
    """piece lengths that add up to `total`, by family: "one", "ones" (pieces of one frame), "255" / "256" / "257" (a cut there,
    where total reaches it), "random" (seeded, with empty pieces), "flush" (random, then an empty final piece)"""
    if family == "one":
        return [total]
    if family == "ones":
        return [1] * total
    if family in ("255", "256", "257"):
        k = int(family)
        return [total] if total <= k else [k, total - k]
    rng = np.random.RandomState(seed + total)
    out, left = [], total
    while left > 0:
        n = 0 if rng.randint(0, 5) == 0 else int(rng.randint(1, max(2, min(left, 150)) + 1))
        n = min(n, left)
        out.append(n)
        left -= n
    if family == "flush":
        out.append(0)
    elif family != "random":
        raise ValueError(family)
    return out or [0]


class AlignChunks:
    """the alignment check of B entries, piece by piece.  push(A_piece [B, m, T_in], last) -> align_ref.Report of the prefix:
    pos / peak / bad hold the frames seen, flags only the live bits unless `last`."""

    def __init__(self, B, T_in, in_len=None, **thresholds):
        self.B, self.T = B, T_in
        self.in_len = in_len
        self.thr = dict(R.OFF)
        self.thr.update(thresholds)
        self.S = [R.clamp(T_in if in_len is None else in_len[b], 1, T_in) for b in range(B)]
        self.pos = np.zeros((B, 0), dtype=np.int32)
        self.peak = np.zeros((B, 0), dtype=np.float32)
        self.bad = np.zeros((B, 0), dtype=np.uint8)
        self.dur = np.zeros((B, T_in), dtype=np.int32)
        self.run_start = [-1] * B
        self.skip, self.back, self.stall, self.bad_rows = [0] * B, [0] * B, [0] * B, [0] * B
        self.part = np.zeros((B, BLOCK), dtype=np.float64)
        self.n = 0

    def push(self, A_piece, last):
        A_piece = np.asarray(A_piece)
        m = A_piece.shape[1]
        pos, peak, bad = R.rows(A_piece, self.in_len) if m else (np.zeros((self.B, 0), np.int32), np.zeros((self.B, 0), np.float32),
                                                               np.zeros((self.B, 0), np.uint8))
        n0 = self.n
        self.pos = np.concatenate([self.pos, pos], 1)
        self.peak = np.concatenate([self.peak, peak], 1)
        self.bad = np.concatenate([self.bad, bad], 1)
        self.n = n = n0 + m
        st = np.zeros((self.B, 8), dtype=np.int32)
        focus = np.zeros(self.B, dtype=np.float64)
        flags = np.zeros(self.B, dtype=np.int32)
        th = self.thr
        for b in range(self.B):
            S = self.S[b]
            with np.errstate(all="ignore"):
                for t in range(n0, n):
                    p = int(self.pos[b, t])
                    if t == 0 or p != int(self.pos[b, t - 1]):
                        self.run_start[b] = t
                    if t > 0:
                        d = p - int(self.pos[b, t - 1])
                        self.skip[b], self.back[b] = max(self.skip[b], d), max(self.back[b], -d)
                    self.stall[b] = max(self.stall[b], t - self.run_start[b] + 1)      # a run still open counts as it stands
                    self.bad_rows[b] += int(self.bad[b, t] != 0)
                    if 0 <= p < S:
                        self.dur[b, p] += 1
                    self.part[b, t % BLOCK] = self.part[b, t % BLOCK] + np.float64(self.peak[b, t])
                f = tree_sum(self.part[b]) / n if n else 0.0
            lastpos = int(self.pos[b, n - 1]) if n else -1
            covered = int((self.dur[b, :S] > 0).sum())
            st[b] = [n, S, self.skip[b], self.back[b], self.stall[b], lastpos, covered, self.bad_rows[b]]
            focus[b] = f
            bits = 0
            if th["skip_max"] >= 0 and self.skip[b] > th["skip_max"]:
                bits |= R.SKIP
            if th["back_max"] >= 0 and self.back[b] > th["back_max"]:
                bits |= R.BACK
            if th["stall_max"] >= 0 and self.stall[b] > th["stall_max"]:
                bits |= R.STALL
            if self.bad_rows[b] > 0:
                bits |= R.NONFINITE
            if last:
                if th["max_frames"] > 0 and n >= th["max_frames"]:
                    bits |= R.TRUNCATED
                if th["end_slack"] >= 0 and lastpos < S - 1 - th["end_slack"]:
                    bits |= R.UNFINISHED
                if th["min_focus"] > 0 and not f >= th["min_focus"]:
                    bits |= R.DIFFUSE
                if n == 0:
                    bits |= R.EMPTY
            flags[b] = bits
        return R.Report(self.pos.copy(), self.peak.copy(), self.bad.copy(), st, focus, self.dur.copy(), flags)


def settled(c_prev, c_n, final=False):
    """#{j >= 0 : (2j + 1) Q <= c[n - 1] + c[n]} by counting; on the final push the warped length's integer"""
    if final:
        return 0 if c_n == 0 else max(1, (c_n + Q // 2) >> 20)
    if c_n == 0:
        return 0
    j = 0
    while (2 * j + 1) * Q <= c_prev + c_n:
        j += 1
    return j


class WarpChunks:
    """the time warp of one entry, piece by piece.  push(x_piece [C, m], last, stretch) -> the warped columns that became settled,
    [C, m'] of x's dtype.  c (Python ints) is the map so far; first_last follows a path where one is given."""

    def __init__(self, C, dtype, path=None, in_len=None, T_in=0):
        self.x = np.zeros((C, 0), dtype=dtype)
        self.c = [0]
        self.out = 0
        self.path, self.T_in = path, T_in
        self.S = min(max(int(T_in if in_len is None else in_len), 1), T_in) if T_in else 0
        self.fl = np.full((T_in, 2), -1, dtype=np.int32)

    def push(self, x_piece, last, stretch):
        x_piece = np.asarray(x_piece)
        n0 = self.x.shape[1]
        self.x = np.concatenate([self.x, x_piece], 1)
        n = self.x.shape[1]
        for _ in range(n0, n):
            self.c.append(self.c[-1] + int(stretch))
        if self.path is not None:
            for f in range(n0, n):
                k = int(self.path[f])
                if 0 <= k < self.S:
                    if f == 0 or int(self.path[f - 1]) != k:
                        self.fl[k, 0] = f if self.fl[k, 0] < 0 else min(int(self.fl[k, 0]), f)
                    if f == n - 1 or int(self.path[f + 1]) != k:
                        self.fl[k, 1] = max(int(self.fl[k, 1]), f)
        j0 = self.out
        j1 = max(j0, settled(self.c[n - 1] if n else 0, self.c[n], last))
        self.out = j1
        if j1 == j0:
            return np.zeros((self.x.shape[0], 0), dtype=self.x.dtype)
        c = np.array(self.c, dtype=np.int64)
        return W.warp_entry(self.x, c, n, j1, j1)[0][:, j0:j1]
