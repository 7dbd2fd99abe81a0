#!/usr/bin/env python3
"""The bits of the alignment check and the time warp (csrc/align.hip, csrc/warp.hip), whole rows and stream pushes, as one sha256
per output buffer.

    python tools/control_bits.py > a.txt                                         # this tree's library
    T2S_LIB_PATH=build/parent/libt2s_hip.so python tools/control_bits.py > b.txt # another build of it, in a fresh process
    diff a.txt b.txt

Calls t2s_align_rows + t2s_align_stats, t2s_align_window, t2s_warp_map + t2s_warp_gather + t2s_warp_spans and t2s_warp_window_map +
t2s_warp_window_gather on seeded inputs and prints `<case> <buffer> <sha256>` lines (the return code where it is not 0).  It asserts
nothing about a library alone: two libraries compute the same iff their outputs are the same text.  A stream's line digests the
buffer as it stood after every push, one after the other.  Every buffer holds the same constant before use, so bytes nobody writes
hash alike.

Alignment: T_in 1 / 65 / 257, N 1 / 257 / 600, B 3, f32 and f16, lengths absent, in range, 0, negative and too large, entry 1 with a
NaN, entry 2 with equal maxima in three lanes' columns, the thresholds of tests/test_stream_ctl_kernels_gpu.py; streams in pieces of
1, 255, 256, 257 and random sizes, with and without `last` on the final push.  Warp: F 1 / 2 / 257 / 600, C 1 / 17 / 80, f32 and
f16, one stretch, one per entry (two outside the clamp) and the rates table (with a NaN) over a path with values outside [0, S_b);
streams with a rate per piece and the output ranges rate.settled_length gives."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import _lib, rate  # noqa: E402

DEV = "cuda:0"
B = 3
THR = (256, 1, 10, 2, 3, 0.45)          # max_frames, skip_max, back_max, stall_max, end_slack, min_focus
RATES = (0.5, 0.8, 1.0, 1.25, 2.0)
Q = 1 << 20
KINDS = (("f32", 1, torch.float32), ("f16", 2, torch.float16))


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())


def emit(case, name, t, rc=0):
    h = t if isinstance(t, str) else sha(t).hexdigest()
    print("%s %s %s%s" % (case, name, h, "" if rc == 0 else " rc=%d" % rc), flush=True)


def filled(n, dtype):
    return torch.full((max(1, n),), 12345.0 if dtype.is_floating_point else 123, dtype=dtype, device=DEV)


def ints(values):
    return None if values is None else torch.tensor(values, dtype=torch.int32, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def cuts_of(total, family, seed):
    """piece lengths: all of 1, a first piece of 255 / 256 / 257, or seeded random sizes with an empty piece among them"""
    if family == "1":
        return [1] * total
    if family == "random":
        g, cuts, left = np.random.RandomState(seed), [], total
        while left:
            cuts.append(int(min(left, g.randint(0, 130))))
            left -= cuts[-1]
        return cuts + [0]
    first = min(total, int(family))
    return [first] + ([total - first] if total > first else [])


class Digests:
    """one running sha256 per buffer of a stream: the buffer after every push"""

    def __init__(self, **bufs):
        self.bufs, self.h = bufs, {k: hashlib.sha256() for k in bufs}

    def push(self):
        for k, t in self.bufs.items():
            self.h[k].update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())

    def emit(self, case, rc):
        for k in self.bufs:
            emit(case, k, self.h[k].hexdigest(), rc)


def alignments(N, T, seed):
    """[B, N, T] in [0, 0.5) around a path that advances, one NaN in entry 1, equal maxima in three columns of entry 2's rows"""
    g = np.random.RandomState(seed)
    A = g.rand(B, N, T) * 0.5
    path = np.minimum(np.cumsum(g.randint(0, 3, (B, N)), axis=1) // 2, T - 1)
    for b in range(B):
        A[b, np.arange(N), path[b]] += 0.5
    A[1, N // 2, T // 2] = np.nan
    for t in range(N):
        A[2, t, [t % T, (t + 64) % T, (7 * t + 70) % T]] = 0.75
    return A


def align_cases(lib, st):
    state_words = lib.t2s_align_window_state() // 8
    for T in (1, 65, 257):
        for N in (1, 257, 600):
            A64 = alignments(N, T, 1000 * T + N)
            lens = ((None, None), ([T + 5, 0, max(1, T - 2)], [N + 7, 0, N - 1]), ([-4, T, T // 2 + 1], [-3, N, N // 2]))
            for kind, sk, dt in KINDS:
                ld_row = T + 3
                src = filled(B * N * ld_row, dt).view(B, N, ld_row)
                src[:, :, :T] = torch.from_numpy(A64).to(dt)
                for li, (in_len, out_len) in enumerate(lens):
                    case = "align T%d N%d %s lens%d" % (T, N, kind, li)
                    il, ol = ints(in_len), ints(out_len)
                    pos, peak, bad = filled(B * N, torch.int32), filled(B * N, torch.float32), filled(B * N, torch.uint8)
                    stats, focus = filled(B * 8, torch.int32), filled(B, torch.float64)
                    dur, flags = filled(B * T, torch.int32), filled(B, torch.int32)
                    rc = lib.t2s_align_rows(src.data_ptr(), sk, B, N, T, ld_row, N * ld_row, ptr(il), ptr(ol), pos.data_ptr(),
                                            peak.data_ptr(), bad.data_ptr(), st)
                    for k, t in (("pos", pos), ("peak", peak), ("bad", bad)):
                        emit(case, k, t, rc)
                    rc = lib.t2s_align_stats(pos.data_ptr(), peak.data_ptr(), bad.data_ptr(), B, N, T, ptr(il), ptr(ol), *THR,
                                             stats.data_ptr(), focus.data_ptr(), dur.data_ptr(), flags.data_ptr(), st)
                    for k, t in (("stats", stats), ("focus", focus), ("dur", dur), ("flags", flags)):
                        emit(case, k, t, rc)
                    for family in ("1", "255", "256", "257", "random"):
                        if family == "1" and (N > 257 or li):
                            continue
                        for last_on in (1, 0):
                            align_stream("%s pieces %s last %d" % (case, family, last_on), lib, st, src, sk, N, T, il,
                                         cuts_of(N, family, T + N), last_on, state_words)


def align_stream(case, lib, st, src, sk, N, T, il, cuts, last_on, state_words):
    N_cap, ld_row = N + 3, src.size(2)
    d = Digests(pos=filled(B * N_cap, torch.int32), peak=filled(B * N_cap, torch.float32), bad=filled(B * N_cap, torch.uint8),
                state=filled(B * state_words, torch.int64), stats=filled(B * 8, torch.int32), focus=filled(B, torch.float64),
                dur=filled(B * T, torch.int32), flags=filled(B, torch.int32))
    n0 = rcs = 0
    for q, m in enumerate(cuts):
        piece = src[:, n0:n0 + m].contiguous() if m else None   # entries m ld_row apart
        last = int(last_on and q == len(cuts) - 1)
        rc = lib.t2s_align_window(ptr(piece), sk, B, N_cap, T, n0, n0 + m, last, ld_row, m * ld_row, ptr(il), *THR,
                                  *[d.bufs[k].data_ptr() for k in ("pos", "peak", "bad", "state", "stats", "focus", "dur", "flags")], st)
        rcs = rcs or rc
        n0 += m
        d.push()
    d.emit(case, rcs)


def warp_cases(lib, st):
    T_in, hop = 23, 256
    for F in (1, 2, 257, 600):
        g = np.random.RandomState(F)
        path_h = np.cumsum(g.randint(0, 2, (B, F)), axis=1) % 29 - 2        # values below 0 and at or behind the symbols as well
        path = torch.from_numpy(path_h.astype(np.int32)).to(DEV).contiguous()
        rates_h = (0.3 + 2.0 * g.rand(B, T_in)).astype(np.float32)
        rates_h[0, 3], rates_h[1, 5], rates_h[2, 0] = np.nan, 100.0, 0.01   # a NaN, and values outside [min_rate, max_rate]
        rates = torch.from_numpy(rates_h).to(DEV)
        il = ints([T_in, 17, -2])
        forms = (("stretch", rate.stretch_q(0.8), None, None), ("stretches", Q, torch.tensor([Q // 16, Q + 12345, 9 * Q], device=DEV), None),
                 ("rates", Q, None, rates))
        for C in (1, 17, 80):
            for kind, sk, dt in KINDS:
                x = (torch.randn(B, C, F, generator=torch.Generator().manual_seed(100 * F + C)) * 2).to(dt).to(DEV)
                ld_row = F + 3
                xs = filled(B * C * ld_row, dt).view(B, C, ld_row)
                xs[:, :, :F] = x
                for name, stretch, stretches, table in forms:
                    for li, lengths in enumerate((None, [F + 3, 0, max(1, F // 2)], [-1, F, F])):
                        case = "warp F%d C%d %s %s lens%d" % (F, C, kind, name, li)
                        ln = ints(lengths)
                        cap = 2 * F + 5
                        cum, ol, fl = filled(B * (F + 1), torch.int64), filled(B, torch.int32), filled(B * T_in * 2, torch.int32)
                        rc = lib.t2s_warp_map(ptr(ln), B, F, stretch, ptr(stretches), path.data_ptr(), F, ptr(table), T_in, ptr(il), T_in,
                                              0.5, 2.0, cap, cum.data_ptr(), ol.data_ptr(), fl.data_ptr(), st)
                        for k, t in (("cum", cum), ("out_len", ol), ("first_last", fl)):
                            emit(case, k, t, rc)
                        out = filled(B * C * cap, dt)
                        rc = lib.t2s_warp_gather(xs.data_ptr(), sk, B, C, F, ld_row, C * ld_row, ptr(ln), cum.data_ptr(), ol.data_ptr(),
                                                 out.data_ptr(), cap, st)
                        emit(case, "mel", out, rc)
                        spans = filled(B * T_in * 2, torch.int64)
                        rc = lib.t2s_warp_spans(cum.data_ptr(), fl.data_ptr(), B, F, T_in, ptr(il), ptr(ln), hop, None, None, None, 80, 441,
                                                10 ** 6, None, spans.data_ptr(), st)
                        emit(case, "spans", spans, rc)
                for family in ("1", "255", "256", "257", "random"):
                    if family == "1" and (F > 257 or C != 17):
                        continue
                    warp_stream("warp F%d C%d %s pieces %s" % (F, C, kind, family), lib, st, xs, sk, F, C, path, il, T_in,
                                cuts_of(F, family, F + C))


def warp_stream(case, lib, st, xs, sk, F, C, path, il, T_in, cuts):
    N_cap, ld_row = F + 2, xs.size(2)
    d = Digests(cum=filled(B * (N_cap + 1), torch.int64), first_last=filled(B * T_in * 2, torch.int32))
    mel = hashlib.sha256()
    n = done = rcs = 0
    c = [0, 0]
    for q, m in enumerate(cuts):
        s = rate.stretch_q(RATES[q % len(RATES)])
        if m:
            rc = lib.t2s_warp_window_map(B, N_cap, n, n + m, s, None, path.data_ptr(), F, ptr(il), T_in, d.bufs["cum"].data_ptr(),
                                         d.bufs["first_last"].data_ptr(), st)
            rcs = rcs or rc
            c = [c[1] + (m - 1) * s, c[1] + m * s]
        n += m
        j1 = max(done, rate.settled_length(c[0], c[1], final=q == len(cuts) - 1))
        out = filled(B * C * (j1 - done), xs.dtype)
        rc = lib.t2s_warp_window_gather(xs.data_ptr(), sk, B, C, N_cap, n, ld_row, C * ld_row, d.bufs["cum"].data_ptr(), done, j1,
                                        out.data_ptr(), st)
        rcs = rcs or rc
        done = j1
        d.push()
        mel.update(out.cpu().view(torch.uint8).numpy().tobytes())
    d.emit(case, rcs)
    emit(case, "mel", mel.hexdigest(), rcs)


def main():
    assert torch.cuda.is_available(), "needs the device"
    lib = _lib.load()
    st = _lib.current_stream()
    for cases in (align_cases, warp_cases):
        cases(lib, st)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
