"""t2s_align_window / t2s_warp_window_map / t2s_warp_window_gather (the window kernels of csrc/align.hip and csrc/warp.hip) called
directly on guarded, pattern-filled buffers; behind every length - and between the rows and the entries - the sources hold NaN and
1e4, which must never be seen.

The claim under test is the header's: after EVERY push the outputs are what the whole-row entry points give for the prefix, bit for
bit, whatever the cuts.  So after every push the alignment buffers are compared with t2s_align_rows + t2s_align_stats run on the
prefix (integers equal, peak and focus bit for bit, flags masked to the live bits except on the last push), and the concatenation of
the warped pieces with rate.warp_mel of the whole mel; after the last push the alignment outputs are also compared with
tests/align_ref.py under the bounds of tests/test_align_kernels_gpu.py.  The cuts come in families (tests/stream_ctl_ref.py cuts_of):
one piece, pieces of one frame, a cut at 255 / 256 / 257 (the entry pass walks 256 frames a step), seeded random cuts with empty
pieces, an empty final flush."""
import numpy as np
import pytest
import torch

import align_ref as R
import stream_ctl_ref as SC
import warp_ref as W
from text2speech_amd import _lib, rate as RT
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
FAMILIES = ("one", "ones", "255", "256", "257", "random", "flush")
THR = dict(max_frames=256, skip_max=1, back_max=10, stall_max=2, end_slack=3, min_focus=0.45)
ORDER = ("max_frames", "skip_max", "back_max", "stall_max", "end_slack", "min_focus")
RATES = (0.5, 0.8, 1.0, 1.25, 2.0)
KIND = {torch.float32: 1, torch.float16: 2}


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class Buf:
    """A device tensor of n elements inside a larger one: GUARD elements of `fill` on either side, and `fill` inside"""

    def __init__(self, n, dtype, fill):
        self.raw = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.raw[GUARD:GUARD + n]
        self.fill = fill

    def is_fill(self, x):
        if isinstance(self.fill, float) and self.fill != self.fill:
            return bool(x.isnan().all())
        return bool((x == self.fill).all())

    def guards_intact(self):
        return self.is_fill(self.raw[:GUARD]) and self.is_fill(self.raw[GUARD + self.t.numel():])

    def untouched(self):
        return self.is_fill(self.raw)

    def ptr(self):
        return self.t.data_ptr()


def _ints(values):
    if values is None:
        return None
    b = Buf(len(values), torch.int32, -77)
    b.t.copy_(torch.tensor(list(values), dtype=torch.int32))
    return b


def _ptr(b):
    return None if b is None else b.ptr()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _laid_out(P, ld_pad, entry_pad, poison_behind=None):
    """host array P [B, m, T] -> (Buf holding it with row stride T + ld_pad and entry stride m (T + ld_pad) + entry_pad, NaN and 1e4
    everywhere else - and behind poison_behind[b] columns of every row -, ld_row, ld_entry)"""
    B, m, T = P.shape
    tdt = torch.float16 if P.dtype == np.float16 else torch.float32
    ld_row = T + ld_pad
    ld_entry = m * ld_row + entry_pad
    n_el = (B - 1) * ld_entry + (m - 1) * ld_row + T
    host = np.empty(n_el, dtype=P.dtype)
    host[0::2] = 1e4
    host[1::2] = np.nan
    for b in range(B):
        view = np.lib.stride_tricks.as_strided(host[b * ld_entry:], (m, T), (ld_row * host.itemsize, host.itemsize))
        S = T if poison_behind is None else poison_behind[b]
        view[:, :S] = P[b][:, :S]
    src = Buf(n_el, tdt, 1e4)
    src.t.copy_(torch.from_numpy(host))
    return src, ld_row, ld_entry


class AlignWindow:
    """the persistent buffers of one stream of B entries, guarded and pattern-filled, and the push through t2s_align_window"""

    def __init__(self, lib, B, N_cap, T, in_len, thr=THR):
        self.lib, self.B, self.N, self.T, self.thr = lib, B, N_cap, T, thr
        self.in_len = in_len
        self.il = _ints(in_len)
        self.S = [R.clamp(T if in_len is None else in_len[b], 1, T) for b in range(B)]
        self.pos, self.peak, self.bad = Buf(B * N_cap, torch.int32, -77), Buf(B * N_cap, torch.float32, NAN), Buf(B * N_cap, torch.uint8, 0xAB)
        self.state = Buf(B * lib.t2s_align_window_state() // 8, torch.int64, -77)
        self.stats, self.focus = Buf(B * 8, torch.int32, -77), Buf(B, torch.float64, NAN)
        self.dur, self.flags = Buf(B * T, torch.int32, -77), Buf(B, torch.int32, -77)
        self.n = 0

    def all(self):
        return (self.pos, self.peak, self.bad, self.state, self.stats, self.focus, self.dur, self.flags)

    def push(self, P, last, ld_pad=0, entry_pad=5):
        """P [B, m, T] host values of the frames [n, n + m)"""
        m = P.shape[1]
        src = None
        ld_row, ld_entry = self.T + ld_pad, m * (self.T + ld_pad) + entry_pad
        if m:
            src, ld_row, ld_entry = _laid_out(P, ld_pad, entry_pad, self.S)
        rc = self.lib.t2s_align_window(_ptr(src), 2 if P.dtype == np.float16 else 1, self.B, self.N, self.T, self.n, self.n + m, int(last),
                                       ld_row, ld_entry, _ptr(self.il), *[self.thr[k] for k in ORDER], self.pos.ptr(), self.peak.ptr(),
                                       self.bad.ptr(), self.state.ptr(), self.stats.ptr(), self.focus.ptr(), self.dur.ptr(),
                                       self.flags.ptr(), _st())
        assert rc == 0
        self.n += m
        torch.cuda.synchronize()
        for b in self.all() + (src, self.il):
            assert b is None or b.guards_intact(), "a guard was written"
        n = self.n
        for buf in (self.pos, self.peak, self.bad):             # nothing at or behind frame n is written
            assert buf.is_fill(buf.t.view(self.B, self.N)[:, n:])

    def report(self):
        """align_ref.Report of what the device holds for the prefix"""
        B, N, n, T = self.B, self.N, self.n, self.T
        c = lambda buf, *sh: buf.t.view(*sh).cpu().numpy()
        return R.Report(c(self.pos, B, N)[:, :n], c(self.peak, B, N)[:, :n], c(self.bad, B, N)[:, :n], c(self.stats, B, 8),
                        c(self.focus, B), c(self.dur, B, T), c(self.flags, B))


def whole_prefix(lib, A, in_len, thr=THR):
    """t2s_align_rows + t2s_align_stats on the dense host array A [B, n, T] -> align_ref.Report of what the device stored"""
    B, n, T = A.shape
    src, ld_row, ld_entry = _laid_out(A, 0, 0)
    il = _ints(in_len)
    dev = lambda *sh, dt: torch.empty(*sh, dtype=dt, device=DEV)
    pos, peak, bad = dev(B, n, dt=torch.int32), dev(B, n, dt=torch.float32), dev(B, n, dt=torch.uint8)
    stats, focus, dur, flags = dev(B, 8, dt=torch.int32), dev(B, dt=torch.float64), dev(B, T, dt=torch.int32), dev(B, dt=torch.int32)
    P = lambda t: t.data_ptr()
    assert lib.t2s_align_rows(src.ptr(), 2 if A.dtype == np.float16 else 1, B, n, T, ld_row, ld_entry, _ptr(il), None, P(pos), P(peak), P(bad),
                              _st()) == 0
    assert lib.t2s_align_stats(P(pos), P(peak), P(bad), B, n, T, _ptr(il), None, *[thr[k] for k in ORDER], P(stats), P(focus), P(dur),
                               P(flags), _st()) == 0
    torch.cuda.synchronize()
    return R.Report(*[t.cpu().numpy() for t in (pos, peak, bad, stats, focus, dur, flags)])


def same_bits(got, want, last, label):
    """a window Report against the whole-row kernels' Report of the prefix: everything equal, peak and focus bit for bit, flags
    masked to the live bits unless last"""
    for name in ("pos", "bad", "stats", "dur"):
        g, w = getattr(got, name), getattr(want, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s %s: first difference at %s: got %r, want %r" % (label, name, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert got.peak.tobytes() == want.peak.tobytes(), (label, "peak bits")
    assert got.focus.tobytes() == want.focus.tobytes(), (label, "focus bits", got.focus, want.focus)
    wf = want.flags if last else want.flags & SC.LIVE
    assert (got.flags == wf).all(), (label, "flags", got.flags, wf)


def same_as_restatement(got, want, n, label):
    """the last push against tests/align_ref.py: integers equal, peak bit for bit, focus inside 2^-53 (F + 1) mean|peak|"""
    for name in ("pos", "bad", "stats", "dur", "flags"):
        assert (getattr(got, name) == getattr(want, name)).all(), (label, name, getattr(got, name), getattr(want, name))
    assert got.peak.tobytes() == want.peak.tobytes(), (label, "peak bits")
    worst = 0.0
    for b in range(len(want.focus)):
        if np.isfinite(want.focus[b]):
            err, bound = abs(float(got.focus[b]) - float(want.focus[b])), R.focus_bound(want.peak[b], n)
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (label, "focus", b, err, bound)
    return worst


def _pieces(total, family, seed=0):
    cuts = SC.cuts_of(total, family, seed)
    edges = np.concatenate([[0], np.cumsum(cuts)]).astype(int)
    return [(int(a), int(b), i == len(cuts) - 1) for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]


ALIGN_SHAPES = [(T, N) for T in (1, 63, 64, 65, 257) for N in (1, 255, 256, 257, 600)]


@pytest.mark.parametrize("T_in,total", ALIGN_SHAPES)
def test_align_window_is_the_whole_row_result_after_every_push(lib, T_in, total):
    i = ALIGN_SHAPES.index((T_in, total))
    f16 = i % 2 == 1
    B = 3 if (i // 2) % 2 == 0 else 1
    in_len = ([T_in + 5, 0, T_in] if i % 3 else [max(1, T_in - 2), T_in, -4]) if B == 3 else (None if i % 4 == 1 else [T_in])
    A = R.random_alignments(B, total, T_in, np.float16 if f16 else np.float32, 31 * i + 5, in_len)
    want_end = R.report(A, in_len, None, **THR)
    worst, pushes = 0.0, 0
    for family in FAMILIES:
        if family == "ones" and total > 257:
            continue
        w = AlignWindow(lib, B, total + 3, T_in, in_len)
        refs = {}
        for a, b, last in _pieces(total, family, i):
            w.push(A[:, a:b], last, ld_pad=(0, 3, 8)[(i + b) % 3])
            if b not in refs:                                   # (the whole-row kernels on this prefix: once per length)
                refs[b] = whole_prefix(lib, A[:, :b], in_len) if b else None
            got = w.report()
            pushes += 1
            if b:
                same_bits(got, refs[b], last, (family, T_in, total, b))
            else:
                assert (got.stats[:, 0] == 0).all() and (got.flags == 0).all() and (got.dur == 0).all()
        worst = max(worst, same_as_restatement(w.report(), want_end, total, (family, T_in, total)))
    print("align window T_in %d, %d frames, B %d %s: %d pushes equal to the whole-row kernels on the prefix; focus vs restatement "
          "worst %.3f of its bound" % (T_in, total, B, "f16" if f16 else "f32", pushes, worst))


def _path_case(name):
    t = np.arange(600)
    if name == "stall across a cut and the block edge":
        return np.where(t < 250, t // 13, np.where(t < 263, 20, 21 + (t - 263) // 13)), [256, 344]
    if name == "stall across two cuts":
        return np.where(t < 100, t // 13, np.where(t < 300, 8, 9 + (t - 300) // 13)), [150, 100, 350]
    if name == "steps at a cut":
        return np.where(t < 256, t // 13, np.where(t < 512, 30 + (t - 256) // 13, 40 + (t - 512) // 13)), [256, 256, 88]
    raise ValueError(name)


@pytest.mark.parametrize("name", ["stall across a cut and the block edge", "stall across two cuts", "steps at a cut"])
def test_align_window_on_hand_built_paths(lib, name):
    path, cuts = _path_case(name)
    N, T = len(path), 65
    A = R.random_alignments(1, N, T, np.float32, 5, None, path[None])
    w = AlignWindow(lib, 1, N, T, None)
    ref = SC.AlignChunks(1, T, None, **THR)
    edges = np.concatenate([[0], np.cumsum(cuts)]).astype(int)
    for k in range(len(cuts)):
        last = k == len(cuts) - 1
        a, b = int(edges[k]), int(edges[k + 1])
        w.push(A[:, a:b], last)
        got = w.report()
        same_bits(got, whole_prefix(lib, A[:, :b], None), last, (name, k))
        want = ref.push(A[:, a:b], last)
        assert (got.stats == want.stats).all() and (got.flags == want.flags).all() and got.focus.tobytes() == want.focus.tobytes()
    print("%s: stats %s flags %d" % (name, got.stats[0].tolist(), int(got.flags[0])))
    if name == "stall across a cut and the block edge":         # the run open at the cut counts as it stands: 6 frames, then 7
        o = AlignWindow(lib, 1, N, T, None, dict(R.OFF, stall_max=6))
        o.push(A[:, 247:256], False)
        first = o.report()
        o.push(A[:, 256:257], False)
        assert first.stats[0, 4] == 6 and first.flags[0] == 0 and o.report().stats[0, 4] == 7 and o.report().flags[0] == R.STALL


def test_align_window_ties_across_lanes_and_a_non_finite_row_in_the_second_piece(lib):
    T, N = 130, 40
    A = R.random_alignments(2, N, T, np.float32, 9)
    for t in range(N):                                          # equal maxima in three lanes' columns: the smallest column wins
        A[0, t, [5 + t % 3, 69, 70 + t % 50]] = 0.75
    A[1, 3] = 0.25                                              # a constant row: column 0
    A[1, 25, 77] = np.nan
    A[1, 30, 2] = np.inf
    w = AlignWindow(lib, 2, N, T, None, R.OFF)
    w.push(A[:, :20], False)
    first = w.report()
    assert (first.flags == 0).all() and first.stats[1, 7] == 0
    same_bits(first, whole_prefix(lib, A[:, :20], None, R.OFF), False, "first piece")
    w.push(A[:, 20:], True)
    got = w.report()
    same_bits(got, whole_prefix(lib, A, None, R.OFF), True, "second piece")
    same_as_restatement(got, R.report(A, None, None, **R.OFF), N, "ties and non-finite")
    assert got.pos[0].tolist() == [5 + t % 3 for t in range(N)] and got.pos[1, 3] == 0 and got.pos[1, 30] == 2
    assert got.flags.tolist() == [0, R.NONFINITE] and got.stats[1, 7] == 2


def test_align_window_flag_bits_each_by_its_own_threshold(lib):
    N, T = 300, 33
    path = np.concatenate([np.arange(100) // 5, np.full(40, 20), [27], np.arange(159) // 9 + 12])[:N]     # a stall, a skip, a step back
    A = R.random_alignments(1, N, T, np.float32, 2, None, path[None])
    st = R.report(A, None, None, **R.OFF)
    skip, back, stall, last_pos = (int(st.stats[0, k]) for k in (2, 3, 4, 5))
    assert skip == 7 and back == 15 and stall == 40
    focus = float(whole_prefix(lib, A, None, R.OFF).focus[0])

    def flags(last, cuts=(170, 130), **thr):
        w = AlignWindow(lib, 1, N, T, None, dict(R.OFF, **thr))
        a = 0
        for k, m in enumerate(cuts):
            w.push(A[:, a:a + m], last and k == len(cuts) - 1)
            a += m
        return int(w.report().flags[0])
    for last in (False, True):
        assert flags(last, skip_max=skip) == 0 and flags(last, skip_max=skip - 1) == R.SKIP
        assert flags(last, back_max=back) == 0 and flags(last, back_max=back - 1) == R.BACK
        assert flags(last, stall_max=stall) == 0 and flags(last, stall_max=stall - 1) == R.STALL
    assert flags(True, max_frames=N + 1) == 0 and flags(True, max_frames=N) == R.TRUNCATED and flags(False, max_frames=N) == 0
    slack = T - 1 - last_pos
    assert slack > 0 and flags(True, end_slack=slack) == 0 and flags(True, end_slack=slack - 1) == R.UNFINISHED
    assert flags(False, end_slack=slack - 1) == 0
    assert flags(True, min_focus=focus) == 0 and flags(True, min_focus=float(np.nextafter(focus, 1.0))) == R.DIFFUSE
    assert flags(False, min_focus=1.0) == 0
    # the stall is flagged by the push in which it crosses the threshold, not at the utterance's end
    assert flags(False, cuts=(100 + stall - 1,), stall_max=stall - 1) == 0 and flags(False, cuts=(100 + stall,), stall_max=stall - 1) == R.STALL
    e = AlignWindow(lib, 1, N, T, None, R.OFF)
    e.push(A[:, :0], True)
    assert int(e.report().flags[0]) == R.EMPTY and e.report().stats[0].tolist() == [0, T, 0, 0, 0, -1, 0, 0] and e.report().focus[0] == 0.0
    e = AlignWindow(lib, 1, N, T, None, R.OFF)
    e.push(A[:, :0], False)
    assert int(e.report().flags[0]) == 0


def test_refused_tuples_write_nothing(lib):
    B, N, T = 2, 50, 9
    w = AlignWindow(lib, B, N, T, [9, 4])
    src, ld_row, ld_entry = _laid_out(R.random_alignments(B, 8, T, np.float32, 1), 0, 0)
    ok = dict(A=src.ptr(), kind=1, B=B, N=N, T=T, n0=0, n=8, last=0, ld_row=ld_row, ld_entry=ld_entry, in_len=w.il.ptr(), mf=0, sk=-1, bk=-1,
              sl=-1, es=-1, fo=0.0, pos=w.pos.ptr(), peak=w.peak.ptr(), bad=w.bad.ptr(), state=w.state.ptr(), stats=w.stats.ptr(),
              focus=w.focus.ptr(), dur=w.dur.ptr(), flags=w.flags.ptr())
    for ch in (dict(A=None), dict(kind=0), dict(B=0), dict(N=0), dict(T=0), dict(n0=-1), dict(n0=9), dict(n=N + 1), dict(last=-1),
               dict(ld_row=T - 1), dict(ld_entry=8 * ld_row - 1), dict(pos=None), dict(state=None), dict(flags=None), dict(focus=w.focus.ptr() + 4),
               dict(A=src.ptr() + 2), dict(N=2 ** 30 + 1)):
        a = dict(ok, **ch)
        assert lib.t2s_align_window(*a.values(), _st()) == -1, "t2s_align_window accepted %r" % (ch,)
    cum, fl = Buf(B * (N + 1), torch.int64, -77), Buf(B * T * 2, torch.int32, -77)
    ok = dict(B=B, N=N, n0=0, n=8, stretch=W.Q, stretches=None, path=w.pos.ptr(), ld_path=N, in_len=w.il.ptr(), T=T, cum=cum.ptr(),
              fl=fl.ptr())
    for ch in (dict(B=0), dict(N=0), dict(n0=-1), dict(n0=9), dict(n=N + 1), dict(stretch=W.Q // 8 - 1), dict(stretch=8 * W.Q + 1), dict(path=None),
               dict(ld_path=7), dict(T=0), dict(cum=None), dict(cum=cum.ptr() + 4)):
        a = dict(ok, **ch)
        assert lib.t2s_warp_window_map(*a.values(), _st()) == -1, "t2s_warp_window_map accepted %r" % (ch,)
    x, out = Buf(B * 3 * 8, torch.float32, 1e4), Buf(B * 3 * 4, torch.float32, NAN)
    ok = dict(x=x.ptr(), kind=1, B=B, C=3, N=N, n=8, ld_row=8, ld_entry=24, cum=cum.ptr(), j0=0, j1=4, out=out.ptr())
    for ch in (dict(x=None), dict(kind=3), dict(B=0), dict(C=0), dict(N=0), dict(n=0), dict(n=N + 1), dict(ld_row=7), dict(ld_entry=23),
               dict(cum=None), dict(j0=-1), dict(j0=5), dict(out=None), dict(out=x.ptr() + 16), dict(out=out.ptr() + 2)):
        a = dict(ok, **ch)
        assert lib.t2s_warp_window_gather(*a.values(), _st()) == -1, "t2s_warp_window_gather accepted %r" % (ch,)
    assert lib.t2s_warp_window_gather(*dict(ok, j0=3, j1=3).values(), _st()) == 0                           # nothing asked for
    torch.cuda.synchronize()
    for b in w.all() + (cum, fl, out):
        assert b.untouched(), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------- the warp
class WarpWindow:
    """one stream of B entries through t2s_warp_window_map / t2s_warp_window_gather on guarded buffers: the source mel is laid out
    with row stride N_cap + ld_pad and holds NaN / 1e4 at every frame that has not been pushed yet"""

    def __init__(self, lib, B, C, N_cap, dtype, ld_pad=3, path=None, T_in=0, in_len=None):
        self.lib, self.B, self.C, self.N, self.dtype = lib, B, C, N_cap, dtype
        self.ld_row = N_cap + ld_pad
        self.ld_entry = C * self.ld_row + 7
        n_el = (B - 1) * self.ld_entry + (C - 1) * self.ld_row + N_cap
        self.x = Buf(n_el, dtype, 1e4)
        self.x.t[0::2] = NAN
        self.cum = Buf(B * (N_cap + 1), torch.int64, -77)
        self.path, self.T_in, self.il = path, T_in, _ints(in_len)
        self.fl = Buf(B * T_in * 2, torch.int32, -77) if path is not None else None
        self.n = self.out = 0
        self.c = [0, 0]

    def rows(self, b):
        return torch.as_strided(self.x.t, (self.C, self.N), (self.ld_row, 1), self.x.t.storage_offset() + b * self.ld_entry)

    def push(self, piece, last, rate):
        """piece [B, C, m] on the device -> the settled warped columns [B, C, m']"""
        m = piece.size(2)
        n0, n, s = self.n, self.n + m, RT.stretch_q(rate)
        for b in range(self.B):
            self.rows(b)[:, n0:n] = piece[b]
        if m:
            rc = self.lib.t2s_warp_window_map(self.B, self.N, n0, n, s, None, None if self.path is None else self.path.data_ptr(),
                                              0 if self.path is None else self.path.size(1), _ptr(self.il), self.T_in, self.cum.ptr(),
                                              _ptr(self.fl), _st())
            assert rc == 0
            self.c = [self.c[1] + (m - 1) * s, self.c[1] + m * s]
        self.n = n
        j0, j1 = self.out, max(self.out, RT.settled_length(self.c[0], self.c[1], final=last))
        assert j1 - j0 == max(0, SC.settled(self.c[0], self.c[1], last) - j0)
        out = Buf(self.B * self.C * (j1 - j0), self.dtype, NAN)
        rc = self.lib.t2s_warp_window_gather(self.x.ptr(), KIND[self.dtype], self.B, self.C, self.N, n, self.ld_row, self.ld_entry,
                                             self.cum.ptr(), j0, j1, out.ptr(), _st())
        assert rc == 0 or (n == 0 and j1 == j0)
        self.out = j1
        torch.cuda.synchronize()
        for b in (self.x, self.cum, self.fl, out):
            assert b is None or b.guards_intact(), "a guard was written"
        assert self.cum.is_fill(self.cum.t.view(self.B, self.N + 1)[:, n + 1:])
        return out.t.view(self.B, self.C, j1 - j0)


def _mel(B, C, F, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, F, generator=g) * 2).to(dtype)
    if F > 4:
        x[0, 0, 3] = -0.0
    return x.to(DEV)


WARP_SHAPES = [(F, C) for F in (1, 2, 255, 256, 257, 600) for C in (1, 17, 80)]


@pytest.mark.parametrize("F,C", WARP_SHAPES)
def test_warp_window_pieces_are_warp_mel_bit_for_bit(lib, F, C):
    i = WARP_SHAPES.index((F, C))
    dtype = torch.float16 if i % 2 else torch.float32
    B = 2 if i % 3 == 0 else 1
    x = _mel(B, C, F, dtype, i)
    runs = 0
    for r, rate in enumerate(RATES):
        want = RT.warp_mel(x, None, rate)
        length = RT.warped_length(F, rate)
        assert want.mel.size(2) == length == int(want.host_lengths[0])
        for family in FAMILIES:
            if family == "ones" and (F > 257 or r != i % len(RATES)):
                continue                                        # pieces of one frame: one rate a shape, totals up to 257
            w = WarpWindow(lib, B, C, F + 2, dtype, ld_pad=(3, 1, 5)[i % 3])
            got = [w.push(x[:, :, a:b], last, rate) for a, b, last in _pieces(F, family, i)]
            got = torch.cat(got, 2)
            assert got.shape == want.mel.shape and torch.equal(_bits32(got), _bits32(want.mel)), (family, F, C, rate)
            assert torch.equal(w.cum.t.view(B, F + 3)[:, :F + 1], want.cum), (family, "cum")
            if rate == 1.0:
                assert torch.equal(_bits32(got), _bits32(x))
            runs += 1
    print("warp window F %d C %d B %d %s: %d streams bit-equal to warp_mel at rates %s" % (F, C, B, dtype, runs, RATES))


def _bits32(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("F,dtype", [(2, torch.float32), (257, torch.float16), (600, torch.float32)])
def test_warp_window_rate_per_piece_is_the_symbol_rate_form(lib, F, dtype):
    x = _mel(1, 17, F, dtype, F)
    pieces = _pieces(F, "random", 3)
    rates = [RATES[(k + 1) % len(RATES)] for k in range(len(pieces))]
    index = torch.zeros(1, F, dtype=torch.int32)
    for k, (a, b, _) in enumerate(pieces):
        index[0, a:b] = k
    want = RT.warp_mel(x, None, 1.0, path=index.to(DEV), symbol_rates=torch.tensor([rates], dtype=torch.float32, device=DEV))
    w = WarpWindow(lib, 1, 17, F, dtype)
    got = torch.cat([w.push(x[:, :, a:b], last, r) for (a, b, last), r in zip(pieces, rates)], 2)
    length = int(want.lengths[0])
    print("rate per piece, F %d in %d pieces at %s: %d output frames" % (F, len(pieces), rates, length))
    assert got.size(2) == length and torch.equal(_bits32(got), _bits32(want.mel[:, :, :length]))
    assert torch.equal(w.cum.t.view(1, F + 1), want.cum)


@pytest.mark.parametrize("F,family", [(257, "256"), (257, "ones"), (600, "random"), (600, "flush")])
def test_first_last_and_spans_after_every_push(lib, F, family):
    B, T_in, hop = 2, 23, 256
    rng = np.random.RandomState(F)
    path_h = np.cumsum(rng.randint(0, 2, (B, F)), axis=1) % 29 - 2         # values below 0 and at or behind the symbols as well
    path_h[1, F // 2:] = path_h[1, :F - F // 2]                             # entry 1 visits its symbols twice
    in_len = [23, 17]
    path = torch.full((B, F + 2), -5, dtype=torch.int32)
    path[:, :F] = torch.from_numpy(path_h.astype(np.int32))
    path = path.to(DEV)
    x = _mel(B, 3, F, torch.float32, 1)
    w = WarpWindow(lib, B, 3, F + 2, torch.float32, path=path, T_in=T_in, in_len=in_len)
    il = torch.tensor(in_len, dtype=torch.int32, device=DEV)
    checked = 0
    for a, b, last in _pieces(F, family, 2):
        w.push(x[:, :, a:b], last, 0.8)
        if b == 0:
            continue
        _, _, fl = RT._map(torch.device(DEV), B, b, None, [RT.stretch_q(0.8)] * B, 1, path[:, :b].contiguous(), b, None, 0, il, T_in, want_cum=False)
        got_fl = w.fl.t.view(B, T_in, 2)
        assert torch.equal(got_fl, fl), (family, b)
        for e in range(B):
            assert (got_fl[e].cpu().numpy() == W.first_last(path_h[e, :b], b, in_len[e], T_in)).all()
        whole = RT.warp_mel(x[:, :, :b], None, 0.8, path=path[:, :b].contiguous(), input_lengths=il, n_symbols=T_in)
        want = RT.symbol_spans(whole, None, il, None, hop, ratio=(80, 441), total=10 ** 6)
        got = RT.symbol_spans(RT.WarpedMel(None, None, w.cum.t.view(B, F + 3), got_fl, None), None, il, [b] * B, hop, ratio=(80, 441),
                              total=10 ** 6)
        assert torch.equal(got, want), (family, b)
        checked += 1
    print("first_last and spans, F %d, cuts %s: equal to t2s_warp_map / t2s_warp_spans on the prefix after each of %d pushes" % (F, family, checked))


def test_warp_stream_and_alignment_stream_classes(lib):
    """the two classes over the same kernels: B = 2, a rate changed between pushes, and exactly settled_length's count per push"""
    from text2speech_amd import alignment
    B, C, F, T = 2, 80, 300, 40
    x = _mel(B, C, F, torch.float32, 4)
    A_h = R.random_alignments(B, F, T, np.float32, 8)
    A = torch.from_numpy(A_h).to(DEV)
    check = alignment.AlignmentCheck(skip_max=1, back_max=10, stall_max=2, end_slack=3, min_focus=0.45)
    al = alignment.AlignmentStream(check, T, F + 5, DEV, B=B)
    ws = RT.WarpStream(C, F + 5, torch.float32, DEV, 0.8, B=B, path=al.path, n_symbols=T)
    refs = [SC.WarpChunks(C, np.float32) for _ in range(B)]
    pieces = _pieces(F, "random", 1)
    rates = [0.8 if k < 2 else 1.25 for k in range(len(pieces))]
    got = []
    for (a, b, last), r in zip(pieces, rates):
        al.push(A[:, a:b], last)
        got.append(ws.push(x[:, :, a:b], last, rate=r))
        for e in range(B):      # the count is settled_length's; the values are warp_mel's bits (below), the restatement's within a rounding
            want = refs[e].push(x[e, :, a:b].cpu().numpy(), last, W.stretch_q(r))
            assert got[-1].size(2) == want.shape[1] and ws.frames_in == b and ws.frames_out == refs[e].out
            err = np.abs(got[-1][e].cpu().numpy().astype(np.float64) - want.astype(np.float64))
            # (one float32 rounding of two doubles that differ by a few 2^-53 (|x[f]| + |x[f + 1]|), |x| < 16: the device contracts
            # the expression into a fused multiply-add, numpy does not)
            assert (err <= 2.0 ** -23 * np.abs(want.astype(np.float64)) + 2.0 ** -40).all()
        rep = al.report()
        whole = alignment.alignment_report(A[:, :b], check=check.with_max_frames(F + 5)) if b else None
        if b:
            assert torch.equal(rep.path, whole.path) and torch.equal(rep.stats, whole.stats) and torch.equal(rep.durations, whole.durations)
            assert torch.equal(_bits(rep.focus), _bits(whole.focus))
            assert torch.equal(rep.flags, whole.flags if last else whole.flags & alignment.LIVE)
            fl, st = al.wait()
            assert torch.equal(fl, rep.flags.cpu()) and torch.equal(st, rep.stats.cpu())
    assert al.poll() is not None and torch.equal(al.poll()[0], al.wait()[0])
    assert torch.equal(ws.cum[:, :F + 1].cpu(), torch.tensor([refs[0].c] * B))
    switch = pieces[2][0] if len(pieces) > 2 else F
    index = (torch.arange(F) >= switch).to(torch.int32).repeat(B, 1).to(DEV)
    whole_w = RT.warp_mel(x, None, 1.0, path=index, symbol_rates=torch.tensor([[0.8, 1.25]] * B, device=DEV))
    got = torch.cat(got, 2)
    assert got.size(2) == int(whole_w.lengths[0]) and torch.equal(_bits32(got), _bits32(whole_w.mel[:, :, :got.size(2)]))
    for e in range(B):
        assert (ws.first_last[e].cpu().numpy() == W.first_last(rep.path[e].cpu().numpy(), F, T, T)).all()
    with pytest.raises(_lib.T2SError):
        ws.push(x[:, :, :1], False)
    with pytest.raises(_lib.T2SError):
        al.push(A[:, :1], False)
