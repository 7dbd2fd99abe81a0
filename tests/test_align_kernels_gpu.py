"""t2s_align_rows / t2s_align_stats (csrc/align.hip, csrc/t2s_api_align.hip) called directly on guarded buffers, against
tests/align_ref.py (pinned by tests/test_align_ref_cpu.py).  Every output buffer is pre-filled with a pattern and lies between
guards; behind every entry's symbols and frames - and between the rows and the entries - the source holds NaN and 1e4, which must
never be seen.  pos, bad, stats, dur and flags equal the restatement, peak bit for bit, focus within 2^-53 (F + 1) mean|peak| of the
correctly rounded mean (a double sum of F terms in any order, and one division), and bit for bit between a solo and a batched call.
The kernels' block sizes are 64 columns and 256 frames, 4 rows to a workgroup: tests/align_cases.py lists shapes on either side."""
import numpy as np
import pytest
import torch

import align_cases as C
import align_ref as R
from text2speech_amd import _lib
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
THR = dict(max_frames=256, skip_max=1, back_max=10, stall_max=2, end_slack=3, min_focus=0.45)
ORDER = ("max_frames", "skip_max", "back_max", "stall_max", "end_slack", "min_focus")


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

    def _is_fill(self, x):
        if isinstance(self.fill, float) and self.fill != self.fill:
            return bool(x.isnan().all())
        return bool((x == self.fill).all())

    def guards_intact(self):
        return self._is_fill(self.raw[:GUARD]) and self._is_fill(self.raw[GUARD + self.t.numel():])

    def untouched(self):
        return self._is_fill(self.raw)

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


def poisoned(A, in_len, out_len):
    """A with NaN and 1e4 alternating behind every entry's symbols and frames"""
    B, N, T = A.shape
    P = np.empty_like(A)
    P.reshape(-1)[0::2] = np.nan
    P.reshape(-1)[1::2] = 1e4
    for b in range(B):
        S = R.clamp(T if in_len is None else in_len[b], 1, T)
        F = R.clamp(N if out_len is None else out_len[b], 0, N)
        P[b, :F, :S] = A[b, :F, :S]
    return P


class Out:
    def __init__(self, B, N, T):
        self.pos, self.peak, self.bad = Buf(B * N, torch.int32, -77), Buf(B * N, torch.float32, NAN), Buf(B * N, torch.uint8, 0xAB)
        self.stats, self.focus = Buf(B * 8, torch.int32, -77), Buf(B, torch.float64, NAN)
        self.dur, self.flags = Buf(B * T, torch.int32, -77), Buf(B, torch.int32, -77)

    def all(self):
        return (self.pos, self.peak, self.bad, self.stats, self.focus, self.dur, self.flags)


def run(lib, P, in_len, out_len, ld_pad=0, entry_pad=5, thr=THR, rows_only=False):
    """both entry points on the dense host array P [B, N, T] laid out with row stride T + ld_pad and entry stride
    N (T + ld_pad) + entry_pad inside a guarded, poisoned buffer -> align_ref.Report of what the device stored"""
    B, N, T = P.shape
    tdt = torch.float16 if P.dtype == np.float16 else torch.float32
    ld_row = T + ld_pad
    ld_entry = N * ld_row + entry_pad
    n_el = (B - 1) * ld_entry + (N - 1) * ld_row + T
    host = np.empty(n_el, dtype=P.dtype)
    host[0::2] = 1e4
    host[1::2] = np.nan
    for b in range(B):
        view = np.lib.stride_tricks.as_strided(host[b * ld_entry:], (N, T), (ld_row * host.itemsize, host.itemsize))
        view[:] = P[b]
    src = Buf(n_el, tdt, 1e4)
    src.t.copy_(torch.from_numpy(host))
    il, ol = _ints(in_len), _ints(out_len)
    o = Out(B, N, T)
    rc = lib.t2s_align_rows(src.ptr(), 2 if P.dtype == np.float16 else 1, B, N, T, ld_row, ld_entry, _ptr(il), _ptr(ol), o.pos.ptr(),
                            o.peak.ptr(), o.bad.ptr(), _st())
    assert rc == 0
    if not rows_only:
        rc = lib.t2s_align_stats(o.pos.ptr(), o.peak.ptr(), o.bad.ptr(), B, N, T, _ptr(il), _ptr(ol), *[thr[k] for k in ORDER],
                                 o.stats.ptr(), o.focus.ptr(), o.dur.ptr(), o.flags.ptr(), _st())
        assert rc == 0
    torch.cuda.synchronize()
    for b in o.all() + (src, il, ol):
        assert b is None or b.guards_intact(), "a guard was written"
    if rows_only:
        assert all(b.untouched() for b in (o.stats, o.focus, o.dur, o.flags))
    return R.Report(o.pos.t.cpu().numpy().reshape(B, N), o.peak.t.cpu().numpy().reshape(B, N), o.bad.t.cpu().numpy().reshape(B, N),
                    o.stats.t.cpu().numpy().reshape(B, 8), o.focus.t.cpu().numpy(), o.dur.t.cpu().numpy().reshape(B, T),
                    o.flags.t.cpu().numpy())


def same(got, want, label=""):
    """every field against the restatement: integers equal, peak bit for bit, focus inside its bound"""
    for name in ("pos", "bad", "stats", "dur", "flags"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s %s: first difference at %s: got %r, want %r (%d differ)" \
            % (label, name, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])], len(bad))
    assert got.peak.dtype == np.float32 and (got.peak.view(np.uint32) == want.peak.view(np.uint32)).all(), (label, "peak bits")
    for b in range(len(want.focus)):
        F = int(want.stats[b, 0])
        bound = R.focus_bound(want.peak[b], F)
        err = abs(float(got.focus[b]) - float(want.focus[b]))
        assert err <= bound, "%s focus[%d]: got %r, want %r, off by %.3e, bound %.3e" % (label, b, got.focus[b], want.focus[b], err, bound)


@pytest.mark.parametrize("case", range(len(C.CASES)), ids=lambda i: "B%d-N%d-T%d-%s" % (C.CASES[i][:3] + ("f16" if C.CASES[i].f16 else "f32",)))
def test_shapes_against_the_restatement(lib, case):
    c = C.CASES[case]
    P = poisoned(C.make(c), c.in_len, c.out_len)
    got = run(lib, P, c.in_len, c.out_len, ld_pad=c.ld_pad)
    same(got, R.report(P, c.in_len, c.out_len, **THR), str(c))


def test_row_pass_alone_writes_its_three_outputs_only(lib):
    c = C.CASES[7]
    P = poisoned(C.make(c), c.in_len, c.out_len)
    got = run(lib, P, c.in_len, c.out_len, ld_pad=c.ld_pad, rows_only=True)
    want = R.rows(P, c.in_len, c.out_len)
    assert (got.pos == want[0]).all() and (got.bad == want[2]).all()
    assert (got.peak.view(np.uint32) == want[1].view(np.uint32)).all()


@pytest.mark.parametrize("which", range(4))
def test_frame_block_edges(lib, which):
    name, c, path, expect = C.edge_cases()[which]
    A = C.make(c, path)
    got = run(lib, A, None, None, ld_pad=c.ld_pad)
    want = R.report(A, **THR)
    assert (want.pos == path).all(), "the path laid out is not the path found"
    for field, value in expect.items():
        assert want.stats[0, field] == value, (name, field, want.stats[0].tolist())
    same(got, want, name)


def test_non_finite_values_inside_the_lengths(lib):
    """a row of NaN, single NaNs, +inf and -inf among the first S columns of the first F rows; the same values behind them"""
    c = C.Case(2, 9, 70, False, 3, [70, 66], [9, 8], 77)
    A = C.make(c)
    A[0, 1, :] = np.nan
    A[0, 2, 69] = np.nan
    A[0, 3, 64] = np.inf
    A[0, 4, :] = -np.inf
    A[1, 0, 65] = -np.inf
    A[1, 7, 0] = np.nan
    A[1, 7, 66:] = np.inf                                       # behind S_1 = 66
    A[1, 8, :] = np.nan                                         # behind F_1 = 8
    got = run(lib, A, c.in_len, c.out_len, ld_pad=c.ld_pad)
    want = R.report(A, c.in_len, c.out_len, **THR)
    assert want.stats[:, 7].tolist() == [4, 2] and want.pos[0, 1] == 0 and want.pos[0, 3] == 64 and want.pos[0, 4] == 0
    assert np.isnan(want.focus[0]) and want.focus[1] > 0
    for name in ("pos", "bad", "stats", "dur", "flags"):
        assert (getattr(got, name) == getattr(want, name)).all(), name
    assert (got.peak.view(np.uint32) == want.peak.view(np.uint32)).all()
    assert np.isnan(got.focus[0]) and abs(got.focus[1] - want.focus[1]) <= R.focus_bound(want.peak[1], 8)
    assert got.flags[0] & R.NONFINITE and got.flags[0] & R.DIFFUSE


def test_ties_go_to_the_smaller_column_across_lanes_and_steps(lib):
    """equal maxima 64 and 128 columns apart (one lane, three steps) and in neighbouring lanes; a row of equal values"""
    A = np.full((1, 5, 200), 0.001, dtype=np.float32)
    A[0, 0, [3, 67, 131]] = 0.5
    A[0, 1, [190, 10, 11]] = 0.5
    A[0, 2, [199, 64]] = 0.25
    A[0, 4, [63, 64]] = 0.75
    got = run(lib, A, None, None)
    assert got.pos[0].tolist() == [3, 10, 64, 0, 63]
    same(got, R.report(A, **THR))
    H = A.astype(np.float16)
    same(run(lib, H, [198], None, ld_pad=1), R.report(H, [198], None, **THR))


def test_an_entry_is_the_same_alone_and_in_any_batch(lib):
    c = C.Case(4, 700, 65, False, 3, [65, 40, 9, 64], [700, 256, 513, 1], 321)
    P = poisoned(C.make(c), c.in_len, c.out_len)
    full = run(lib, P, c.in_len, c.out_len, ld_pad=c.ld_pad)
    same(full, R.report(P, c.in_len, c.out_len, **THR))
    for b in range(4):
        solo = run(lib, P[b:b + 1], c.in_len[b:b + 1], c.out_len[b:b + 1], ld_pad=1)
        # ... and last of three, behind two other entries
        sel = [(b + 1) % 4, (b + 2) % 4, b]
        three = run(lib, P[sel], [c.in_len[i] for i in sel], [c.out_len[i] for i in sel])
        for other, at in ((solo, 0), (three, 2)):
            for name in ("pos", "bad", "stats", "dur", "flags"):
                assert (getattr(other, name)[at] == getattr(full, name)[b]).all(), (b, name)
            assert (other.peak[at].view(np.uint32) == full.peak[b].view(np.uint32)).all()
            assert other.focus[at:at + 1].view(np.uint64)[0] == full.focus[b:b + 1].view(np.uint64)[0], \
                "focus of entry %d differs between batches: %r, %r" % (b, other.focus[at], full.focus[b])


def test_each_flag_follows_its_own_threshold(lib):
    path = [0, 5, 2, 2, 2, 2, 3]                                # skip 5, back 3, stall 4, last 3 of 8 symbols, focus f32(0.9)
    A = np.full((1, 7, 8), 0.0125, dtype=np.float32)
    for t, j in enumerate(path):
        A[0, t, j] = 0.9
    base = dict(max_frames=8, skip_max=5, back_max=3, stall_max=4, end_slack=4, min_focus=0.89)
    assert run(lib, A, None, None, thr=base).flags[0] == 0
    for name, value, bit in (("max_frames", 7, R.TRUNCATED), ("skip_max", 4, R.SKIP), ("back_max", 2, R.BACK),
                             ("stall_max", 3, R.STALL), ("end_slack", 3, R.UNFINISHED), ("min_focus", 0.91, R.DIFFUSE)):
        thr = dict(base, **{name: value})
        got = run(lib, A, None, None, thr=thr)
        assert got.flags[0] == bit == R.report(A, **thr).flags[0], name
        off = dict(thr, **{name: 0.0 if name == "min_focus" else (0 if name == "max_frames" else -1)})
        assert run(lib, A, None, None, thr=off).flags[0] == 0, name
    every = dict(max_frames=1, skip_max=0, back_max=0, stall_max=0, end_slack=0, min_focus=0.95)
    assert run(lib, A, None, None, thr=every).flags[0] == 63
    assert run(lib, A, None, None, thr=R.OFF).flags[0] == 0
    assert run(lib, A, None, [0], thr=R.OFF).flags[0] == R.EMPTY
    A[0, 3, 1] = np.nan
    assert run(lib, A, None, None, thr=R.OFF).flags[0] == R.NONFINITE


def test_invalid_arguments_launch_nothing(lib):
    B, N, T = 2, 6, 10
    src = Buf(B * N * T, torch.float32, 0.5)
    il, ol = _ints([10, 4]), _ints([6, 2])
    o = Out(B, N, T)
    ok_r = dict(A=src.ptr(), src_kind=1, B=B, N=N, T_in=T, ld_row=T, ld_entry=N * T, in_len=il.ptr(), out_len=ol.ptr(), pos=o.pos.ptr(),
                peak=o.peak.ptr(), bad=o.bad.ptr())
    ok_s = dict(pos=o.pos.ptr(), peak=o.peak.ptr(), bad=o.bad.ptr(), B=B, N=N, T_in=T, in_len=il.ptr(), out_len=ol.ptr(), max_frames=0,
                skip_max=1, back_max=1, stall_max=1, end_slack=1, min_focus=0.5, stats=o.stats.ptr(), focus=o.focus.ptr(),
                dur=o.dur.ptr(), flags=o.flags.ptr())
    bad_r = [dict(A=None), dict(pos=None), dict(peak=None), dict(bad=None), dict(src_kind=0), dict(src_kind=3), dict(B=0), dict(B=-1),
             dict(N=0), dict(T_in=0), dict(T_in=-5), dict(ld_row=T - 1), dict(ld_entry=N * T - 1), dict(A=src.ptr() + 2),
             dict(A=src.ptr() + 1, src_kind=2), dict(pos=o.pos.ptr() + 2), dict(peak=o.peak.ptr() + 1), dict(in_len=il.ptr() + 2),
             dict(out_len=ol.ptr() + 1), dict(B=65536, N=32768)]
    bad_s = [dict(pos=None), dict(peak=None), dict(bad=None), dict(stats=None), dict(focus=None), dict(dur=None), dict(flags=None),
             dict(B=0), dict(N=0), dict(N=-1), dict(T_in=0), dict(pos=o.pos.ptr() + 2), dict(peak=o.peak.ptr() + 2),
             dict(stats=o.stats.ptr() + 1), dict(focus=o.focus.ptr() + 4), dict(dur=o.dur.ptr() + 2), dict(flags=o.flags.ptr() + 3),
             dict(in_len=il.ptr() + 1), dict(out_len=ol.ptr() + 2), dict(B=65536, N=32768)]
    for ch in bad_r:
        a = dict(ok_r, **ch)
        assert lib.t2s_align_rows(*[a[k] for k in ok_r], _st()) == -1, "t2s_align_rows accepted %r" % (ch,)
    for ch in bad_s:
        a = dict(ok_s, **ch)
        assert lib.t2s_align_stats(*[a[k] for k in ok_s], _st()) == -1, "t2s_align_stats accepted %r" % (ch,)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in o.all()), "a refused call wrote to an output"
    assert bool((src.raw == 0.5).all())
