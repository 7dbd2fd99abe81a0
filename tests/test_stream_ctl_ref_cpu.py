"""tests/stream_ctl_ref.py (the control inside a stream, restated piece by piece) against the whole-row restatements
tests/align_ref.py and tests/warp_ref.py for any cuts; rate.settled_length against its definition; the entry points' refusals and
StreamControl's argument errors.  No device."""
import ctypes

import numpy as np
import pytest

import align_ref as R
import stream_ctl_ref as SC
import warp_ref as W
from text2speech_amd import _lib, rate as RT

Q = W.Q
FAMILIES = ("one", "ones", "255", "256", "257", "random", "flush")
THR = dict(max_frames=256, skip_max=1, back_max=10, stall_max=2, end_slack=3, min_focus=0.45)
RATES = (0.5, 0.8, 1.0, 1.25, 2.0)


def _pieces(total, family, seed=0):
    cuts = SC.cuts_of(total, family, seed)
    assert sum(cuts) == total
    edges = np.concatenate([[0], np.cumsum(cuts)]).astype(int)
    return [(int(a), int(b), i == len(cuts) - 1) for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]


def _same_prefix(got, whole, n, last, label):
    """a chunked Report against the whole-row restatement of the prefix: integers equal, peak bit for bit, flags masked to the live
    bits unless last, focus the device order's bits and inside align_ref's bound of the correctly rounded mean"""
    for name in ("pos", "bad", "stats", "dur"):
        assert (getattr(got, name) == getattr(whole, name)).all(), (label, name)
    assert got.peak.tobytes() == whole.peak.tobytes(), (label, "peak")
    assert (got.flags == (whole.flags if last else whole.flags & SC.LIVE)).all(), (label, "flags", got.flags, whole.flags)
    for b in range(len(whole.focus)):
        dev = SC.device_focus(whole.peak[b], n)
        assert np.float64(got.focus[b]).tobytes() == np.float64(dev).tobytes() or (got.focus[b] != got.focus[b] and dev != dev), (label, "focus")
        if np.isfinite(whole.focus[b]):
            assert abs(got.focus[b] - whole.focus[b]) <= R.focus_bound(whole.peak[b], n), (label, "focus bound")


def _with_families(shapes):
    """every shape with every family of cuts; pieces of one frame for totals up to 257"""
    return [(f,) + sh for sh in shapes for f in FAMILIES if f != "ones" or sh[0] <= 257]


@pytest.mark.parametrize("family,total,T_in", _with_families([(1, 1), (255, 63), (256, 64), (257, 65), (600, 17)]))
def test_chunked_alignment_check_is_the_whole_row_one(family, total, T_in):
    B = 2
    in_len = [T_in, max(1, T_in - 3)]
    A = R.random_alignments(B, total, T_in, np.float32 if total % 2 else np.float16, 7 * total + T_in, in_len)
    ch = SC.AlignChunks(B, T_in, in_len, **THR)
    for a, b, last in _pieces(total, family, T_in):
        got = ch.push(A[:, a:b], last)
        _same_prefix(got, R.report(A[:, :b], in_len, None, **THR), b, last, (family, total, T_in, b))


def _path_case(name):
    """hand-built paths -> (path [N], cuts, expected stats fields at the end)"""
    t = np.arange(600)
    if name == "stall across a cut and the block edge":       # symbol 20 from frame 250 to 262: 13 frames over the cut at 256
        return np.where(t < 250, t // 13, np.where(t < 263, 20, 21 + (t - 263) // 13)), [256, 344], dict(longest_stall=13)
    if name == "stall across two cuts":
        return np.where(t < 100, t // 13, np.where(t < 300, 8, 9 + (t - 300) // 13)), [150, 100, 350], dict(longest_stall=200)
    if name == "steps at a cut":                               # the largest skip between 255 | 256, the largest step back at 511 | 512
        p = np.where(t < 256, t // 13, np.where(t < 512, 30 + (t - 256) // 13, 40 + (t - 512) // 13))
        return p, [256, 256, 88], dict(max_skip=30 - 255 // 13, max_back=30 + 255 // 13 - 40)
    raise ValueError(name)


@pytest.mark.parametrize("name", ["stall across a cut and the block edge", "stall across two cuts", "steps at a cut"])
def test_chunked_alignment_check_on_hand_built_paths(name):
    path, cuts, want = _path_case(name)
    N, T = len(path), 65
    A = R.random_alignments(1, N, T, np.float32, 5, None, path[None])
    ch = SC.AlignChunks(1, T, None, **THR)
    edges = np.concatenate([[0], np.cumsum(cuts)]).astype(int)
    assert edges[-1] == N
    for i in range(len(cuts)):
        last = i == len(cuts) - 1
        got = ch.push(A[:, edges[i]:edges[i + 1]], last)
        _same_prefix(got, R.report(A[:, :edges[i + 1]], None, None, **THR), int(edges[i + 1]), last, (name, i))
    names = ("frames", "symbols", "max_skip", "max_back", "longest_stall", "last_pos", "covered", "bad_rows")
    for k, v in want.items():
        assert got.stats[0, names.index(k)] == v, (name, k, got.stats[0])
    if name == "stall across a cut and the block edge":         # a stall is seen while it happens: the run open at a cut counts
        first = SC.AlignChunks(1, T, None, **dict(THR, stall_max=6)).push(A[:, :256], False)
        assert first.stats[0, 4] == 13 and first.flags[0] & R.STALL        # (every symbol before it holds 13 frames)
        open_run = SC.AlignChunks(1, T, None, **dict(R.OFF, stall_max=6))
        assert open_run.push(A[:, 247:256], False).stats[0, 4] == 6 and open_run.push(A[:, 256:257], False).stats[0, 4] == 7


def test_a_non_finite_row_in_the_second_piece():
    A = R.random_alignments(1, 40, 9, np.float32, 3)
    A[0, 25, 4] = np.nan
    ch = SC.AlignChunks(1, 9, None, **R.OFF)
    assert ch.push(A[:, :20], False).flags[0] == 0
    got = ch.push(A[:, 20:], False)
    assert got.flags[0] == R.NONFINITE and got.stats[0, 7] == 1
    _same_prefix(got, R.report(A, None, None, **R.OFF), 40, False, "nan")


@pytest.mark.parametrize("family,F,C", _with_families([(1, 1), (2, 17), (255, 3), (256, 2), (257, 5), (600, 4)]))
def test_chunked_warp_is_the_whole_row_one(family, F, C):
    rng = np.random.RandomState(F + C)
    dtype = np.float32 if (F + C) % 2 else np.float16
    x = rng.uniform(-4, 4, (C, F)).astype(dtype)
    path = np.cumsum(rng.randint(0, 2, F)) % 11
    for rate in RATES:
        s = W.stretch_q(rate)
        c, n_out = W.cum_map(s, F, F)
        want = W.warp_entry(x, c, F, n_out, n_out)[0]
        ch = SC.WarpChunks(C, dtype, path, 11, 11)
        got = []
        for a, b, last in _pieces(F, family, C):
            got.append(ch.push(x[:, a:b], last, s))
            assert got[-1].shape[1] == ch.out - sum(g.shape[1] for g in got[:-1])
            assert (ch.fl == W.first_last(path[:b], b, 11, 11)).all(), (family, F, rate, b)
            assert ch.c == c[:b + 1].tolist()
        got = np.concatenate(got, 1)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (family, F, C, rate)
        assert n_out == W.warped_length(F, rate)
        if rate == 1.0:
            assert got.tobytes() == x.tobytes()


@pytest.mark.parametrize("F", [2, 257, 600])
def test_a_rate_per_piece_is_the_symbol_rate_form(F):
    rng = np.random.RandomState(F)
    x = rng.uniform(-4, 4, (3, F)).astype(np.float32)
    pieces = _pieces(F, "random", 3)
    rates = [RATES[i % len(RATES)] for i in range(len(pieces))]
    index = np.zeros(F, dtype=np.int64)
    for i, (a, b, _) in enumerate(pieces):
        index[a:b] = i
    s = W.symbol_stretches(index, np.array(rates, dtype=np.float32), len(pieces))
    c, n_out = W.cum_map(s, F, F)
    want = W.warp_entry(x, c, F, n_out, n_out)[0]
    ch = SC.WarpChunks(3, np.float32)
    got = np.concatenate([ch.push(x[:, a:b], last, W.stretch_q(r)) for (a, b, last), r in zip(pieces, rates)], 1)
    assert got.tobytes() == want.tobytes()


def _check_settled(stretches):
    """settled_length along a map whose frame f has stretches[f]: the brute-force count, monotone, never above the warped length,
    equal to it on the final push"""
    c = [0]
    before = 0
    for n in range(0, len(stretches) + 1):
        if n:
            c.append(c[-1] + stretches[n - 1])
        c_prev = c[n - 1] if n else 0
        got = RT.settled_length(c_prev, c[n])
        final = RT.settled_length(c_prev, c[n], final=True)
        assert got == SC.settled(c_prev, c[n]) == sum(1 for j in range(8 * n + 2) if (2 * j + 1) * Q <= c_prev + c[n])
        assert final == SC.settled(c_prev, c[n], True) == (0 if n == 0 else max(1, (c[n] + Q // 2) >> 20))
        assert before <= got <= final
        before = got
    return c


@pytest.mark.parametrize("rate", RATES)
def test_settled_length_at_a_uniform_rate(rate):
    s = RT.stretch_q(rate)
    c = _check_settled([s] * 300)
    for n in range(301):
        assert RT.settled_length(c[n - 1] if n else 0, c[n], final=True) == RT.warped_length(n, rate) == W.warped_length(n, rate)
        if rate == 1.0:
            assert RT.settled_length(c[n - 1] if n else 0, c[n]) == n


def test_settled_length_at_a_rate_that_changes_at_every_cut():
    rng = np.random.RandomState(11)
    s = []
    while len(s) < 300:
        s += [RT.stretch_q(RATES[int(rng.randint(0, len(RATES)))])] * int(rng.randint(1, 40))
    _check_settled(s[:300])
    for bad in [(-1, 0), (5, 4), (True, 2), (1.5, 2), (None, 1)]:
        with pytest.raises(ValueError):
            RT.settled_length(*bad)


def test_stream_control_arguments():
    from text2speech_amd import alignment, streaming
    ctl = streaming.StreamControl()
    assert ctl.speed is None and ctl.check is None and ctl.on_fail == "stop" and ctl.timestamps is False
    assert (ctl.frames_in, ctl.frames_out, ctl.flags, ctl.aborted) == (0, 0, 0, False)
    for bad in (0.1, 9.0, float("nan"), "fast", True):
        with pytest.raises(ValueError):
            streaming.StreamControl(speed=bad)
        with pytest.raises(ValueError):
            ctl.speed = bad
    ctl.speed = 1.25
    assert ctl.speed == 1.25
    with pytest.raises(_lib.T2SError):
        streaming.StreamControl(check=dict(stall_max=3))
    with pytest.raises(ValueError):
        streaming.StreamControl(on_fail="raise")
    with pytest.raises(ValueError):
        streaming.StreamControl(timestamps=1)
    streaming.StreamControl(0.8, alignment.AlignmentCheck(stall_max=30), "flag", True)
    for what in (ctl.report, ctl.spans, lambda: ctl.path):
        with pytest.raises(_lib.T2SError):
            what()
    ctl._begin(1000, 256)
    with pytest.raises(_lib.T2SError, match="one utterance"):
        ctl._begin(1000, 256)
    plain = streaming.StreamControl()
    plain._begin(1000, 256)
    with pytest.raises(_lib.T2SError, match="no warp"):
        plain.speed = 0.8


def test_entry_points_refuse_without_a_device():
    """every refused tuple of the three entry points returns T2S_EINVAL before anything is launched: no device is needed"""
    lib = _lib.load()
    assert lib.t2s_align_window_state() == 32 + 8 * 256
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(A=p, kind=1, B=1, N=100, T=4, n0=0, n=8, last=0, ld_row=4, ld_entry=32, in_len=None, mf=0, sk=-1, bk=-1, sl=-1, es=-1,
              fo=0.0, pos=p, peak=p, bad=p, state=p, stats=p, focus=p, dur=p, flags=p)
    for ch in (dict(A=None), dict(kind=3), dict(B=0), dict(N=0), dict(N=2 ** 30 + 1), dict(T=0), dict(n0=-1), dict(n0=9), dict(n=101),
               dict(last=2), dict(ld_row=3), dict(ld_entry=31), dict(pos=None), dict(peak=None), dict(bad=None), dict(state=None),
               dict(stats=None), dict(focus=None), dict(dur=None), dict(flags=None), dict(A=p + 2), dict(state=p + 4), dict(focus=p + 4),
               dict(pos=p + 2), dict(in_len=p + 1), dict(B=3, N=2 ** 30)):
        a = dict(ok, **ch)
        assert lib.t2s_align_window(*a.values(), None) == -1, "t2s_align_window accepted %r" % (ch,)
    ok = dict(B=1, N=100, n0=0, n=8, stretch=Q, stretches=None, path=p, ld_path=100, in_len=None, T=4, cum=p, fl=p)
    for ch in (dict(B=0), dict(B=65536), dict(N=0), dict(n0=-1), dict(n0=9), dict(n=101), dict(stretch=Q // 8 - 1), dict(stretch=8 * Q + 1),
               dict(stretches=p + 4), dict(path=None), dict(ld_path=7), dict(T=0), dict(cum=None), dict(cum=p + 4), dict(fl=p + 2),
               dict(path=p + 2)):
        a = dict(ok, **ch)
        assert lib.t2s_warp_window_map(*a.values(), None) == -1, "t2s_warp_window_map accepted %r" % (ch,)
    ok = dict(x=p, kind=1, B=1, C=2, N=100, n=8, ld_row=8, ld_entry=16, cum=p + 256, j0=0, j1=4, out=p + 128)
    for ch in (dict(x=None), dict(kind=0), dict(B=0), dict(C=0), dict(N=0), dict(n=0), dict(n=101), dict(ld_row=7), dict(ld_entry=15),
               dict(cum=None), dict(j0=-1), dict(j0=5), dict(j1=2 ** 31), dict(out=None), dict(out=p + 130), dict(out=p + 32), dict(x=p + 2)):
        a = dict(ok, **ch)
        assert lib.t2s_warp_window_gather(*a.values(), None) == -1, "t2s_warp_window_gather accepted %r" % (ch,)
    assert lib.t2s_warp_window_gather(*dict(ok, j0=4, j1=4, x=None, out=None, n=0).values(), None) == 0      # nothing asked for
