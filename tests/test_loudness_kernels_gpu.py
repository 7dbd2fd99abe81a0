"""t2s_loud_measure / t2s_loud_apply (csrc/loudness.hip, csrc/t2s_api_audio.hip) called directly on guarded buffers, against the
sequential float64 restatement of tests/loudness_ref.py.  tests/test_loudness_ref_cpu.py asserts that no block of these seeded rows
lies within 1e-6 relative of a gate and that no int16 pool output lies within 1e-6 of a half-integer, so counts, flags and int16
samples are compared for EQUALITY.  peak is compared for equality with the host's; ms and g are held to BAR relative (16 x the worst
case measured on an MI355X over the sweep, profiles/loudness_tests.md; never looser than 1e-9), lufs to what follows from it.

Every source is a view into a larger tensor filled with +-32767 (or NaN / 1e4), every destination, scratch and table a view into a
larger tensor of sentinels which must come back untouched."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as R
from text2speech_amd import _lib, audio
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
TORCH_OF = {"int16": torch.int16, "float32": torch.float32, "float16": torch.float16}
KIND = {torch.int16: 0, torch.float32: 1, torch.float16: 2}
S_FILL, C_FILL, T_FILL = -7.0, -99, -99
# worst measured over the sweep below: ms 1.58e-14, g 7.9e-15 relative (profiles/loudness_tests.md); 16 x the larger
BAR = 2.6e-13
LUFS_BAR = 10.0 / math.log(10.0) * BAR + 8 * 2.0 ** -46         # d lufs = 4.34 d ms / ms, and 8 ulp of a value below 128 for the log
WORST = dict(ms=0.0, g=0.0, lufs=0.0)
_WANT = {}                  # the reference of a row, computed once


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.t2s_loud_tile() == R.TILE and lib.t2s_loud_segment() == R.SEGMENT
    return lib


class Buf:
    """A device tensor of n elements inside a larger one: GUARD + shift elements of `fill` in front, GUARD behind."""

    def __init__(self, n, dtype, fill, shift=0):
        self.raw = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device=DEV)
        self.lo = GUARD + shift
        self.t = self.raw[self.lo:self.lo + n]
        self.fill = fill

    def guards_intact(self):
        a, b = self.raw[:self.lo], self.raw[self.lo + self.t.numel():]
        return bool((a == self.fill).all()) and bool((b == self.fill).all())

    def untouched(self):
        return self.guards_intact() and bool((self.t == self.fill).all())


def _src_buf(n, dtype, shift=0):
    """sentinels in front, behind and (until rows are copied in) everywhere: +-32767, or NaN and 1e4 in turns"""
    b = Buf(max(n, 1), dtype, 32767 if dtype == torch.int16 else 1e4, shift)
    b.t[::2] = -32767 if dtype == torch.int16 else float("nan")
    return b


def _dst(n, dtype, shift=0):
    return Buf(max(n, 1), dtype, 12345 if dtype == torch.int16 else 12345.678, shift)


_COEF = {}


def _coef(fs):
    if fs not in _COEF:
        _COEF[fs] = Buf(160, torch.float64, S_FILL)
        _COEF[fs].t.copy_(torch.from_numpy(audio.loudness_table(fs, R.SEGMENT)))
    return _COEF[fs]


def measure(lib, src, rows, fs, target=-23.0, limit=None, max_count=None):
    """rows: (src_start, src_count) -> (stats [n, 4], counts [n, 4], the stats Buf for an apply)"""
    n_rows = len(rows)
    max_count = max_count or max(1, max(c for _, c in rows))
    need = lib.t2s_loud_scratch(n_rows, max_count)
    scratch, stats, counts = Buf(need, torch.float64, S_FILL), Buf(4 * n_rows, torch.float64, S_FILL), Buf(4 * n_rows, torch.int32, C_FILL)
    table = Buf(2 * n_rows, torch.int64, T_FILL)
    table.t.copy_(torch.tensor(rows, dtype=torch.int64).view(-1))
    coef = _coef(fs)
    rc = lib.t2s_loud_measure(src.data_ptr(), KIND[src.dtype], src.numel(), table.t.data_ptr(), n_rows, max_count, R.hop(fs),
                              coef.t.data_ptr(), scratch.t.data_ptr(), need, R.GATE_ABS, 10.0 ** ((target + 0.691) / 10.0),
                              0.0 if limit is None else limit, stats.t.data_ptr(), counts.t.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert scratch.guards_intact() and stats.guards_intact() and counts.guards_intact() and table.guards_intact() and coef.guards_intact()
    assert bool((table.t.cpu() == torch.tensor(rows, dtype=torch.int64).view(-1)).all())
    return stats.t.cpu().numpy().reshape(n_rows, 4), counts.t.cpu().numpy().reshape(n_rows, 4), stats


def apply(lib, src, rows4, stats, dst, max_out, want_lengths=True):
    n_rows = len(rows4)
    table = torch.tensor(rows4, dtype=torch.int64, device=DEV)
    lens = torch.full((n_rows,), -77, dtype=torch.int32, device=DEV) if want_lengths else None
    rc = lib.t2s_loud_apply(src.data_ptr(), KIND[src.dtype], src.numel(), table.data_ptr(), n_rows, stats.t.data_ptr(), dst.t.data_ptr(),
                            KIND[dst.t.dtype], dst.t.numel(), max_out, lens.data_ptr() if want_lengths else None, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert dst.guards_intact(), "wrote outside the destination"
    return lens.cpu().numpy() if want_lengths else None


def _out_dtype(dtype):
    return torch.int16 if dtype == torch.int16 else torch.float32


def _pool(clips, dtype, shift, gen):
    """the clips in a pool with 1 .. 8 sentinels between them -> (Buf, starts)"""
    starts, pos = [], 5
    for c in clips:
        starts.append(pos)
        pos += c.size + int(gen.randint(1, 9))
    src = _src_buf(pos + 3, dtype, shift)
    for c, s in zip(clips, starts):
        if c.size:
            src.t[s:s + c.size].copy_(torch.from_numpy(c))
    return src, starts


def _apply_rows(lib, src, rows, stats, dtype, shift, gen):
    """every row gathered with dst_cap = its length -> list of outputs; the gaps between the rows stay sentinels"""
    dst_starts, pos = [], 3
    for _, c in rows:
        dst_starts.append(pos)
        pos += c + int(gen.randint(1, 9))
    dst = _dst(pos + 2, _out_dtype(dtype), shift)
    lens = apply(lib, src.t, [(s, c, t, c) for (s, c), t in zip(rows, dst_starts)], stats, dst, max(1, max(c for _, c in rows)))
    got = dst.t.cpu().numpy()
    written = np.zeros(got.size, dtype=bool)
    outs = []
    for (_, c), t, ln in zip(rows, dst_starts, lens):
        assert ln == c
        outs.append(got[t:t + c].copy())
        written[t:t + c] = True
    assert bool((got[~written] == got.dtype.type(dst.fill)).all()), "the gaps between the rows were written"
    return outs


def _check_row(label, x, fs, st, ct, target=-23.0, limit=None):
    """one row's stats and counts against the reference; -> the reference"""
    key = (x.dtype.str, x.tobytes(), fs, target, limit)
    if key not in _WANT:
        _WANT[key] = R.measure(x, fs, target, limit)
    want = _WANT[key]
    assert ct.tolist() == [want["J"], want["nA"], want["nR"], want["flags"]], "%s: counts %r" % (label, ct.tolist())
    ms, lufs, peak, g = st.tolist()
    assert peak == want["peak"], "%s: peak %r, host %r" % (label, peak, want["peak"])
    if want["flags"] & (R.SHORT | R.SILENT | R.NONFINITE):
        assert ms == 0.0 and g == 1.0 and (math.isnan(lufs) if want["flags"] & R.NONFINITE else lufs == -math.inf), label
        return want
    e_ms, e_g, e_l = abs(ms - want["ms"]) / want["ms"], abs(g - want["g"]) / want["g"], abs(lufs - want["lufs"])
    WORST.update(ms=max(WORST["ms"], e_ms), g=max(WORST["g"], e_g), lufs=max(WORST["lufs"], e_l))
    assert e_ms <= BAR and e_g <= BAR and e_l <= LUFS_BAR, "%s: ms off %.3e, g off %.3e relative, lufs off %.3e dB" % (label, e_ms, e_g, e_l)
    return want


# ---- the sweep: every length at every rate and kind, scattered in a pool at both 2-byte parities ----------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("fs", R.RATES)
def test_rows_scattered_in_a_pool_match_the_reference(lib, fs, kind):
    dtype = TORCH_OF[kind]
    clips = [R.clip(fs, n, seed, kind) for n, seed in R.lengths_for(fs)]
    gen = np.random.RandomState(fs % 97)
    first = None
    for shift in (0, 1):
        src, starts = _pool(clips, dtype, shift, gen)
        rows = [(s, c.size) for s, c in zip(starts, clips)]
        st, ct, stats = measure(lib, src.t, rows, fs)
        outs = _apply_rows(lib, src, rows, stats, dtype, shift, gen)
        assert src.guards_intact()
        for q, c in enumerate(clips):
            label = "fs %d %s n %d shift %d" % (fs, kind, c.size, shift)
            _check_row(label, c, fs, st[q], ct[q])
            g = float(st[q, 3])
            want = R.apply_int16(c, g) if kind == "int16" else R.apply_float(c, g)
            assert outs[q].dtype == want.dtype and outs[q].tobytes() == want.tobytes(), "%s: applied samples" % label
        if first is None:
            first = (st.tobytes(), ct.tobytes(), [o.tobytes() for o in outs])
        else:
            assert first == (st.tobytes(), ct.tobytes(), [o.tobytes() for o in outs]), "the base's parity changed a bit"
    print("LOUDNESS fs %d %s: worst so far ms %.3e g %.3e relative, lufs %.3e dB (bar %.1e)" % (fs, kind, WORST["ms"], WORST["g"],
                                                                                            WORST["lufs"], BAR))


# ---- a row alone, and at every place of a 5-row batch with an odd row stride, in rotated and in shuffled order -------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("fs", R.RATES)
def test_a_row_is_the_same_bits_alone_and_anywhere_in_a_batch(lib, fs, kind):
    dtype = TORCH_OF[kind]
    clips = [R.clip(fs, n, seed, kind) for n, seed in R.batch_rows(fs)]
    gen = np.random.RandomState(3)
    alone = []
    for q, c in enumerate(clips):
        src, starts = _pool([c], dtype, q & 1, gen)
        st, ct, stats = measure(lib, src.t, [(starts[0], c.size)], fs)
        _check_row("fs %d %s n %d alone" % (fs, kind, c.size), c, fs, st[0], ct[0])
        alone.append((st[0].tobytes(), ct[0].tobytes(), _apply_rows(lib, src, [(starts[0], c.size)], stats, dtype, q & 1, gen)[0].tobytes()))
    N = max(c.size for c in clips)
    ldx = N + 3 if (N + 3) & 1 else N + 4                       # odd: the rows fall on both parities
    rotations = [[(q + k) % 5 for q in range(5)] for k in range(5)]       # every row at every place
    for order in rotations + [[3, 0, 4, 2, 1]]:
        src = _src_buf(5 * ldx, dtype, 1)                       # NaN / 1e4 / +-32767 behind every length
        for b, q in enumerate(order):
            src.t[b * ldx:b * ldx + clips[q].size].copy_(torch.from_numpy(clips[q]))
        rows = [(b * ldx, clips[q].size) for b, q in enumerate(order)]
        st, ct, stats = measure(lib, src.t, rows, fs, max_count=N)
        outs = _apply_rows(lib, src, rows, stats, dtype, 0, gen)
        for b, q in enumerate(order):
            assert (st[b].tobytes(), ct[b].tobytes(), outs[b].tobytes()) == alone[q], "row %d at place %d of %r" % (q, b, order)


# ---- an int16 pool: counts, flags and samples equal the reference's ------------------------------------------------------------------
@pytest.mark.parametrize("fs", R.RATES)
def test_int16_pool_equals_the_reference(lib, fs):
    clips = [R.clip(fs, n, seed, "int16") for n, seed in R.pool_rows(fs)]
    gen = np.random.RandomState(11)
    flagged = 0
    for shift in (0, 1):
        src, starts = _pool(clips, torch.int16, shift, gen)
        rows = [(s, c.size) for s, c in zip(starts, clips)]
        st, ct, stats = measure(lib, src.t, rows, fs, R.POOL_TARGET, R.POOL_PEAK_LIMIT)
        outs = _apply_rows(lib, src, rows, stats, torch.int16, shift, gen)
        for q, c in enumerate(clips):
            want = _check_row("fs %d pool clip %d" % (fs, q), c, fs, st[q], ct[q], R.POOL_TARGET, R.POOL_PEAK_LIMIT)
            assert np.array_equal(outs[q], R.apply_int16(c, want["g"])), "clip %d: int16 output differs from rint of the reference" % q
            if want["flags"] & (R.SHORT | R.SILENT):
                flagged += 1
                assert outs[q].tobytes() == c.tobytes(), "a flagged clip is copied"
    assert flagged >= 4


# ---- flagged rows are copied bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float32", "float16"])
def test_flagged_float_rows_are_copied(lib, kind):
    fs, h, dtype = 8000, 800, TORCH_OF[kind]
    good = R.clip(fs, 13 * h + 17, 2, kind)
    clips = [good, R.clip(fs, 3 * h, 0, kind), R.clip(fs, 4 * h, 1, kind)]
    for bad, at in ((np.nan, 1500), (np.inf, 0), (-np.inf, good.size - 1)):
        c = good.copy()
        c[at] = bad
        clips.append(c)
    src, starts = _pool(clips, dtype, 1, np.random.RandomState(2))
    rows = [(s, c.size) for s, c in zip(starts, clips)]
    st, ct, stats = measure(lib, src.t, rows, fs)
    outs = _apply_rows(lib, src, rows, stats, dtype, 0, np.random.RandomState(2))
    assert ct[:, 3].tolist() == [0, R.SHORT, R.SILENT, R.NONFINITE, R.NONFINITE, R.NONFINITE]
    for q, c in enumerate(clips):
        _check_row("flagged %d" % q, c, fs, st[q], ct[q])
        if q:
            assert outs[q].tobytes() == c.astype(np.float32).tobytes(), "row %d is copied bit for bit" % q
    assert outs[0].tobytes() == R.apply_float(good, float(st[0, 3])).tobytes() and st[0, 3] != 1.0


# ---- the destination ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_dst_cap_truncates_or_zero_fills_and_out_lengths_count(lib, kind):
    fs, h, dtype = 8000, 800, TORCH_OF[kind]
    clip = R.clip(fs, 6 * h + 11, 4, kind)
    n = clip.size
    src, starts = _pool([clip], dtype, 0, np.random.RandomState(1))
    st, ct, stats = measure(lib, src.t, [(starts[0], n)], fs)
    full = R.apply_int16(clip, float(st[0, 3])) if kind == "int16" else R.apply_float(clip, float(st[0, 3]))
    assert ct[0, 3] == 0 and st[0, 3] != 1.0
    caps = [1, 2047, 2048, 2049, n - 1, n, n + 1, n + 700, 0]
    stride = n + 800
    many = Buf(4 * len(caps), torch.float64, S_FILL)
    many.t.copy_(stats.t.repeat(len(caps)))
    dst = _dst(stride * len(caps), _out_dtype(dtype))
    lens = apply(lib, src.t, [(starts[0], n, q * stride, cap) for q, cap in enumerate(caps)], many, dst, max(caps))
    got = dst.t.cpu().numpy()
    for q, cap in enumerate(caps):
        row = got[q * stride:(q + 1) * stride]
        v = min(cap, n)
        assert lens[q] == v and row[:v].tobytes() == full[:v].tobytes(), "cap %d" % cap
        assert row[v:cap].tobytes() == np.zeros(cap - v, dtype=row.dtype).tobytes(), "cap %d: +0 behind the samples" % cap
        assert bool((row[cap:] == row.dtype.type(dst.fill)).all()), "cap %d: wrote behind dst_cap" % cap
    dst = _dst(n, _out_dtype(dtype))                            # max_out below the row's cap cuts the row there
    apply(lib, src.t, [(starts[0], n, 0, n)], stats, dst, 100, want_lengths=False)
    got = dst.t.cpu().numpy()
    assert got[:100].tobytes() == full[:100].tobytes() and bool((got[100:] == got.dtype.type(dst.fill)).all())


def test_a_click_in_a_quiet_row_is_held_by_the_peak_limit(lib):
    fs, limit, target = 44100, 0.9, -3.0
    for kind in ("float32", "float16"):
        clip = R.click_row(fs, kind)
        src, starts = _pool([clip], TORCH_OF[kind], 1, np.random.RandomState(4))
        rows = [(starts[0], clip.size)]
        st, ct, stats = measure(lib, src.t, rows, fs, target, limit)
        want = _check_row("click " + kind, clip, fs, st[0], ct[0], target, limit)
        assert ct[0, 3] == R.PEAK == want["flags"] and st[0, 2] == 1.0
        out = _apply_rows(lib, src, rows, stats, TORCH_OF[kind], 0, np.random.RandomState(4))[0]
        assert float(np.abs(out.astype(np.float64)).max()) <= limit * (1.0 + 2.0 ** -24)
        assert out.tobytes() == R.apply_float(clip, float(st[0, 3])).tobytes()


def test_any_table_value_is_safe(lib):
    """rows whose source lies outside the pool have no samples (J = 0, peak 0, a row of zeros); a count that runs past the pool's
    end is cut there; destinations outside dst write nothing; a row longer than max_count is cut there"""
    fs, h = 8000, 800
    pool_len, cap = 9 * h, 90
    clip = R.clip(fs, pool_len, 2, "int16")
    src = _src_buf(pool_len, torch.int16)
    src.t.copy_(torch.from_numpy(clip))
    bad_src = [(-1, 50), (-(1 << 40), 50), (pool_len, 50), (pool_len + 7, 5), (1 << 40, 50), (1 << 62, 1 << 62), (10, -1),
               (10, -(1 << 62)), (-(1 << 63), (1 << 63) - 1), (10, 0)]
    cut_src = [(pool_len - 5 * h, 5 * h + 1), (pool_len - 5 * h, 1 << 40), (pool_len - 33, (1 << 63) - 1), (0, 1 << 50)]
    rows = bad_src + cut_src
    st, ct, stats = measure(lib, src.t, rows, fs, max_count=pool_len)
    assert src.guards_intact()
    for q in range(len(bad_src)):
        assert st[q, [0, 2, 3]].tolist() == [0.0, 0.0, 1.0] and st[q, 1] == -math.inf and ct[q].tolist() == [0, 0, 0, R.SHORT], rows[q]
    for k, (s, _) in enumerate(cut_src):
        _check_row("cut row %r" % (rows[len(bad_src) + k],), clip[s:], fs, st[len(bad_src) + k], ct[len(bad_src) + k])
    st2, ct2, _ = measure(lib, src.t, [(0, pool_len)], fs, max_count=5 * h + 3)         # cut at max_count
    _check_row("max_count", clip[:5 * h + 3], fs, st2[0], ct2[0])
    rows4 = [(s, c, q * cap, cap) for q, (s, c) in enumerate(rows)]
    n_ok, dst_len = len(rows4), len(rows4) * cap
    dst = _dst(dst_len + 40, torch.int16)
    rows4 += [(0, 100, -1, cap), (0, 100, -(1 << 62), cap), (0, 100, dst_len + 40, cap), (0, 100, 1 << 62, 1 << 62), (0, 100, 5, -3),
              (0, 100, 5, -(1 << 63)), (0, 100, dst_len + 10, 1 << 40)]
    many = Buf(4 * len(rows4), torch.float64, S_FILL)
    many.t.copy_(torch.tensor([0.0, 0.0, 0.0, 1.0] * len(rows4), dtype=torch.float64))
    lens = apply(lib, src.t, rows4, many, dst, cap)
    got = dst.t.cpu().numpy()
    for q in range(len(bad_src)):
        assert lens[q] == 0 and bool((got[q * cap:(q + 1) * cap] == 0).all()), rows4[q]
    for k, (s, _) in enumerate(cut_src):
        q, v = len(bad_src) + k, min(pool_len - s, cap)
        assert lens[q] == v and np.array_equal(got[q * cap:q * cap + v], clip[s:s + v]) and bool((got[q * cap + v:(q + 1) * cap] == 0).all())
    assert lens[n_ok:n_ok + 6].tolist() == [0] * 6 and bool((got[dst_len:dst_len + 10] == 12345).all())
    assert lens[-1] == 30 and np.array_equal(got[dst_len + 10:], clip[:30])
    assert src.guards_intact()


def test_refused_calls_launch_nothing(lib):
    """every T2S_EINVAL case of tests/loudness_ref.py's lists, here with real buffers: sentinels everywhere stay"""
    fs, n = 8000, 5000
    clip = R.clip(fs, n, 0, "int16")
    src = _src_buf(2 * n, torch.int16)
    src.t[:n].copy_(torch.from_numpy(clip))
    before = src.raw.clone()
    need = lib.t2s_loud_scratch(1, n)
    scratch, stats, counts, dst = Buf(need, torch.float64, S_FILL), Buf(4, torch.float64, S_FILL), Buf(4, torch.int32, C_FILL), _dst(n, torch.int16)
    table = torch.tensor([(0, n)], dtype=torch.int64, device=DEV)
    table4 = torch.tensor([(0, n, 0, n)], dtype=torch.int64, device=DEV)
    fsrc = torch.zeros(n, dtype=torch.float32, device=DEV)
    good = dict(src=src.t.data_ptr(), table=table.data_ptr(), coef=_coef(fs).t.data_ptr(), scratch=scratch.t.data_ptr(),
                stats=stats.t.data_ptr(), counts=counts.t.data_ptr(), dst=dst.t.data_ptr())
    ptr = lambda kw, k, g=None: R.refused_pointer(kw.get(k), (g or good)[k])

    def measure_call(**kw):
        a = dict(kind=0, src_len=n, rows=1, max_count=n, h=R.hop(fs), scratch_len=need, gate=R.GATE_ABS, T=10.0 ** ((-23.0 + 0.691) / 10.0), limit=0.0)
        a.update({k: v for k, v in kw.items() if k not in good})
        if a["scratch_len"] == "short":
            a["scratch_len"] = need - 1
        return lib.t2s_loud_measure(ptr(kw, "src"), a["kind"], a["src_len"], ptr(kw, "table"), a["rows"], a["max_count"], a["h"],
                                    ptr(kw, "coef"), ptr(kw, "scratch"), a["scratch_len"], a["gate"], a["T"], a["limit"],
                                    ptr(kw, "stats"), ptr(kw, "counts"), _st())

    good4 = dict(good, table=table4.data_ptr())

    def apply_call(**kw):
        a = dict(kind=0, src_len=2 * n, rows=1, dkind=0, dst_len=n, max_out=n)
        a.update({k: v for k, v in kw.items() if k not in good})
        d = {"src": good["src"], "inside src": good["src"] + 2 * n}.get(kw.get("dst"), ptr(kw, "dst"))
        s = fsrc.data_ptr() if a["kind"] in (1, 2) else ptr(kw, "src")
        return lib.t2s_loud_apply(s, a["kind"], a["src_len"], ptr(kw, "table", good4), a["rows"], ptr(kw, "stats"), d, a["dkind"],
                                  a["dst_len"], a["max_out"], None, _st())

    for kw in R.REFUSED_MEASURE:
        assert measure_call(**kw) == -1, kw
    for kw in R.REFUSED_APPLY:
        assert apply_call(**kw) == -1, kw
    assert apply_call(kind=1, dkind=0, src_len=n) == -1 and apply_call(kind=2, dkind=0, src_len=n) == -1
    torch.cuda.synchronize()
    for b in (scratch, stats, counts, dst):
        assert b.untouched(), "a refused call wrote something"
    assert bool((src.raw == before).all())
    # and the accepted calls do write
    assert measure_call() == 0 and apply_call() == 0
    torch.cuda.synchronize()
    want = _check_row("accepted", clip, fs, stats.t.cpu().numpy(), counts.t.cpu().numpy())
    assert want["flags"] == 0 and np.array_equal(dst.t.cpu().numpy(), R.apply_int16(clip, float(stats.t[3])))


def test_two_identical_calls_give_identical_bits(lib):
    clip = R.clip(44100, 2 * R.TILE + 17, 5, "float32")
    src, starts = _pool([clip], torch.float32, 0, np.random.RandomState(0))
    a = measure(lib, src.t, [(starts[0], clip.size)], 44100)
    b = measure(lib, src.t, [(starts[0], clip.size)], 44100)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
