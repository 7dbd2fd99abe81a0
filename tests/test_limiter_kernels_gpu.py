"""t2s_limit_measure / t2s_limit_apply (csrc/limiter.hip) called directly on guarded buffers, against the float64 restatement of
tests/limiter_ref.py.  tests/test_limiter_ref_cpu.py asserts that no p of these seeded rows lies within 1e-9 relative of the ceiling
and that no int16 reference output lies within 1e-6 of a half-integer, so counts, flags and int16 samples are compared for
EQUALITY.  sample_peak is compared for equality; true_peak, s_min and the float32 samples are held to the rounding bounds that
limiter_ref.bounds derives from the sums (profiles/limiter_tests.md states the derivation and the worst measured fraction).
No stored sample may exceed the ceiling, exactly.

Every source is a view into a larger tensor filled with +-32767 (or NaN / 1e4), every destination, scratch, table and statistic a
view into a larger tensor of sentinels which must come back untouched."""
import numpy as np
import pytest
import torch

import limiter_ref as R
from text2speech_amd import _lib, audio
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
TORCH_OF = {"int16": torch.int16, "float32": torch.float32, "float16": torch.float16}
KIND = {torch.int16: 0, torch.float32: 1, torch.float16: 2}
S_FILL, C_FILL, T_FILL = -7.0, -99, -99
C = R.ceiling(R.CEILING_DB)
HW = R.HALF_WIDTH
GAINS = (1.0, 3.0, 8.0)
WORST = dict(tp=0.0, smin=0.0, out=0.0)         # the largest fraction of its bound a quantity used


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.t2s_limit_tile() == R.TILE and lib.t2s_limit_max_lookahead() == max(R.LOOKAHEADS) == audio.LIMIT_MAX_LOOKAHEAD
    assert lib.t2s_limit_max_half_width() == audio.LIMIT_MAX_HALF_WIDTH and lib.t2s_abi_version() == 4
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


def _out_dtype(dtype):
    return torch.int16 if dtype == torch.int16 else torch.float32


_TABLES = {}


def _hw(os, L):
    """(h Buf, w Buf) of the package's own filter and window, guarded, uploaded once"""
    if (os, L) not in _TABLES:
        h, w = audio.resample_filter(1, os, HW, 5.0)[2], audio.limiter_window(L)
        bh, bw = Buf(h.size, torch.float64, S_FILL), Buf(w.size, torch.float64, S_FILL)
        bh.t.copy_(torch.from_numpy(h))
        bw.t.copy_(torch.from_numpy(w))
        _TABLES[(os, L)] = (bh, bw)
    return _TABLES[(os, L)]


def _gains(gains):
    if gains is None:
        return None
    b = Buf(len(gains), torch.float64, S_FILL)
    b.t.copy_(torch.tensor(gains, dtype=torch.float64))
    return b


def measure(lib, src, rows, os, L, gains=None, max_count=None, c=C):
    """rows: (src_start, src_count) -> (stats [n, 4], counts [n, 2], the counts Buf for an apply)"""
    n_rows = len(rows)
    max_count = max_count or max(1, max(cnt for _, cnt in rows))
    need = lib.t2s_limit_scratch(n_rows, max_count)
    scratch, stats, counts = Buf(need, torch.float64, S_FILL), Buf(4 * n_rows, torch.float64, S_FILL), Buf(2 * n_rows, torch.int32, C_FILL)
    table = Buf(2 * n_rows, torch.int64, T_FILL)
    table.t.copy_(torch.tensor(rows, dtype=torch.int64).view(-1))
    h, w = _hw(os, L)
    g = _gains(gains)
    rc = lib.t2s_limit_measure(src.data_ptr(), KIND[src.dtype], src.numel(), table.t.data_ptr(), n_rows, max_count,
                               g.t.data_ptr() if g else None, h.t.data_ptr(), h.t.numel(), os, HW, w.t.data_ptr(), L, c,
                               scratch.t.data_ptr(), need, stats.t.data_ptr(), counts.t.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    for b in (scratch, stats, counts, table, h, w) + ((g,) if g else ()):
        assert b.guards_intact()
    assert bool((table.t.cpu() == torch.tensor(rows, dtype=torch.int64).view(-1)).all())
    return stats.t.cpu().numpy().reshape(n_rows, 4), counts.t.cpu().numpy().reshape(n_rows, 2), counts


def apply(lib, src, rows4, os, L, counts, dst, max_out, gains=None, want_lengths=True, c=C):
    n_rows = len(rows4)
    table = torch.tensor(rows4, dtype=torch.int64, device=DEV)
    lens = torch.full((n_rows,), -77, dtype=torch.int32, device=DEV) if want_lengths else None
    h, w = _hw(os, L)
    g = _gains(gains)
    rc = lib.t2s_limit_apply(src.data_ptr(), KIND[src.dtype], src.numel(), table.data_ptr(), n_rows, g.t.data_ptr() if g else None,
                             h.t.data_ptr(), h.t.numel(), os, HW, w.t.data_ptr(), L, c, counts.t.data_ptr(), dst.t.data_ptr(),
                             KIND[dst.t.dtype], dst.t.numel(), max_out, lens.data_ptr() if want_lengths else None, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert dst.guards_intact(), "wrote outside the destination"
    assert h.guards_intact() and w.guards_intact() and counts.guards_intact()
    return lens.cpu().numpy() if want_lengths else None


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


def _apply_rows(lib, src, rows, os, L, counts, dtype, shift, gen, gains=None):
    """every row with dst_cap = its length -> list of outputs; the gaps between the rows stay sentinels"""
    dst_starts, pos = [], 3
    for _, c in rows:
        dst_starts.append(pos)
        pos += c + int(gen.randint(1, 9))
    dst = _dst(pos + 2, _out_dtype(dtype), shift)
    lens = apply(lib, src.t, [(s, c, t, c) for (s, c), t in zip(rows, dst_starts)], os, L, counts, dst, max(1, max(c for _, c in rows)),
                 gains)
    got = dst.t.cpu().numpy()
    written = np.zeros(got.size, dtype=bool)
    outs = []
    for (_, c), t, ln in zip(rows, dst_starts, lens):
        assert ln == c
        outs.append(got[t:t + c].copy())
        written[t:t + c] = True
    assert bool((got[~written] == got.dtype.type(dst.fill)).all()), "the gaps between the rows were written"
    return outs


def _check_row(label, x, os, L, g, st, ct, out=None, c=C):
    """one row's statistics, counts and (where given) samples against the reference; -> the reference"""
    ref = R.reference(x, c, L, os, g)
    assert tuple(ct.tolist()) == ref.counts, "%s: counts %r, reference %r" % (label, ct.tolist(), ref.counts)
    tp, sp, smin, zero = st.tolist()
    assert zero == 0.0 and sp == ref.stats[1], "%s: sample peak %r, host %r" % (label, sp, ref.stats[1])
    if ref.counts[1] & R.FLAG_NONFINITE:
        assert tp == np.inf and smin == 1.0, label
        if out is not None:
            assert out.tobytes() == ref.out.tobytes(), "%s: a row that is not finite is copied" % label
        return ref
    if x.size == 0:
        assert (tp, smin) == (0.0, 1.0), label
        return ref
    b_p, b_s = R.bounds(ref, L, os)
    e_tp, e_s = abs(tp - ref.stats[0]), abs(smin - ref.stats[2])
    if os == 1:
        assert e_tp == 0.0, "%s: without oversampling the true peak is the sample peak" % label
    elif b_p.max() > 0.0:
        WORST["tp"] = max(WORST["tp"], e_tp / b_p.max())
    WORST["smin"] = max(WORST["smin"], e_s / b_s)
    assert e_tp <= b_p.max() and e_s <= b_s, "%s: true peak off %.3e (bound %.3e), s_min off %.3e (bound %.3e)" % (label, e_tp, b_p.max(),
                                                                                                                 e_s, b_s)
    if out is None:
        return ref
    assert out.dtype == ref.out.dtype and out.size == x.size, label
    if out.dtype == np.int16:
        assert np.array_equal(out, ref.out), "%s: %d int16 samples differ from rint of the reference" % (label, int((out != ref.out).sum()))
        assert np.abs(out.astype(np.int64)).max() <= np.rint(32768.0 * c), "%s: a code over the ceiling" % label
    else:
        tol = 2.0 ** -24 * np.abs(ref.o) + np.abs(ref.u) * b_s + 2.0 ** -52 * np.abs(ref.o) + 2.0 ** -149
        err = np.abs(out.astype(np.float64) - ref.o)
        WORST["out"] = max(WORST["out"], float((err / tol).max()))
        assert (err <= tol).all(), "%s: float32 sample off %.3e of its bound" % (label, float((err / tol).max()))
        assert np.abs(out).max() <= np.float32(c), "%s: a sample over the ceiling" % label
    if ref.counts[0] == 0 and g == 1.0:
        assert out.tobytes() == (x if x.dtype == np.int16 else x.astype(np.float32)).tobytes(), "%s: an untouched row keeps its bits" % label
    return ref


# ---- the sweep: every length at every look-ahead, oversampling and kind, scattered in a pool at both 2-byte parities -------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("os", R.OVERSAMPLES)
@pytest.mark.parametrize("L", R.LOOKAHEADS)
def test_rows_scattered_in_a_pool_match_the_reference(lib, L, os, kind):
    dtype = TORCH_OF[kind]
    clips = [R.clip(n, R.seed_of(n, L, os, kind), kind, L) for n in R.lengths_for(L)]
    gains = [GAINS[(q + os + R.KINDS.index(kind)) % 3] for q in range(len(clips))]
    gen = np.random.RandomState(L + os)
    first, limited = None, 0
    for shift in (0, 1):
        src, starts = _pool(clips, dtype, shift, gen)
        rows = [(s, c.size) for s, c in zip(starts, clips)]
        st, ct, counts = measure(lib, src.t, rows, os, L, gains)
        outs = _apply_rows(lib, src, rows, os, L, counts, dtype, shift, gen, gains)
        assert src.guards_intact()
        for q, c in enumerate(clips):
            ref = _check_row("L %d os %d %s n %d g %g shift %d" % (L, os, kind, c.size, gains[q], shift), c, os, L, gains[q], st[q], ct[q],
                             outs[q])
            limited += ref.counts[0]
        if first is None:
            first = (st.tobytes(), ct.tobytes(), [o.tobytes() for o in outs])
        else:
            assert first == (st.tobytes(), ct.tobytes(), [o.tobytes() for o in outs]), "the base's parity changed a bit"
    assert limited > 200
    print("LIMITER L %d os %d %s: worst fraction of the bound so far: true peak %.3f, s_min %.3f, float32 samples %.3f"
          % (L, os, kind, WORST["tp"], WORST["smin"], WORST["out"]))


# ---- without a gains table g = 1: placed peaks only, and the untouched stretches keep their bits -------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("L", (0, 67, 1024))
def test_without_gains_the_gain_is_one(lib, L, kind):
    dtype, os = TORCH_OF[kind], 4
    clips = [R.clip(n, R.seed_of(n, L, os, kind), kind, L) for n in R.lengths_for(L)]
    quiet = R.clip(1500, 9, kind, L)                            # a quarter of it: nothing over the ceiling
    clips.append(quiet // 4 if kind == "int16" else (quiet.astype(np.float64) / 4).astype(quiet.dtype))
    gen = np.random.RandomState(L)
    src, starts = _pool(clips, dtype, 1, gen)
    rows = [(s, c.size) for s, c in zip(starts, clips)]
    st, ct, counts = measure(lib, src.t, rows, os, L)
    outs = _apply_rows(lib, src, rows, os, L, counts, dtype, 0, gen)
    for q, c in enumerate(clips):
        _check_row("no gains L %d %s n %d" % (L, kind, c.size), c, os, L, 1.0, st[q], ct[q], outs[q])
    assert ct[-1].tolist() == [0, 0] and st[-1, 2] == 1.0       # (the quiet row: _check_row asserted its bits)


# ---- a row alone, and at every place of a 5-row batch with an odd row stride, in rotated and in shuffled order --------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("L,os", [(0, 4), (1, 4), (16, 1), (16, 2), (16, 4), (67, 4), (1024, 4)])
def test_a_row_is_the_same_bits_alone_and_anywhere_in_a_batch(lib, L, os, kind):
    dtype = TORCH_OF[kind]
    sizes = [R.TILE + 1, 2 * L + 1, 2 * R.TILE + 1, 2, R.TILE - 1]
    clips = [R.clip(n, R.seed_of(n, L, os, kind), kind, L) for n in sizes]
    gains = [3.0, 1.0, 8.0, 3.0, 1.0]
    gen = np.random.RandomState(3)
    alone = []
    for q, c in enumerate(clips):
        src, starts = _pool([c], dtype, q & 1, gen)
        rows = [(starts[0], c.size)]
        st, ct, counts = measure(lib, src.t, rows, os, L, [gains[q]])
        out = _apply_rows(lib, src, rows, os, L, counts, dtype, q & 1, gen, [gains[q]])[0]
        _check_row("L %d os %d %s n %d alone" % (L, os, kind, c.size), c, os, L, gains[q], st[0], ct[0], out)
        alone.append((st[0].tobytes(), ct[0].tobytes(), out.tobytes()))
    N = max(sizes)
    ldx = N + 3 if (N + 3) & 1 else N + 4                       # odd: the rows fall on both parities
    rotations = [[(q + k) % 5 for q in range(5)] for k in range(5)]       # every row at every place
    for order in rotations + [[3, 0, 4, 2, 1]]:
        src = _src_buf(5 * ldx, dtype, 1)                       # NaN / 1e4 / +-32767 behind every length
        for b, q in enumerate(order):
            src.t[b * ldx:b * ldx + clips[q].size].copy_(torch.from_numpy(clips[q]))
        rows = [(b * ldx, clips[q].size) for b, q in enumerate(order)]
        g = [gains[q] for q in order]
        st, ct, counts = measure(lib, src.t, rows, os, L, g, max_count=N)
        outs = _apply_rows(lib, src, rows, os, L, counts, dtype, 0, gen, g)
        for b, q in enumerate(order):
            assert (st[b].tobytes(), ct[b].tobytes(), outs[b].tobytes()) == alone[q], "row %d at place %d of %r" % (q, b, order)


# ---- a gain of 0, and rows that are not finite: flagged, copied WITHOUT their gain, their neighbours unaffected ------------------------------
@pytest.mark.parametrize("kind", ["float32", "float16"])
def test_a_zero_gain_and_rows_that_are_not_finite(lib, kind):
    dtype, L, os = TORCH_OF[kind], 16, 4
    good = R.clip(R.TILE + 300, 21, kind, L)
    clips, gains = [good, good], [3.0, 0.0]
    for bad, at in ((np.nan, 1100), (np.inf, 0), (-np.inf, good.size - 1)):
        c = good.copy()
        c[at] = bad
        clips.append(c)
        gains.append(3.0)
    clips += [good, good]
    gains += [np.inf, 8.0]                                      # a gain that is not finite makes u not finite
    src, starts = _pool(clips, dtype, 1, np.random.RandomState(2))
    rows = [(s, c.size) for s, c in zip(starts, clips)]
    st, ct, counts = measure(lib, src.t, rows, os, L, gains)
    outs = _apply_rows(lib, src, rows, os, L, counts, dtype, 0, np.random.RandomState(2), gains)
    assert ct[:, 1].tolist() == [1, 0, 8, 8, 8, 8, 1]
    for q, c in enumerate(clips):
        _check_row("row %d" % q, c, os, L, gains[q], st[q], ct[q], outs[q])
    assert st[1].tolist() == [0.0, 0.0, 1.0, 0.0] and not outs[1].any()
    for q in (2, 3, 4, 5):
        assert outs[q].tobytes() == clips[q].astype(np.float32).tobytes(), "row %d is copied bit for bit, without its gain" % q
    solo_src, solo_starts = _pool([good], dtype, 0, np.random.RandomState(5))
    st1, ct1, counts1 = measure(lib, solo_src.t, [(solo_starts[0], good.size)], os, L, [8.0])
    out1 = _apply_rows(lib, solo_src, [(solo_starts[0], good.size)], os, L, counts1, dtype, 0, np.random.RandomState(5), [8.0])[0]
    assert (st1[0].tobytes(), ct1[0].tobytes(), out1.tobytes()) == (st[6].tobytes(), ct[6].tobytes(), outs[6].tobytes())


def test_an_int16_row_with_a_gain_that_is_not_finite_is_copied(lib):
    clip = R.clip(1500, 4, "int16", 16)
    src, starts = _pool([clip, clip], torch.int16, 1, np.random.RandomState(2))
    rows = [(s, clip.size) for s in starts]
    st, ct, counts = measure(lib, src.t, rows, 2, 16, [np.nan, 3.0])
    outs = _apply_rows(lib, src, rows, 2, 16, counts, torch.int16, 1, np.random.RandomState(2), [np.nan, 3.0])
    assert ct[0].tolist() == [0, 8] and outs[0].tobytes() == clip.tobytes()
    _check_row("beside it", clip, 2, 16, 3.0, st[1], ct[1], outs[1])


# ---- the destination ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32"])
@pytest.mark.parametrize("limited", [True, False])
def test_dst_cap_truncates_or_zero_fills_and_out_lengths_count(lib, kind, limited):
    dtype, L, os = TORCH_OF[kind], 67, 4
    n = 2 * R.TILE + 1
    clip = R.clip(n, R.seed_of(n, L, os, kind), kind, L)
    g = 3.0 if limited else 0.25
    src, starts = _pool([clip], dtype, 0, np.random.RandomState(1))
    caps = [1, R.TILE - 1, R.TILE, R.TILE + 1, n - 1, n, n + 1, n + 1500, 0]
    rows = [(starts[0], n)] * len(caps)
    st, ct, counts = measure(lib, src.t, rows, os, L, [g] * len(caps))
    ref = _check_row("cap", clip, os, L, g, st[0], ct[0])
    assert (ref.counts[0] > 0) == limited
    stride = n + 1600
    dst = _dst(stride * len(caps), _out_dtype(dtype))
    lens = apply(lib, src.t, [(starts[0], n, q * stride, cap) for q, cap in enumerate(caps)], os, L, counts, dst, max(caps), [g] * len(caps))
    got = dst.t.cpu().numpy()
    full = got[5 * stride:5 * stride + n].copy()
    _check_row("cap n", clip, os, L, g, st[5], ct[5], full)
    for q, cap in enumerate(caps):
        row = got[q * stride:(q + 1) * stride]
        v = min(cap, n)
        assert lens[q] == v and row[:v].tobytes() == full[:v].tobytes(), "cap %d" % cap
        assert row[v:cap].tobytes() == np.zeros(cap - v, dtype=row.dtype).tobytes(), "cap %d: +0 behind the samples" % cap
        assert bool((row[cap:] == row.dtype.type(dst.fill)).all()), "cap %d: wrote behind dst_cap" % cap
    dst = _dst(n, _out_dtype(dtype))                            # max_out below the row's cap cuts the row there
    apply(lib, src.t, [(starts[0], n, 0, n)], os, L, counts, dst, 100, [g], want_lengths=False)
    got = dst.t.cpu().numpy()
    assert got[:100].tobytes() == full[:100].tobytes() and bool((got[100:] == got.dtype.type(dst.fill)).all())


def test_any_table_value_is_safe(lib):
    """rows whose source lies outside the pool have no samples; a count that runs past the pool's end is cut there; destinations
    outside dst write nothing; a row longer than max_count is measured up to there"""
    L, os, g = 16, 4, 3.0
    pool_len, cap = 3000, 90
    clip = R.clip(pool_len, 2, "int16", L)
    src = _src_buf(pool_len, torch.int16)
    src.t.copy_(torch.from_numpy(clip))
    bad_src = [(-1, 50), (-(1 << 40), 50), (pool_len, 50), (pool_len + 7, 5), (1 << 40, 50), (1 << 62, 1 << 62), (10, -1),
               (10, -(1 << 62)), (-(1 << 63), (1 << 63) - 1), (10, 0)]
    cut_src = [(pool_len - 1300, 1301), (pool_len - 1300, 1 << 40), (pool_len - 33, (1 << 63) - 1), (0, 1 << 50)]
    rows = bad_src + cut_src
    st, ct, counts = measure(lib, src.t, rows, os, L, [g] * len(rows), max_count=pool_len)
    assert src.guards_intact()
    for q in range(len(bad_src)):
        assert st[q].tolist() == [0.0, 0.0, 1.0, 0.0] and ct[q].tolist() == [0, 0], rows[q]
    for k, (s, _) in enumerate(cut_src):
        _check_row("cut row %r" % (rows[len(bad_src) + k],), clip[s:], os, L, g, st[len(bad_src) + k], ct[len(bad_src) + k])
    st2, ct2, _ = measure(lib, src.t, [(0, pool_len)], os, L, [g], max_count=R.TILE + 3)          # cut at max_count
    _check_row("max_count", clip[:R.TILE + 3], os, L, g, st2[0], ct2[0])
    rows4 = [(s, c, q * cap, cap) for q, (s, c) in enumerate(rows)]
    n_ok, dst_len = len(rows4), len(rows4) * cap
    dst = _dst(dst_len + 40, torch.int16)
    rows4 += [(0, 100, -1, cap), (0, 100, -(1 << 62), cap), (0, 100, dst_len + 40, cap), (0, 100, 1 << 62, 1 << 62), (0, 100, 5, -3),
              (0, 100, 5, -(1 << 63)), (0, 100, dst_len + 10, 1 << 40)]
    first100 = R.reference(clip[:100], C, L, os, g)
    many = Buf(2 * len(rows4), torch.int32, C_FILL)
    many.t.copy_(torch.cat([counts.t, torch.tensor([first100.counts[0], first100.counts[1]] * 7, dtype=torch.int32, device=DEV)]))
    lens = apply(lib, src.t, rows4, os, L, many, dst, cap, [g] * len(rows4))
    got = dst.t.cpu().numpy()
    for q in range(len(bad_src)):
        assert lens[q] == 0 and bool((got[q * cap:(q + 1) * cap] == 0).all()), rows4[q]
    for k, (s, _) in enumerate(cut_src):
        q, v = len(bad_src) + k, min(pool_len - s, cap)
        want = R.reference(clip[s:], C, L, os, g).out
        assert lens[q] == v and np.array_equal(got[q * cap:q * cap + v], want[:v]) and bool((got[q * cap + v:(q + 1) * cap] == 0).all())
    assert lens[n_ok:n_ok + 6].tolist() == [0] * 6 and bool((got[dst_len:dst_len + 10] == 12345).all())
    assert first100.counts[0] > 0 and lens[-1] == 30 and np.array_equal(got[dst_len + 10:], first100.out[:30])
    assert src.guards_intact()


# ---- finite reach: a window of the row with `reach` samples to either side gives the row's own bits -----------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("L,os", [(0, 4), (16, 2), (67, 4), (67, 1), (1024, 4)])
def test_a_window_with_reach_is_bit_equal_to_the_whole_row(lib, L, os, kind):
    dtype = TORCH_OF[kind]
    reach = 2 * L + HW
    n = 2 * reach + 3 * R.TILE + 40
    clip = R.clip(n, 31 + L, kind, L)
    spans = [(reach, reach + 500), (reach + 777, reach + 777 + R.TILE + 1), (n - reach - 1, n - reach)]
    src, starts = _pool([clip], dtype, 1, np.random.RandomState(6))
    rows = [(starts[0], n)] + [(starts[0] + a - reach, b - a + 2 * reach) for a, b in spans]
    g = [3.0] * len(rows)
    st, ct, counts = measure(lib, src.t, rows, os, L, g)
    outs = _apply_rows(lib, src, rows, os, L, counts, dtype, 0, np.random.RandomState(6), g)
    _check_row("whole", clip, os, L, 3.0, st[0], ct[0], outs[0])
    for (a, b), out in zip(spans, outs[1:]):
        assert out[reach:reach + b - a].tobytes() == outs[0][a:b].tobytes(), "the window [%d, %d) with reach %d" % (a, b, reach)


def test_another_ceiling_and_half_width(lib):
    """-6 dB and a 4-sample half width through the public tables (not the module's cached ones)"""
    c, hw, L, os = R.ceiling(-6.0), 4, 16, 4
    clip = R.clip(R.TILE + 77, 8, "float32", L)
    h = torch.from_numpy(audio.resample_filter(1, os, hw, 5.0)[2]).to(DEV)
    w = torch.from_numpy(audio.limiter_window(L)).to(DEV)
    src = torch.from_numpy(clip).to(DEV)
    n = clip.size
    table4 = torch.tensor([(0, n, 0, n)], dtype=torch.int64, device=DEV)
    need = lib.t2s_limit_scratch(1, n)
    scratch = torch.empty(need, dtype=torch.float64, device=DEV)
    stats, counts = torch.empty(4, dtype=torch.float64, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    assert lib.t2s_limit_measure(src.data_ptr(), 1, n, table4.data_ptr(), 1, n, None, h.data_ptr(), h.numel(), os, hw, w.data_ptr(), L, c,
                                 scratch.data_ptr(), need, stats.data_ptr(), counts.data_ptr(), _st()) == 0
    assert lib.t2s_limit_apply(src.data_ptr(), 1, n, table4.data_ptr(), 1, None, h.data_ptr(), h.numel(), os, hw, w.data_ptr(), L, c,
                               counts.data_ptr(), out.data_ptr(), 1, n, n, None, _st()) == 0
    ref = R.limit(clip, c, L, os, hw, 5.0, 1.0)
    assert tuple(counts.tolist()) == ref.counts and ref.counts[0] > 50
    got = out.cpu().numpy()
    assert np.abs(got).max() <= np.float32(c) and np.abs(got.astype(np.float64) - ref.o).max() <= 2.0 ** -23


def test_refused_calls_launch_nothing(lib):
    """every T2S_EINVAL case the header lists, with real buffers: sentinels everywhere stay"""
    n, L, os = 5000, 16, 4
    clip = R.clip(n, 0, "int16", L)
    src = _src_buf(2 * n, torch.int16)
    src.t[:n].copy_(torch.from_numpy(clip))
    before = src.raw.clone()
    need = lib.t2s_limit_scratch(1, n)
    assert need == 4 * ((n + R.TILE - 1) // R.TILE)
    assert [lib.t2s_limit_scratch(*a) for a in ((0, n), (65536, n), (1, 0), (1, 1 << 31), (-1, n), (1, -5))] == [-1] * 6
    scratch, stats, counts, dst = Buf(need, torch.float64, S_FILL), Buf(4, torch.float64, S_FILL), Buf(2, torch.int32, C_FILL), _dst(n, torch.int16)
    table = torch.tensor([(0, n)], dtype=torch.int64, device=DEV)
    table4 = torch.tensor([(0, n, 0, n)], dtype=torch.int64, device=DEV)
    fsrc = torch.zeros(n, dtype=torch.float32, device=DEV)
    gains = torch.ones(3, dtype=torch.float64, device=DEV)
    lens = torch.full((3,), -77, dtype=torch.int32, device=DEV)
    h, w = _hw(os, L)
    good = dict(src=src.t.data_ptr(), table=table.data_ptr(), gains=gains.data_ptr(), h=h.t.data_ptr(), w=w.t.data_ptr(),
                scratch=scratch.t.data_ptr(), stats=stats.t.data_ptr(), counts=counts.t.data_ptr(), dst=dst.t.data_ptr(), lens=lens.data_ptr())
    scalars = dict(kind=0, src_len=n, rows=1, max_count=n, n_taps=h.t.numel(), os=os, hw=HW, L=L, c=C, scratch_len=need, dkind=0, dst_len=n,
                   max_out=n)

    def ptr(kw, k, base):
        v = kw.get(k, "good")
        return {"good": base[k], "null": None}.get(v, base[k] + (v if isinstance(v, int) else 0))

    def measure_call(**kw):
        a = dict(scalars, **{k: v for k, v in kw.items() if k in scalars})
        p = lambda k: ptr(kw, k, good)
        return lib.t2s_limit_measure(p("src"), a["kind"], a["src_len"], p("table"), a["rows"], a["max_count"], p("gains"), p("h"), a["n_taps"],
                                     a["os"], a["hw"], p("w"), a["L"], a["c"], p("scratch"), a["scratch_len"], p("stats"), p("counts"), _st())

    good4 = dict(good, table=table4.data_ptr())

    def apply_call(**kw):
        a = dict(scalars, src_len=2 * n)
        a.update({k: v for k, v in kw.items() if k in scalars})
        p = lambda k: ptr(kw, k, good4)
        d = {"src": good["src"], "inside src": good["src"] + 2 * n}.get(kw.get("dst"), None) or p("dst")
        s = fsrc.data_ptr() if a["kind"] in (1, 2) and "src" not in kw else p("src")
        return lib.t2s_limit_apply(s, a["kind"], a["src_len"], p("table"), a["rows"], p("gains"), p("h"), a["n_taps"], a["os"], a["hw"], p("w"),
                                   a["L"], a["c"], p("counts"), d, a["dkind"], a["dst_len"], a["max_out"], p("lens"), _st())

    shared = [dict(src="null"), dict(table="null"), dict(h="null"), dict(w="null"), dict(table=4), dict(gains=4), dict(h=4), dict(w=4),
              dict(kind=-1), dict(kind=3), dict(src_len=0), dict(src_len=-5), dict(rows=0), dict(rows=-1), dict(rows=65536),
              dict(os=0), dict(os=3), dict(os=8), dict(os=-1), dict(os=2), dict(n_taps=h.t.numel() - 1), dict(n_taps=h.t.numel() + 1),
              dict(n_taps=h.t.numel() + 2), dict(hw=0), dict(hw=-1), dict(hw=33, n_taps=2 * 33 * os + 1), dict(L=-1), dict(L=1025),
              dict(c=0.0), dict(c=-0.5), dict(c=float("nan")), dict(c=float("inf")), dict(c=0.1), dict(c=10.0 ** (-1.0 / 20.0))]
    refused_measure = shared + [dict(scratch="null"), dict(stats="null"), dict(counts="null"), dict(scratch=4), dict(stats=4), dict(counts=2),
                                dict(max_count=0), dict(max_count=-1), dict(max_count=1 << 31), dict(scratch_len=need - 1),
                                dict(scratch_len=0), dict(scratch_len=-1)]
    refused_apply = shared + [dict(counts="null"), dict(dst="null"), dict(counts=2), dict(lens=2), dict(dkind=1), dict(dkind=-1), dict(dkind=2),
                              dict(kind=1, dkind=0, src_len=n), dict(kind=2, dkind=0, src_len=n), dict(kind=1, dkind=2, src_len=n),
                              dict(dst_len=0), dict(dst_len=-1), dict(max_out=0), dict(max_out=-1), dict(max_out=(1 << 40) + 1),
                              dict(dst="src"), dict(dst="inside src", dst_len=n)]
    for kw in refused_measure:
        assert measure_call(**kw) == -1, kw
    for kw in refused_apply:
        assert apply_call(**kw) == -1, kw
    torch.cuda.synchronize()
    for b in (scratch, stats, counts, dst):
        assert b.untouched(), "a refused call wrote something"
    assert bool((src.raw == before).all()) and bool((lens == -77).all())
    print("LIMITER refused: %d measure and %d apply tuples" % (len(refused_measure), len(refused_apply)))
    # and the accepted calls do write
    assert measure_call() == 0
    torch.cuda.synchronize()
    counts_d = counts.t.clone()
    good4["counts"] = counts_d.data_ptr()
    assert apply_call() == 0
    torch.cuda.synchronize()
    assert int(lens[0]) == n and dst.guards_intact()
    _check_row("accepted", clip, os, L, 1.0, stats.t.cpu().numpy(), counts_d.cpu().numpy(), dst.t.cpu().numpy())


def test_two_identical_calls_give_identical_bits(lib):
    L, os = 67, 4
    clip = R.clip(2 * R.TILE + 17, 5, "float32", L)
    src, starts = _pool([clip], torch.float32, 0, np.random.RandomState(0))
    rows = [(starts[0], clip.size)]
    a = measure(lib, src.t, rows, os, L, [3.0])
    b = measure(lib, src.t, rows, os, L, [3.0])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    oa = _apply_rows(lib, src, rows, os, L, a[2], torch.float32, 0, np.random.RandomState(0), [3.0])[0]
    ob = _apply_rows(lib, src, rows, os, L, b[2], torch.float32, 0, np.random.RandomState(0), [3.0])[0]
    assert oa.tobytes() == ob.tobytes()
