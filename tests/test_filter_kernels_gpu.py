"""t2s_sos_filter / t2s_sos_window (csrc/sosfilt.hip, csrc/t2s_api_sosfilt.hip) called directly on guarded buffers, against the
float64 restatement of tests/filter_ref.py.

The bar for a float32 output y[i] is 2^-24 |ref[i]| + 16 max(E, 2^-50 G max|x|): ref the sequential float64 scipy.signal.sosfilt, G the
l1 norm of the cascade's impulse response and E the largest difference between the parallel-order and the sequential float64
forms - measured on the CPU between two references, never from the device (tests/test_filter_ref_cpu.py asserts that this second
term stays below a quarter of a float32 ulp at the row's peak for the accuracy cases).  An int16 output equals pcm_round16(ref)
except where ref lies within that second term of a half-integer.  Bits are compared for EQUALITY: a row alone, at each place of a
batch, scattered in a pool, and cut into the pieces of a stream.

Every source is a view into a larger tensor of sentinels (+-32767, or NaN / 1e4), every destination, scratch, carry and table a
view into a larger tensor of sentinels which must come back untouched."""
import numpy as np
import pytest
import torch

import filter_ref as R
from text2speech_amd import _lib, audio
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
T, S = R.TILE, R.SEGMENT
ROW_LENGTHS = (0, 1, 2, S - 1, S, S + 1, T - 1, T, T + 1, 2 * T + 777)
KIND = {torch.int16: 0, torch.float32: 1, torch.float16: 2}
NP_OF = {torch.int16: np.int16, torch.float32: np.float32, torch.float16: np.float16}
D_FILL, C_FILL, T_FILL = -7.0, -99, -99
WORST = {}                  # case -> the worst device error / bar seen (printed; profiles/filter_tests.md records a run)


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.t2s_sos_tile() == T and lib.t2s_sos_segment() == S and lib.t2s_sos_max_sections() == R.MAX_SECTIONS
    assert lib.t2s_sos_table_doubles() == R.TAB_DOUBLES
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


_TAB = {}


def _tab(sos):
    key = np.asarray(sos).tobytes()
    if key not in _TAB:
        b = Buf(R.TAB_DOUBLES, torch.float64, D_FILL)
        b.t.copy_(torch.from_numpy(audio.sos_table(sos, S, R.LANES)))
        _TAB[key] = b
    return _TAB[key]


def run_filter(lib, src, rows4, sos, dst, gains=None, max_count=None, max_out=None):
    """rows4: (src_start, src_count, dst_start, dst_cap) -> counts [n, 2]; src a tensor, dst a Buf"""
    n_rows, n = len(rows4), np.asarray(sos).shape[0]
    max_count = max_count or max(1, max(r[1] for r in rows4))
    max_out = max_out or max(1, max(r[3] for r in rows4))
    need = lib.t2s_sos_scratch(n_rows, max_count, n)
    assert need > 0
    scratch, counts, table = Buf(need, torch.float64, D_FILL), Buf(2 * n_rows, torch.int32, C_FILL), Buf(4 * n_rows, torch.int64, T_FILL)
    table.t.copy_(torch.tensor(rows4, dtype=torch.int64).view(-1))
    g = None
    if gains is not None:
        g = Buf(n_rows, torch.float64, D_FILL)
        g.t.copy_(torch.tensor(gains, dtype=torch.float64))
    tab = _tab(sos)
    rc = lib.t2s_sos_filter(src.data_ptr(), KIND[src.dtype], src.numel(), table.t.data_ptr(), n_rows, max_count,
                            g.t.data_ptr() if g else None, tab.t.data_ptr(), n, scratch.t.data_ptr(), need, dst.t.data_ptr(),
                            KIND[dst.t.dtype], dst.t.numel(), max_out, counts.t.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert dst.guards_intact(), "wrote outside the destination"
    assert scratch.guards_intact() and counts.guards_intact() and table.guards_intact() and tab.guards_intact()
    assert g is None or g.guards_intact()
    assert bool((table.t.cpu() == torch.tensor(rows4, dtype=torch.int64).view(-1)).all())
    return counts.t.cpu().numpy().reshape(n_rows, 2)


_SOLO = {}


def solo(lib, sos, x, out_dtype, gain=None):
    """the row alone in a buffer of its own -> (output, counts [2]); computed once per (filter, row, destination, gain)"""
    key = (np.asarray(sos).tobytes(), x.tobytes(), x.dtype.str, out_dtype, gain)
    if key not in _SOLO:
        src = _src_buf(x.size, {v: k for k, v in NP_OF.items()}[x.dtype.type])
        if x.size:
            src.t[:x.size].copy_(torch.from_numpy(x))
        dst = _dst(x.size, out_dtype)
        counts = run_filter(lib, src.t, [(0, x.size, 0, x.size)], sos, dst, None if gain is None else [gain])
        _SOLO[key] = (dst.t[:x.size].cpu().numpy(), counts[0])
    return _SOLO[key]


def _rows(dtype, lengths, seed):
    """seeded rows of the given lengths as the device receives them"""
    rng = np.random.RandomState(seed)
    out = []
    for L in lengths:
        if dtype == torch.int16:
            out.append(np.clip(np.rint(5000.0 * rng.randn(L)), -32768, 32767).astype(np.int16))
        else:
            out.append((0.4 * rng.randn(L)).astype(NP_OF[dtype]))
    return out


def _E_G(sos, x, gain):
    """(ref, the bar's second term) of a row, on the CPU"""
    ref, _ = R.sequential(sos, x, gain)
    if x.size == 0:
        return ref, 0.0
    par, _ = R.parallel(sos, audio.sos_table(sos, S, R.LANES), x, gain)
    v = R.substitute(x, gain)[0]
    return ref, R.second_term(float(np.max(np.abs(par - ref))), R.impulse_l1(sos), float(np.max(np.abs(v))))


def _check_f32(case, got, ref, term):
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    if ref.size == 0:
        return
    ratio = float(np.max(np.abs(got.astype(np.float64) - ref) / (2.0 ** -24 * np.abs(ref) + term)))
    WORST[case] = max(WORST.get(case, 0.0), ratio)
    print("%-40s worst |device - ref| / bar %.4f" % (case, ratio))
    assert ratio <= 1.0, case


def _check_i16(case, got, ref, term, max_share=1e-3):
    want, _ = R.round16(ref)
    diff = got.astype(np.int64) - want.astype(np.int64)
    exempt = R.int16_exempt(ref, term)
    assert np.all(diff[~exempt] == 0), case
    assert np.all(np.abs(diff) <= 1), case
    assert ref.size == 0 or float(np.mean(exempt)) <= max_share, case
    print("%-40s int16: %d of %d samples differ by one code (all exempt)" % (case, int(np.count_nonzero(diff)), ref.size))


PAIRS = ((torch.int16, torch.int16), (torch.int16, torch.float32), (torch.float32, torch.float32), (torch.float16, torch.float32))


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s-%s" % (str(p[0])[6:], str(p[1])[6:]))
@pytest.mark.parametrize("n", (1, 2, 4, R.MAX_SECTIONS))
def test_rows_scattered_in_a_pool(lib, n, pair):
    """every row length, each row scattered in a pool at either 2-byte parity, dst_cap either side of the length and +0 behind:
    the bits of the row alone, and the reference under the bar"""
    src_t, dst_t = pair
    sos = R.sections_case(n)
    rows = _rows(src_t, ROW_LENGTHS, 100 + n)
    gain = 1.0 / 32768.0 if (src_t == torch.int16 and dst_t == torch.float32) else None
    for shift in (0, 1):
        starts, pos = [], 3 + shift
        for x in rows:
            starts.append(pos)
            pos += x.size + 1 + (len(starts) % 4)
        pool = _src_buf(pos + 5, src_t, shift)
        for x, s0 in zip(rows, starts):
            if x.size:
                pool.t[s0:s0 + x.size].copy_(torch.from_numpy(x))
        caps = [max(0, x.size + d) for x, d in zip(rows, (3, 0, -1, 5, 0, -7, 9, 0, -100, 11))]
        dstarts, dpos = [], 2 - shift
        for c in caps:
            dstarts.append(dpos)
            dpos += c + 2
        dst = _dst(dpos + 3, dst_t, shift)
        table = [(s0, x.size, d0, c) for x, s0, d0, c in zip(rows, starts, dstarts, caps)]
        counts = run_filter(lib, pool.t, table, sos, dst, None if gain is None else [gain] * len(rows))
        out = dst.t.cpu().numpy()
        fill = np.array(dst.fill, dtype=out.dtype)
        written = np.zeros(out.size, dtype=bool)
        for r, (x, d0, c) in enumerate(zip(rows, dstarts, caps)):
            want, want_counts = solo(lib, sos, x, dst_t, gain)
            k = min(x.size, c)
            assert np.array_equal(out[d0:d0 + k].view(np.uint8), want[:k].view(np.uint8)), (shift, r)
            assert not np.any(out[d0 + k:d0 + c]) and not np.any(np.signbit(out[d0 + k:d0 + c].astype(np.float64))), (shift, r)
            written[d0:d0 + c] = True
            assert counts[r, 0] == want_counts[0] == 0
            if c >= x.size:
                assert counts[r, 1] == want_counts[1]
        assert np.all(out[~written] == fill), "a store outside every row's [dst_start, dst_start + dst_cap)"
    for x in rows[3:]:
        want, _ = solo(lib, sos, x, dst_t, gain)
        ref, term = _E_G(sos, x, 1.0 if gain is None else gain)
        case = "sections=%d %s->%s L=%d" % (n, str(src_t)[6:], str(dst_t)[6:], x.size)
        if dst_t == torch.int16:
            _check_i16(case, want, ref, term, max_share=1.0)        # (the share is the accuracy cases' business)
        else:
            _check_f32(case, want, ref, term)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("f32", "f16"))
def test_ragged_batch_every_place(lib, dtype):
    """B = 3, rows an odd stride apart, NaN / 1e4 behind every length, per-row gains 0, 1 and 32768: every row's bits are the row's
    alone, at each place of the batch"""
    sos = R.ACCURACY_CASES["telephone_300_3400_o4_8000"]
    lengths = (T + 1, 2 * T + 777, S - 1)
    rows = _rows(dtype, lengths, 7)
    N, ld = max(lengths), max(lengths) + 3
    for perm, gains in (((0, 1, 2), (1.0, 32768.0, 0.0)), ((2, 0, 1), (32768.0, 1.0, 1.0)), ((1, 2, 0), (0.0, 1.0, 32768.0))):
        batch = _src_buf(3 * ld, dtype, 1)
        for b, r in enumerate(perm):
            batch.t[b * ld:b * ld + lengths[r]].copy_(torch.from_numpy(rows[r]))
        dst = _dst(3 * N, torch.float32)
        table = [(b * ld, lengths[r], b * N, N) for b, r in enumerate(perm)]
        counts = run_filter(lib, batch.t, table, sos, dst, gains)
        out = dst.t.cpu().numpy().reshape(3, N)
        for b, r in enumerate(perm):
            want, _ = solo(lib, sos, rows[r], torch.float32, gains[b])
            assert np.array_equal(out[b, :lengths[r]].view(np.uint32), want.view(np.uint32)), (perm, b)
            assert not np.any(out[b, lengths[r]:].view(np.uint32)), (perm, b)
            assert counts[b].tolist() == [0, 0]
            if gains[b] == 0.0:
                assert not np.any(want)
    x = rows[1]
    for g in (1.0, 32768.0):
        want, _ = solo(lib, sos, x, torch.float32, g)
        ref, term = _E_G(sos, x, g)
        _check_f32("telephone gain=%g %s" % (g, str(dtype)[6:]), want, ref, term)


def test_nonfinite_samples_are_zero_and_counted(lib):
    """NaN and infinities inside a row, at a segment edge and a tile edge: counted, treated as +0, the output finite and the
    reference's on the substituted row"""
    for case in ("deemphasis_0.97", "highpass_80_o4_44800"):
        sos = R.ACCURACY_CASES[case]
        for dtype in (torch.float32, torch.float16):
            x = _rows(dtype, (2 * T + 777,), 11)[0]
            at = [0, 5, S - 1, S, T - 1, T, T + 1, 2 * T, x.size - 1]
            x[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, np.nan, -np.inf, np.nan]
            got, counts = solo(lib, sos, x, torch.float32)
            assert counts.tolist() == [len(at), 0] and np.all(np.isfinite(got))
            ref, term = _E_G(sos, x, 1.0)
            _check_f32("%s with non-finite samples %s" % (case, str(dtype)[6:]), got, ref, term)
            # a gain that takes the product out of range is the same substitution
            big = np.array([1.0, 3e38, -2.0], dtype=np.float32)
            if dtype == torch.float32:
                got, counts = solo(lib, sos, big, torch.float32, float("inf"))
                assert counts.tolist() == [3, 0] and not np.any(got)


def test_int16_saturation_is_counted(lib):
    sos = np.array([[4.0, 0.0, 0.0, 1.0, 0.0, 0.0]])
    x = np.array([8191, 8192, -8192, -8193, 20000, -20000, 0, 1], dtype=np.int16)
    got, counts = solo(lib, sos, x, torch.int16)
    assert got.tolist() == [32764, 32767, -32768, -32768, 32767, -32768, 0, 4] and counts.tolist() == [0, 4]


@pytest.mark.parametrize("case", sorted(R.ACCURACY_CASES))
def test_accuracy_cases(lib, case):
    """the cases of the issue's table on the accuracy rows: float32 under the bar, the int16 pool row equal to pcm_round16(ref)
    except within the bar's second term of a half-integer"""
    for row in sorted(R.input_rows()):
        sos, x, ref, E, G, term = R.measure(case, row)
        if x.dtype == np.int16:
            got, counts = solo(lib, sos, x, torch.int16)
            _check_i16("%s %s" % (case, row), got, ref, term)
            assert counts.tolist() == [0, R.round16(ref)[1]]
            got32, _ = solo(lib, sos, x, torch.float32, 1.0 / 32768.0)
            ref32, term32 = _E_G(sos, x, 1.0 / 32768.0)
            _check_f32("%s %s / 32768" % (case, row), got32, ref32, term32)
        else:
            got, counts = solo(lib, sos, x, torch.float32)
            _check_f32("%s %s" % (case, row), got, ref, term)
            assert counts.tolist() == [0, 0]
            x16 = x.astype(np.float16)
            got, _ = solo(lib, sos, x16, torch.float32)
            ref16, term16 = _E_G(sos, x16, 1.0)
            _check_f32("%s %s as f16" % (case, row), got, ref16, term16)


def test_nonsense_table_values_are_safe(lib):
    sos = R.sections_case(2)
    x = _rows(torch.float32, (T + 50,), 3)[0]
    src = _src_buf(x.size + 10, torch.float32)
    src.t[4:4 + x.size].copy_(torch.from_numpy(x))
    n_dst = x.size + 20
    big = 2 ** 62
    table = [(4, x.size, 3, x.size),                            # a good row
             (-1, 10, 0, 0), (4, -5, 0, 0), (big, 10, 0, 0), (4, big, -3, 10), (4, 10, big, 10), (4, 10, 5, -big),
             (src.t.numel() - 2, 100, n_dst - 2, 100),          # cut at both ends: two samples in, two out
             (-big, big, -big, big), (src.t.numel(), 1, n_dst, 1)]
    dst = _dst(n_dst, torch.float32)
    good, _ = solo(lib, sos, x, torch.float32)
    run_filter(lib, src.t, table[:1], sos, dst, max_count=T + 50, max_out=T + 50)
    one = dst.t.cpu().numpy().copy()
    assert np.array_equal(one[3:3 + x.size].view(np.uint32), good.view(np.uint32))
    dst2 = _dst(n_dst, torch.float32)
    run_filter(lib, src.t, table, sos, dst2, max_count=T + 50, max_out=T + 50)
    out = dst2.t.cpu().numpy()
    assert np.array_equal(out[3:3 + x.size].view(np.uint32), good.view(np.uint32))
    assert np.all(out[:3] == np.float32(dst2.fill)) and np.all(out[3 + x.size:n_dst - 2] == np.float32(dst2.fill))
    assert np.all(np.isfinite(out[n_dst - 2:]))                 # the cut row: two filtered samples of the sentinels' substitution
    # a row longer than max_count is cut there, and max_out cuts the stores
    dst3 = _dst(n_dst, torch.float32)
    run_filter(lib, src.t, [(4, x.size, 0, n_dst)], sos, dst3, max_count=T - 5, max_out=T + 9)
    out = dst3.t.cpu().numpy()
    short, _ = solo(lib, sos, x[:T - 5], torch.float32)
    assert np.array_equal(out[:T - 5].view(np.uint32), short.view(np.uint32)) and not np.any(out[T - 5:T + 9].view(np.uint32))
    assert np.all(out[T + 9:] == np.float32(dst3.fill))


def _ptr(v):
    return None if v is None else int(v)


def test_refused_calls_write_nothing(lib):
    """every T2S_EINVAL case of tests/filter_ref.py's lists, here with real buffers: sentinels everywhere stay"""
    sos, n, B, L = R.sections_case(2), 2, 2, 100
    tab = _tab(sos)
    src, dst = _src_buf(B * L, torch.float32), _dst(B * L, torch.float32)
    table, gains = Buf(4 * B, torch.int64, T_FILL), Buf(B, torch.float64, D_FILL)
    table.t.copy_(torch.tensor([(0, L, 0, L), (L, L, L, L)], dtype=torch.int64).view(-1))
    gains.t.fill_(1.0)
    need = lib.t2s_sos_scratch(B, L, n)
    scratch, counts = Buf(need, torch.float64, D_FILL), Buf(2 * B, torch.int32, C_FILL)
    base = dict(src=src.t.data_ptr(), src_kind=1, src_len=B * L, table=table.t.data_ptr(), n_rows=B, max_count=L,
                gains=gains.t.data_ptr(), tab=tab.t.data_ptr(), n_sections=n, scratch=scratch.t.data_ptr(), scratch_len=need,
                dst=dst.t.data_ptr(), dst_kind=1, dst_len=B * L, max_out=L, counts=counts.t.data_ptr(), stream=None)
    for label, changes in R.filter_refusals():
        a = R.apply_changes(base, changes)
        assert lib.t2s_sos_filter(*[_ptr(a[p]) if p in ("src", "table", "gains", "tab", "scratch", "dst", "counts", "stream") else a[p]
                                    for p in R.FILTER_PARAMS]) == -1, label
    words = lib.t2s_sos_window_carry(n) // 8
    carry = [Buf(B * words, torch.float64, D_FILL) for _ in range(2)]
    piece, out = _src_buf(B * L, torch.float32), _dst(B * L, torch.float32)
    wbase = dict(carry_in=carry[0].t.data_ptr(), carry_out=carry[1].t.data_ptr(), piece=piece.t.data_ptr(), is_half=0, B=B, n=L, ldp=L,
                 N0=0, gains=gains.t.data_ptr(), tab=tab.t.data_ptr(), n_sections=n, scratch=scratch.t.data_ptr(), scratch_len=need,
                 out=out.t.data_ptr(), ldo=L, counts=counts.t.data_ptr(), stream=None)
    for label, changes in R.window_refusals():
        a = R.apply_changes(wbase, changes)
        assert lib.t2s_sos_window(*[_ptr(a[p]) if p in ("carry_in", "carry_out", "piece", "gains", "tab", "scratch", "out", "counts",
                                                         "stream") else a[p] for p in R.WINDOW_PARAMS]) == -1, label
    torch.cuda.synchronize()
    for b in (dst, scratch, counts, out, carry[0], carry[1]):
        assert b.untouched()
    assert tab.guards_intact() and table.guards_intact()


class Window:
    """a stream at the entry points: two guarded carries used in turn, guarded counts, the position on the host"""

    def __init__(self, lib, sos, B, gains=None):
        self.lib, self.n, self.B, self.tab = lib, np.asarray(sos).shape[0], B, _tab(sos)
        self.words = lib.t2s_sos_window_carry(self.n) // 8
        self.carry = [Buf(B * self.words, torch.float64, D_FILL) for _ in range(2)]
        self.carry[0].t.zero_()
        self.counts = Buf(2 * B, torch.int32, C_FILL)
        self.counts.t.zero_()
        self.gains = None
        if gains is not None:
            self.gains = Buf(B, torch.float64, D_FILL)
            self.gains.t.copy_(torch.tensor(gains, dtype=torch.float64))
        self.i, self.pos, self.bufs = 0, 0, []

    def push(self, piece, n, ldp):
        """piece: a device tensor holding [B] rows of n samples ldp apart (None for n = 0) -> (out Buf of [B, n + 1], counts clone)"""
        need = max(1, self.lib.t2s_sos_scratch(self.B, self.pos % T + max(n, 1), self.n))
        scratch, out = Buf(need, torch.float64, D_FILL), _dst(self.B * (n + 1), torch.float32, 1)
        rc = self.lib.t2s_sos_window(self.carry[self.i].t.data_ptr(), self.carry[1 - self.i].t.data_ptr(),
                                     piece.data_ptr() if n else None, int(n and piece.dtype == torch.float16), self.B, n, ldp, self.pos,
                                     self.gains.t.data_ptr() if self.gains else None, self.tab.t.data_ptr(), self.n,
                                     scratch.t.data_ptr(), need, out.t.data_ptr() if n else None, n + 1, self.counts.t.data_ptr(), _st())
        assert rc == 0
        self.i, self.pos = 1 - self.i, self.pos + n
        self.bufs += [scratch, out]
        return out, self.counts.t.clone()

    def feed(self, rows, cuts):
        """rows: numpy [B, L]; -> (outputs [B, L], counts after every push [pushes, B, 2]); one synchronisation at the end"""
        B, L = rows.shape
        dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}[rows.dtype]
        ld = L + 5
        src = _src_buf(B * ld, dtype, 1)
        for b in range(B):
            src.t[b * ld:b * ld + L].copy_(torch.from_numpy(rows[b]))
        outs, cnts, at = [], [], 0
        for n in cuts:
            out, c = self.push(src.t[at:] if n else None, n, ld)
            outs.append((out, n))
            cnts.append(c)
            at += n
        torch.cuda.synchronize()
        for b in self.bufs + self.carry + [self.counts, self.tab]:
            assert b.guards_intact()
        got = np.concatenate([o.t.cpu().numpy().reshape(B, n + 1)[:, :n] for o, n in outs], 1)
        for o, n in outs:
            assert np.all(o.t.cpu().numpy().reshape(B, n + 1)[:, n] == np.float32(o.fill)), "a store behind a row's n outputs"
        return got, torch.stack(cnts).cpu().numpy().reshape(len(cuts), B, 2)


def _stream_rows(B, L, dtype, seed):
    rows = np.stack(_rows(torch.float32, (L,) * B, seed)).astype(dtype)
    bad = [[L // 3], [], [1, min(L - 1, T + 1)]][:B]
    for b, at in enumerate(bad):
        if L > 4:
            rows[b, at] = np.nan
    return rows, [[a for a in at] if L > 4 else [] for at in bad]


@pytest.mark.parametrize("case", sorted(R.BIT_CASES) + ["sections_8"])
def test_stream_is_the_whole_row_bit_for_bit(lib, case):
    """any cuts: the concatenated outputs are t2s_sos_filter's row, and the counts after every push are those of the samples seen"""
    sos = R.sections_case(8) if case == "sections_8" else R.BIT_CASES[case]
    plans = [(3, 2 * T + 777, np.float32, None), (1, 2 * T + 777, np.float16, ("random", "T+1", "long")), (1, 300, np.float32, None),
             (3, 300, np.float16, ("ones", "S")), (1, T, np.float32, ("one", "T-1", "random")), (3, 1, np.float32, None)]
    for B, L, dtype, only in plans:
        rows, bad = _stream_rows(B, L, dtype, 40 + B)
        whole = [solo(lib, sos, rows[b], torch.float32) for b in range(B)]
        for b in range(B):
            assert whole[b][1].tolist() == [len(bad[b]), 0]
        for name, cuts in R.cut_patterns(L, seed=B).items():
            if only is not None and name not in only:
                continue
            got, cnts = Window(lib, sos, B).feed(rows, cuts)
            for b in range(B):
                assert np.array_equal(got[b].view(np.uint32), whole[b][0].view(np.uint32)), (case, B, L, dtype, name, b)
                seen = np.cumsum(cuts)
                want = [sum(1 for a in bad[b] if a < s) for s in seen]
                assert cnts[:, b, 0].tolist() == want and not np.any(cnts[:, b, 1]), (case, B, L, name, b)


def test_stream_with_gains(lib):
    sos = R.ACCURACY_CASES["highpass_80_o4_44800"]
    rows, _ = _stream_rows(3, T + 300, np.float32, 9)
    gains = (0.0, 1.0, 32768.0)
    got, _ = Window(lib, sos, 3, gains).feed(rows, R.cut_patterns(T + 300, seed=5)["random"])
    for b in range(3):
        want, _ = solo(lib, sos, rows[b], torch.float32, gains[b])
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), b


def test_worst_ratios_are_reported():
    """(runs last in this file) the worst device error over the bar per case, for profiles/filter_tests.md"""
    for case in sorted(WORST):
        print("%-44s %.4f" % (case, WORST[case]))
    assert all(v <= 1.0 for v in WORST.values())
