"""t2s_join_offsets / t2s_join_gather (csrc/join.hip, csrc/t2s_api_audio.hip) called directly on guarded buffers, against
tests/join_ref.py (pinned by tests/test_join_ref_cpu.py).  The destination is pre-filled with NaN and compared with the reference
BIT FOR BIT: every element of dst[0 : dst_cap) must be defined afterwards, and nothing at or beyond dst_cap - or in the guards
around any buffer - may be touched.  Behind every row's length the sources hold NaN and 1e4, which must never reach dst."""
import numpy as np
import pytest
import torch

import join_ref as J
from text2speech_amd import _lib
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
KIND = {torch.float32: 1, torch.float16: 2}
NP_OF = {torch.float32: np.float32, torch.float16: np.float16}
F = 8
NAN = float("nan")


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def T(lib):
    return lib.t2s_join_tile()


class Buf:
    """A device tensor of n elements inside a larger one: GUARD + shift elements of `fill` in front, GUARD behind."""

    def __init__(self, n, dtype, fill, shift=0):
        self.raw = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device=DEV)
        self.lo = GUARD + shift
        self.t = self.raw[self.lo:self.lo + n]
        self.fill = fill

    def guards_intact(self):
        a, b = self.raw[:self.lo], self.raw[self.lo + self.t.numel():]
        if isinstance(self.fill, float) and self.fill != self.fill:
            return bool(a.isnan().all()) and bool(b.isnan().all())
        return bool((a == self.fill).all()) and bool((b == self.fill).all())


def _ints(values, fill=-77):
    b = Buf(max(1, len(values)), torch.int32, fill)
    if len(values):
        b.t[:len(values)].copy_(torch.tensor(list(values), dtype=torch.int32))
    return b


class Batch:
    """B rows of N samples, ldx apart, inside a guarded buffer; row b holds seeded samples up to max(0, min(lengths[b], N)) and
    NaN / 1e4 alternating behind them (and between the rows)."""

    def __init__(self, lengths, N, dtype=torch.float32, ldx=None, seed=0):
        self.B, self.N, self.ldx, self.dtype = len(lengths), N, ldx or N, dtype
        self.lengths = list(lengths)
        n_el = (self.B - 1) * self.ldx + N
        self.buf = Buf(n_el, dtype, 1e4)
        host = np.empty(n_el, dtype=NP_OF[dtype])
        host[0::2] = np.nan
        host[1::2] = 1e4
        rng = np.random.RandomState(seed)
        self.rows = []
        for b, ln in enumerate(lengths):
            ln = max(0, min(ln, N))
            x = rng.uniform(-1, 1, ln).astype(NP_OF[dtype])
            host[b * self.ldx:b * self.ldx + ln] = x
            row = np.full(N, np.nan, dtype=NP_OF[dtype])
            row[:ln] = x
            self.rows.append(row)
        self.buf.t.copy_(torch.from_numpy(host))
        self.lens_d = _ints(lengths)


def scan(lib, lengths, caps, order, gaps, gap, dst, dst_cap):
    """t2s_join_offsets -> (offsets Buf, length), dst zeroed up to dst_cap"""
    n = len(lengths)
    lens_d, caps_d = _ints(lengths), _ints(caps)
    order_d = None if order is None else _ints(order)
    gaps_d = None if gaps is None else _ints(gaps)
    off = Buf(n + 1, torch.int64, -99)
    length = Buf(1, torch.int32, -77)
    rc = lib.t2s_join_offsets(lens_d.t.data_ptr(), caps_d.t.data_ptr(), None if order is None else order_d.t.data_ptr(),
                              None if gaps is None else gaps_d.t.data_ptr(), gap, n, dst.t.data_ptr(), dst_cap, off.t.data_ptr(),
                              length.t.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    for b in (lens_d, caps_d, order_d, gaps_d, off, length):
        assert b is None or b.guards_intact()
    return off, int(length.t.item())


def gather(lib, batch, pos, off, n, fade, fade_ends, dst, dst_cap):
    pos_d = _ints(pos)
    rc = lib.t2s_join_gather(batch.buf.t.data_ptr(), KIND[batch.dtype], batch.B, batch.N, batch.ldx, batch.lens_d.t.data_ptr(),
                             pos_d.t.data_ptr(), off.t.data_ptr(), n, fade, int(fade_ends), dst.t.data_ptr(), dst_cap, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert pos_d.guards_intact() and batch.buf.guards_intact() and batch.lens_d.guards_intact()


def _same_bits(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "first difference at %d: got %r, want %r (%d differ)" % (bad[0], got[bad[0]], want[bad[0]], bad.size)


def check(lib, lengths, N, order=None, gaps=None, gap=0, fade=F, fade_ends=False, dtype=torch.float32, ldx=None, shift=0,
          cap_delta=None, seed=0):
    """One batch of len(lengths) rows joined whole; dst_cap = total + cap_delta (None: some room behind the total)."""
    n = len(lengths)
    batch = Batch(lengths, N, dtype, ldx, seed)
    want_full, total, want_off = J.join(batch.rows, lengths, order, gaps, gap, fade, fade_ends)
    dst_cap = max(1, total + (37 if cap_delta is None else cap_delta))
    want, want_len, _ = J.join(batch.rows, lengths, order, gaps, gap, fade, fade_ends, dst_cap=dst_cap)
    dst = Buf(dst_cap, torch.float32, NAN, shift)
    off, length = scan(lib, lengths, [N] * n, order, gaps, gap, dst, dst_cap)
    pos = [0] * n
    for p, r in enumerate(range(n) if order is None else order):
        pos[r] = p
    gather(lib, batch, pos, off, n, fade, fade_ends, dst, dst_cap)
    assert dst.guards_intact(), "wrote outside dst[0 : dst_cap)"
    assert off.t.cpu().tolist() == want_off.tolist()
    assert length == want_len == min(total, dst_cap)
    _same_bits(dst.t.cpu().numpy(), want)
    return want


def _edge_lengths(T):
    return [0, 1, F - 1, F, 2 * F - 1, 2 * F, T - 1, T, T + 1, 2 * T + 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("which", ["ascending", "shuffled"])
def test_edge_lengths_in_two_orders(lib, T, dtype, which):
    lengths = _edge_lengths(T)
    n = len(lengths)
    order = None if which == "ascending" else [9, 0, 3, 7, 1, 8, 2, 6, 4, 5]
    check(lib, lengths, 2 * T + 3, order=order, gap=3, dtype=dtype, ldx=2 * T + 3 + 4)        # ldx odd
    assert n == 10


@pytest.mark.parametrize("fade_ends", [False, True])
@pytest.mark.parametrize("ln", [1, 5, 40])
def test_one_segment(lib, ln, fade_ends):
    check(lib, [ln], 41, fade_ends=fade_ends)


@pytest.mark.parametrize("gap", [0, 3])
def test_two_segments(lib, T, gap):
    check(lib, [T + 1, 2 * F], T + 2, gap=gap)
    check(lib, [3, 0], 5, gap=gap, fade_ends=True)


def test_scan_past_one_workgroups_width(lib):
    lengths = [(7 * i + i // 6) % 6 for i in range(300)]
    assert set(lengths) == set(range(6))
    order = list(np.random.RandomState(5).permutation(300))
    check(lib, lengths, 5, gap=1, fade=2)
    check(lib, lengths, 5, order=[int(v) for v in order], gaps=[i % 3 for i in range(299)], fade=2, ldx=7)


@pytest.mark.parametrize("gaps, gap", [(None, 0), (None, 3), ([0, 5, 0, 1, 2], 0)])
def test_pauses(lib, gaps, gap):
    check(lib, [20, 0, 17, 33, 1, 16], 33, gaps=gaps, gap=gap)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("fade", [0, 1, 8, 50, 65536])
def test_fades(lib, fade, dtype):
    """0 copies bit for bit; 50 and 65536 are larger than every segment"""
    check(lib, [20, 45, 3, 31], 45, gap=2, fade=fade, dtype=dtype, fade_ends=fade == 50)


def test_no_fade_is_a_copy(lib):
    batch_lengths = [9, 30, 12]
    out = check(lib, batch_lengths, 30, fade=0, gap=0, seed=11)
    b = Batch(batch_lengths, 30, seed=11)
    _same_bits(out[:51], np.concatenate([r[:ln] for r, ln in zip(b.rows, batch_lengths)]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_dst_base_off_by_one_element(lib, T, dtype):
    check(lib, [T + 5, 77, 2 * T], 2 * T, gap=3, dtype=dtype, ldx=2 * T + 1, shift=1)


@pytest.mark.parametrize("delta", [-100, -1, 0, 1, 50])
def test_dst_cap_either_side_of_total(lib, T, delta):
    check(lib, [T + 9, 300, 40], T + 9, gap=7, cap_delta=delta)


def test_dst_cap_inside_the_first_segment(lib):
    check(lib, [50, 20], 50, gap=4, cap_delta=-(74 - 10))


def test_out_of_range_lengths_act_as_0_and_N(lib):
    N = 40
    a = check(lib, [-5, N + 7, 13], N, gap=2)
    b = check(lib, [0, N, 13], N, gap=2)
    _same_bits(a, b)


def test_two_batches_with_interleaved_positions(lib, T):
    """Segments 0, 2, 4 come from a batch of N = T + 7, segments 1, 3 from an f16 batch of N = 90: two gather calls into one dst,
    in either order of the calls.  Each batch also has a row that is not part of the join (pos = -1, pos = n): it writes nothing."""
    la, lb = [T + 7, 13, 0, 31], [90, 55, 2 * F - 1]
    A = Batch(la, T + 7, torch.float32, ldx=T + 8, seed=1)
    Bb = Batch(lb, 90, torch.float16, ldx=91, seed=2)
    n = 5
    rows = [A.rows[0], Bb.rows[0], A.rows[1], Bb.rows[2], A.rows[2]]
    lengths, caps = [la[0], lb[0], la[1], lb[2], la[2]], [T + 7, 90, T + 7, 90, T + 7]
    gaps = [3, 0, 4, 1]
    total = sum(lengths) + sum(gaps)
    dst_cap = total + 11
    want, want_len, want_off = J.join(rows, lengths, gaps=gaps, fade=F, dst_cap=dst_cap)
    calls = [(A, [0, 2, 4, -1]), (Bb, [1, n, 3])]
    for these in (calls, calls[::-1]):
        dst = Buf(dst_cap, torch.float32, NAN)
        off, length = scan(lib, lengths, caps, None, gaps, 0, dst, dst_cap)
        for batch, pos in these:
            gather(lib, batch, pos, off, n, F, False, dst, dst_cap)
        assert dst.guards_intact() and length == want_len == total
        assert off.t.cpu().tolist() == want_off.tolist()
        _same_bits(dst.t.cpu().numpy(), want)


def test_two_batches_equal_the_one_batch_join(lib, T):
    """The same five segments once as rows of one batch and once split over two batches of different N, interleaved."""
    lengths = [T + 3, 50, 17, 64, 2]
    N1 = T + 3
    one = Batch(lengths, N1, seed=9)
    dst_cap = sum(lengths) + 4 * 6 + 5
    d1 = Buf(dst_cap, torch.float32, NAN)
    off1, len1 = scan(lib, lengths, [N1] * 5, None, None, 6, d1, dst_cap)
    gather(lib, one, [0, 1, 2, 3, 4], off1, 5, F, False, d1, dst_cap)
    # rows 0, 2, 4 in a batch of N = T + 3, rows 1, 3 in a batch of N = 64
    A = Batch([lengths[0], lengths[2], lengths[4]], N1, ldx=N1 + 2, seed=9)
    Bb = Batch([lengths[1], lengths[3]], 64, ldx=67, seed=9)
    for b, src in ((A, (0, 2, 4)), (Bb, (1, 3))):               # the same samples as the one-batch rows
        for k, r in enumerate(src):
            ln = lengths[r]
            b.buf.t[k * b.ldx:k * b.ldx + ln].copy_(torch.from_numpy(one.rows[r][:ln].copy()))
    d2 = Buf(dst_cap, torch.float32, NAN)
    # rows are numbered through the batches: A's 0, 1, 2 then B's 3, 4; position -> row
    off2, len2 = scan(lib, A.lengths + Bb.lengths, [N1] * 3 + [64] * 2, [0, 3, 1, 4, 2], None, 6, d2, dst_cap)
    gather(lib, Bb, [1, 3], off2, 5, F, False, d2, dst_cap)
    gather(lib, A, [0, 2, 4], off2, 5, F, False, d2, dst_cap)
    assert d1.guards_intact() and d2.guards_intact()
    assert len1 == len2 and off1.t.cpu().tolist() == off2.t.cpu().tolist()
    _same_bits(d2.t.cpu().numpy(), d1.t.cpu().numpy())
    assert not np.isnan(d1.t.cpu().numpy()).any()


def test_row_outside_the_join_writes_nothing(lib):
    batch = Batch([10, 20, 30], 30)
    dst = Buf(100, torch.float32, NAN)
    off = Buf(4, torch.int64, -99)
    off.t.copy_(torch.tensor([0, 10, 30, 60], dtype=torch.int64))
    gather(lib, batch, [-1, 3, 65535], off, 3, F, False, dst, 100)
    assert dst.guards_intact() and bool(dst.t.isnan().all())


def test_wild_offsets_stay_inside_dst(lib):
    """the gather trusts no offset: one far below 0 and one far beyond dst_cap write nothing outside [0, dst_cap)"""
    batch = Batch([10, 20, 30], 30)
    dst = Buf(25, torch.float32, NAN)
    off = Buf(4, torch.int64, -99)
    off.t.copy_(torch.tensor([-5, 2 ** 40, 20, 0], dtype=torch.int64))
    gather(lib, batch, [0, 1, 2], off, 3, 0, False, dst, 25)
    assert dst.guards_intact()
    got = dst.t.cpu().numpy()
    _same_bits(got[:5], batch.rows[0][5:10])
    assert np.isnan(got[5:20]).all()
    _same_bits(got[20:25], batch.rows[2][:5])


def test_invalid_arguments_launch_nothing(lib):
    batch = Batch([10, 20], 20)
    dst = Buf(64, torch.float32, NAN)
    lens, caps, off, length, pos = _ints([10, 20]), _ints([20, 20]), Buf(3, torch.int64, -99), Buf(1, torch.int32, -77), _ints([0, 1])
    p = lambda b: b.t.data_ptr()                                # noqa: E731
    ok_o = dict(lengths=p(lens), row_caps=p(caps), order=None, gaps=None, gap=0, n=2, dst=p(dst), dst_cap=64, offsets=p(off),
                length=p(length))
    ok_g = dict(src=p(batch.buf), src_kind=1, B=2, N=20, ldx=20, lengths=p(lens), pos=p(pos), offsets=p(off), n=2, fade=4,
                fade_ends=0, dst=p(dst), dst_cap=64)
    bad_o = [dict(lengths=None), dict(row_caps=None), dict(dst=None), dict(offsets=None), dict(length=None), dict(n=0), dict(n=-1),
             dict(n=65536), dict(dst_cap=0), dict(dst_cap=-3), dict(dst_cap=2 ** 31), dict(gap=-1), dict(offsets=p(off) + 4)]
    bad_g = [dict(src=None), dict(lengths=None), dict(pos=None), dict(offsets=None), dict(dst=None), dict(src_kind=0),
             dict(src_kind=3), dict(B=0), dict(B=65536), dict(N=0), dict(N=-2), dict(ldx=19), dict(n=0), dict(n=65536),
             dict(fade=-1), dict(fade=65537), dict(dst_cap=0), dict(dst_cap=2 ** 31), dict(offsets=p(off) + 4),
             dict(dst=p(batch.buf) + 8), dict(src=p(dst) + 16)]          # the last two: src overlapping dst
    for ch in bad_o:
        a = dict(ok_o, **ch)
        rc = lib.t2s_join_offsets(a["lengths"], a["row_caps"], a["order"], a["gaps"], a["gap"], a["n"], a["dst"], a["dst_cap"],
                                  a["offsets"], a["length"], _st())
        assert rc == -1, "t2s_join_offsets accepted %r" % (ch,)
    for ch in bad_g:
        a = dict(ok_g, **ch)
        rc = lib.t2s_join_gather(a["src"], a["src_kind"], a["B"], a["N"], a["ldx"], a["lengths"], a["pos"], a["offsets"], a["n"],
                                 a["fade"], a["fade_ends"], a["dst"], a["dst_cap"], _st())
        assert rc == -1, "t2s_join_gather accepted %r" % (ch,)
    torch.cuda.synchronize()
    assert bool(dst.raw.isnan().all()), "a refused call wrote to dst"
    assert bool((off.raw == -99).all()) and bool((length.raw == -77).all())
    assert batch.buf.guards_intact()
