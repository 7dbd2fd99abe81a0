"""t2s_resample_window / t2s_limit_window / t2s_g711 (csrc/delivery.hip) called directly on guarded buffers.  The window entry points
are held to their whole-row partners - t2s_resample_batch, t2s_limit_measure + t2s_limit_apply, whose own tests hold them to the
float64 restatements - BIT FOR BIT: the windows of a stream, concatenated, are the partner's row, and the stream's final state is
the measure's stats and counts.  G.711 is compared with tests/delivery_ref.py (which the CPU tests compare with audioop) over all
65 536 codes.

Every piece is a view into a larger tensor of NaN and 1e4 with odd strides between its rows; a new stream's carries hold NaN;
every output, carry and state is a view into sentinels which must come back untouched around what the call owns."""
import numpy as np
import pytest
import torch

import delivery_ref as D
import limiter_ref as LR
import resample_ref as RR
from text2speech_amd import _lib, audio
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
C = LR.ceiling(LR.CEILING_DB)
HW = D.HALF_WIDTH
TILE = D.TILE
N_ROW = 3 * TILE + 40
OUT_FILL, STATE_FILL = 12345.678, -99
ONE_BITS = 0x3FF0000000000000


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.t2s_limit_tile() == TILE == lib.t2s_resample_tile() and lib.t2s_abi_version() == 4
    return lib


class Buf:
    """A device tensor of n elements inside a larger one: GUARD elements of `fill` in front and behind (float fills alternate with
    NaN: whatever reads a guard shows)"""

    def __init__(self, n, dtype, fill, nan=False):
        self.raw = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        if nan:
            self.raw[::2] = float("nan")
        self.before = self.raw.clone()
        self.t = self.raw[GUARD:GUARD + n]
        self.n = n

    def guards_intact(self):
        a, b = self.raw.view(torch.uint8), self.before.view(torch.uint8)
        k = GUARD * self.raw.element_size()
        return bool((a[:k] == b[:k]).all()) and bool((a[a.numel() - k:] == b[b.numel() - k:]).all())

    def untouched(self):
        return bool((self.raw.view(torch.uint8) == self.before.view(torch.uint8)).all())


def _rows_buf(rows, dtype, pad):
    """rows np [B, n] -> (Buf holding them `ld` = n + pad apart, ld); NaN / 1e4 between the rows and behind every end"""
    B, n = rows.shape
    ld = n + pad
    b = Buf(max(1, B * ld), dtype, 1e4, nan=True)
    if n:
        b.t[:B * ld].view(B, ld)[:, :n].copy_(torch.from_numpy(rows))
        b.before = b.raw.clone()
    return b, ld


def _gains(g, B):
    if g is None:
        return None
    b = Buf(B, torch.float64, float("inf"))
    b.t.copy_(torch.tensor([g * (1 + 0.25 * r) for r in range(B)], dtype=torch.float64))
    b.before = b.raw.clone()
    return b


_TABLES = {}


def _lim_tables(os, L):
    if (os, L) not in _TABLES:
        h, w = audio.resample_filter(1, os, HW, 5.0)[2], audio.limiter_window(L)
        _TABLES[(os, L)] = (torch.from_numpy(h).to(DEV), torch.from_numpy(w).to(DEV))
    return _TABLES[(os, L)]


def _rs_filter(up, down):
    key = ("rs", up, down)
    if key not in _TABLES:
        u, d, h = audio.resample_filter(down, up)
        assert (u, d) == (up, down)
        _TABLES[key] = torch.from_numpy(h).to(DEV)
    return _TABLES[key]


class Stream:
    """the host side of one stage's stream: the two carries, the positions, the state"""

    def __init__(self, lib, B, Cn, state=False):
        self.lib, self.B, self.C = lib, B, Cn
        self.carry = [Buf(B * Cn, torch.float32, 1e4, nan=True), Buf(B * Cn, torch.float32, 1e4, nan=True)]
        self.i = 0
        self.pos = self.out = 0
        self.state = None
        if state:
            self.state = Buf(5 * B, torch.int64, STATE_FILL)
            self.state.t.view(B, 5).copy_(torch.tensor([0, 0, ONE_BITS, 0, 0], dtype=torch.int64))

    def window(self, piece, dtype, final, call, end):
        """piece np [B, n] -> np [B, m]"""
        B, n = piece.shape
        src, ldp = _rows_buf(piece, dtype, 3 if n % 2 == 0 else 2)
        m = end(self.pos + n, self.out, final) - self.out
        ldo = m + 1
        dst = Buf(max(1, B * ldo), torch.float32, OUT_FILL)
        cin, cout = self.carry[self.i], self.carry[1 - self.i]
        cin.before = cin.raw.clone()
        rc = call(cin.t.data_ptr(), cout.t.data_ptr(), src.t.data_ptr() if n else None, int(dtype == torch.float16), B, n, ldp, self.pos,
                  self.out, int(final), dst.t.data_ptr() if m else None, m, ldo)
        assert rc == 0
        torch.cuda.synchronize()
        assert src.untouched() and cin.untouched(), "an input was written"
        assert dst.guards_intact() and cout.guards_intact() and (self.state is None or self.state.guards_intact())
        got = dst.t[:B * ldo].view(B, ldo).cpu().numpy()
        assert (got[:, m:] == np.float32(OUT_FILL)).all(), "wrote behind a row's outputs"
        # the next carry: the last C samples of carry | piece (where those exist: a position below 0 may hold anything)
        have = min(self.C, self.pos + n)
        if have:
            both = np.concatenate([cin.t.view(B, self.C).cpu().numpy(), piece.astype(np.float32)], axis=1)
            assert cout.t.view(B, self.C).cpu().numpy()[:, self.C - have:].tobytes() == both[:, both.shape[1] - have:].tobytes()
        self.i = 1 - self.i
        self.pos += n
        self.out += m
        return got[:, :m].copy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the resampler ---------------------------------------------------------------------------------------------------------------------
def _resample_whole(lib, rows, dtype, up, down):
    B, n = rows.shape
    src, ldx = _rows_buf(rows, dtype, 1)
    h = _rs_filter(up, down)
    n_out = RR.out_length(n, up, down)
    dst = Buf(B * n_out, torch.float32, OUT_FILL)
    assert lib.t2s_resample_batch(src.t.data_ptr(), int(dtype == torch.float16), B, n, ldx, None, h.data_ptr(), h.numel(), up, down,
                                  dst.t.data_ptr(), n_out, n_out, None, _st()) == 0
    torch.cuda.synchronize()
    assert dst.guards_intact()
    return dst.t.view(B, n_out).cpu().numpy()


def _resample_cuts(n, up, down, n_taps, Cn):
    """source piece lengths: the outputs delivered so far reach 1023, 1024 and 1025 (a window ends at, and either side of, the tile),
    pieces shorter than the carry, of one sample and of none, and the rest"""
    marks = []
    for target in (TILE - 1, TILE, TILE + 1):
        K = 0
        while D.resample_end(K, 0, n_taps, up, down, False) < target:
            K += 1
        marks.append(K)
    cuts, pos = [], 0
    for K in marks + [marks[-1] + 1, marks[-1] + 1, marks[-1] + Cn, marks[-1] + 2 * Cn + 1]:
        K = min(K, n)
        cuts.append(K - pos)
        pos = K
    return cuts + [n - pos]


@pytest.mark.parametrize("kind", ("float32", "float16"))
@pytest.mark.parametrize("ratio", D.RATIOS)
def test_resample_windows_are_the_whole_row(lib, ratio, kind):
    up, down = ratio
    dtype = torch.float32 if kind == "float32" else torch.float16
    h = _rs_filter(up, down)
    n_taps = h.numel()
    Cn = lib.t2s_resample_window_carry(n_taps, up)
    assert Cn == D.resample_carry(n_taps, up)
    n = D.n_in_for(N_ROW, up, down)
    cuts = _resample_cuts(n, up, down, n_taps, Cn)
    assert sum(cuts) == n and min(cuts) == 0 and 1 in cuts

    def call(cin, cout, piece, is_half, B_, n_, ldp, K0, M0, final, out, cap, ldo):
        return lib.t2s_resample_window(cin, cout, piece, is_half, B_, n_, ldp, K0, M0, final, h.data_ptr(), n_taps, up, down, out, cap, ldo,
                                       _st())

    def end(K1, M0, final):
        M1 = lib.t2s_resample_window_end(K1, M0, n_taps, up, down, int(final))
        assert M1 == D.resample_end(K1, M0, n_taps, up, down, final)
        return M1

    def stream(rows, flush):
        s = Stream(lib, rows.shape[0], Cn)
        pieces = cuts + [0] if flush else cuts
        outs, pos = [], 0
        for q, c in enumerate(pieces):
            outs.append(s.window(rows[:, pos:pos + c], dtype, q == len(pieces) - 1, call, end))
            pos += c
        return np.concatenate(outs, axis=1)

    for B, flush in ((1, True), (3, False)):
        rows = np.stack([D.row(n, 100 * up + down + b, kind, level=0.3) for b in range(B)])
        whole = _resample_whole(lib, rows, dtype, up, down)
        assert whole.shape[1] >= N_ROW and _same(stream(rows, flush), whole)
        if B == 3:      # a row at any place of the batch gives the bits it gives alone
            assert _same(stream(rows[2:3], True), whole[2:3])


# ---- the limiter -----------------------------------------------------------------------------------------------------------------------
def _limit_whole(lib, rows, dtype, os, L, gains):
    """t2s_limit_measure + t2s_limit_apply over the rows -> (out [B, n], stats [B, 4], counts [B, 2])"""
    B, n = rows.shape
    src, ldx = _rows_buf(rows, dtype, 1)
    h, w = _lim_tables(os, L)
    table2 = torch.tensor([(b * ldx, n) for b in range(B)], dtype=torch.int64, device=DEV)
    table4 = torch.tensor([(b * ldx, n, b * n, n) for b in range(B)], dtype=torch.int64, device=DEV)
    need = lib.t2s_limit_scratch(B, n)
    scratch = torch.empty(need, dtype=torch.float64, device=DEV)
    stats, counts = torch.empty(B, 4, dtype=torch.float64, device=DEV), torch.empty(B, 2, dtype=torch.int32, device=DEV)
    dst = Buf(B * n, torch.float32, OUT_FILL)
    kind = 2 if dtype == torch.float16 else 1
    g = gains.t.data_ptr() if gains else None
    assert lib.t2s_limit_measure(src.t.data_ptr(), kind, src.t.numel(), table2.data_ptr(), B, n, g, h.data_ptr(), h.numel(), os, HW,
                                 w.data_ptr(), L, C, scratch.data_ptr(), need, stats.data_ptr(), counts.data_ptr(), _st()) == 0
    assert lib.t2s_limit_apply(src.t.data_ptr(), kind, src.t.numel(), table4.data_ptr(), B, g, h.data_ptr(), h.numel(), os, HW,
                               w.data_ptr(), L, C, counts.data_ptr(), dst.t.data_ptr(), 1, B * n, n, None, _st()) == 0
    torch.cuda.synchronize()
    assert dst.guards_intact()
    return dst.t.view(B, n).cpu().numpy(), stats.cpu().numpy(), counts.cpu().numpy()


def _limit_stream(lib, rows, dtype, os, L, gains, cuts):
    B = rows.shape[0]
    h, w = _lim_tables(os, L)
    Cn = lib.t2s_limit_window_carry(L, HW)
    assert Cn == D.limit_carry(L)
    s = Stream(lib, B, Cn, state=True)
    g = gains.t.data_ptr() if gains else None

    def call(cin, cout, piece, is_half, B_, n_, ldp, N0, O0, final, out, cap, ldo):
        return lib.t2s_limit_window(cin, cout, piece, is_half, B_, n_, ldp, N0, O0, final, g, h.data_ptr(), h.numel(), os, HW, w.data_ptr(),
                                    L, C, out, cap, ldo, s.state.t.data_ptr(), _st())

    def end(N1, O0, final):
        O1 = lib.t2s_limit_window_end(N1, O0, L, HW, int(final))
        assert O1 == D.limit_end(N1, O0, L, HW, final)
        return O1

    outs, pos = [], 0
    for q, c in enumerate(cuts):
        outs.append(s.window(rows[:, pos:pos + c], dtype, q == len(cuts) - 1, call, end))
        pos += c
    assert pos == rows.shape[1]
    if gains:
        assert gains.untouched()
    st = s.state.t.view(B, 5).cpu()
    return np.concatenate(outs, axis=1), st[:, :4].contiguous().view(torch.float64).numpy(), st[:, 4:].contiguous().view(torch.int32).numpy()


def _limit_cuts(n, L, flush):
    """windows that end at, and either side of, the tile (what is delivered trails what was seen by the reach); pieces of one
    sample, of none and shorter than the carry; the rest; with flush an empty last piece"""
    reach = D.limit_reach(L)
    marks = sorted({m for m in (reach + TILE - 1, reach + TILE, reach + TILE + 1, reach + TILE + 6, 2 * TILE + 3, 2 * TILE + reach) if m < n})
    cuts, pos = [], 0
    for m in marks:
        cuts.append(m - pos)
        pos = m
    cuts.insert(2, 0)
    cuts.append(n - pos)
    return cuts + [0] if flush else cuts


@pytest.mark.parametrize("kind", ("float32", "float16"))
@pytest.mark.parametrize("L,os", D.LIMITERS + ((1024, 4),))
def test_limit_windows_are_the_whole_row(lib, L, os, kind):
    dtype = torch.float32 if kind == "float32" else torch.float16
    n = N_ROW
    for B, g, flush in ((1, None, True), (3, 1.0, False), (3, 3.0, True)):
        cuts = _limit_cuts(n, L, flush)
        assert sum(cuts) == n
        rows = np.stack([D.row(n, 1000 * L + 10 * os + b, kind, peaks=D.peaks_at(n, cuts, L)) for b in range(B)])
        gains = _gains(g, B)
        whole, stats, counts = _limit_whole(lib, rows, dtype, os, L, gains)
        got, st, ct = _limit_stream(lib, rows, dtype, os, L, gains, cuts)
        assert _same(got, whole)
        assert _same(st, stats) and _same(ct, counts), (st, stats, ct, counts)
        assert (counts[:, 0] > 0).all() and (counts[:, 1] == 1).all(), "every row was limited"
        assert np.abs(got).max() <= np.float32(C)
        if B == 3:
            one, st1, ct1 = _limit_stream(lib, rows[1:2], dtype, os, L, None if g is None else _gains_row(g, 1), cuts)
            assert _same(one, whole[1:2]) and _same(st1, stats[1:2]) and _same(ct1, counts[1:2])


def _gains_row(g, r):
    b = Buf(1, torch.float64, float("inf"))
    b.t.fill_(g * (1 + 0.25 * r))
    b.before = b.raw.clone()
    return b


def test_pieces_of_one_sample_and_of_none(lib):
    L, os, n = 16, 4, 200
    rows = D.row(n, 5, peaks=(0, 50, 51, 120, 199))[None]
    whole, stats, counts = _limit_whole(lib, rows, torch.float32, os, L, None)
    cuts = [1, 0, 0, 1] + [1] * 60 + [0, 83, 1, 0] + [n - 146]
    got, st, ct = _limit_stream(lib, rows, torch.float32, os, L, None, cuts + [0])
    assert _same(got, whole) and _same(st, stats) and _same(ct, counts) and counts[0, 0] > 0


def test_a_sample_that_is_not_finite_mutes_the_stream(lib):
    L, os, n = 16, 4, TILE + 300
    reach = D.limit_reach(L)
    x = D.row(n, 9, peaks=(100, 500, TILE + 5))
    bad = (300, TILE - 1, TILE + 200)
    clean = x.copy()
    clean[list(bad)] = 0
    x[300], x[TILE - 1], x[TILE + 200] = np.nan, np.inf, -np.inf
    cuts = [250, 60, 800, n - 1110]
    got, st, ct = _limit_stream(lib, x[None], torch.float32, os, L, None, cuts)
    ref, _, _ = _limit_whole(lib, clean[None], torch.float32, os, L, None)
    state = D.new_state()
    outs, lc, N, O = [], np.zeros(D.limit_carry(L), np.float32), 0, 0
    for q, c in enumerate(cuts):
        o, lc = D.limit_window(lc, x[N:N + c], N, O, q == len(cuts) - 1, C, L, os, state)
        outs.append(o)
        N, O = N + c, O + o.size
    restated = np.concatenate(outs)
    assert np.isfinite(got).all() and np.abs(got).max() <= np.float32(C)
    assert ct[0, 1] & audio.LIMIT_FLAG_NONFINITE and ct[0, 1] == state["flags"] and st[0, 0] == np.inf and st[0, 1] == np.inf and st[0, 2] == 0.0
    assert all(got[0, b] == 0 and not np.signbit(got[0, b]) for b in bad)
    assert (got[0] == 0).tolist() == (restated == 0).tolist(), "muted where the restatement mutes"
    far = np.ones(n, bool)
    for b in bad:
        far[max(0, b - reach):b + reach + 1] = False
    assert _same(got[0][far], ref[0][far]), "beyond the reach of what is not finite the stream is the whole row's"
    assert np.abs(got[0].astype(np.float64) - restated).max() <= 2.0 ** -22


# ---- G.711 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", (0, 1))
def test_g711_over_every_code(lib, law):
    codes = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    src = Buf(codes.size + 1, torch.int16, 32767)
    src.t[1:].copy_(torch.from_numpy(codes))                    # (an odd element offset: no alignment beyond the element)
    dst = Buf(codes.size, torch.uint8, 0xAB)
    assert lib.t2s_g711(src.t[1:].data_ptr(), codes.size, law, dst.t.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert dst.guards_intact()
    assert _same(dst.t.cpu().numpy(), (D.alaw if law else D.ulaw)(codes))
    short = Buf(7, torch.uint8, 0xAB)
    assert lib.t2s_g711(src.t[1:].data_ptr(), 5, law, short.t.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert short.guards_intact() and short.t[5:].tolist() == [0xAB, 0xAB]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(lib):
    L, os, up, down = 16, 4, 5, 14
    B, n = 2, 300
    h, w = _lim_tables(os, L)
    hr = _rs_filter(up, down)
    Cr, Cl = lib.t2s_resample_window_carry(hr.numel(), up), lib.t2s_limit_window_carry(L, HW)
    piece, ldp = _rows_buf(np.stack([D.row(n, 1), D.row(n, 2)]), torch.float32, 3)
    cin, cout = Buf(B * Cl, torch.float32, 1e4, nan=True), Buf(B * Cl, torch.float32, 1e4, nan=True)
    out = Buf(B * 400, torch.float32, OUT_FILL)
    state = Buf(5 * B, torch.int64, STATE_FILL)

    def rs(carry_in=cin.t.data_ptr(), carry_out=cout.t.data_ptr(), p=piece.t.data_ptr(), B_=B, n_=n, ld=ldp, K0=0, M0=0, final=0,
           hp=hr.data_ptr(), n_taps=hr.numel(), u=up, d=down, o=out.t.data_ptr(), cap=400, ldo=400):
        return lib.t2s_resample_window(carry_in, carry_out, p, 0, B_, n_, ld, K0, M0, final, hp, n_taps, u, d, o, cap, ldo, _st())

    def lm(carry_in=cin.t.data_ptr(), carry_out=cout.t.data_ptr(), p=piece.t.data_ptr(), B_=B, n_=n, ld=ldp, N0=0, O0=0, final=0,
           hp=h.data_ptr(), n_taps=h.numel(), os_=os, hw=HW, wp=w.data_ptr(), L_=L, c=C, o=out.t.data_ptr(), cap=400, ldo=400,
           st=state.t.data_ptr()):
        return lib.t2s_limit_window(carry_in, carry_out, p, 0, B_, n_, ld, N0, O0, final, None, hp, n_taps, os_, hw, wp, L_, c, o, cap, ldo,
                                    st, _st())

    refused = [rs(carry_in=None), rs(carry_out=None), rs(p=None), rs(hp=None), rs(o=None), rs(carry_out=cin.t.data_ptr()),
               rs(carry_out=cin.t.data_ptr() + 4 * (B * Cr - 1)), rs(B_=0), rs(B_=65536), rs(n_=-1), rs(ld=n - 1), rs(K0=-1), rs(M0=-1),
               rs(u=0), rs(d=0), rs(u=10, d=28), rs(u=513, d=1), rs(n_taps=hr.numel() - 1), rs(n_taps=1), rs(hp=hr.data_ptr() + 4),
               rs(cap=10), rs(ldo=10), rs(final=1, cap=107), rs(M0=2 ** 41), rs(K0=2 ** 40),
               lm(carry_in=None), lm(carry_out=None), lm(p=None), lm(hp=None), lm(wp=None), lm(st=None), lm(o=None),
               lm(carry_out=cin.t.data_ptr() + 4), lm(B_=0), lm(B_=-3), lm(n_=-1), lm(ld=n - 1), lm(N0=-1), lm(O0=-1), lm(O0=n + 1),
               lm(os_=3), lm(os_=2), lm(hw=0), lm(hw=33), lm(n_taps=h.numel() + 2), lm(L_=-1), lm(L_=1025), lm(c=0.0), lm(c=-1.0),
               lm(c=float("nan")), lm(c=float("inf")), lm(c=0.1), lm(cap=n - D.limit_reach(L) - 1), lm(ldo=5), lm(final=1, cap=n - 1),
               lm(wp=w.data_ptr() + 4), lm(st=state.t.data_ptr() + 4),
               lib.t2s_g711(None, 5, 0, out.t.data_ptr(), _st()), lib.t2s_g711(piece.t.data_ptr(), 5, 0, None, _st()),
               lib.t2s_g711(piece.t.data_ptr(), 0, 0, out.t.data_ptr(), _st()), lib.t2s_g711(piece.t.data_ptr(), 5, 2, out.t.data_ptr(), _st()),
               lib.t2s_g711(piece.t.data_ptr() + 1, 5, 1, out.t.data_ptr(), _st())]
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in refused), refused
    for b in (piece, cin, cout, out, state):
        assert b.untouched()
    # ... and the same buffers accepted: the refusals above were about the one argument each
    assert rs() == 0 and lm() == 0
    torch.cuda.synchronize()
    assert not out.untouched() and out.guards_intact() and cout.guards_intact() and state.guards_intact()


def test_two_identical_streams_give_identical_bits(lib):
    L, os = 67, 4
    rows = np.stack([D.row(N_ROW, 40 + b, peaks=(5, 900, 1024, 2500)) for b in range(3)])
    cuts = _limit_cuts(N_ROW, L, True)
    g = _gains(3.0, 3)
    a = _limit_stream(lib, rows, torch.float32, os, L, g, cuts)
    b = _limit_stream(lib, rows, torch.float32, os, L, g, cuts)
    assert all(_same(p, q) for p, q in zip(a, b))


# ---- positions past 2^31 ------------------------------------------------------------------------------------------------------------------
def test_a_window_far_into_a_stream_gives_the_bits_it_gives_near_its_start(lib):
    """Both stages are shift-invariant once the row's start is out of reach, so the second window of a stream, called again with its
    positions moved up by 2^33 samples (the resampler: by a whole number of filter periods), must give the same bits: the index
    arithmetic holds past 2^31"""
    L, os, up, down = 67, 4, 5, 14
    h, w = _lim_tables(os, L)
    hr = _rs_filter(up, down)
    rows = np.stack([D.row(2 * TILE + 900, 60 + b, peaks=(700, 1500, 2047, 2048, 2500)) for b in range(2)])
    p1, p2 = rows[:, :1100], rows[:, 1100:]
    state = []

    def lm(cin, cout, piece, is_half, B_, n_, ldp, N0, O0, final, out, cap, ldo):
        return lib.t2s_limit_window(cin, cout, piece, is_half, B_, n_, ldp, N0, O0, final, None, h.data_ptr(), h.numel(), os, HW, w.data_ptr(),
                                    L, C, out, cap, ldo, state[-1].state.t.data_ptr(), _st())

    def rs(cin, cout, piece, is_half, B_, n_, ldp, K0, M0, final, out, cap, ldo):
        return lib.t2s_resample_window(cin, cout, piece, is_half, B_, n_, ldp, K0, M0, final, hr.data_ptr(), hr.numel(), up, down, out, cap,
                                       ldo, _st())
    stages = ((lm, lambda N1, O0, f: lib.t2s_limit_window_end(N1, O0, L, HW, int(f)), lib.t2s_limit_window_carry(L, HW), True, 2 ** 33, 2 ** 33),
              (rs, lambda K1, M0, f: lib.t2s_resample_window_end(K1, M0, hr.numel(), up, down, int(f)),
               lib.t2s_resample_window_carry(hr.numel(), up), False, down * 2 ** 31, up * 2 ** 31))
    for call, end, Cn, has_state, shift_in, shift_out in stages:
        got = []
        for shift in (False, True):
            s = Stream(lib, 2, Cn, state=has_state)
            state.append(s)
            s.window(p1, torch.float32, False, call, end)
            if shift:
                s.pos, s.out = s.pos + shift_in, s.out + shift_out
            got.append(s.window(p2, torch.float32, False, call, end))
            if has_state:
                got.append(s.state.t.cpu().numpy().copy())
        assert got[0].shape[1] > (TILE if has_state else 600) and all(_same(a, b) for a, b in zip(got[:len(got) // 2], got[len(got) // 2:]))
