"""t2s_warp_map / t2s_warp_gather / t2s_warp_spans (csrc/warp.hip, csrc/t2s_api_warp.hip) called directly on guarded, pattern-filled
buffers, against tests/warp_ref.py (pinned by tests/test_warp_ref_cpu.py).

Integers - the cumulative map, the warped lengths, first / last, the spans - must EQUAL the restatement: the map is exact, there is no
near-tie set to exclude.  A mel value must lie within correct rounding of the restatement's float64 value plus the contraction of
the one double expression: 2^-24 |ref| + 2^-40 (|x[f]| + |x[f+1]|) for float32, 2^-11 |ref| plus the same small term for float16.
That bound is relative, i.e. what correct rounding gives for results that are normal numbers of the type; the float16 mels here keep
one sign per channel and magnitudes in [0.25, 11.5] (log-mel's range), so that no interpolated value is a float16 subnormal.  Behind
every length the mels hold NaN and 1e4, which must never reach an output; every output buffer is pre-filled and guarded.

Sizes: the map walks frames in steps of t2s_warp_block() = 256 and the gather's tile is 256 output frames x 16 channels, so F runs
over 1, 2, 255, 256, 257, 1000 and C over 1, 17, 80; B <= 3, ragged, with an empty entry; T_in 1, 40, 65."""
import numpy as np
import pytest
import torch

import warp_ref as W
from text2speech_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
Q = W.Q
KIND = {torch.float32: 1, torch.float16: 2}
NP_OF = {torch.float32: np.float32, torch.float16: np.float16}
REL = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11}
NAN = float("nan")
WORST = {}                                          # dtype -> the worst observed fraction of the bound (printed)


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.t2s_warp_block() == 256
    return lib


def _st():
    return _lib.current_stream()


class Buf:
    """A device tensor of n elements inside a larger one: GUARD elements of `fill` in front and behind."""

    def __init__(self, n, dtype, fill, host=None):
        self.raw = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.raw[GUARD:GUARD + n]
        self.fill = fill
        if host is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(host)).view(dtype).reshape(-1))

    def _is_fill(self, a):
        if isinstance(self.fill, float) and self.fill != self.fill:
            return bool(a.isnan().all())
        return bool((a == self.fill).all())

    def guards_intact(self):
        return self._is_fill(self.raw[:GUARD]) and self._is_fill(self.raw[GUARD + self.t.numel():])

    def untouched(self):
        return self._is_fill(self.raw)

    def np(self, *shape):
        return self.t.cpu().numpy().reshape(shape)


def P(buf):
    return None if buf is None else buf.t.data_ptr()


def _ints(values, dtype=torch.int32, fill=-77):
    return Buf(len(values), dtype, fill, np.asarray(values, dtype=np.int64 if dtype == torch.int64 else np.int32))


class Mel:
    """B entries of C rows of F frames, ld_row / ld_entry apart, inside a guarded buffer: seeded values up to each entry's clamped
    length, NaN / 1e4 alternating behind it and between the rows"""

    def __init__(self, lengths, C, F, dtype=torch.float32, ld_row=None, ld_entry=None, seed=0):
        self.B, self.C, self.F, self.dtype = len(lengths), C, F, dtype
        self.ld_row = ld_row or F
        self.ld_entry = ld_entry or C * self.ld_row
        npt = NP_OF[dtype]
        n_el = (self.B - 1) * self.ld_entry + (C - 1) * self.ld_row + F
        host = np.empty(n_el, dtype=npt)
        host[0::2] = np.nan
        host[1::2] = 1e4
        rng = np.random.RandomState(seed)
        self.x = []
        for b, ln in enumerate(lengths):
            Fb = max(0, min(ln, F))
            if dtype == torch.float32:
                x = rng.uniform(-1, 1, (C, Fb)).astype(npt)
            else:
                x = (rng.choice([-1.0, 1.0], (C, 1)) * rng.uniform(0.25, 11.5, (C, Fb))).astype(npt)
            for c in range(C):
                at = b * self.ld_entry + c * self.ld_row
                host[at:at + Fb] = x[c]
            self.x.append(x)
        self.buf = Buf(n_el, dtype, 1e4, host)


def want_map(lengths, F, cap, stretch=Q, stretches=None, path=None, rates=None, in_len=None, T_in=0, lo=0.5, hi=2.0):
    """the restatement's (c [B, F + 1], F' [B], first_last [B, T_in, 2] or None)"""
    B = len(lengths)
    cs, ns, fls = [], [], []
    for b in range(B):
        if rates is not None:
            s = W.symbol_stretches(path[b, :F], rates[b], T_in if in_len is None else in_len[b], lo, hi)
        elif stretches is not None:
            s = min(max(int(stretches[b]), Q >> 3), Q << 3)
        else:
            s = stretch
        c, n = W.cum_map(s, F, lengths[b], cap)
        cs.append(c)
        ns.append(n)
        if path is not None:
            fls.append(W.first_last(path[b, :F], lengths[b], T_in if in_len is None else in_len[b], T_in))
    return np.stack(cs), np.array(ns), (np.stack(fls) if fls else None)


def run_map(lib, lengths, F, cap, stretch=Q, stretches=None, path=None, ld_path=None, rates=None, ld_rates=None, in_len=None, T_in=0,
            lo=0.5, hi=2.0, outputs="cnf"):
    """t2s_warp_map on guarded buffers -> (cum Buf, out_len Buf, first_last Buf or None); NaN / -1 patterns survive in the guards"""
    B = len(lengths)
    lens_d = None if lengths is None else _ints(lengths)
    s_d = None if stretches is None else _ints(stretches, torch.int64)
    path_d = rates_d = in_d = None
    if path is not None:
        ld_path = ld_path or F
        wide = np.full((B, ld_path), 2 ** 30, dtype=np.int32)
        wide[:, :F] = path[:, :F]
        path_d = Buf(B * ld_path, torch.int32, -7, wide)
    if rates is not None:
        ld_rates = ld_rates or T_in
        wide = np.full((B, ld_rates), 1e9, dtype=np.float32)
        wide[:, :T_in] = rates
        rates_d = Buf(B * ld_rates, torch.float32, 1e9, wide)
    if in_len is not None:
        in_d = _ints(in_len)
    cum = Buf(B * (F + 1), torch.int64, -99) if "c" in outputs else None
    out_len = Buf(B, torch.int32, -77) if "n" in outputs else None
    fl = Buf(B * T_in * 2, torch.int32, -55) if "f" in outputs and path is not None else None
    rc = lib.t2s_warp_map(P(lens_d), B, F, stretch, P(s_d), P(path_d), ld_path or 0, P(rates_d), ld_rates or 0, P(in_d), T_in, lo, hi,
                          cap, P(cum), P(out_len), P(fl), _st())
    assert rc == 0
    torch.cuda.synchronize()
    for b in (lens_d, s_d, path_d, rates_d, in_d, cum, out_len, fl):
        assert b is None or b.guards_intact()
    return cum, out_len, fl, lens_d, in_d


def run_gather(lib, mel, lens_d, cum, out_len, cap):
    out = Buf(mel.B * mel.C * cap, mel.dtype, NAN)
    rc = lib.t2s_warp_gather(P(mel.buf), KIND[mel.dtype], mel.B, mel.C, mel.F, mel.ld_row, mel.ld_entry, P(lens_d), P(cum), P(out_len),
                             P(out), cap, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert out.guards_intact(), "wrote outside out[B, C, cap]"
    assert mel.buf.guards_intact() and cum.guards_intact() and out_len.guards_intact()
    return out.np(mel.B, mel.C, cap)


def check_values(got, mel, c, n, lengths, cap):
    """every entry of the gather's output against the restatement: the bound on the warped frames, +0 behind them"""
    bits = np.uint32 if mel.dtype == torch.float32 else np.uint16
    for b in range(mel.B):
        Fb = max(0, min(lengths[b], mel.F))
        want, exact, small = W.warp_entry(mel.x[b], c[b], Fb, int(n[b]), cap)
        g = got[b]
        assert not g[:, n[b]:].view(bits).any(), "entry %d: not +0 behind its %d warped frames" % (b, n[b])
        if n[b] == 0:
            continue
        assert np.isfinite(g[:, :n[b]].astype(np.float64)).all(), "entry %d: the padding reached an output" % b
        err = np.abs(g[:, :n[b]].astype(np.float64) - exact)
        bound = REL[mel.dtype] * np.abs(exact) + 2.0 ** -40 * small
        assert (err <= bound).all(), "entry %d: worst error %.3g of its bound" % (b, float((err / bound).max()))
        frac = float((err / np.maximum(bound, 1e-300)).max())
        WORST[mel.dtype] = max(WORST.get(mel.dtype, 0.0), frac)
        # a frame that is copied (a = 0) is copied bit for bit
        f, a = W.coords(c[b], Fb, int(n[b]))
        copy = a == 0.0
        assert g[:, :n[b]][:, copy].tobytes() == want[:, :n[b]][:, copy].tobytes()


def check_warp(lib, lengths, C, F, dtype=torch.float32, cap=None, cap_delta=0, ld_row=None, ld_entry=None, seed=0, **how):
    """map + gather of one batch against the restatement -> (the gather's output, the mel, c, F')"""
    mel = Mel(lengths, C, F, dtype, ld_row, ld_entry, seed)
    if cap is None:
        _, need, _ = want_map(lengths, F, 2 ** 30, **{k: v for k, v in how.items() if k not in ("ld_path", "ld_rates")})
        cap = max(1, int(need.max()) + cap_delta)
    c, n, fl = want_map(lengths, F, cap, **{k: v for k, v in how.items() if k not in ("ld_path", "ld_rates")})
    cum, out_len, fl_d, lens_d, _ = run_map(lib, lengths, F, cap, **how)
    assert cum.np(len(lengths), F + 1).tolist() == c.tolist()
    assert out_len.np(len(lengths)).tolist() == n.tolist()
    if fl is not None:
        assert fl_d.np(*fl.shape).tolist() == fl.tolist()
    got = run_gather(lib, mel, lens_d, cum, out_len, cap)
    check_values(got, mel, c, n, lengths, cap)
    return got, mel, c, n


RATES = [0.5, 0.8, 1.0, 1.25, 2.0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("rate", RATES)
def test_uniform_rate_at_the_block_and_tile_edges(lib, rate, dtype):
    s = W.stretch_q(rate)
    for F, C in ((1, 80), (2, 17), (255, 80), (256, 1), (257, 80), (1000, 80)):
        lengths = [F, 0, max(1, F // 3)]
        got, mel, c, n = check_warp(lib, lengths, C, F, dtype, stretch=s, seed=F)
        assert n.tolist() == [W.warped_length(ln, rate) for ln in lengths]
        if rate == 1.0:                                         # the identity, bit for bit
            for b, ln in enumerate(lengths):
                assert got[b, :, :ln].tobytes() == mel.x[b].tobytes()
    print("warp kernels %s rate %.2f: worst fraction of the bound so far %.4f" % (dtype, rate, WORST.get(dtype, 0.0)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_one_stretch_per_entry_and_wild_values(lib, dtype):
    """entry stretches from device memory: a mix of rates, and values outside [Q / 8, 8 Q] that the kernel clamps"""
    F = 257
    check_warp(lib, [257, 100, 31], 80, F, dtype, stretches=[W.stretch_q(0.5), W.stretch_q(1.25), W.stretch_q(2.0)])
    check_warp(lib, [40, 257, 0], 17, F, dtype, stretches=[0, -5, 1 << 40])
    check_warp(lib, [40, 257, 3], 17, F, dtype, stretches=[1 << 62, Q + 1, -(1 << 62)])


def _path(rng, B, F, lengths, in_len, T_in, wild=True):
    """a mostly monotone path per entry with revisits, and - with `wild` - values -1, S_b, T_in and 2^31 - 1 sprinkled in"""
    path = np.zeros((B, F), dtype=np.int32)
    for b in range(B):
        S = min(max(in_len[b], 1), T_in)
        steps = rng.choice([0, 0, 1, 1, 2, -1], F)
        p = np.clip(np.cumsum(steps), 0, S - 1)
        if wild and F > 4:
            at = rng.choice(F, max(1, F // 10), replace=False)
            p[at] = rng.choice([-1, S, T_in, 2 ** 31 - 1, -2 ** 31], at.size)
        path[b] = p
    return path


def _table(rng, B, T_in):
    t = rng.uniform(0.3, 3.0, (B, T_in)).astype(np.float32)
    wild = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 1e-30, 1e30, 0.25, 4.0, 0.5, 2.0, 1.0], dtype=np.float32)
    at = rng.choice(B * T_in, min(B * T_in, max(1, B * T_in // 3)), replace=False)
    t.reshape(-1)[at] = rng.choice(wild, at.size)
    return t


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("T_in", [1, 40, 65])
def test_per_symbol_tables(lib, T_in, dtype):
    rng = np.random.RandomState(T_in)
    for F, lengths, in_len in ((257, [257, 0, 90], [T_in, T_in, max(1, T_in // 2)]), (1000, [1000, 513, 1], [T_in + 9, -4, T_in]),
                               (2, [2, 1, 5], [T_in, 1, 0])):
        path = _path(rng, 3, F, lengths, in_len, T_in)
        rates = _table(rng, 3, T_in)
        check_warp(lib, lengths, 17, F, dtype, path=path, rates=rates, in_len=in_len, T_in=T_in, seed=F)
        check_warp(lib, lengths, 1, F, dtype, path=path, rates=rates, in_len=None, T_in=T_in, lo=0.125, hi=8.0, seed=F)
        check_warp(lib, lengths, 1, F, dtype, path=path, rates=rates, in_len=in_len, T_in=T_in, lo=1.25, hi=1.25, seed=F)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_an_entry_has_the_same_bits_alone_and_anywhere_in_a_batch(lib, dtype):
    F, C, T_in = 300, 80, 40
    lengths, in_len = [300, 120, 257], [40, 33, 17]
    rng = np.random.RandomState(3)
    path, rates = _path(rng, 3, F, lengths, in_len, T_in), _table(rng, 3, T_in)
    for how in (dict(stretch=W.stretch_q(0.8)), dict(path=path, rates=rates, in_len=in_len, T_in=T_in)):
        cap = 700
        got, mel, c, n = check_warp(lib, lengths, C, F, dtype, cap=cap, seed=5, **how)
        for order in ([2, 1, 0], [0], [1], [2]):
            sub = dict(how)
            if "path" in sub:
                sub.update(path=path[order], rates=rates[order], in_len=[in_len[b] for b in order])
            m2 = Mel([lengths[b] for b in order], C, F, dtype, seed=5)
            for k, b in enumerate(order):                       # the same values as the batch's entry b
                m2.x[k] = mel.x[b]
                for ch in range(C):
                    at = k * m2.ld_entry + ch * m2.ld_row
                    m2.buf.t[at:at + mel.x[b].shape[1]].copy_(torch.from_numpy(mel.x[b][ch].copy()))
            cum, out_len, _, lens_d, _ = run_map(lib, [lengths[b] for b in order], F, cap, **sub)
            g2 = run_gather(lib, m2, lens_d, cum, out_len, cap)
            for k, b in enumerate(order):
                assert g2[k].tobytes() == got[b].tobytes(), "entry %d differs at place %d of %s" % (b, k, order)
                assert cum.np(len(order), F + 1)[k].tolist() == c[b].tolist()


@pytest.mark.parametrize("delta", [-200, -1, 0, 1, 37])
def test_cap_either_side_of_the_needed_length(lib, delta):
    """needed: 514 frames (257 at rate 0.5) - caps 314, 513, 514, 515, 551 lie on both sides of it and of the tile edge 512"""
    got, mel, c, n = check_warp(lib, [257, 0, 100], 17, 257, cap_delta=delta, stretch=W.stretch_q(0.5))
    assert n.tolist() == [min(514, 514 + delta), 0, 200]
    check_warp(lib, [257, 256, 255], 1, 257, torch.float16, cap=256, stretch=Q)        # one tile exactly, cut from 257


def test_strided_views(lib):
    """rows and entries of the mel, the path and the table wider than what is read, odd strides"""
    F, C, T_in = 257, 17, 40
    lengths, in_len = [257, 77, 0], [40, 12, 40]
    rng = np.random.RandomState(8)
    path, rates = _path(rng, 3, F, lengths, in_len, T_in), _table(rng, 3, T_in)
    for dtype in (torch.float32, torch.float16):
        a, _, _, _ = check_warp(lib, lengths, C, F, dtype, ld_row=F + 3, ld_entry=C * (F + 3) + 5, seed=2, path=path, ld_path=F + 2,
                                rates=rates, ld_rates=T_in + 1, in_len=in_len, T_in=T_in)
        b, _, _, _ = check_warp(lib, lengths, C, F, dtype, seed=2, path=path, rates=rates, in_len=in_len, T_in=T_in)
        assert a.tobytes() == b.tobytes()


def test_out_of_range_lengths_act_as_0_and_F(lib):
    a, _, ca, na = check_warp(lib, [-5, 300, 9], 17, 257, stretch=W.stretch_q(0.8), seed=4)
    b, _, cb, nb = check_warp(lib, [0, 257, 9], 17, 257, stretch=W.stretch_q(0.8), seed=4)
    assert ca.tolist() == cb.tolist() and na.tolist() == nb.tolist()
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    # NULL lengths: every entry whole
    mel = Mel([40, 40], 3, 40)
    cum, out_len = Buf(2 * 41, torch.int64, -99), Buf(2, torch.int32, -77)
    rc = lib.t2s_warp_map(None, 2, 40, W.stretch_q(0.8), None, None, 0, None, 0, None, 0, 0.5, 2.0, 50, P(cum), P(out_len), None, _st())
    assert rc == 0
    got = Buf(2 * 3 * 50, torch.float32, NAN)
    assert lib.t2s_warp_gather(P(mel.buf), 1, 2, 3, 40, 40, 120, None, P(cum), P(out_len), P(got), 50, _st()) == 0
    torch.cuda.synchronize()
    c, n, _ = want_map([40, 40], 40, 50, stretch=W.stretch_q(0.8))
    assert cum.np(2, 41).tolist() == c.tolist() and out_len.np(2).tolist() == n.tolist() == [50, 50]
    check_values(got.np(2, 3, 50), mel, c, n, [40, 40], 50)


def test_the_gather_trusts_no_map(lib):
    """a cumulative map and lengths full of nonsense: nothing outside out is written, nothing behind an entry's frames is read"""
    mel = Mel([50, 20, 0], 17, 60)
    lens_d = _ints([50, 20, 0])
    rng = np.random.RandomState(1)
    cum = Buf(3 * 61, torch.int64, -99, rng.randint(-2 ** 59, 2 ** 59, 3 * 61).astype(np.int64))
    out_len = _ints([2 ** 31 - 1, -7, 33])
    got = run_gather(lib, mel, lens_d, cum, out_len, 90)
    assert lens_d.guards_intact()
    assert not (np.abs(got[0]) == 1e4).any() and not (np.abs(got[1]) == 1e4).any()           # (0 / 0 may give a NaN of its own)
    assert not got[2].view(np.uint32).any() and not got[1].view(np.uint32).any()           # F' = 0 and F'= clamp(-7) = 0: all +0
    cum.t.zero_()                                               # every centre equal: 0 / 0, still inside the entry
    got = run_gather(lib, mel, lens_d, cum, out_len, 90)
    assert not (np.abs(got) == 1e4).any()


def run_spans(lib, c, fl, lengths, in_len, hop, trim=None, offsets=None, ratio=(1, 1), total=None, total_dev=False):
    B, F, T_in = c.shape[0], c.shape[1] - 1, fl.shape[1]
    cum, fl_d = Buf(c.size, torch.int64, -99, c), Buf(fl.size, torch.int32, -55, fl)
    lens_d = None if lengths is None else _ints(lengths)
    in_d = None if in_len is None else _ints(in_len)
    t0 = t1 = off = tot = None
    if trim is not None:
        t0, t1 = _ints(trim[0], torch.int64), _ints(trim[1], torch.int64)
    if offsets is not None:
        off = _ints(offsets, torch.int64)
    if total_dev:
        tot = _ints([total], torch.int64)
    spans = Buf(B * T_in * 2, torch.int64, -99)
    rc = lib.t2s_warp_spans(P(cum), P(fl_d), B, F, T_in, P(in_d), P(lens_d), hop, P(t0), P(t1), P(off), ratio[0], ratio[1],
                            0 if total_dev else (1 << 62 if total is None else total), P(tot), P(spans), _st())
    assert rc == 0
    torch.cuda.synchronize()
    for b in (cum, fl_d, lens_d, in_d, t0, t1, off, tot, spans):
        assert b is None or b.guards_intact()
    want = np.stack([W.spans(c[b], fl[b], F if lengths is None else lengths[b], T_in if in_len is None else in_len[b], hop,
                             None if trim is None else (trim[0][b], trim[1][b] - trim[0][b]),
                             None if offsets is None else offsets[b], ratio, total) for b in range(B)])
    assert spans.np(B, T_in, 2).tolist() == want.tolist()
    return want


@pytest.mark.parametrize("T_in", [1, 40, 65])
def test_spans_equal_the_restatement(lib, T_in):
    rng = np.random.RandomState(100 + T_in)
    F, lengths, in_len = 300, [300, 0, 131], [T_in, T_in, max(1, T_in - 3)]
    for wild in (False, True):
        path = _path(rng, 3, F, lengths, in_len, T_in, wild)
        rates = _table(rng, 3, T_in)
        c, n, fl = want_map(lengths, F, 2 ** 30, path=path, rates=rates, in_len=in_len, T_in=T_in)
        cum, _, fl_d, _, _ = run_map(lib, lengths, F, 2 ** 30, path=path, rates=rates, in_len=in_len, T_in=T_in)
        assert cum.np(3, F + 1).tolist() == c.tolist() and fl_d.np(3, T_in, 2).tolist() == fl.tolist()
        plain = run_spans(lib, c, fl, lengths, in_len, 256)
        if not wild and T_in > 1:                               # a monotone stretch of the path: neighbouring spans abut
            cov = [k for k in range(in_len[0]) if plain[0, k, 0] >= 0]
            assert len(cov) >= 2
        ends = [int(c[b, max(0, min(lengths[b], F))]) * 256 >> 20 for b in range(3)]
        trim = ([100, 0, 5000], [ends[0] - 300, 0, ends[2] + 999])
        run_spans(lib, c, fl, lengths, in_len, 256, trim=trim)
        run_spans(lib, c, fl, lengths, in_len, 256, offsets=[7, 10 ** 9, 123456])
        run_spans(lib, c, fl, lengths, in_len, 256, ratio=(15, 14), total=70000)
        run_spans(lib, c, fl, lengths, None, 256, trim=trim, offsets=[90000, 5, 0], ratio=(441, 448), total=150000, total_dev=True)
        run_spans(lib, c, fl, None, in_len, 1, trim=([0, 0, 0], [0, 3, 10 ** 12]), ratio=(1, 7))


def test_spans_of_a_monotone_path_abut_and_wild_first_last_give_no_span(lib):
    path = np.array([[0, 0, 1, 1, 1, 2, 3, 3, -1, -1]], dtype=np.int32)
    rates = np.array([[1.0, 0.5, 2.0, 0.8, 1.0]], dtype=np.float32)
    c, n, fl = want_map([8], 10, 100, path=path, rates=rates, in_len=[4], T_in=5)
    sp = run_spans(lib, c, fl, [8], [4], 256)
    assert sp[0].tolist() == [[0, 512], [512, 2048], [2048, 2176], [2176, 2816], [-1, -1]]
    wild = np.array([[[0, 8], [-3, 2], [5, 4], [2 ** 31 - 1, 2 ** 31 - 1], [7, 7]]], dtype=np.int32)
    sp = run_spans(lib, c, wild, [8], [5], 256)
    assert sp[0, :4].tolist() == [[-1, -1]] * 4 and sp[0, 4, 0] >= 0


def test_refused_tuples_write_nothing(lib):
    mel = Mel([20, 10], 3, 20)
    lens, cum, out_len = _ints([20, 10]), Buf(2 * 21, torch.int64, -99), Buf(2, torch.int32, -77)
    fl, spans, out = Buf(2 * 4 * 2, torch.int32, -55), Buf(2 * 4 * 2, torch.int64, -99), Buf(2 * 3 * 30, torch.float32, NAN)
    path, rates, s_d = _ints([0] * 40), Buf(8, torch.float32, 1.0), _ints([Q, Q], torch.int64)
    ok_m = dict(lengths=P(lens), B=2, F=20, stretch=Q, stretches=None, path=P(path), ld_path=20, rates=P(rates), ld_rates=4,
                in_len=None, T_in=4, lo=0.5, hi=2.0, cap=30, cum=P(cum), out_len=P(out_len), fl=P(fl))
    bad_m = [dict(cum=None, out_len=None, fl=None), dict(B=0), dict(B=65536), dict(F=0), dict(F=2 ** 30 + 1), dict(cap=0), dict(T_in=0),
             dict(path=None), dict(path=None, rates=None), dict(ld_path=19), dict(ld_rates=3), dict(stretch=Q + 1),
             dict(stretches=P(s_d)), dict(rates=None, stretch=(Q >> 3) - 1), dict(rates=None, stretch=(Q << 3) + 1), dict(lo=0.1),
             dict(hi=8.5), dict(lo=1.5, hi=1.0), dict(lo=NAN), dict(hi=NAN), dict(cum=P(cum) + 4), dict(out_len=P(out_len) + 2),
             dict(lengths=P(lens) + 1), dict(rates=None, stretches=P(s_d) + 4)]
    for ch in bad_m:
        a = dict(ok_m, **ch)
        rc = lib.t2s_warp_map(a["lengths"], a["B"], a["F"], a["stretch"], a["stretches"], a["path"], a["ld_path"], a["rates"],
                              a["ld_rates"], a["in_len"], a["T_in"], a["lo"], a["hi"], a["cap"], a["cum"], a["out_len"], a["fl"], _st())
        assert rc == -1, "t2s_warp_map accepted %r" % (ch,)
    ok_g = dict(x=P(mel.buf), kind=1, B=2, C=3, F=20, ld_row=20, ld_entry=60, lengths=P(lens), cum=P(cum), out_len=P(out_len),
                out=P(out), cap=30)
    bad_g = [dict(x=None), dict(cum=None), dict(out_len=None), dict(out=None), dict(kind=0), dict(kind=3), dict(B=0), dict(B=65536),
             dict(C=0), dict(F=0), dict(cap=0), dict(ld_row=19), dict(ld_entry=59), dict(x=P(mel.buf) + 2), dict(out=P(out) + 2),
             dict(cum=P(cum) + 4), dict(out=P(mel.buf) + 16), dict(x=P(out) + 64)]
    for ch in bad_g:
        a = dict(ok_g, **ch)
        rc = lib.t2s_warp_gather(a["x"], a["kind"], a["B"], a["C"], a["F"], a["ld_row"], a["ld_entry"], a["lengths"], a["cum"],
                                 a["out_len"], a["out"], a["cap"], _st())
        assert rc == -1, "t2s_warp_gather accepted %r" % (ch,)
    ok_s = dict(cum=P(cum), fl=P(fl), B=2, F=20, T_in=4, in_len=None, lengths=P(lens), hop=256, t0=None, t1=None, off=None, up=1, down=1,
                total=1 << 62, tot=None, spans=P(spans))
    bad_s = [dict(cum=None), dict(fl=None), dict(spans=None), dict(B=0), dict(F=0), dict(T_in=0), dict(hop=0), dict(hop=(1 << 20) + 1),
             dict(F=1 << 30, hop=1024), dict(t0=P(cum)), dict(t1=P(cum)), dict(up=0), dict(down=0), dict(up=(1 << 20) + 1), dict(total=-1),
             dict(spans=P(spans) + 4), dict(off=P(cum) + 4), dict(tot=P(cum) + 4)]
    for ch in bad_s:
        a = dict(ok_s, **ch)
        rc = lib.t2s_warp_spans(a["cum"], a["fl"], a["B"], a["F"], a["T_in"], a["in_len"], a["lengths"], a["hop"], a["t0"], a["t1"],
                                a["off"], a["up"], a["down"], a["total"], a["tot"], a["spans"], _st())
        assert rc == -1, "t2s_warp_spans accepted %r" % (ch,)
    torch.cuda.synchronize()
    for b in (cum, out_len, fl, spans, out):
        assert b.untouched(), "a refused call wrote to an output"
    assert mel.buf.guards_intact()
