"""t2s_trim_energy / t2s_trim_bounds / t2s_trim_gather (csrc/trim.hip, csrc/t2s_api_audio.hip) called directly on guarded buffers,
against the float64 restatement of tests/trim_ref.py (librosa's formulas restated; tests/test_trim_ref_cpu.py asserts that its two
forms agree and that no frame of these seeded clips lies within 1e-6 dB of the threshold, so nothing here is exempt).

int16 energies are compared for EQUALITY with the integer sums, peaks with the host's, bounds with the reference's, int16 output
with the reference's and float32 output with the bits of the stated formula.  Float energies are held to (fl + 1) 2^-53 relative:
fl exact squares summed in double in some order, (fl - 1) roundings at most, plus the reference's own.

Every source is a view into a larger tensor filled with +-32767 (or NaN / 1e4), every destination, scratch and table a view into a
larger tensor of sentinels which must come back untouched."""
import numpy as np
import pytest
import torch

import trim_ref as R
from text2speech_amd import _lib
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
NP_OF = {torch.int16: np.int16, torch.float32: np.float32, torch.float16: np.float16}
KIND = {torch.int16: 0, torch.float32: 1, torch.float16: 2}
MODE = {"reflect": 0, "constant": 1}
E_FILL, B_FILL = -7.0, -99
WORST = {}


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def tile(lib):
    return lib.t2s_trim_tile()


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


class Held:
    """a plain device tensor where a Buf is expected"""

    def __init__(self, t):
        self.t = t


def _src_buf(n, dtype, shift=0):
    return Buf(n, dtype, 32767 if dtype == torch.int16 else 1e4, shift)


def _frames(n, fl, h, mode):
    return 0 if n <= 0 or (mode == "reflect" and n <= fl // 2) else R.n_frames(n, fl, h)


def run(lib, src, rows, fl, h, mode, decisions=(), floor=0.0):
    """rows: (src_start, src_count), all inside src.  Energy pass, then one bounds pass per (top_db, rescaling_max).
    -> (energies per row, stats [n, 2], {decision: bounds [n, 2]}, the device tensors for a gather)"""
    n_rows = len(rows)
    nfs = [_frames(c, fl, h, mode) for _, c in rows]
    e_starts, pos = [], 3
    for nf in nfs:
        e_starts.append(pos)
        pos += nf + 2
    energy = Buf(pos + 1, torch.float64, E_FILL)
    stats = Buf(2 * n_rows, torch.float64, E_FILL)              # the call initialises it
    table = Buf(3 * n_rows, torch.int64, B_FILL)
    table.t.copy_(torch.tensor([(s, c, e) for (s, c), e in zip(rows, e_starts)], dtype=torch.int64).view(-1))
    max_frames = max(1, max(nfs))
    rc = lib.t2s_trim_energy(src.data_ptr(), KIND[src.dtype], src.numel(), table.t.data_ptr(), n_rows, fl, h, MODE[mode], max_frames,
                             energy.t.data_ptr(), energy.t.numel(), stats.t.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert energy.guards_intact() and stats.guards_intact() and table.guards_intact()
    E = energy.t.cpu().numpy()
    written = np.zeros(E.size, dtype=bool)
    per_row = []
    for e, nf in zip(e_starts, nfs):
        per_row.append(E[e:e + nf].copy())
        written[e:e + nf] = True
    assert bool((E[~written] == E_FILL).all()), "the scratch between the rows was written"
    st = stats.t.cpu().numpy().reshape(n_rows, 2)
    found = {}
    bounds_d = {}
    for top_db, r in decisions:
        bounds = Buf(2 * n_rows, torch.int64, B_FILL)
        rc = lib.t2s_trim_bounds(table.t.data_ptr(), n_rows, KIND[src.dtype], src.numel(), fl, h, MODE[mode], max_frames,
                                 energy.t.data_ptr(), energy.t.numel(), stats.t.data_ptr(), float(top_db), int(r is not None),
                                 0.0 if r is None else r, floor, bounds.t.data_ptr(), _st())
        assert rc == 0
        torch.cuda.synchronize()
        assert bounds.guards_intact()
        found[(top_db, r)] = bounds.t.cpu().numpy().reshape(n_rows, 2)
        bounds_d[(top_db, r)] = bounds
    return per_row, st, found, (stats, bounds_d)


def gather(lib, src, rows4, bounds, stats, r, dst, max_out, floor=0.0, want_lengths=True):
    """rows4: (src_start, src_count, dst_start, dst_cap); bounds / stats: Buf or None (stats go in only with a rescaling_max r)
    -> out_lengths"""
    n_rows = len(rows4)
    table = torch.tensor(rows4, dtype=torch.int64, device=DEV)
    lens = torch.full((n_rows,), -77, dtype=torch.int32, device=DEV) if want_lengths else None
    rc = lib.t2s_trim_gather(src.data_ptr(), KIND[src.dtype], src.numel(), table.data_ptr(), n_rows,
                             None if bounds is None else bounds.t.data_ptr(), None if stats is None or r is None else stats.t.data_ptr(),
                             0.0 if r is None else r, floor, dst.t.data_ptr(), KIND[dst.t.dtype], dst.t.numel(), max_out,
                             lens.data_ptr() if want_lengths else None, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert dst.guards_intact(), "wrote outside the destination"
    return lens.cpu().numpy() if want_lengths else None


def _dst(n, dtype, shift=0):
    return Buf(n, dtype, 12345 if dtype == torch.int16 else 12345.678, shift)


def _alone(lib, clip, fl, h, mode, decisions, shift=0, floor=0.0):
    """one clip in a buffer of its own -> (energies, stats row, {decision: (start, end)}, {decision: gathered output})"""
    dtype = {np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}[clip.dtype]
    src = _src_buf(clip.size, dtype, shift)
    src.t.copy_(torch.from_numpy(clip))
    E, st, found, (stats, bounds_d) = run(lib, src.t, [(0, clip.size)], fl, h, mode, decisions, floor)
    outs = {}
    out_dtype = torch.int16 if dtype == torch.int16 else torch.float32
    for d in decisions:
        s, e = found[d][0]
        dst = _dst(clip.size, out_dtype, shift)
        lens = gather(lib, src.t, [(0, clip.size, 0, clip.size)], bounds_d[d], stats, d[1], dst, clip.size, floor)
        assert lens[0] == e - s
        got = dst.t.cpu().numpy()
        assert got[e - s:].tobytes() == np.zeros(clip.size - (e - s), dtype=got.dtype).tobytes(), "+0 behind the kept range"
        outs[d] = got[:e - s]
    assert src.guards_intact()
    return E[0], st[0], {d: tuple(int(v) for v in found[d][0]) for d in decisions}, outs


# ---- int16: energies, peaks, bounds and output equal the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("fl,h", R.FRAMES)
def test_int16_equals_the_reference(lib, tile, fl, h, mode):
    trimmed = 0
    for n in R.lengths_for(fl, h, mode, tile):
        clip = R.clip_int16(R.seed_of(fl, h, mode, n), n)
        want_E = R.frame_energies(clip, fl, h, mode)
        want_b = {d: R.trim_bounds(clip, fl, h, mode, d[0], d[1]) for d in R.DECISIONS}
        want_o = {d: R.rescale_trim(clip, fl, h, mode, d[0], d[1]) for d in R.DECISIONS}
        for shift in (0, 1):                                    # both 2-byte parities of source and destination
            E, st, b, outs = _alone(lib, clip, fl, h, mode, R.DECISIONS, shift)
            assert E.size == want_E.size and np.array_equal(E, want_E), "n %d shift %d: energies" % (n, shift)
            assert st[0] == float(np.abs(clip.astype(np.int32)).max()) and st[1] == want_E.max()
            for d in R.DECISIONS:
                assert b[d] == want_b[d], "n %d shift %d %r: bounds %r, reference %r" % (n, shift, d, b[d], want_b[d])
                assert np.array_equal(outs[d], want_o[d]), "n %d shift %d %r: output" % (n, shift, d)
                if d[1] is None:
                    assert outs[d].tobytes() == clip[b[d][0]:b[d][1]].tobytes(), "without rescaling: a copy"
                trimmed += b[d] != (0, n)
    assert trimmed, "some case must cut something"


def test_known_answers(lib):
    burst = R.burst_clip()
    ds = ((23, None), (23, 0.999), (100, 0.999))
    _, st, b, outs = _alone(lib, burst, 512, 128, "reflect", ds)
    assert st.tolist() == [3.0, 900.0]
    assert b[(23, None)] == (0, 5000) and b[(23, 0.999)] == (1792, 2432) and b[(100, 0.999)] == (0, 5000)
    assert outs[(23, 0.999)].size == 640 and set(outs[(23, 0.999)].tolist()) == {0, 32735}
    zeros = np.zeros(3000, dtype=np.int16)
    for mode in R.MODES:
        _, st, b, outs = _alone(lib, zeros, 512, 128, mode, ((23, None), (23, 0.999)))
        assert st.tolist() == [0.0, 0.0] and set(b.values()) == {(0, 0)} and all(o.size == 0 for o in outs.values())
    # +-peak -> +-rint(rescaling_max 32768), at the range's ends too; rescaling alone (no bounds) keeps every sample
    for peak in (3, 20000, 32767):
        clip = np.array([peak, -peak, 0, 1, -1] * 60, dtype=np.int16)
        src = _src_buf(clip.size, torch.int16)
        src.t.copy_(torch.from_numpy(clip))
        _, _, _, (stats, _) = run(lib, src.t, [(0, clip.size)], 64, 16, "constant")
        dst = _dst(clip.size, torch.int16)
        assert gather(lib, src.t, [(0, clip.size, 0, clip.size)], None, stats, 0.999, dst, clip.size).tolist() == [clip.size]
        got = dst.t.cpu().numpy()
        assert got[0] == 32735 and got[1] == -32735 and got[2] == 0 and np.array_equal(got, R.rescale(clip, 0.999))
    clip = np.array([-32768, 32767, 5], dtype=np.int16)
    src = _src_buf(3, torch.int16)
    src.t.copy_(torch.from_numpy(clip))
    _, st, _, (stats, _) = run(lib, src.t, [(0, 3)], 4, 2, "constant")
    assert st[0, 0] == 32768.0
    dst = _dst(3, torch.int16)
    gather(lib, src.t, [(0, 3, 0, 3)], None, stats, 1.0, dst, 3)
    assert dst.t.cpu().numpy().tolist() == [-32768, 32767, 5] == R.rescale(clip, 1.0).tolist()


# ---- float sources ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("fl,h", R.FRAMES)
def test_float_sources(lib, tile, src_dtype, fl, h, mode):
    key = str(src_dtype)
    for n in R.lengths_for(fl, h, mode, tile):
        clip = R.clip_float(R.seed_of(fl, h, mode, n), n, NP_OF[src_dtype])
        want_E = R.frame_energies(clip, fl, h, mode)
        E, st, b, outs = _alone(lib, clip, fl, h, mode, R.DECISIONS, shift=n & 1)
        assert E.size == want_E.size
        rel = float((np.abs(E - want_E) / np.maximum(want_E, 1e-300)).max())
        WORST[key] = max(WORST.get(key, 0.0), rel / ((fl + 1) * 2.0 ** -53))
        assert rel <= (fl + 1) * 2.0 ** -53, "n %d: energies off by %.3e relative" % (n, rel)
        assert st[0] == float(np.abs(clip.astype(np.float64)).max()) and st[1] == E.max()
        for d in R.DECISIONS:
            assert b[d] == R.trim_bounds(clip, fl, h, mode, d[0], d[1]), "n %d %r" % (n, d)
            want = R.rescale(clip, d[1])[b[d][0]:b[d][1]]
            assert outs[d].dtype == np.float32 and outs[d].tobytes() == want.tobytes(), "n %d %r: output bits" % (n, d)
    print("TRIM %s (%d, %d) %s: worst energy error so far %.3e of (fl + 1) 2^-53" % (src_dtype, fl, h, mode, WORST[key]))


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.float16])
def test_non_finite_samples_trim_to_nothing_and_padding_is_never_read(lib, src_dtype):
    fl, h, mode, ds = 512, 128, "reflect", ((23, None), (23, 0.999))
    good = R.clip_float(11, 3000, NP_OF[src_dtype])
    clips = [good]
    for bad, at in ((np.nan, 1500), (np.inf, 0), (-np.inf, 2999), (np.nan, 2999)):
        c = good.copy()
        c[at] = bad
        clips.append(c)
    # the clips back to back with NaN / 1e4 between them and behind the last
    gap = 9
    src = _src_buf(len(clips) * (3000 + gap), src_dtype)
    src.t[::2] = float("nan")
    rows = []
    for q, c in enumerate(clips):
        s = q * (3000 + gap) + 4
        src.t[s:s + 3000].copy_(torch.from_numpy(c))
        rows.append((s, 3000))
    E, st, b, _ = run(lib, src.t, rows, fl, h, mode, ds)
    E0, st0, b0, _ = _alone(lib, good, fl, h, mode, ds)
    assert E[0].tobytes() == E0.tobytes() and st[0].tobytes() == st0.tobytes(), "neighbours changed a clip's energies"
    for d in ds:
        assert tuple(b[d][0]) == b0[d] == R.trim_bounds(good, fl, h, mode, d[0], d[1]) and b0[d] != (0, 0)
        for q in range(1, len(clips)):
            assert tuple(b[d][q]) == (0, 0), "clip %d holds a non-finite sample" % q
    assert np.isinf(st[1:, 0]).all()


# ---- several clips in one pool ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dtype", [torch.int16, torch.float32, torch.float16])
@pytest.mark.parametrize("fl,h,mode", [(512, 128, "reflect"), (50, 20, "constant")])
def test_pool_clips_are_bit_equal_to_the_clip_alone(lib, src_dtype, fl, h, mode):
    ds = ((23, 0.999), (40, None))
    lengths = [n for n in R.POOL_LENGTHS if mode == "constant" or n > fl // 2]
    clips = [R.clip_int16(600 + q, n) if src_dtype == torch.int16 else R.clip_float(600 + q, n, NP_OF[src_dtype])
             for q, n in enumerate(lengths)]
    alone = [_alone(lib, c, fl, h, mode, ds) for c in clips]
    out_dtype = torch.int16 if src_dtype == torch.int16 else torch.float32
    gen = np.random.RandomState(5)
    for shift in (0, 1):
        src_starts, pos = [], 5
        for c in clips:
            src_starts.append(pos)
            pos += c.size + int(gen.randint(1, 9))
        src = _src_buf(pos + 3, src_dtype, shift)
        src.t[::2] = -32767 if src_dtype == torch.int16 else float("nan")
        for c, s in zip(clips, src_starts):
            src.t[s:s + c.size].copy_(torch.from_numpy(c))
        order = gen.permutation(len(clips))                     # the rows in another order than the clips lie in the pool
        rows = [(src_starts[q], clips[q].size) for q in order]
        E, st, b, (stats, bounds_d) = run(lib, src.t, rows, fl, h, mode, ds)
        for k, q in enumerate(order):
            assert E[k].tobytes() == alone[q][0].tobytes() and st[k].tobytes() == alone[q][1].tobytes(), "clip %d shift %d" % (q, shift)
        for d in ds:
            dst_starts, pos = [], 3
            for k, q in enumerate(order):
                assert tuple(b[d][k]) == alone[q][2][d]
                dst_starts.append(pos)
                pos += alone[q][3][d].size + int(gen.randint(1, 9))
            dst = _dst(pos + 2, out_dtype, shift)
            rows4 = [(s, c, t, alone[q][3][d].size) for (s, c), t, q in zip(rows, dst_starts, order)]
            lens = gather(lib, src.t, rows4, bounds_d[d], stats, d[1], dst, max(r[3] for r in rows4))
            got = dst.t.cpu().numpy()
            written = np.zeros(got.size, dtype=bool)
            for k, q in enumerate(order):
                a, t = alone[q][3][d], dst_starts[k]
                assert lens[k] == a.size and got[t:t + a.size].tobytes() == a.tobytes(), "clip %d differs from the clip alone" % q
                written[t:t + a.size] = True
            assert bool((got[~written] == NP_OF[out_dtype](dst.fill)).all()), "the gaps between the rows were written"


# ---- the gather's destination ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dtype", [torch.int16, torch.float32])
def test_dst_cap_truncates_or_zero_fills_and_out_lengths_count(lib, src_dtype):
    fl, h, mode, d = 512, 128, "reflect", (23, 0.999)
    clip = R.clip_int16(9, 5000) if src_dtype == torch.int16 else R.clip_float(9, 5000, np.float32)
    full = R.rescale_trim(clip, fl, h, mode, *d)
    kept = full.size
    assert 2049 < kept < 5000
    src = _src_buf(clip.size, src_dtype)
    src.t.copy_(torch.from_numpy(clip))
    _, _, b, (stats, bounds_d) = run(lib, src.t, [(0, clip.size)], fl, h, mode, (d,))
    assert tuple(b[d][0]) == R.trim_bounds(clip, fl, h, mode, *d)
    caps = [1, 2047, 2048, 2049, kept - 1, kept, kept + 1, kept + 700, 0]
    stride = kept + 800
    out_dtype = torch.int16 if src_dtype == torch.int16 else torch.float32
    dst = _dst(stride * len(caps), out_dtype)
    # (the row's bounds and stats, once per cap)
    bnd = Held(torch.tensor(b[d][0].tolist() * len(caps), dtype=torch.int64, device=DEV))
    sts = Held(stats.t.repeat(len(caps)).contiguous())
    lens = gather(lib, src.t, [(0, clip.size, q * stride, cap) for q, cap in enumerate(caps)], bnd, sts, d[1], dst, max(caps))
    got = dst.t.cpu().numpy()
    for q, cap in enumerate(caps):
        row = got[q * stride:(q + 1) * stride]
        v = min(cap, kept)
        assert lens[q] == v
        assert row[:v].tobytes() == full[:v].tobytes(), "cap %d" % cap
        assert row[v:cap].tobytes() == np.zeros(cap - v, dtype=row.dtype).tobytes(), "cap %d: +0 behind the samples" % cap
        assert bool((row[cap:] == NP_OF[out_dtype](dst.fill)).all()), "cap %d: wrote behind dst_cap" % cap
    # max_out below a row's cap cuts the row there; no out_lengths is fine
    dst = _dst(kept, out_dtype)
    gather(lib, src.t, [(0, clip.size, 0, kept)], bounds_d[d], stats, d[1], dst, 100, want_lengths=False)
    got = dst.t.cpu().numpy()
    assert got[:100].tobytes() == full[:100].tobytes() and bool((got[100:] == NP_OF[out_dtype](dst.fill)).all())


def test_any_table_value_is_safe(lib):
    """rows whose source lies outside the pool have no samples: no frames, peak 0, bounds (0, 0), a row of zeros (the pool's
    neighbours hold +-32767: a read outside would show); a count that runs past the pool's end is cut there; a reflect row of at
    most frame_length // 2 samples is flagged and gets no frames; energy rows outside the scratch and destination rows outside dst
    write nothing; hostile bounds are cut to the row"""
    fl, h, mode, d = 64, 16, "reflect", (23, None)
    pool_len, cap = 400, 90
    src = _src_buf(pool_len, torch.int16)
    clip = R.clip_int16(12, pool_len)
    src.t.copy_(torch.from_numpy(clip))
    bad_src = [(-1, 50), (-(1 << 40), 50), (pool_len, 50), (pool_len + 7, 5), (1 << 40, 50), (1 << 62, 1 << 62), (10, -1),
               (10, -(1 << 62)), (-(1 << 63), (1 << 63) - 1), (10, 0)]
    cut_src = [(pool_len - 50, 51), (pool_len - 50, 1 << 40), (pool_len - 33, (1 << 63) - 1), (0, 1 << 50)]
    short = [(100, 32), (100, 1)]                               # reflect, at most pad = 32 samples
    rows = bad_src + cut_src + short
    n_rows = len(rows)
    cut_n = [min(c, pool_len - s) for s, c in cut_src]
    nfs = [0] * len(bad_src) + [R.n_frames(n, fl, h) for n in cut_n] + [0, 0]
    # two more rows whose energy_start lies outside the scratch
    rows3 = [(s, c, 40 * q) for q, (s, c) in enumerate(rows)] + [(0, 200, -5), (0, 200, 1 << 40)]
    energy = Buf(40 * n_rows, torch.float64, E_FILL)
    stats = Buf(2 * len(rows3), torch.float64, E_FILL)
    table = torch.tensor(rows3, dtype=torch.int64, device=DEV)
    rc = lib.t2s_trim_energy(src.t.data_ptr(), 0, pool_len, table.data_ptr(), len(rows3), fl, h, 0, 40, energy.t.data_ptr(),
                             energy.t.numel(), stats.t.data_ptr(), _st())
    assert rc == 0
    bounds = Buf(2 * len(rows3), torch.int64, B_FILL)
    rc = lib.t2s_trim_bounds(table.data_ptr(), len(rows3), 0, pool_len, fl, h, 0, 40, energy.t.data_ptr(), energy.t.numel(),
                             stats.t.data_ptr(), 23.0, 0, 0.0, 0.0, bounds.t.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert energy.guards_intact() and stats.guards_intact() and bounds.guards_intact() and src.guards_intact()
    E = energy.t.cpu().numpy().reshape(n_rows, 40)
    st = stats.t.cpu().numpy().reshape(-1, 2)
    bd = bounds.t.cpu().numpy().reshape(-1, 2)
    for q in range(len(bad_src)):
        assert bool((E[q] == E_FILL).all()) and st[q].tolist() == [0.0, 0.0] and bd[q].tolist() == [0, 0], "row %r" % (rows[q],)
    for k, ((s, _), n) in enumerate(zip(cut_src, cut_n)):
        q = len(bad_src) + k
        want = R.frame_energies(clip[s:s + n], fl, h, mode)
        assert np.array_equal(E[q, :nfs[q]], want) and bool((E[q, nfs[q]:] == E_FILL).all()), "row %r" % (rows[q],)
        assert st[q].tolist() == [float(np.abs(clip[s:s + n].astype(np.int32)).max()), want.max()]
        assert tuple(bd[q]) == R.trim_bounds(clip[s:s + n], fl, h, mode, 23)
    for k, (s, n) in enumerate(short):
        q = len(bad_src) + len(cut_src) + k
        assert bool((E[q] == E_FILL).all()) and bd[q].tolist() == [0, 0]
        assert st[q].tolist() == [float(np.abs(clip[s:s + n].astype(np.int32)).max()), -1.0], "the flag of a short reflect row"
    for q in (n_rows, n_rows + 1):                              # no room in the scratch: the peak alone
        assert st[q].tolist() == [float(np.abs(clip[:200].astype(np.int32)).max()), 0.0] and bd[q].tolist() == [0, 0]

    # the gather: sources as above, then destinations outside dst, then hostile bounds
    rows4 = [(s, c, q * cap, cap) for q, (s, c) in enumerate(bad_src + cut_src)]
    n_ok = len(rows4)
    dst_len = n_ok * cap
    dst = _dst(dst_len + 40, torch.int16)
    rows4 += [(0, 100, -1, cap), (0, 100, -(1 << 62), cap), (0, 100, dst_len + 40, cap), (0, 100, 1 << 62, 1 << 62), (0, 100, 5, -3),
              (0, 100, 5, -(1 << 63))]
    rows4.append((0, 100, dst_len + 10, 1 << 40))               # a cap that runs past the destination's end is cut there: 30 samples
    lens = gather(lib, src.t, rows4, None, None, None, dst, cap)
    got = dst.t.cpu().numpy()
    for q in range(len(bad_src)):
        assert lens[q] == 0 and bool((got[q * cap:(q + 1) * cap] == 0).all()), "row %r" % (rows4[q],)
    for k, ((s, _), n) in enumerate(zip(cut_src, cut_n)):
        q = len(bad_src) + k
        v = min(n, cap)
        assert lens[q] == v and np.array_equal(got[q * cap:q * cap + v], clip[s:s + v]) and bool((got[q * cap + v:(q + 1) * cap] == 0).all())
    assert lens[n_ok:n_ok + 6].tolist() == [0] * 6
    assert bool((got[dst_len:dst_len + 10] == 12345).all())
    assert lens[-1] == 30 and np.array_equal(got[dst_len + 10:], clip[:30])
    hostile = [(-5, 50), (20, 10), (30, 1 << 62), (-(1 << 63), (1 << 63) - 1), (1 << 62, 5), (100, 100), (0, 0), (7, 60)]
    want = [(0, 50), (20, 20), (30, 100), (0, 100), (100, 100), (100, 100), (0, 0), (7, 60)]
    bnd = Buf(2 * len(hostile), torch.int64, B_FILL)
    bnd.t.copy_(torch.tensor(hostile, dtype=torch.int64).view(-1))
    dst = _dst(len(hostile) * 100, torch.int16)
    lens = gather(lib, src.t, [(200, 100, q * 100, 100) for q in range(len(hostile))], bnd, None, None, dst, 100)
    got = dst.t.cpu().numpy().reshape(len(hostile), 100)
    for q, (s, e) in enumerate(want):
        assert lens[q] == e - s and np.array_equal(got[q, :e - s], clip[200 + s:200 + e]) and bool((got[q, e - s:] == 0).all()), hostile[q]
    assert src.guards_intact()


def test_refused_calls_launch_nothing(lib):
    """every T2S_EINVAL case of tests/test_trim_ref_cpu.py's list, here with real buffers: sentinels everywhere stay"""
    fl, h = 64, 16
    clip = R.clip_int16(3, 500)
    src = _src_buf(500, torch.int16)
    src.t.copy_(torch.from_numpy(clip))
    table = torch.tensor([(0, 500, 0)], dtype=torch.int64, device=DEV)
    table4 = torch.tensor([(0, 500, 0, 500)], dtype=torch.int64, device=DEV)
    energy, stats, bounds, dst = Buf(40, torch.float64, E_FILL), Buf(2, torch.float64, E_FILL), Buf(2, torch.int64, B_FILL), _dst(500, torch.int16)
    p = lambda b: b.t.data_ptr()
    nan, inf = float("nan"), float("inf")

    def energy_call(**kw):
        a = dict(src=src.t.data_ptr(), kind=0, src_len=500, table=table.data_ptr(), rows=1, fl=fl, hop=h, mode=0, max_frames=40,
                 en=p(energy), en_len=40, stats=p(stats))
        a.update(kw)
        return lib.t2s_trim_energy(a["src"], a["kind"], a["src_len"], a["table"], a["rows"], a["fl"], a["hop"], a["mode"],
                                   a["max_frames"], a["en"], a["en_len"], a["stats"], _st())

    def bounds_call(**kw):
        a = dict(table=table.data_ptr(), rows=1, kind=0, src_len=500, fl=fl, hop=h, mode=0, max_frames=40, en=p(energy), en_len=40,
                 stats=p(stats), top_db=23.0, rescale=1, r=0.999, floor=0.0, out=p(bounds))
        a.update(kw)
        return lib.t2s_trim_bounds(a["table"], a["rows"], a["kind"], a["src_len"], a["fl"], a["hop"], a["mode"], a["max_frames"],
                                   a["en"], a["en_len"], a["stats"], a["top_db"], a["rescale"], a["r"], a["floor"], a["out"], _st())

    def gather_call(**kw):
        a = dict(src=src.t.data_ptr(), kind=0, src_len=500, table=table4.data_ptr(), rows=1, bnd=p(bounds), stats=p(stats), r=0.999,
                 floor=0.0, dst=p(dst), dkind=0, dst_len=500, max_out=500)
        a.update(kw)
        return lib.t2s_trim_gather(a["src"], a["kind"], a["src_len"], a["table"], a["rows"], a["bnd"], a["stats"], a["r"], a["floor"],
                                   a["dst"], a["dkind"], a["dst_len"], a["max_out"], None, _st())

    frames = [dict(fl=1), dict(fl=8193), dict(hop=0), dict(hop=fl + 1), dict(mode=2), dict(mode=-1), dict(max_frames=0),
              dict(max_frames=(1 << 40) + 1)]
    common = [dict(table=None), dict(rows=0), dict(rows=-1), dict(rows=65536), dict(kind=3), dict(kind=-1), dict(src_len=0),
              dict(src_len=-5)]
    for kw in frames + common + [dict(src=None), dict(stats=None), dict(en_len=0), dict(stats=p(stats) + 4), dict(en=p(energy) + 4)]:
        assert energy_call(**kw) == -1, kw
    for kw in frames + common + [dict(en=None), dict(stats=None), dict(out=None), dict(en_len=0), dict(top_db=-1.0), dict(top_db=nan),
                                 dict(top_db=inf), dict(r=-0.5), dict(r=nan), dict(r=inf), dict(r=0.0), dict(floor=-1.0), dict(floor=nan),
                                 dict(floor=inf), dict(rescale=2)]:
        assert bounds_call(**kw) == -1, kw
    for kw in common + [dict(src=None), dict(dst=None), dict(dst_len=0), dict(max_out=0), dict(max_out=(1 << 40) + 1), dict(dkind=1),
                        dict(dkind=2), dict(dkind=-1), dict(r=-1.0), dict(r=nan), dict(r=inf), dict(r=0.0), dict(floor=-1.0),
                        dict(floor=nan), dict(dst=src.t.data_ptr(), dst_len=500), dict(dst=src.t.data_ptr() + 200, dst_len=100)]:
        assert gather_call(**kw) == -1, kw
    fsrc = torch.zeros(500, dtype=torch.float32, device=DEV)
    assert gather_call(src=fsrc.data_ptr(), kind=1, dkind=0) == -1 and gather_call(src=fsrc.data_ptr(), kind=2, dkind=0) == -1
    torch.cuda.synchronize()
    for b in (energy, stats, bounds, dst):
        assert b.guards_intact() and bool((b.t == b.fill).all()), "a refused call wrote something"
    # and the accepted calls do write
    assert energy_call() == 0 and bounds_call() == 0 and gather_call() == 0
    torch.cuda.synchronize()
    assert tuple(bounds.t.cpu().tolist()) == R.trim_bounds(clip, fl, h, "reflect", 23, 0.999)
    s, e = bounds.t.cpu().tolist()
    assert np.array_equal(dst.t.cpu().numpy()[:e - s], R.rescale_trim(clip, fl, h, "reflect", 23, 0.999))


def test_two_identical_calls_give_identical_bits(lib):
    clip = R.clip_float(5, 9000, np.float32)
    a = _alone(lib, clip, 512, 128, "reflect", ((23, 0.999),))
    b = _alone(lib, clip, 512, 128, "reflect", ((23, 0.999),))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert a[3][(23, 0.999)].tobytes() == b[3][(23, 0.999)].tobytes()


def test_peaks_only_and_a_long_hop(lib):
    """energy = NULL gives the peaks alone; with hop = frame_length samples behind the last frame still count for the peak"""
    n = 5040
    clip = R.clip_int16(8, n)
    clip[5035] = 32000                                          # (64, 64) constant: 79 frames, the last ends at sample 5023
    src = _src_buf(n, torch.int16)
    src.t.copy_(torch.from_numpy(clip))
    E, st, _, _ = run(lib, src.t, [(0, n)], 64, 64, "constant")
    assert np.array_equal(E[0], R.frame_energies(clip, 64, 64, "constant")) and st[0].tolist() == [32000.0, E[0].max()]
    assert E[0].size == 79 and 78 * 64 + 64 - 32 <= 5035
    stats = Buf(2, torch.float64, E_FILL)
    table = torch.tensor([(0, n, 0)], dtype=torch.int64, device=DEV)
    assert lib.t2s_trim_energy(src.t.data_ptr(), 0, n, table.data_ptr(), 1, 512, 128, 0, 40, None, 0, stats.t.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert stats.guards_intact() and stats.t.cpu().tolist() == [32000.0, 0.0]
