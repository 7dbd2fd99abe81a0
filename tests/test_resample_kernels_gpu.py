"""t2s_resample_table / t2s_resample_batch (csrc/resample.hip, csrc/t2s_api_audio.hip) called directly on guarded buffers, against the
float64 restatement of tests/resample_ref.py (which tests/test_resample_ref_cpu.py compares with scipy.signal.resample_poly).

int16 -> int16 is compared for EQUALITY with rint(reference), saturated: the kernel's sums are double precision, and the CPU test
asserts that no reference sample of these seeded inputs lies within 1e-6 of a half-integer, so nothing is exempt.  Float sources to
float32 are held to
    |got - ref| <= 2^-24 |ref| + (taps per output + 1) 2^-53 sum_k |h| |x|
- one float32 rounding of the result plus the rounding of a double-precision sum of that many terms.

Lengths: 1, 2, one more than the filter reaches, and what gives TILE - 1, TILE, TILE + 1 and 2 TILE + 1 outputs (where the ratio can
give that count; 2 / 1 gives even counts only and takes the next one).  Every source is a view into a larger tensor filled with
+-32767 (or NaN / 1e4), every destination a view into a larger tensor of sentinels which must come back untouched."""
import numpy as np
import pytest
import torch

import resample_ref as R
from text2speech_amd import _lib
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64
I16_SENTINEL, F32_SENTINEL = 12345, 12345.678
NP_OF = {torch.int16: np.int16, torch.float32: np.float32, torch.float16: np.float16}
KIND = {torch.int16: 0, torch.float32: 1, torch.float16: 2}
WORST = {}          # (source dtype) -> worst observed fraction of the float bound


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def tile(lib):
    return lib.t2s_resample_tile()


_FILTERS = {}


def _filter(up, down):
    """(up, down, host h, device h) of a ratio, built once"""
    if (up, down) not in _FILTERS:
        u, d, h = R.filter_ref(up, down)
        _FILTERS[(up, down)] = (u, d, h, torch.from_numpy(h).to(DEV))
    return _FILTERS[(up, down)]


class Buf:
    """A device tensor of n elements inside a larger one: GUARD + shift elements of `fill` in front, GUARD behind."""

    def __init__(self, n, dtype, fill, shift=0):
        self.raw = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device=DEV)
        self.lo = GUARD + shift
        self.t = self.raw[self.lo:self.lo + n]
        self.fill = fill

    def guards_intact(self):
        return bool((self.raw[:self.lo] == self.fill).all()) and bool((self.raw[self.lo + self.t.numel():] == self.fill).all())


def _dst(n, dtype, shift=0):
    return Buf(n, dtype, I16_SENTINEL if dtype == torch.int16 else F32_SENTINEL, shift)


def _table_call(lib, src, rows, up, down, dst, max_out, want_lengths=True):
    """rows: (src_start, src_count, dst_start, dst_cap).  Returns out_lengths (numpy int32) or None."""
    u, d, h, h_d = _filter(up, down)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    lens = torch.full((len(rows),), -77, dtype=torch.int32, device=DEV) if want_lengths else None
    rc = lib.t2s_resample_table(src.data_ptr(), KIND[src.dtype], src.numel(), table.data_ptr(), len(rows), h_d.data_ptr(), h.size,
                                u, d, dst.t.data_ptr(), KIND[dst.t.dtype], dst.t.numel(), max_out,
                                lens.data_ptr() if want_lengths else None, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert dst.guards_intact(), "wrote outside the destination"
    return lens.cpu().numpy() if want_lengths else None


def _alone(lib, clip, up, down, dst_dtype=torch.int16, src_dtype=torch.int16, shift=0):
    """one clip in a pool of its own (neighbours hold the largest value) -> numpy result [n_out]"""
    n = clip.size
    big = 32767 if src_dtype == torch.int16 else 1e4
    src = Buf(n, src_dtype, big, shift)
    src.t.copy_(torch.from_numpy(clip.astype(NP_OF[src_dtype])))
    u, d, _, _ = _filter(up, down)
    n_out = R.out_length(n, u, d)
    dst = _dst(n_out, dst_dtype, shift)
    lens = _table_call(lib, src.t, [(0, n, 0, n_out)], up, down, dst, n_out)
    assert lens.tolist() == [n_out]
    return dst.t.cpu().numpy()


# ---- int16 -> int16: equal to the rounded reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", R.RATIOS)
def test_int16_equals_rounded_reference(lib, tile, up, down):
    for n in R.kernel_lengths(up, down, tile):
        clip = R.clip_int16(1000 * R.RATIOS.index((up, down)) + n % 997, n)
        want = R.to_int16(R.resample_ref(clip, up, down))
        for shift in (0, 1):                                    # both 2-byte parities of source and destination
            got = _alone(lib, clip, up, down, shift=shift)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%d/%d n %d shift %d: %d differ, first at %d: got %d want %d" % (
                up, down, n, shift, bad.size, bad[0], got[bad[0]], want[bad[0]])
    clip = R.clip_int16(77 + R.RATIOS.index((up, down)), 700, 32768)          # full scale: some samples saturate
    assert np.array_equal(_alone(lib, clip, up, down), R.to_int16(R.resample_ref(clip, up, down)))


@pytest.mark.parametrize("up,down", [(64, 63), (1, 2)])
def test_square_wave_saturates_and_never_wraps(lib, up, down):
    clip = R.square_wave(900)
    ref = R.resample_ref(clip, up, down)
    got = _alone(lib, clip, up, down)
    assert np.array_equal(got, R.to_int16(ref))
    over, under = ref > 32767.5, ref < -32768.5
    assert over.any() and under.any(), "the reference overshoots at both ends"
    assert bool((got[over] == 32767).all()) and bool((got[under] == -32768).all())


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.float16])
def test_float_sources_to_int16_round_the_same_way(lib, src_dtype):
    """integer-valued float samples (exact in f32; |x| <= 2048 exact in f16) give the int16 source's result"""
    amp = 20000 if src_dtype == torch.float32 else 2048
    for up, down in ((64, 63), (5, 14)):
        clip = R.clip_int16(31, 1501, amp)
        want = R.to_int16(R.resample_ref(clip, up, down))
        assert np.array_equal(_alone(lib, clip, up, down, src_dtype=src_dtype), want)
    x = np.zeros(120, dtype=np.float32)
    x[0], x[1], x[80] = 1e9, -1e9, np.nan
    got = _alone(lib, x, 1, 2, src_dtype=torch.float32)
    with np.errstate(invalid="ignore"):
        ref = R.resample_ref(x, 1, 2)
    assert np.isnan(ref[40]) and ref[0] > 1e8 and ref[1] < -1e8
    assert np.array_equal(got, R.to_int16(ref)), "NaN gives 0, +-1e9 saturates"
    assert got[40] == 0 and got[0] == 32767 and got[1] == -32768


# ---- several clips in one pool ------------------------------------------------------------------------------------------------------------
def _pool_layout(up, down, seed):
    """clips with gaps of +-32767 between them; destination rows scattered in a shuffled order with gaps"""
    u, d, _, _ = _filter(up, down)
    clips = [R.clip_int16(500 + q, n) for q, n in enumerate(R.POOL_CLIP_LENGTHS)]
    gen = np.random.RandomState(seed)
    src_starts, pos = [], 5
    for c in clips:
        src_starts.append(pos)
        pos += c.size + int(gen.randint(1, 9))
    src_len = pos + 3
    order = gen.permutation(len(clips))
    dst_starts, pos = [0] * len(clips), 3
    for q in order:
        dst_starts[q] = pos
        pos += R.out_length(clips[q].size, u, d) + int(gen.randint(1, 9))
    return clips, src_starts, src_len, dst_starts, pos + 2


@pytest.mark.parametrize("up,down", [(64, 63), (5, 14)])
@pytest.mark.parametrize("dst_dtype", [torch.int16, torch.float32])
def test_pool_clips_are_bit_equal_to_the_clip_alone(lib, up, down, dst_dtype):
    u, d, _, _ = _filter(up, down)
    clips, src_starts, src_len, dst_starts, dst_len = _pool_layout(up, down, 3)
    alone = [_alone(lib, c, up, down, dst_dtype) for c in clips]
    if dst_dtype == torch.int16:
        for c, a in zip(clips, alone):
            assert np.array_equal(a, R.to_int16(R.resample_ref(c, up, down)))
    for shift in (0, 1):                                        # the pool's base at both 2-byte parities
        src = Buf(src_len, torch.int16, 32767, shift)
        src.t[::2] = -32767
        for c, s in zip(clips, src_starts):
            src.t[s:s + c.size].copy_(torch.from_numpy(c))
        dst = _dst(dst_len, dst_dtype, shift)
        rows = [(s, c.size, t, R.out_length(c.size, u, d)) for c, s, t in zip(clips, src_starts, dst_starts)]
        lens = _table_call(lib, src.t, rows, up, down, dst, max(r[3] for r in rows))
        assert lens.tolist() == [r[3] for r in rows]
        got = dst.t.cpu().numpy()
        written = np.zeros(dst_len, dtype=bool)
        for q, (a, t) in enumerate(zip(alone, dst_starts)):
            assert got[t:t + a.size].tobytes() == a.tobytes(), "clip %d (shift %d) differs from the clip alone" % (q, shift)
            written[t:t + a.size] = True
        assert bool((got[~written] == NP_OF[dst_dtype](dst.fill)).all()), "the gaps between the rows were written"


def test_dst_cap_truncates_or_zero_fills_and_out_lengths_count(lib, tile):
    up, down = 64, 63
    u, d, _, _ = _filter(up, down)
    clip = R.clip_int16(9, 1501)
    n_out = R.out_length(clip.size, u, d)
    full = _alone(lib, clip, up, down)
    full32 = _alone(lib, clip, up, down, torch.float32)
    src = Buf(clip.size, torch.int16, 32767)
    src.t.copy_(torch.from_numpy(clip))
    caps = [1, tile - 1, tile, tile + 1, n_out - 1, n_out, n_out + 1, n_out + 700, 2 * tile + 5, 0]
    for dst_dtype, want_full in ((torch.int16, full), (torch.float32, full32)):
        stride = n_out + 800
        dst = _dst(stride * len(caps), dst_dtype)
        rows = [(0, clip.size, q * stride, cap) for q, cap in enumerate(caps)]
        lens = _table_call(lib, src.t, rows, up, down, dst, max(caps))
        got = dst.t.cpu().numpy()
        for q, cap in enumerate(caps):
            row = got[q * stride:(q + 1) * stride]
            v = min(cap, n_out)
            assert lens[q] == v
            assert row[:v].tobytes() == want_full[:v].tobytes(), "cap %d" % cap
            assert row[v:cap].tobytes() == np.zeros(cap - v, dtype=row.dtype).tobytes(), "cap %d: +0 behind the samples" % cap
            assert bool((row[cap:] == NP_OF[dst_dtype](dst.fill)).all()), "cap %d: wrote behind dst_cap" % cap
    # max_out below a row's cap cuts the row there
    dst = _dst(n_out, torch.int16)
    lens = _table_call(lib, src.t, [(0, clip.size, 0, n_out)], up, down, dst, 100)
    got = dst.t.cpu().numpy()
    assert lens.tolist() == [100] and np.array_equal(got[:100], full[:100]) and bool((got[100:] == I16_SENTINEL).all())


def test_any_table_value_is_safe(lib):
    """rows whose source lies outside the pool write only zeros (the pool's neighbours hold +-32767: a read outside would show);
    a count that runs past the pool's end is cut there; rows whose destination lies outside dst write nothing"""
    up, down = 3, 7
    u, d, _, _ = _filter(up, down)
    pool_len, cap = 400, 90
    src = Buf(pool_len, torch.int16, 32767)
    clip = R.clip_int16(12, pool_len)
    src.t.copy_(torch.from_numpy(clip))
    bad_src = [(-1, 50), (-(1 << 40), 50), (pool_len, 50), (pool_len + 7, 5), (1 << 40, 50), (1 << 62, 1 << 62), (10, -1),
               (10, -(1 << 62)), (-(1 << 63), (1 << 63) - 1), (10, 0)]
    cut_src = [(pool_len - 30, 31), (pool_len - 30, 1 << 40), (pool_len - 1, (1 << 63) - 1), (0, 1 << 50)]
    rows = [(s, c, q * cap, cap) for q, (s, c) in enumerate(bad_src + cut_src)]
    n_ok = len(rows)
    dst_len = n_ok * cap
    dst = _dst(dst_len + 40, torch.int16)           # 40 more than the rows above use
    rows += [(0, 100, -1, cap), (0, 100, -(1 << 62), cap), (0, 100, dst_len + 40, cap), (0, 100, 1 << 62, 1 << 62), (0, 100, 5, -3),
             (0, 100, 5, -(1 << 63))]
    rows.append((0, 100, dst_len + 10, 1 << 40))    # a cap that runs past the destination's end is cut there: 30 samples
    lens = _table_call(lib, src.t, rows, up, down, dst, cap)
    got = dst.t.cpu().numpy()
    for q in range(len(bad_src)):
        assert lens[q] == 0 and bool((got[q * cap:(q + 1) * cap] == 0).all()), "row %r" % (rows[q],)
    for q, (s, c) in enumerate(cut_src, len(bad_src)):
        want = R.to_int16(R.resample_ref(clip[s:], up, down))[:cap]
        assert lens[q] == want.size, "row %r" % (rows[q],)
        assert np.array_equal(got[q * cap:q * cap + want.size], want) and bool((got[q * cap + want.size:(q + 1) * cap] == 0).all())
    assert lens[n_ok:n_ok + 6].tolist() == [0] * 6
    assert bool((got[dst_len:dst_len + 10] == I16_SENTINEL).all())
    want = R.to_int16(R.resample_ref(clip[:100], up, down))[:30]
    assert lens[-1] == 30 and np.array_equal(got[dst_len + 10:], want)


# ---- float sources ------------------------------------------------------------------------------------------------------------------------
def _float_clip(seed, n, dtype):
    gen = np.random.RandomState(seed)
    return gen.uniform(-1, 1, n).astype(NP_OF[dtype])


def _check_float(got, clip, up, down, label, key):
    u, d, h, _ = _filter(up, down)
    ref, mag = R.resample_ref(clip, up, down, with_magnitude=True)
    bound = 2.0 ** -24 * np.abs(ref) + (R.taps_per_output(h.size, u) + 1) * 2.0 ** -53 * mag
    err = np.abs(got.astype(np.float64) - ref)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), frac)
    assert bool((err <= bound).all()), "%s: worst fraction of the bound %.3f" % (label, frac)


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("up,down", R.RATIOS)
def test_float_sources_to_float32(lib, tile, src_dtype, up, down):
    for n in R.kernel_lengths(up, down, tile):
        clip = _float_clip(n, n, src_dtype)
        got = _alone(lib, clip, up, down, torch.float32, src_dtype)
        _check_float(got, clip, up, down, "%s %d/%d n %d" % (src_dtype, up, down, n), str(src_dtype))
    print("RESAMPLE %s -> f32 %d/%d: worst observed fraction of the bound so far %.3f" % (src_dtype, up, down, WORST[str(src_dtype)]))


def _batch_call(lib, x, is_half, B, N, ldx, lengths, up, down, N_out, ldo):
    u, d, h, h_d = _filter(up, down)
    out = _dst(B * ldo, torch.float32)
    lens_d = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    out_lens = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    rc = lib.t2s_resample_batch(x.data_ptr(), is_half, B, N, ldx, None if lens_d is None else lens_d.data_ptr(), h_d.data_ptr(), h.size,
                                u, d, out.t.data_ptr(), N_out, ldo, out_lens.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.t.cpu().numpy().reshape(B, ldo)
    assert bool((got[:, N_out:] == np.float32(F32_SENTINEL)).all()), "columns N_out .. ldo were written"
    return got[:, :N_out], out_lens.cpu().numpy()


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("up,down", [(64, 63), (5, 14), (2, 1)])
def test_batch_rows_equal_the_row_alone(lib, src_dtype, up, down):
    u, d, _, _ = _filter(up, down)
    N, ldx = 1500, 1503
    lengths = [1500, 700, 1, 0]
    B = len(lengths)
    N_out, ldo = R.out_length(N, u, d), R.out_length(N, u, d) + 5
    rows = [_float_clip(40 + b, N, src_dtype) for b in range(B)]
    x = Buf(B * ldx, src_dtype, 1e4)
    xv = x.t.view(B, ldx)
    for b, n in enumerate(lengths):
        xv[b, :N].copy_(torch.from_numpy(rows[b]))
        xv[b, n:N:2] = float("nan")                             # NaN and 1e4 behind each entry's end
        xv[b, n + 1:N:2] = 1e4
    is_half = int(src_dtype == torch.float16)
    got, out_lens = _batch_call(lib, x.t, is_half, B, N, ldx, lengths, up, down, N_out, ldo)
    for b, n in enumerate(lengths):
        v = R.out_length(n, u, d)
        assert out_lens[b] == v
        assert not np.isnan(got[b]).any() and bool((got[b, v:] == 0).all()) and not np.signbit(got[b, v:]).any()
        if n:
            alone = _alone(lib, rows[b][:n], up, down, torch.float32, src_dtype)
            assert got[b, :v].tobytes() == alone.tobytes(), "entry %d differs from the entry alone" % b
            _check_float(got[b, :v], rows[b][:n], up, down, "batch entry %d" % b, str(src_dtype))
    # lengths = NULL is every row at N; -3 and N + 5 are clamped to 0 and N
    for b in range(B):
        xv[b, :N].copy_(torch.from_numpy(rows[b]))
    full, full_lens = _batch_call(lib, x.t, is_half, B, N, ldx, [N] * B, up, down, N_out, ldo)
    null, null_lens = _batch_call(lib, x.t, is_half, B, N, ldx, None, up, down, N_out, ldo)
    assert full.tobytes() == null.tobytes() and full_lens.tolist() == null_lens.tolist() == [N_out] * B
    clamped, clamped_lens = _batch_call(lib, x.t, is_half, B, N, ldx, [-3, N + 5, N, -(1 << 31)], up, down, N_out, ldo)
    assert clamped_lens.tolist() == [0, N_out, N_out, 0]
    assert bool((clamped[0] == 0).all()) and bool((clamped[3] == 0).all())
    assert clamped[1].tobytes() == full[1].tobytes() and clamped[2].tobytes() == full[2].tobytes()
    # the same call twice: the same bits
    again, _ = _batch_call(lib, x.t, is_half, B, N, ldx, None, up, down, N_out, ldo)
    assert again.tobytes() == null.tobytes()


def test_two_identical_table_calls_give_identical_bits(lib):
    clip = R.clip_int16(5, 3000, 32768)
    for dst_dtype in (torch.int16, torch.float32):
        a = _alone(lib, clip, 160, 147, dst_dtype)
        b = _alone(lib, clip, 160, 147, dst_dtype)
        assert a.tobytes() == b.tobytes()


def test_largest_factor_uses_the_large_lds_table(lib):
    """max(up, down) = 512: the 84 KB phase table (above the 64 KB that needs no opt-in), in both directions"""
    for up, down in ((512, 511), (3, 512)):
        clip = R.clip_int16(21, 2100 if up == 512 else 40000)
        got = _alone(lib, clip, up, down, torch.float32)
        _check_float(got, clip, up, down, "%d/%d" % (up, down), "int16")
