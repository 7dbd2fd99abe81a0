"""The PCM kernels with a row, a source or a destination beyond element 2^31 / byte 2^32 of its buffer: include/t2s_hip.h promises
64-bit clamps, tables and strides (`long src_len`, `long ldx / ldo / ld_row / ld_entry / ldp / ld_dst / dst_off`), and every kernel of
these families forms its pointers as (size_t) row * stride or src + start.  One int or unsigned in such an expression reads another
clip or writes into one, and no other test places data that far.

Placement (tests/far_util.py; the rows are tests/far_cases.py's; both checked by tests/test_far_util_cpu.py): one raw buffer of 2^33 + 2^20 bytes from torch.empty, never
filled as a whole, viewed as int16 / f16 / f32 from a base 2^19 bytes into it.  Row A is near, row B starts at element 2^32 + k
(2-byte kinds) or 2^30 + k (f32: byte 2^32 + 4 k), row C starts 700 elements before that line and runs across it.  Wherever an index
of a far row lands when it - or its byte offset - is cut to 32 bits, unsigned or signed, there is a decoy window: other samples for a
source, sentinels for a destination.  A truncated index therefore fails an assert and never leaves the allocation.  A case is far on
one side only (far source and small destination, or the reverse), so the peak stays under 10 GiB.

Asserted per entry point: (a) rows A, B and C - samples, statistics, counts, out_lengths - are bit for bit those of the same call
on the same samples in a small buffer; (b) that near result passes the float64 comparison of the entry point's own test module at
that module's bars (imported, not restated; the CPU test asserts the decision margins of these seeds); (c) every decoy and every
guard window (1024 elements around each row and decoy, the buffer's first and last 1024) is untouched.  No row is exempt.

Out of scope: rows longer than 2^31 samples; WaveGlow / Tacotron plane tensors past 2^32 bytes (tens of GB and seconds of GEMM);
t2s_wg_noise_keyed at B G L > 2^31."""
import types

import numpy as np
import pytest
import torch

import align_ref
import audio_ragged_ref
import data_ref
import far_cases as FC
import far_util as FU
import filter_ref as FR
import join_ref
import limiter_ref as MR
import loudness_ref as LR
import resample_ref as RR
import test_filter_kernels_gpu as FK
import test_join_kernels_gpu as JK
import test_limiter_kernels_gpu as MK
import test_loudness_kernels_gpu as LK
import test_resample_kernels_gpu as RK
import test_streaming_kernels_gpu as SK
import test_trim_kernels_gpu as TK
import test_warp_kernels_gpu as WK
import trim_ref as TR
from text2speech_amd import _lib
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

W = FU.WINDOW
TORCH_OF = {"int16": torch.int16, "float16": torch.float16, "float32": torch.float32, "int32": torch.int32}
SRC_FILL = {"int16": (32767, -32767), "int32": (1 << 30, -7), "float16": (1e4, float("nan")), "float32": (1e4, float("nan"))}
OUT_OF = FC.OUT_KIND
BITS = {2: torch.int16, 4: torch.int32}
I16_FILL, F32_FILL = 12345, 12345.678


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.t2s_loud_tile() == LR.TILE and lib.t2s_limit_tile() == MR.TILE and lib.t2s_sos_tile() == FR.TILE
    return lib


@pytest.fixture(scope="module")
def big():
    """the raw buffer, allocated once and freed at the module's end"""
    torch.cuda.reset_peak_memory_stats()
    raw = torch.empty(FU.BUF_BYTES, dtype=torch.uint8, device=DEV)
    yield raw
    torch.cuda.synchronize()
    print("FAR OFFSETS: peak torch.cuda.max_memory_allocated() %.3f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))
    del raw
    torch.cuda.empty_cache()


def _noise(seed, n, kind):
    gen = np.random.RandomState(seed)
    if kind in ("int16", "int32"):
        return gen.randint(-20000, 20000, n).astype(FU.NP_OF[kind])
    return gen.uniform(-1, 1, n).astype(FU.NP_OF[kind])


def _bits(t):
    return t.view(BITS[t.element_size()])


class Far:
    """The big buffer as one kind, where the kernel tests' Buf is expected: `.t` is the view from the base to the buffer's end (what
    a kernel gets as src or dst, with its length), starts are elements from that base.  A source holds the clips at the layout's
    rows, other samples in every decoy and the largest values around both; a destination holds sentinels there."""

    def __init__(self, raw, kind, counts, clips=None):
        self.kind, self.dtype = kind, TORCH_OF[kind]
        size = FU.ITEMSIZE[kind]
        self.lay = FU.layout(size, counts)
        FU.check_layout(self.lay)
        self.whole = raw.view(self.dtype)
        self.base = FU.BASE_BYTES // size
        self.t = self.whole[self.base:]
        self.rows = list(zip(self.lay.starts, counts))
        self.is_source = clips is not None
        spans = self.rows + list(self.lay.decoys)
        self.windows = [(s - W, s + n + W) for s, n in spans] + [(-self.base, -self.base + W), (self.t.numel() - W, self.t.numel())]
        if self.is_source:
            self.fill, other = SRC_FILL[kind]
            for lo, hi in self.windows:
                self._at(lo, hi).fill_(self.fill)
                self._at(lo, hi)[::2] = other
            for q, (s, n) in enumerate(self.lay.decoys):
                self._at(s, s + n).copy_(torch.from_numpy(_noise(9000 + q, n, kind)))
            for (s, n), c in zip(self.rows, clips):
                assert c.size == n
                self._at(s, s + n).copy_(torch.from_numpy(c))
            self.kept = [_bits(self._at(lo, hi)).clone() for lo, hi in self.windows]
        else:
            self.fill = I16_FILL if kind == "int16" else F32_FILL
            for lo, hi in self.windows:
                self._at(lo, hi).fill_(self.fill)
        torch.cuda.synchronize()

    def _at(self, lo, hi):
        return self.whole[self.base + lo:self.base + hi]

    def guards_intact(self):
        """a source: every window holds the bits it was given; a destination: sentinels everywhere outside the rows"""
        for k, (lo, hi) in enumerate(self.windows):
            if self.is_source:
                if not torch.equal(_bits(self._at(lo, hi)), self.kept[k]):
                    return False
                continue
            cur = self._at(lo, hi).cpu().numpy()
            free = np.ones(cur.size, dtype=bool)
            for s, n in self.rows:
                free[max(0, s - lo):max(0, s + n - lo)] = False
            if not bool((cur[free] == cur.dtype.type(self.fill)).all()):
                return False
        return True

    def row(self, q):
        s, n = self.rows[q]
        return self.t[s:s + n].cpu().numpy()


class Near:
    """The same three rows in a small buffer of the kernel tests' kind: odd starts, a few sentinels between the rows"""

    def __init__(self, kind, counts, clips=None):
        self.kind, dtype = kind, TORCH_OF[kind]
        starts, pos = [], 5
        for n in counts:
            starts.append(pos)
            pos += n + 6 + (pos & 1)
        self.rows = list(zip(starts, counts))
        if clips is not None:
            self.buf = LK._src_buf(pos + 3, dtype, 1)
            for (s, n), c in zip(self.rows, clips):
                self.buf.t[s:s + n].copy_(torch.from_numpy(c))
        else:
            self.buf = LK._dst(pos + 3, dtype, 1)
        self.t, self.fill = self.buf.t, self.buf.fill
        self.is_source = clips is not None

    def guards_intact(self):
        if not self.buf.guards_intact():
            return False
        if self.is_source:
            return True
        cur = self.t.cpu().numpy()
        free = np.ones(cur.size, dtype=bool)
        for s, n in self.rows:
            free[s:s + n] = False
        return bool((cur[free] == cur.dtype.type(self.fill)).all())

    def row(self, q):
        s, n = self.rows[q]
        return self.t[s:s + n].cpu().numpy()


def _rows4(src, dst):
    return [(s, c, d, cap) for (s, c), (d, cap) in zip(src.rows, dst.rows)]


# ---- the table-addressed entry points: run(lib, kind, src, dst) -> a dict of per-row results; check(kind, clips, result) --------------
class Resample:
    name, case = "resample_table", "resample"

    @staticmethod
    def run(lib, kind, src, dst):
        up, down = FC.RESAMPLE_RATIOS[kind]
        rows4 = _rows4(src, dst)
        return dict(lens=RK._table_call(lib, src.t, rows4, up, down, dst, max(r[3] for r in rows4)))

    @staticmethod
    def check(kind, clips, res):
        up, down = FC.RESAMPLE_RATIOS[kind]
        for q, c in enumerate(clips):
            v = int(res["lens"][q])
            if kind == "int16":
                want = RR.to_int16(RR.resample_ref(c, up, down))
                assert v == want.size and np.array_equal(res["outs"][q][:v], want), "row %d" % q
            else:
                assert v == RR.out_length(c.size, *RR.filter_ref(up, down)[:2])
                RK._check_float(res["outs"][q][:v], c, up, down, "far rows %s row %d" % (kind, q), "far " + kind)


class Trim:
    name, case = "trim_energy_bounds_gather", "trim"

    @staticmethod
    def run(lib, kind, src, dst):
        fl, h, mode, d = FC.TRIM
        E, st, found, (stats, bounds_d) = TK.run(lib, src.t, src.rows, fl, h, mode, (d,))
        rows4 = _rows4(src, dst)
        lens = TK.gather(lib, src.t, rows4, bounds_d[d], stats, d[1], dst, max(r[3] for r in rows4))
        return dict(lens=lens, energy=E, stats=st, bounds=found[d])

    @staticmethod
    def check(kind, clips, res):
        fl, h, mode, d = FC.TRIM
        cut = 0
        for q, c in enumerate(clips):
            want_E = TR.frame_energies(c, fl, h, mode)
            E, st = res["energy"][q], res["stats"][q]
            assert E.size == want_E.size
            if kind == "int16":
                assert np.array_equal(E, want_E) and st[0] == float(np.abs(c.astype(np.int32)).max()) and st[1] == want_E.max()
            else:
                rel = float((np.abs(E - want_E) / np.maximum(want_E, 1e-300)).max())
                # (the bar of tests/test_trim_kernels_gpu.py:223, test_float_sources - an inline expression there)
                assert rel <= (fl + 1) * 2.0 ** -53, "row %d: energies off by %.3e relative" % (q, rel)
                assert st[0] == float(np.abs(c.astype(np.float64)).max()) and st[1] == E.max()
            s, e = TR.trim_bounds(c, fl, h, mode, d[0], d[1])
            assert tuple(int(v) for v in res["bounds"][q]) == (s, e) and int(res["lens"][q]) == e - s, "row %d" % q
            want = TR.rescale(c, d[1])[s:e]
            got = res["outs"][q]
            assert got.dtype == want.dtype and got[:e - s].tobytes() == want.tobytes(), "row %d: output bits" % q
            cut += (s, e) != (0, c.size)
        assert cut, "some row must be cut"


class Loud:
    name, case = "loud_measure_apply", "loud"

    @staticmethod
    def run(lib, kind, src, dst):
        st, ct, stats = LK.measure(lib, src.t, src.rows, FC.LOUD_FS)
        rows4 = _rows4(src, dst)
        lens = LK.apply(lib, src.t, rows4, stats, dst, max(r[3] for r in rows4))
        return dict(lens=lens, stats=st, counts=ct)

    @staticmethod
    def check(kind, clips, res):
        for q, c in enumerate(clips):
            want = LK._check_row("far rows %s row %d" % (kind, q), c, FC.LOUD_FS, res["stats"][q], res["counts"][q])
            assert want["flags"] == 0 and int(res["lens"][q]) == c.size
            g = float(res["stats"][q, 3])
            out = LR.apply_int16(c, g) if kind == "int16" else LR.apply_float(c, g)
            assert res["outs"][q][:c.size].tobytes() == out.tobytes(), "row %d: applied samples" % q


class Limit:
    name, case = "limit_measure_apply", "limit"

    @staticmethod
    def run(lib, kind, src, dst):
        st, ct, counts = MK.measure(lib, src.t, src.rows, FC.LIMIT_OS, FC.LIMIT_L)
        rows4 = _rows4(src, dst)
        lens = MK.apply(lib, src.t, rows4, FC.LIMIT_OS, FC.LIMIT_L, counts, dst, max(r[3] for r in rows4))
        return dict(lens=lens, stats=st, counts=ct)

    @staticmethod
    def check(kind, clips, res):
        for q, c in enumerate(clips):
            assert int(res["lens"][q]) == c.size
            ref = MK._check_row("far rows %s row %d" % (kind, q), c, FC.LIMIT_OS, FC.LIMIT_L, 1.0, res["stats"][q], res["counts"][q],
                                res["outs"][q][:c.size])
            assert ref.counts[0] > 0, "row %d is limited" % q


class Sos:
    name, case = "sos_filter", "sos"
    sos = FR.sections_case(FC.SOS_SECTIONS)

    @staticmethod
    def run(lib, kind, src, dst):
        return dict(counts=FK.run_filter(lib, src.t, _rows4(src, dst), Sos.sos, dst))

    @staticmethod
    def check(kind, clips, res):
        for q, c in enumerate(clips):
            ref, term = FK._E_G(Sos.sos, c, 1.0)
            case = "far rows %s row %d" % (kind, q)
            got = res["outs"][q][:c.size]
            assert res["counts"][q, 0] == 0
            if kind == "int16":
                FK._check_i16(case, got, ref, term)         # its default share of exempt samples, the accuracy cases' 1e-3
                # the clipped count: only a sample within the bar of a half-integer may round to the other side of saturation
                assert abs(int(res["counts"][q, 1]) - FR.round16(ref)[1]) <= int(np.count_nonzero(FR.int16_exempt(ref, term))), case
            else:
                FK._check_f32(case, got, ref, term)


TABLE_EPS = (Resample, Trim, Loud, Limit, Sos)
PAD = FC.PAD
_NEAR = {}


def _finish(res, dst, counts):
    """the rows of the destination, and +0 in the PAD behind each row's samples"""
    res["outs"] = [dst.row(q) for q in range(3)]
    for q, n in enumerate(counts):
        tail = res["outs"][q][n:] if "lens" not in res else res["outs"][q][int(res["lens"][q]):]
        assert tail.size >= PAD and not np.any(tail) and not np.any(np.signbit(tail.astype(np.float64))), "row %d: +0 behind the samples" % q
    return res


def _near(lib, ep, kind):
    """(clips, output counts, result) of the three rows in small buffers, held to the float64 reference; computed once"""
    if (ep.name, kind) not in _NEAR:
        clips = FC.table_clips(ep.case, kind, lib.t2s_resample_tile(), lib.t2s_trim_tile())
        counts = FC.table_out_counts(ep.case, kind, clips)
        src = Near(kind, [c.size for c in clips], clips)
        dst = Near(OUT_OF[kind], [n + PAD for n in counts])
        res = _finish(ep.run(lib, kind, src, dst), dst, counts)
        assert src.guards_intact() and dst.guards_intact()
        ep.check(kind, clips, res)
        _NEAR[(ep.name, kind)] = (clips, counts, res)
    return _NEAR[(ep.name, kind)]


def _assert_same(far, near, label):
    assert sorted(far) == sorted(near)
    for key in near:
        a, b = far[key], near[key]
        for q in range(3):
            assert a[q].dtype == b[q].dtype and a[q].shape == b[q].shape and a[q].tobytes() == b[q].tobytes(), \
                "%s: %s of row %s differs from the same row placed near" % (label, key, "ABC"[q])


@pytest.mark.parametrize("side", ("src", "dst"))
@pytest.mark.parametrize("kind", ("int16", "float16"))
@pytest.mark.parametrize("ep", TABLE_EPS, ids=lambda e: e.name)
def test_table_addressed_rows_far_in_the_buffer(lib, big, ep, kind, side):
    clips, counts, near = _near(lib, ep, kind)
    if side == "src":
        src = Far(big, kind, [c.size for c in clips], clips)
        dst = Near(OUT_OF[kind], [n + PAD for n in counts])
    else:
        src = Near(kind, [c.size for c in clips], clips)
        dst = Far(big, OUT_OF[kind], [n + PAD for n in counts])
    far = _finish(ep.run(lib, kind, src, dst), dst, counts)
    assert src.guards_intact(), "a source, a decoy or a guard window changed"
    assert dst.guards_intact(), "a store outside the rows: a decoy or a guard window of the destination changed"
    _assert_same(far, near, "%s %s far %s" % (ep.name, kind, side))


def test_a_row_addressed_at_its_truncated_start_is_noticed(lib, big):
    """The check of the checks, without touching a kernel: the table itself names the spot that 32 bits cut row B's start to.  As a
    source the row then reads its decoy and its statistics and samples differ; as a destination it lands in the decoy's sentinels
    and the guard check reports it."""
    ep, kind = Loud, "int16"
    clips, counts, near = _near(lib, ep, kind)
    src = Far(big, kind, [c.size for c in clips], clips)
    dst = Near(OUT_OF[kind], [n + PAD for n in counts])
    (spot,) = FU.truncations(src.rows[1][0], FU.ITEMSIZE[kind])
    src.rows[1] = (spot, src.rows[1][1])
    far = _finish(ep.run(lib, kind, src, dst), dst, counts)
    for q in (0, 2):
        assert far["outs"][q].tobytes() == near["outs"][q].tobytes() and far["stats"][q].tobytes() == near["stats"][q].tobytes()
    assert far["outs"][1].tobytes() != near["outs"][1].tobytes() and far["stats"][1].tobytes() != near["stats"][1].tobytes()
    src = Near(kind, [c.size for c in clips], clips)
    dst = Far(big, OUT_OF[kind], [n + PAD for n in counts])
    honest = list(dst.rows)
    (spot,) = FU.truncations(honest[1][0], FU.ITEMSIZE[OUT_OF[kind]])
    dst.rows = [honest[0], (spot, honest[1][1]), honest[2]]
    far = _finish(ep.run(lib, kind, src, dst), dst, counts)
    assert far["outs"][1].tobytes() == near["outs"][1].tobytes(), "the samples themselves are right, in the wrong place"
    dst.rows = honest
    assert not dst.guards_intact(), "stores into a decoy window go unseen"


# ---- t2s_pcm16_gather: a far pool, then rows of the output far through ldo ---------------------------------------------------------
def _gather(lib, pool, rows, N, out_t, ldo):
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    rc = lib.t2s_pcm16_gather(pool.data_ptr(), pool.numel(), table.data_ptr(), len(rows), N, 32768.0, out_t.data_ptr(), ldo, _st())
    assert rc == 0
    torch.cuda.synchronize()


def test_pcm16_gather_from_a_far_pool(lib, big):
    clips = FC.gather_clips()
    N = FC.GATHER_N
    src = Far(big, "int16", [c.size for c in clips], clips)
    out = LK._dst(3 * (N + 3), torch.float32)
    rows = [(s, n - 7 * q) for q, (s, n) in enumerate(src.rows)]       # counts N + 1, N - 3, N - 3: row A is cut at N, B and C are padded
    _gather(lib, src.t, rows, N, out.t, N + 3)
    assert out.guards_intact() and src.guards_intact()
    got = out.t.cpu().numpy().reshape(3, N + 3)
    assert bool((got[:, N:] == np.float32(F32_FILL)).all()), "columns N .. ldo were written"
    whole = np.concatenate(clips)
    near_rows, pos = [], 0
    for (_, cnt), c in zip(rows, clips):
        near_rows.append((pos, cnt))
        pos += c.size
    want = data_ref.pcm16_gather_ref(whole, near_rows, N)
    assert all(cnt <= c.size for (_, cnt), c in zip(rows, clips))
    assert got[:, :N].view(np.int32).tobytes() == want.view(np.int32).tobytes()


@pytest.mark.parametrize("second", ("B", "C"))
def test_pcm16_gather_into_rows_far_apart(lib, big, second):
    """B = 2: the second output row lies ldo floats behind the first - beyond byte 2^32, or across it"""
    clips = FC.gather_clips()[:2]
    N = FC.GATHER_N
    dst = Far(big, "float32", [N, N, N + 900])
    a, b = dst.lay.starts[0], dst.lay.starts[1 if second == "B" else 2]
    ldo = b - a
    pool = LK._src_buf(sum(c.size for c in clips), torch.int16)
    pool.t.copy_(torch.from_numpy(np.concatenate(clips)))
    rows = [(0, N - 5), (clips[0].size, N)]
    dst.rows = [(a, N), (b, N)]
    _gather(lib, pool.t, rows, N, dst.t[a:], ldo)
    assert dst.guards_intact(), "a store outside the two rows"
    want = data_ref.pcm16_gather_ref(np.concatenate(clips), rows, N)
    got = np.stack([dst.row(0), dst.row(1)])
    assert got.view(np.int32).tobytes() == want.view(np.int32).tobytes()


# ---- the row-strided entry points: B = 2, the second row (entry, piece) far behind the first through the stride ---------------------
class Pair:
    """Two blocks of `count` elements in the big buffer: the first at row A, the second at row B (second = "B") or at the straddling
    row C.  `.t` starts at the first block, `.ld` is the distance; a source holds `blocks`, a destination sentinels."""

    def __init__(self, raw, kind, count, second, blocks=None):
        counts = FC.pair_counts(count)
        clips = None
        if blocks is not None:
            assert blocks[0].size == blocks[1].size == count
            clips = [blocks[0], blocks[1], np.concatenate([blocks[1], _noise(77, counts[2] - count, kind)])]
        self.far = Far(raw, kind, counts, clips)
        a, b = self.far.lay.starts[0], self.far.lay.starts[1 if second == "B" else 2]
        self.far.rows = [(a, count), (b, count)]            # what a destination's stores may touch
        self.t, self.ld, self.fill = self.far.t[a:], b - a, self.far.fill

    def guards_intact(self):
        return self.far.guards_intact()

    def block(self, q):
        return self.far.row(q)


class NearPair:
    """the same two blocks count + 7 elements apart in a small buffer"""

    def __init__(self, kind, count, blocks=None):
        self.ld, self.count = count + 7, count
        n = self.ld + count
        if blocks is None:
            self.buf = LK._dst(n, TORCH_OF[kind], 1)
        else:
            self.buf = LK.Buf(n, TORCH_OF[kind], SRC_FILL[kind][0], 1)
            self.buf.t[::2] = SRC_FILL[kind][1]
        self.t, self.fill = self.buf.t, self.buf.fill
        if blocks is not None:
            for q in range(2):
                self.t[q * self.ld:q * self.ld + count].copy_(torch.from_numpy(blocks[q]))
        self.is_source = blocks is not None

    def guards_intact(self):
        gap = self.t[self.count:self.ld].cpu().numpy()
        return self.buf.guards_intact() and (self.is_source or bool((gap == gap.dtype.type(self.fill)).all()))

    def block(self, q):
        return self.t[q * self.ld:q * self.ld + self.count].cpu().numpy()


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _poisoned(shape, dtype):
    x = np.empty(shape, dtype=dtype)
    x.reshape(-1)[0::2] = np.nan
    x.reshape(-1)[1::2] = 1e4
    return x


class Pcm16:
    name, src_kind, dst_kind, dst_count = "pcm16 ldx", "float16", None, 0
    N, lengths = FC.PCM16_N, [FC.PCM16_N - 3, FC.PCM16_N]

    @classmethod
    def blocks(cls, lib):
        return list((np.random.RandomState(5100).uniform(-1, 1, (2, cls.N)) * 0.999).astype(np.float16))

    @classmethod
    def run(cls, lib, src, dst):
        out = LK._dst(2 * cls.N, torch.int16)
        lens = _i32(cls.lengths)
        assert lib.t2s_pcm16(src.t.data_ptr(), 1, 2, cls.N, src.ld, lens.data_ptr(), out.t.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert out.guards_intact()
        return dict(out=out.t.cpu().numpy().reshape(2, cls.N))

    @classmethod
    def check(cls, lib, blocks, res):
        assert np.array_equal(res["out"], audio_ragged_ref.pcm16_ref(np.stack(blocks), cls.lengths))


class ResampleBatch:
    name, src_kind, dst_kind = "resample_batch", "float16", "float32"

    @classmethod
    def shape(cls, lib):
        up, down, n = FC.resample_rows(lib.t2s_resample_tile())
        return up, down, n, RR.out_length(n, up, down), [n, n - 7]

    @classmethod
    def blocks(cls, lib):
        n = cls.shape(lib)[2]
        return list(np.random.RandomState(5200).uniform(-1, 1, (2, n)).astype(np.float16))

    @classmethod
    def dst_count(cls, lib):
        return cls.shape(lib)[3]

    @classmethod
    def run(cls, lib, src, dst):
        up, down, n, n_out, lengths = cls.shape(lib)
        u, d, h, h_d = RK._filter(up, down)
        lens, out_lens = _i32(lengths), _i32([-77, -77])
        assert lib.t2s_resample_batch(src.t.data_ptr(), 1, 2, n, src.ld, lens.data_ptr(), h_d.data_ptr(), h.size, u, d, dst.t.data_ptr(),
                                      n_out, dst.ld, out_lens.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        return dict(lens=out_lens.cpu().numpy(), rows=np.stack([dst.block(0), dst.block(1)]))

    @classmethod
    def check(cls, lib, blocks, res):
        up, down, n, n_out, lengths = cls.shape(lib)
        for b, ln in enumerate(lengths):
            v = RR.out_length(ln, up, down)
            assert res["lens"][b] == v and not res["rows"][b, v:].view(np.uint32).any(), "+0 behind the row's samples"
            RK._check_float(res["rows"][b, :v], blocks[b][:ln], up, down, "far %s row %d" % (cls.name, b), "far float16")


class ResampleWindow(ResampleBatch):
    """one window that is the whole row: a new stream, K0 = M0 = 0, final"""
    name = "resample_window"

    @classmethod
    def run(cls, lib, src, dst):
        up, down, n, n_out, _ = cls.shape(lib)
        u, d, h, h_d = RK._filter(up, down)
        Cn = lib.t2s_resample_window_carry(h.size, u)
        assert lib.t2s_resample_window_end(n, 0, h.size, u, d, 1) == n_out
        carry = [LK.Buf(2 * Cn, torch.float32, 1e4), LK.Buf(2 * Cn, torch.float32, 1e4)]
        assert lib.t2s_resample_window(carry[0].t.data_ptr(), carry[1].t.data_ptr(), src.t.data_ptr(), 1, 2, n, src.ld, 0, 0, 1,
                                       h_d.data_ptr(), h.size, u, d, dst.t.data_ptr(), n_out, dst.ld, _st()) == 0
        torch.cuda.synchronize()
        assert carry[0].untouched() and carry[1].guards_intact()
        return dict(carry=carry[1].t.cpu().numpy(), rows=np.stack([dst.block(0), dst.block(1)]))

    @classmethod
    def check(cls, lib, blocks, res):
        up, down, n, n_out, _ = cls.shape(lib)
        Cn = res["carry"].size // 2
        for b in range(2):
            RK._check_float(res["rows"][b], blocks[b], up, down, "far %s row %d" % (cls.name, b), "far float16")
            assert res["carry"].reshape(2, Cn)[b].tobytes() == blocks[b][n - Cn:].astype(np.float32).tobytes(), "the next carry"


class LimitWindow:
    """one window that is the whole row; the state then holds t2s_limit_measure's statistics and counts"""
    name, src_kind, dst_kind = "limit_window", "float16", "float32"
    n = 2 * MR.TILE + 77

    @classmethod
    def blocks(cls, lib):
        return [MR.clip(cls.n, 5300 + b, "float16", FC.LIMIT_L) for b in range(2)]

    @classmethod
    def dst_count(cls, lib):
        return cls.n

    @classmethod
    def run(cls, lib, src, dst):
        L, os, n = FC.LIMIT_L, FC.LIMIT_OS, cls.n
        h, w = MK._hw(os, L)
        Cn = lib.t2s_limit_window_carry(L, MK.HW)
        assert lib.t2s_limit_window_end(n, 0, L, MK.HW, 1) == n
        carry = [LK.Buf(2 * Cn, torch.float32, 1e4), LK.Buf(2 * Cn, torch.float32, 1e4)]
        state = LK.Buf(10, torch.int64, -99)
        state.t.view(2, 5).copy_(torch.tensor([0, 0, 0x3FF0000000000000, 0, 0], dtype=torch.int64))
        assert lib.t2s_limit_window(carry[0].t.data_ptr(), carry[1].t.data_ptr(), src.t.data_ptr(), 1, 2, n, src.ld, 0, 0, 1, None,
                                    h.t.data_ptr(), h.t.numel(), os, MK.HW, w.t.data_ptr(), L, MK.C, dst.t.data_ptr(), n, dst.ld,
                                    state.t.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert carry[0].untouched() and carry[1].guards_intact() and state.guards_intact()
        st = state.t.view(2, 5).cpu()
        return dict(stats=st[:, :4].contiguous().view(torch.float64).numpy(), counts=st[:, 4:].contiguous().view(torch.int32).numpy(),
                    rows=np.stack([dst.block(0), dst.block(1)]))

    @classmethod
    def check(cls, lib, blocks, res):
        for b in range(2):
            ref = MK._check_row("far %s row %d" % (cls.name, b), blocks[b], FC.LIMIT_OS, FC.LIMIT_L, 1.0, res["stats"][b],
                                res["counts"][b], res["rows"][b])
            assert ref.counts[0] > 0


class SosWindow:
    name, src_kind, dst_kind = "sos_window", "float16", "float32"
    n = 2 * FR.TILE + 777

    @classmethod
    def blocks(cls, lib):
        return list((0.4 * np.random.RandomState(5400).randn(2, cls.n)).astype(np.float16))

    @classmethod
    def dst_count(cls, lib):
        return cls.n

    @classmethod
    def run(cls, lib, src, dst):
        n, n_sec = cls.n, FC.SOS_SECTIONS
        tab = FK._tab(Sos.sos)
        words = lib.t2s_sos_window_carry(n_sec) // 8
        carry = [LK.Buf(2 * words, torch.float64, -3.5), LK.Buf(2 * words, torch.float64, -3.5)]
        carry[0].t.zero_()
        counts = torch.zeros(4, dtype=torch.int32, device=DEV)
        need = lib.t2s_sos_scratch(2, n, n_sec)
        scratch = LK.Buf(need, torch.float64, -3.5)
        assert lib.t2s_sos_window(carry[0].t.data_ptr(), carry[1].t.data_ptr(), src.t.data_ptr(), 1, 2, n, src.ld, 0, None,
                                  tab.t.data_ptr(), n_sec, scratch.t.data_ptr(), need, dst.t.data_ptr(), dst.ld, counts.data_ptr(),
                                  _st()) == 0
        torch.cuda.synchronize()
        assert carry[1].guards_intact() and scratch.guards_intact() and tab.guards_intact()
        return dict(counts=counts.cpu().numpy().reshape(2, 2), carry=carry[1].t.cpu().numpy(), rows=np.stack([dst.block(0), dst.block(1)]))

    @classmethod
    def check(cls, lib, blocks, res):
        for b in range(2):
            ref, term = FK._E_G(Sos.sos, blocks[b], 1.0)
            FK._check_f32("far %s row %d" % (cls.name, b), res["rows"][b], ref, term)
        assert not res["counts"].any()


class JoinGather:
    name, src_kind, dst_kind, dst_count = "join_gather ldx", "float16", None, 0
    N, lengths, gap, fade = FC.JOIN_N, [FC.JOIN_N - 3, FC.JOIN_N], 5, 8

    @classmethod
    def blocks(cls, lib):
        assert cls.N > 2 * lib.t2s_join_tile()
        return list(np.random.RandomState(5500).uniform(-1, 1, (2, cls.N)).astype(np.float16))

    @classmethod
    def run(cls, lib, src, dst):
        dst_cap = sum(cls.lengths) + cls.gap + 37
        out = JK.Buf(dst_cap, torch.float32, float("nan"))
        off, length = JK.scan(lib, cls.lengths, [cls.N] * 2, None, None, cls.gap, out, dst_cap)
        lens, pos = _i32(cls.lengths), _i32([0, 1])
        assert lib.t2s_join_gather(src.t.data_ptr(), 2, 2, cls.N, src.ld, lens.data_ptr(), pos.data_ptr(), off.t.data_ptr(), 2, cls.fade, 0,
                                   out.t.data_ptr(), dst_cap, _st()) == 0
        torch.cuda.synchronize()
        assert out.guards_intact() and off.guards_intact()
        return dict(out=out.t.cpu().numpy(), length=np.asarray(length))

    @classmethod
    def check(cls, lib, blocks, res):
        rows = [np.where(np.arange(cls.N) < ln, x, np.float16(np.nan)) for x, ln in zip(blocks, cls.lengths)]
        want, want_len, _ = join_ref.join(rows, cls.lengths, None, None, cls.gap, cls.fade, False, dst_cap=res["out"].size)
        assert int(res["length"]) == want_len
        JK._same_bits(res["out"], want)


class AlignRows:
    """ld_entry carries the distance: two entries of N rows, ld_row apart"""
    name, src_kind, dst_kind, dst_count = "align_rows ld_entry", "float16", None, 0
    B, (N, T, ld_row) = 2, FC.ALIGN
    in_len, out_len = [FC.ALIGN[1], FC.ALIGN[1] - 10], [FC.ALIGN[0], FC.ALIGN[0] - 1]

    @classmethod
    def A(cls):
        return align_ref.random_alignments(cls.B, cls.N, cls.T, np.float16, 5600, cls.in_len)

    @classmethod
    def blocks(cls, lib):
        wide = _poisoned((cls.B, cls.N, cls.ld_row), np.float16)
        wide[:, :, :cls.T] = cls.A()
        return [wide[b].reshape(-1)[:(cls.N - 1) * cls.ld_row + cls.T].copy() for b in range(cls.B)]

    @classmethod
    def strides(cls, src):
        return cls.ld_row, src.ld

    @classmethod
    def run(cls, lib, src, dst):
        B, N = cls.B, cls.N
        pos, peak, bad = LK.Buf(B * N, torch.int32, -77), LK.Buf(B * N, torch.float32, 7.5), LK.Buf(B * N, torch.uint8, 0xAB)
        il, ol = _i32(cls.in_len), _i32(cls.out_len)
        ld_row, ld_entry = cls.strides(src)
        assert lib.t2s_align_rows(src.t.data_ptr(), 2, B, N, cls.T, ld_row, ld_entry, il.data_ptr(), ol.data_ptr(), pos.t.data_ptr(),
                                  peak.t.data_ptr(), bad.t.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert pos.guards_intact() and peak.guards_intact() and bad.guards_intact()
        return dict(pos=pos.t.cpu().numpy().reshape(B, N), peak=peak.t.cpu().numpy().reshape(B, N), bad=bad.t.cpu().numpy().reshape(B, N))

    @classmethod
    def check(cls, lib, blocks, res):
        pos, peak, bad = align_ref.rows(cls.A(), cls.in_len, cls.out_len)
        assert np.array_equal(res["pos"], pos) and np.array_equal(res["bad"], bad)
        assert res["peak"].view(np.uint32).tobytes() == peak.view(np.uint32).tobytes()


class AlignRowsLdRow(AlignRows):
    """ld_row carries the distance: one entry of two rows"""
    name = "align_rows ld_row"
    B, N, T = 1, 2, FC.ALIGN_ROW_T
    in_len, out_len = [FC.ALIGN_ROW_T - 10], [2]

    @classmethod
    def blocks(cls, lib):
        return list(cls.A()[0])

    @classmethod
    def strides(cls, src):
        return src.ld, 2 * src.ld


class WarpGather:
    """ld_entry carries the distance: two entries of C rows"""
    name, src_kind, dst_kind, dst_count = "warp_gather ld_entry", "float16", None, 0
    B, (C, F, ld_row) = 2, FC.WARP
    lengths = [FC.WARP[1], FC.WARP[1] - 9]

    @classmethod
    def x(cls):
        rng = np.random.RandomState(5700)
        return [(rng.choice([-1.0, 1.0], (cls.C, 1)) * rng.uniform(0.25, 11.5, (cls.C, ln))).astype(np.float16) for ln in cls.lengths]

    @classmethod
    def blocks(cls, lib):
        assert cls.F > 2 * lib.t2s_warp_block()
        wide = _poisoned((cls.B, cls.C, cls.ld_row), np.float16)
        for b, x in enumerate(cls.x()):
            wide[b, :, :x.shape[1]] = x
        return [wide[b].reshape(-1)[:(cls.C - 1) * cls.ld_row + cls.F].copy() for b in range(cls.B)]

    @classmethod
    def strides(cls, src):
        return cls.ld_row, src.ld

    @classmethod
    def how(cls):
        stretch = int(np.rint(WK.Q / 0.8))
        c, n, _ = WK.want_map(cls.lengths, cls.F, 1 << 30, stretch=stretch)
        return WK, stretch, c, n, int(n.max()) + 3

    @classmethod
    def run(cls, lib, src, dst):
        WK, stretch, c, n, cap = cls.how()
        cum, out_len, _, lens_d, _ = WK.run_map(lib, cls.lengths, cls.F, cap, stretch=stretch)
        assert cum.np(cls.B, cls.F + 1).tolist() == c.tolist() and out_len.np(cls.B).tolist() == n.tolist()
        out = WK.Buf(cls.B * cls.C * cap, torch.float16, float("nan"))
        ld_row, ld_entry = cls.strides(src)
        assert lib.t2s_warp_gather(src.t.data_ptr(), 2, cls.B, cls.C, cls.F, ld_row, ld_entry, WK.P(lens_d), WK.P(cum), WK.P(out_len),
                                   WK.P(out), cap, _st()) == 0
        torch.cuda.synchronize()
        assert out.guards_intact() and cum.guards_intact() and out_len.guards_intact()
        return dict(out=out.np(cls.B, cls.C, cap))

    @classmethod
    def check(cls, lib, blocks, res):
        WK, stretch, c, n, cap = cls.how()
        mel = types.SimpleNamespace(B=cls.B, C=cls.C, F=cls.F, dtype=torch.float16, x=cls.x())
        WK.check_values(res["out"], mel, c, n, cls.lengths, cap)


class WarpGatherLdRow(WarpGather):
    """ld_row carries the distance: one entry of two rows"""
    name = "warp_gather ld_row"
    B, C, F = 1, 2, FC.WARP_ROW_F
    lengths = [FC.WARP_ROW_F - 9]

    @classmethod
    def blocks(cls, lib):
        wide = _poisoned((cls.C, cls.F), np.float16)
        x = cls.x()[0]
        wide[:, :x.shape[1]] = x
        return list(wide)

    @classmethod
    def strides(cls, src):
        return src.ld, 2 * src.ld


class WarpMap:
    """ld_path carries the distance: the path of the second entry, int32"""
    name, src_kind, dst_kind, dst_count = "warp_map ld_path", "int32", None, 0
    F, T_in = FC.WARP_MAP
    lengths, in_len, cap = [FC.WARP_MAP[0], FC.WARP_MAP[0] - 9], [FC.WARP_MAP[1], FC.WARP_MAP[1] - 7], 4000

    @classmethod
    def inputs(cls):
        rng = np.random.RandomState(5800)
        path = (np.arange(cls.F)[None, :] * cls.T_in // cls.F + rng.randint(0, 2, (2, cls.F))).astype(np.int32)
        path[:, 100] = -3
        path[:, 700] = cls.T_in + 5                             # wild values: rate 1 there
        rates = rng.uniform(0.4, 2.5, (2, cls.T_in)).astype(np.float32)
        return path, rates

    @classmethod
    def blocks(cls, lib):
        return list(cls.inputs()[0])

    @classmethod
    def run(cls, lib, src, dst):
        _, rates = cls.inputs()
        rates_d = WK.Buf(2 * cls.T_in, torch.float32, 1e9, rates)
        lens, il = _i32(cls.lengths), _i32(cls.in_len)
        cum, out_len, fl = WK.Buf(2 * (cls.F + 1), torch.int64, -99), WK.Buf(2, torch.int32, -77), WK.Buf(2 * cls.T_in * 2, torch.int32, -55)
        assert lib.t2s_warp_map(lens.data_ptr(), 2, cls.F, WK.Q, None, src.t.data_ptr(), src.ld, WK.P(rates_d), cls.T_in, il.data_ptr(),
                                cls.T_in, 0.5, 2.0, cls.cap, WK.P(cum), WK.P(out_len), WK.P(fl), _st()) == 0
        torch.cuda.synchronize()
        assert cum.guards_intact() and out_len.guards_intact() and fl.guards_intact() and rates_d.guards_intact()
        return dict(cum=cum.np(2, cls.F + 1), out_len=out_len.np(2), first_last=fl.np(2, cls.T_in, 2))

    @classmethod
    def check(cls, lib, blocks, res):
        path, rates = cls.inputs()
        c, n, fl = WK.want_map(cls.lengths, cls.F, cls.cap, path=path, rates=rates, in_len=cls.in_len, T_in=cls.T_in)
        assert res["cum"].tolist() == c.tolist() and res["out_len"].tolist() == n.tolist() and res["first_last"].tolist() == fl.tolist()


class AudioWindow:
    """ld_dst carries the distance: B = 2, each row's window WINDOW_OFF floats into its row"""
    name, src_kind, dst_kind = "wg_audio_window ld_dst", None, "float32"
    B = 2

    @classmethod
    def dst_count(cls, lib):
        return FC.WINDOW_OFF + FC.WINDOW_GL[0] * FC.WINDOW_GL[1] + FC.WINDOW_PAD

    @classmethod
    def blocks(cls, lib):
        return None

    @classmethod
    def z(cls):
        G, L = FC.WINDOW_GL
        return torch.randn(2, G, L, generator=torch.Generator().manual_seed(59)).to(DEV)[:cls.B].contiguous()

    @classmethod
    def place(cls, dst):
        """(ld_dst, dst_off)"""
        return dst.ld, FC.WINDOW_OFF

    @classmethod
    def run(cls, lib, src, dst):
        G, L = FC.WINDOW_GL
        ld, off = cls.place(dst)
        assert lib.t2s_wg_audio_window(cls.z().data_ptr(), cls.B, G, L, 0, L, dst.t.data_ptr(), ld, off, _st()) == 0
        torch.cuda.synchronize()
        return dict(rows=np.stack([dst.block(q) for q in range(2)]))

    @classmethod
    def check(cls, lib, blocks, res):
        G, L = FC.WINDOW_GL
        assert SK.G == G
        want = SK._squeezed(lib, cls.z(), cls.B, L)
        fill = np.float32(F32_FILL)
        first = 2 - cls.B                                   # with dst_off far the one row lands in the second block
        for b in range(cls.B):
            row = res["rows"][first + b]
            assert row[FC.WINDOW_OFF:FC.WINDOW_OFF + G * L].view(np.uint32).tobytes() == want[b].view(np.uint32).tobytes()
            assert (row[:FC.WINDOW_OFF] == fill).all() and (row[FC.WINDOW_OFF + G * L:] == fill).all(), "wrote a row outside its window"
        assert cls.B == 2 or (res["rows"][0] == fill).all()


class AudioWindowOff(AudioWindow):
    """dst_off carries the distance (and ld_dst with it: the window must fit its row): B = 1, the row lands in the second block"""
    name, B = "wg_audio_window dst_off", 1

    @classmethod
    def place(cls, dst):
        return dst.ld + cls.dst_count(None), dst.ld + FC.WINDOW_OFF


STRIDED = [(Pcm16, "src"), (ResampleBatch, "src"), (ResampleBatch, "dst"), (JoinGather, "src"), (AlignRows, "src"), (AlignRowsLdRow, "src"),
           (WarpGather, "src"), (WarpGatherLdRow, "src"), (WarpMap, "src"), (AudioWindow, "dst"), (AudioWindowOff, "dst"),
           (ResampleWindow, "src"), (ResampleWindow, "dst"), (LimitWindow, "src"), (LimitWindow, "dst"), (SosWindow, "src"),
           (SosWindow, "dst")]
_NEAR_STRIDED = {}


def _count(ep, lib):
    return ep.dst_count(lib) if callable(ep.dst_count) else ep.dst_count


def _near_strided(lib, ep):
    if ep.name not in _NEAR_STRIDED:
        blocks = ep.blocks(lib)
        src = NearPair(ep.src_kind, blocks[0].size, blocks) if ep.src_kind else None
        dst = NearPair(ep.dst_kind, _count(ep, lib)) if ep.dst_kind else None
        res = ep.run(lib, src, dst)
        assert (src is None or src.guards_intact()) and (dst is None or dst.guards_intact())
        ep.check(lib, blocks, res)
        _NEAR_STRIDED[ep.name] = (blocks, res)
    return _NEAR_STRIDED[ep.name]


@pytest.mark.parametrize("second", ("B", "C"))
@pytest.mark.parametrize("case", STRIDED, ids=lambda c: "%s-far-%s" % (c[0].name.replace(" ", "-"), c[1]))
def test_strided_rows_far_apart(lib, big, case, second):
    """the second row beyond the line (B) and across it (C), through ldx / ldo / ld_entry / ld_row / ld_path / ld_dst / dst_off / ldp"""
    ep, side = case
    blocks, near = _near_strided(lib, ep)
    if side == "src":
        src = Pair(big, ep.src_kind, blocks[0].size, second, blocks)
        dst = NearPair(ep.dst_kind, _count(ep, lib)) if ep.dst_kind else None
    else:
        src = NearPair(ep.src_kind, blocks[0].size, blocks) if ep.src_kind else None
        dst = Pair(big, ep.dst_kind, _count(ep, lib), second)
    far = ep.run(lib, src, dst)
    assert src is None or src.guards_intact(), "a source, a decoy or a guard window changed"
    assert dst is None or dst.guards_intact(), "a store outside the rows: a decoy or a guard window of the destination changed"
    assert sorted(far) == sorted(near)
    for key in near:
        assert far[key].dtype == near[key].dtype and far[key].shape == near[key].shape and far[key].tobytes() == near[key].tobytes(), \
            "%s far %s (%s): %s differs from the same call on rows placed near" % (ep.name, side, second, key)
