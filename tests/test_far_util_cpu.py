"""tests/far_util.py on the host: where 32-bit truncations of a far index land, that every placement of
tests/test_far_offsets_kernels_gpu.py keeps those landing spots inside decoy windows and inside the buffer, and that the seeded
inputs of that module and of tests/test_pool_chunks_gpu.py keep the decision margins the existing tests demand of theirs (so the GPU
modules compare for equality and exempt no row)."""
import numpy as np

import far_cases as FC
import far_util as FU
import limiter_ref as MR
import loudness_ref as LR
import pool_chunk_cases as PC
import resample_ref as RR
import trim_ref as TR
from test_loudness_ref_cpu import GATE_MARGIN, HALF_MARGIN
from test_trim_ref_cpu import MARGIN_DB

# the margins are those the existing CPU tests demand of their own seeds, imported; the limiter's two are inline literals there
# (tests/test_limiter_ref_cpu.py:121, `closest_p > 1e-9 and closest_half > 1e-6`) and are restated; resample_ref.near_half_integer
# carries its own (1e-6)
LIMIT_P_MARGIN, LIMIT_HALF_MARGIN = 1e-9, 1e-6
C = MR.ceiling(MR.CEILING_DB)


def _tiles():
    from text2speech_amd import _lib
    lib = _lib.load()
    return lib.t2s_resample_tile(), lib.t2s_trim_tile()


def test_truncations_known_answers():
    k = 4097
    assert FU.truncations((1 << 32) + k, 2) == [k]                      # index and byte offset, unsigned and signed: all k
    assert FU.truncations((1 << 30) + k, 4) == [k]                      # the index fits; byte offset 2^32 + 4 k
    assert FU.truncations((1 << 32) - 700, 2) == [-700, (1 << 31) - 700]
    assert FU.truncations((1 << 30) - 700, 4) == [-700]
    assert FU.truncations(12345, 2) == [] and FU.truncations(12345, 4) == []
    assert FU.decoys((1 << 32) - 700, 1500, 2) == [(-700, 700), (0, 800), ((1 << 31) - 700, 700)]
    assert FU.decoys((1 << 30) - 700, 1500, 4) == [(-700, 700), (0, 800)]
    assert FU.decoys(5, 3000, 2) == []


def test_every_placement_of_the_gpu_module_lands_in_decoys_inside_the_buffer():
    layouts = FC.table_layouts(*_tiles()) + FC.gather_layouts() + FC.strided_layouts(_tiles()[0])
    assert len(layouts) == 20 + 2 + 16
    for label, lay in layouts:
        assert FU.check_layout(lay), label
        a, b, c = lay.starts
        far = FU.far_element(lay.itemsize)
        assert a < (1 << 20) and b * lay.itemsize > FU.LINE and c < far < c + lay.counts[2], label
        assert (b + lay.counts[1]) * lay.itemsize + FU.BASE_BYTES + FU.WINDOW * lay.itemsize <= FU.BUF_BYTES, label
        assert any(s < 0 for s, _ in lay.decoys), "%s: the straddling row's signed landing lies in front of the base" % label
        for q in (1, 2):                                    # every element of both far rows, not only the corners check_layout tries
            e = np.arange(lay.starts[q], lay.starts[q] + lay.counts[q], dtype=np.int64)
            inside = np.zeros(e.size, dtype=bool)
            low = (e * lay.itemsize % FU.LINE) // lay.itemsize              # the unsigned byte-offset cut; the others are among the corners'
            for s, n in lay.decoys:
                inside |= (low >= s) & (low < s + n)
            assert bool((inside | (low == e)).all()), label


def test_far_rows_keep_their_decision_margins():
    rt, tt = _tiles()
    for kind in FC.TABLE_KINDS:
        if kind == "int16":
            up, down = FC.RESAMPLE_RATIOS[kind]
            for q, c in enumerate(FC.resample_clips(kind, rt)):
                assert RR.near_half_integer(RR.resample_ref(c, up, down)) == 0, "resample row %d" % q
        fl, h, mode, (top_db, r) = FC.TRIM
        for q, c in enumerate(FC.trim_clips(kind, tt)):
            assert TR.n_frames(c.size, fl, h) > 2 * tt
            _, margin = TR.trim_bounds(c, fl, h, mode, top_db, r, with_margin=True)
            assert margin >= MARGIN_DB, "trim %s row %d: a frame %.2e dB from the threshold" % (kind, q, margin)
        for q, c in enumerate(FC.loud_clips(kind)):
            m = LR.measure(c, FC.LOUD_FS)
            assert m["flags"] == 0 and m["margin"] > GATE_MARGIN, "loudness %s row %d" % (kind, q)
        for q, c in enumerate(FC.limit_clips(kind)):
            ref = MR.reference(c, C, FC.LIMIT_L, FC.LIMIT_OS, 1.0)
            assert float(np.abs(ref.p / C - 1.0).min()) > LIMIT_P_MARGIN and ref.counts[0] > 0, "limiter %s row %d" % (kind, q)
            if kind == "int16":
                v = 32768.0 * ref.o
                assert float(np.abs(v - np.floor(v) - 0.5).min()) > LIMIT_HALF_MARGIN, "limiter row %d" % q


def test_chunked_pools_put_different_clips_on_both_sides_of_the_seam():
    idx = PC.cycle(4, 6)
    assert len(idx) == PC.N_CLIPS == 65544 and PC.SEAM == (65533, 65534, 65535, 65536, 65537)
    assert [idx[k] for k in PC.SEAM] == [5, 6, 7, 8, 9] and idx[0] == 4 and idx[-1] == 4 and idx[65532] < 4 and idx[65538] < 4
    for k in range(PC.SEAM[0] - 1, PC.SEAM[-1] + 1):
        assert idx[k] != idx[k + 1]
    for clips in (PC.resample_pool_clips, PC.loud_pool_clips, PC.limit_pool_clips, PC.limit_loud_pool_clips, PC.filter_pool_clips):
        base, special = clips()
        both = base + special
        sizes = [c.size for c in both]
        place = PC.cycle(len(base), len(special))
        assert all(c.dtype == np.int16 for c in both)
        assert len({sizes[place[k]] for k in PC.SEAM}) >= 4, "the seam's clips differ in length"
        assert sizes[place[PC.CHUNK - 1]] != sizes[place[PC.CHUNK]], "the last row of a launch and the first of the next differ"


def test_chunked_pool_clips_keep_their_decision_margins():
    base, special = PC.resample_pool_clips()
    for target in PC.RESAMPLE_POOL_TARGETS:
        for q, c in enumerate(base + special):
            assert RR.near_half_integer(RR.resample_ref(c, target, PC.RESAMPLE_POOL_RATE)) == 0, "resample to %d clip %d" % (target, q)
    base, special = PC.loud_pool_clips()
    seen = set()
    for q, c in enumerate(base + special):
        m = LR.measure(c, PC.LOUD_POOL_FS, PC.LOUD_POOL_TARGET, LR.POOL_PEAK_LIMIT)
        seen.add(m["flags"] & (LR.SHORT | LR.SILENT))
        assert m["margin"] > GATE_MARGIN, "loudness clip %d" % q
        if not m["flags"] & (LR.SHORT | LR.SILENT):
            assert LR.half_integer_margin(c, m["g"]) > HALF_MARGIN, "loudness clip %d" % q
    assert seen == {0, LR.SHORT, LR.SILENT}
    base, special = PC.limit_pool_clips()
    limited = 0
    for q, c in enumerate(base + special):
        ref = MR.reference(c, C, PC.LIMIT_L, PC.LIMIT_OS, 1.0)
        limited += ref.counts[0]
        v = 32768.0 * ref.o
        assert float(np.abs(ref.p / C - 1.0).min()) > LIMIT_P_MARGIN and float(np.abs(v - np.floor(v) - 0.5).min()) > LIMIT_HALF_MARGIN, "limiter clip %d" % q
    assert limited > 20
    base, special = PC.limit_loud_pool_clips()
    L = int(round(PC.LOUD_POOL_FS * 1.5 / 1000.0))          # audio.Limiter's default look-ahead at that rate
    limited = 0
    for q, c in enumerate(base + special):
        m = LR.measure(c, PC.LOUD_POOL_FS, PC.LIMIT_POOL_TARGET)
        assert m["margin"] > GATE_MARGIN, "limit behind loudness, clip %d" % q
        ref = MR.limit(c, C, L, 4, g=m["g"])
        limited += ref.counts[0]
        v = 32768.0 * ref.o
        assert float(np.abs(ref.p / C - 1.0).min()) > LIMIT_P_MARGIN and float(np.abs(v - np.floor(v) - 0.5).min()) > LIMIT_HALF_MARGIN, "clip %d" % q
    assert limited > 100
