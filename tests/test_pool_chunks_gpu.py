"""PcmPool and Resampler._table on more than 65535 clips: every operation cuts its work into launches of 65535 rows and slices its
tables, statistics, counts, gains and bounds by the launch, and a wrong slice shows on such a corpus only.  As
test_pool_of_more_than_65535_clips_goes_in_chunks does for rescale_trim (which keeps covering that operation's two loops), a handful
of distinct clips is cycled to n = 65535 + 9 and the reference is computed once per distinct clip; the WHOLE output pool and every
per-clip report entry is compared.  Clips that differ from their neighbours in length, level and flags sit at indices 65533 .. 65537
and at both ends (tests/pool_chunk_cases.py; tests/test_far_util_cpu.py asserts that, and the decision margins of these clips), so a slice
that is off by a launch or by a row cannot pass.

Comparisons are those of the existing pool tests: int16 pools for equality with the float64 reference, float reports at the bars of
tests/test_loudness_gpu.py, tests/test_limiter_gpu.py and tests/test_resample_kernels_gpu.py, imported."""
import numpy as np
import pytest
import torch

import filter_ref as FR
import limiter_ref as MR
import loudness_ref as LR
import pool_chunk_cases as PC
import resample_ref as RR
import test_filter_kernels_gpu as FK
import test_limiter_gpu as TM
import test_loudness_gpu as TL
import test_resample_kernels_gpu as RK
from text2speech_amd import _lib, audio, data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = PC.N_CLIPS


@pytest.fixture(scope="module", autouse=True)
def _peak_memory():
    torch.cuda.reset_peak_memory_stats()
    yield
    print("POOL CHUNKS: peak torch.cuda.max_memory_allocated() %.3f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))


def _pool(clips, fs):
    """(the distinct clips, place [N]: which of them sits at each index, first [distinct]: its first index, the pool)"""
    base, special = clips
    both = base + special
    place = np.asarray(PC.cycle(len(base), len(special)))
    first = np.asarray([int(np.flatnonzero(place == d)[0]) for d in range(len(both))])
    pool = data.PcmPool([both[d] for d in place], fs, DEV)
    assert len(pool) == N > PC.CHUNK
    return both, place, first, pool


def _whole(per_clip, place):
    return torch.from_numpy(np.concatenate([per_clip[d] for d in place]))


def _each_equals_its_first(rep, place, first):
    """every entry of a per-clip report holds the bits of the first clip with the same samples -> the report of the distinct clips"""
    sub = []
    for name, t in zip(rep._fields, rep):
        a = t.cpu().numpy()
        assert a.shape == (N,), name
        assert a.tobytes() == a[first][place].tobytes(), "%s: a clip's entry depends on its place in the pool" % name
        sub.append(t[torch.from_numpy(first).to(t.device)])
    return type(rep)(*sub)


# ---- resample, and Resampler._table directly --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", PC.RESAMPLE_POOL_TARGETS)
def test_resample_of_more_than_65535_clips(target):
    both, place, _, pool = _pool(PC.resample_pool_clips(), PC.RESAMPLE_POOL_RATE)
    want = [RR.to_int16(RR.resample_ref(c, target, PC.RESAMPLE_POOL_RATE)) for c in both]
    out = pool.resample(target)
    assert len(out) == N and out.sampling_rate == target and out.lengths.tolist() == [want[d].size for d in place]
    assert torch.equal(out.pcm.cpu(), _whole(want, place))
    assert torch.equal(pool.pcm.cpu(), _whole(both, place)), "the source pool is untouched"


def test_resampler_table_of_more_than_65535_rows_int16_to_float32():
    """what from_wav_files(resample=True) runs per source rate, with a float32 destination and sentinels between the rows"""
    both, place, first, pool = _pool(PC.resample_pool_clips(), PC.RESAMPLE_POOL_RATE)
    target = PC.RESAMPLE_POOL_TARGETS[0]
    rs = audio.Resampler(PC.RESAMPLE_POOL_RATE, target, device=DEV)
    n_out = np.asarray([rs.out_length(c.size) for c in both])[place]
    starts = np.cumsum(n_out + 1) - n_out                   # one sentinel in front of every row
    dst = torch.full((int(starts[-1] + n_out[-1]),), 12345.678, dtype=torch.float32, device=DEV)
    table = torch.stack([pool.offsets, pool.lengths, torch.from_numpy(starts), torch.from_numpy(n_out)], 1)
    rs._table(pool.pcm, table, dst, int(n_out.max()))
    got = dst.cpu().numpy()
    gaps = np.ones(got.size, dtype=bool)
    rows = {}
    for d, k in enumerate(first):
        rows[d] = got[starts[k]:starts[k] + n_out[k]].copy()
        RK._check_float(rows[d], both[d], target, PC.RESAMPLE_POOL_RATE, "table row %d" % k, "int16")
    want = np.full(got.size, np.float32(12345.678), dtype=np.float32)
    idx = np.concatenate([np.arange(s, s + m) for s, m in zip(starts, n_out)])
    want[idx] = np.concatenate([rows[d] for d in place])
    gaps[idx] = False
    assert bool((got[gaps] == np.float32(12345.678)).all()), "a store between the rows"
    assert got.view(np.int32).tobytes() == want.view(np.int32).tobytes(), "a row differs from the first row with the same samples"


# ---- loudness ------------------------------------------------------------------------------------------------------------------------------
def test_loudness_and_normalize_loudness_of_more_than_65535_clips():
    fs, target, limit = PC.LOUD_POOL_FS, PC.LOUD_POOL_TARGET, LR.POOL_PEAK_LIMIT
    both, place, first, pool = _pool(PC.loud_pool_clips(), fs)
    rep = pool.loudness(target)
    TL._check_report(_each_equals_its_first(rep, place, first), both, fs, target, None)
    want = [LR.measure(c, fs, target, limit) for c in both]
    flags = np.asarray([w["flags"] for w in want])[place]
    short, silent = np.flatnonzero(flags & LR.SHORT).tolist(), np.flatnonzero(flags & LR.SILENT).tolist()
    measured = np.flatnonzero(flags & (LR.SHORT | LR.SILENT) == 0).tolist()
    for group in (short, measured):
        assert group[0] < PC.CHUNK - 4 and any(PC.CHUNK - 4 <= k < PC.CHUNK for k in group) and any(PC.CHUNK <= k < PC.CHUNK + 4 for k in group)
    assert silent and all(PC.SEAM[0] <= k <= PC.SEAM[-1] for k in silent)
    with pytest.raises(_lib.T2SError) as e:
        pool.normalize_loudness(target)
    text = str(e.value)
    assert "clips %s are shorter" % short in text and "clips %s hold nothing" % silent in text, "the flags of both launches, in pool order"
    assert "65532" in text and "65533" in text and "65538" in text and "65542" in text
    out = pool.normalize_loudness(target, limit, allow_unmeasured=True)
    assert out.pcm.dtype == torch.int16 and torch.equal(out.lengths, pool.lengths) and out.sampling_rate == fs
    assert torch.equal(out.pcm.cpu(), _whole([LR.apply_int16(c, w["g"]) for c, w in zip(both, want)], place))
    assert sum(1 for w in want if w["g"] != 1.0) >= 3


# ---- true peak and limiter ---------------------------------------------------------------------------------------------------------------
def test_true_peak_and_limit_of_more_than_65535_clips():
    L, os = PC.LIMIT_L, PC.LIMIT_OS
    lim = audio.Limiter(PC.LIMIT_POOL_FS)
    assert (lim.lookahead, lim.oversample, lim.ceiling) == (L, os, TM.C)
    both, place, first, pool = _pool(PC.limit_pool_clips(), PC.LIMIT_POOL_FS)
    TM._check_report(_each_equals_its_first(pool.true_peak(lim), place, first), both, L, os)
    out = pool.limit(lim)
    assert out.pcm.dtype == torch.int16 and torch.equal(out.lengths, pool.lengths) and out is not pool
    refs = [MR.reference(c, TM.C, L, os, 1.0) for c in both]
    assert sum(r.counts[0] for r in refs) > 20
    assert torch.equal(out.pcm.cpu(), _whole([r.out for r in refs], place))
    assert torch.equal(pool.pcm.cpu(), _whole(both, place)), "the source pool is untouched"


def test_limit_behind_a_loudness_of_more_than_65535_clips():
    """the gains of the loudness pass, one per clip, sliced by the launch in the limiter's measure and apply passes; the reference
    is fed the gain the device measured (tests/test_loudness_gpu.py bounds that), as tests/test_limiter_gpu.py does"""
    fs = PC.LOUD_POOL_FS
    lim, ld = audio.Limiter(fs), audio.Loudness(fs, PC.LIMIT_POOL_TARGET)
    both, place, first, pool = _pool(PC.limit_loud_pool_clips(), fs)
    rep = _each_equals_its_first(pool.loudness(PC.LIMIT_POOL_TARGET), place, first)
    TL._check_report(rep, both, fs, PC.LIMIT_POOL_TARGET, None)
    gains = rep.gain.cpu().numpy()
    assert (gains[:4] == 1.0).all() and gains[4] > 1.5 and len({float(g) for g in gains[4:]}) == len(gains) - 4
    out = pool.limit(lim, ld)
    want, limited = [], 0
    for d, c in enumerate(both):
        ref = MR.limit(c, TM.C, lim.lookahead, 4, g=float(gains[d]))
        v = 32768.0 * ref.o
        # (the margin of tests/test_limiter_gpu.py:255, an inline literal there)
        assert float(np.abs(v - np.floor(v) - 0.5).min()) > 1e-6, "clip %d: the input cannot ask for equal samples" % d
        want.append(ref.out)
        limited += ref.counts[0]
    assert limited > 100 and torch.equal(out.lengths, pool.lengths)
    assert torch.equal(out.pcm.cpu(), _whole(want, place))


# ---- filter --------------------------------------------------------------------------------------------------------------------------------
def test_filter_of_more_than_65535_clips():
    fs = PC.FILTER_POOL_FS
    both, place, first, pool = _pool(PC.filter_pool_clips(), fs)
    sos = audio.sos_butter(4, 80.0, "highpass", fs)
    f = audio.SosFilter(sos, fs, device=DEV)
    out = pool.filter(f)
    assert out.pcm.dtype == torch.int16 and torch.equal(out.lengths, pool.lengths) and torch.equal(out.offsets, pool.offsets)
    pcm, tab = out.pcm.cpu().numpy(), f.table()
    got, clipped = [], []
    for d, c in enumerate(both):                            # tests/test_filter_gpu.py's comparison, on the first clip of each kind
        ref, _ = FR.sequential(sos, c)
        par, _ = FR.parallel(sos, tab, c)
        term = FR.second_term(float(np.max(np.abs(par - ref))), FR.impulse_l1(sos), float(np.max(np.abs(c.astype(np.float64)))))
        _, n_clipped = FR.round16(ref)
        o = int(pool.offsets[first[d]])
        got.append(pcm[o:o + c.size].copy())
        FK._check_i16("pool clip %d" % first[d], got[d], ref, term)        # equal outside the exempt samples, whose share is its default
        assert int(out.clipped[first[d]]) == n_clipped
        clipped.append(n_clipped)
    assert sum(clipped) > 0, "some clip saturates"
    assert torch.equal(out.pcm.cpu(), _whole(got, place)), "a clip's samples depend on its place in the pool"
    assert out.clipped.cpu().tolist() == [clipped[d] for d in place] and out.nonfinite.cpu().tolist() == [0] * N
