"""Host side of the alignment check (text2speech_amd/alignment.py, longform.py): attempt_seeds, the retry planner on made-up flag
tables, argument checks, the two entry points' refusals with made-up pointers, and synthesize_long's signature."""
import inspect

import pytest
import torch

from text2speech_amd import _lib, alignment as AL, build, longform as L


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_attempt_seeds():
    for s in (0, 1, 20240611, 2 ** 63 - 1):
        assert AL.attempt_seeds(s, 0) == s
        later = [AL.attempt_seeds(s, k) for k in range(1, 50)]
        assert all(isinstance(v, int) and 0 <= v < 2 ** 63 for v in later)
        assert len(set(later + [s])) == 50
    # known answers: mix(seed + k C) >> 1 with C = 0xD1342543DE82EF95, worked out with longform.mix
    assert AL.ATTEMPT_STEP == 0xD1342543DE82EF95 and AL.ATTEMPT_STEP % 2 == 1
    assert AL.attempt_seeds(5, 1) == L.mix(5 + 0xD1342543DE82EF95) >> 1 == 6071123456432614494
    assert AL.attempt_seeds(1, 2) == L.mix((1 + 2 * 0xD1342543DE82EF95) % 2 ** 64) >> 1 == 8049564717916323955
    assert AL.attempt_seeds([1, 2], 2) == [8049564717916323955, 7825829594988383656]
    assert AL.attempt_seeds(2 ** 63 - 1, 3) == L.mix((2 ** 63 - 1 + 3 * AL.ATTEMPT_STEP) & (2 ** 64 - 1)) >> 1
    for bad in (-1, 2 ** 63, 1.5, "7"):
        with pytest.raises(ValueError):
            AL.attempt_seeds(bad, 1)
    for bad in (-1, 1.0, True, None):
        with pytest.raises(ValueError):
            AL.attempt_seeds(3, bad)


N_IDS = [8, 7, 6, 5, 6]                 # the sorted order is 0, 1, 2, 4, 3
SEEDS = [11, 12, 13, 14, 15]


def _s(c, k):
    return AL.attempt_seeds(SEEDS[c], k)


def test_planner_all_pass():
    passes, attempts, order = L.plan_retries(N_IDS, SEEDS, [[0] * 5] * 3, batch_size=2, max_attempts=3)
    assert passes == [[([0, 1], [11, 12], [0, 1]), ([2, 4], [13, 15], [0, 1]), ([3], [14], [0])]]
    assert attempts == [0] * 5
    groups, plain = L._plan(N_IDS, 2, True)
    assert [g[0] for g in passes[0]] == groups and order == plain == [0, 1, 2, 4, 3]


def test_planner_none_pass():
    table = [[2, 4, 8, 16, 32]] * 3
    passes, attempts, order = L.plan_retries(N_IDS, SEEDS, table, batch_size=2, max_attempts=3)
    assert len(passes) == 3
    for k in (0, 1):
        assert passes[k] == [([0, 1], [_s(0, k), _s(1, k)], []), ([2, 4], [_s(2, k), _s(4, k)], []), ([3], [_s(3, k)], [])]
    assert passes[2] == [([0, 1], [_s(0, 2), _s(1, 2)], [0, 1]), ([2, 4], [_s(2, 2), _s(4, 2)], [0, 1]), ([3], [_s(3, 2)], [0])]
    assert attempts == [2] * 5 and order == [0, 1, 2, 4, 3]


def test_planner_one_chunk_passes_at_attempt_2():
    table = [[0, 2, 0, 4, 0], [0, 0, 0, 8, 0], [0, 0, 0, 0, 0], [9, 9, 9, 9, 9]]
    passes, attempts, order = L.plan_retries(N_IDS, SEEDS, table, batch_size=2, max_attempts=4)
    assert passes == [
        [([0, 1], [11, 12], [0]), ([2, 4], [13, 15], [0, 1]), ([3], [14], [])],
        [([1, 3], [_s(1, 1), _s(3, 1)], [0])],                  # the two that go again share a group
        [([3], [_s(3, 2)], [0])],
    ]
    assert attempts == [0, 1, 0, 2, 0]
    # rows as they are kept: chunk 0, chunks 2 and 4, chunk 1, chunk 3
    assert order == [0, 3, 1, 4, 2]
    # unsorted, one big batch: the same attempts
    passes, attempts2, order = L.plan_retries(N_IDS, SEEDS, table, batch_size=8, sort_by_length=False, max_attempts=4)
    assert attempts2 == attempts and [g[0] for g in passes[0]] == [[0, 1, 2, 3, 4]] and passes[0][0][2] == [0, 2, 4]
    assert passes[1] == [([1, 3], [_s(1, 1), _s(3, 1)], [0])] and order == [0, 3, 1, 4, 2]
    # ... and a chunk that never passes is kept at its last attempt
    never = [[0, 2, 0, 4, 0], [0, 0, 0, 8, 0], [0, 0, 0, 8, 0]]
    passes, attempts, order = L.plan_retries(N_IDS, SEEDS, never, batch_size=2, max_attempts=3)
    assert attempts == [0, 1, 0, 2, 0] and passes[2] == [([3], [_s(3, 2)], [0])]


def test_planner_max_attempts_1():
    passes, attempts, order = L.plan_retries(N_IDS, SEEDS, [[0, 2, 0, 4, 0]], batch_size=2, max_attempts=1)
    assert passes == [[([0, 1], [11, 12], [0, 1]), ([2, 4], [13, 15], [0, 1]), ([3], [14], [0])]]
    assert attempts == [0] * 5 and order == L._plan(N_IDS, 2, True)[1]
    assert L.settle_pass([0, 3, 0], 0, 2) == [0, 2] and L.settle_pass([0, 3, 0], 1, 2) == [0, 1, 2]


def test_alignment_check_arguments():
    c = AL.AlignmentCheck()
    assert (c.skip_max, c.back_max, c.stall_max, c.end_slack, c.min_focus, c.max_frames) == (4, 2, 80, 2, 0.3, None)
    assert c.thresholds() == (0, 4, 2, 80, 2, 0.3) and c.thresholds(1000) == (1000, 4, 2, 80, 2, 0.3)
    assert c.with_max_frames(40).max_frames == 40 and c.with_max_frames(40).stall_max == 80
    own = AL.AlignmentCheck(max_frames=7, skip_max=-1, min_focus=0)
    assert own.with_max_frames(40) is own and own.thresholds(1000) == (7, -1, 2, 80, 2, 0.0)
    for kw in (dict(skip_max=1.5), dict(back_max="2"), dict(stall_max=None), dict(end_slack=True), dict(max_frames=2.0),
               dict(skip_max=2 ** 31), dict(min_focus=None), dict(min_focus="x"), dict(min_focus=float("nan"))):
        with pytest.raises(ValueError):
            AL.AlignmentCheck(**kw)
    with pytest.raises(_lib.T2SError, match="HBM"):
        AL.alignment_report(torch.zeros(1, 3, 4))


def test_synthesize_long_new_keywords():
    t, w = torch.nn.Identity().eval(), torch.nn.Identity().eval()
    with pytest.raises(ValueError, match="max_attempts"):
        L.synthesize_long(t, w, "가. 나.", seed=1, max_attempts=0)
    with pytest.raises(ValueError, match="max_attempts"):
        L.synthesize_long(t, w, "가. 나.", seed=1, max_attempts=1.0)
    with pytest.raises(ValueError, match="needs a check"):
        L.synthesize_long(t, w, "가. 나.", seed=1, max_attempts=2)
    with pytest.raises(_lib.T2SError, match="AlignmentCheck"):
        L.synthesize_long(t, w, "가. 나.", seed=1, check=dict(skip_max=1))
    with pytest.raises(_lib.T2SError, match="seed"):            # the existing checks still come first
        L.synthesize_long(t, w, "가. 나.", check=AL.AlignmentCheck())


def test_synthesize_long_signature_accepts_every_existing_call():
    p = inspect.signature(L.synthesize_long).parameters
    old = ["tacotron", "waveglow", "text", "chunks", "seed", "seeds", "sigma", "batch_size", "max_symbols", "sort_by_length",
           "denoiser", "strength", "trimmer", "pause_ms", "pauses_ms", "fade_ms", "resampler", "pcm16", "sampling_rate"]
    assert list(p)[:len(old)] == old and list(p)[len(old):] == ["check", "max_attempts"]
    assert [p[n].kind for n in old[:3]] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 3
    assert all(p[n].kind == inspect.Parameter.KEYWORD_ONLY for n in list(p)[3:])
    assert p["check"].default is None and p["max_attempts"].default == 1
    assert (p["sigma"].default, p["batch_size"].default, p["max_symbols"].default, p["sort_by_length"].default) == (0.666, 8, 64, True)
    assert L.LongFormChecked._fields[:5] == L.LongForm._fields == ("audio", "length", "offsets", "chunks", "truncated")
    assert L.LongFormChecked._fields[5:] == ("flags", "attempts", "stats", "focus", "durations")


_ROWS = "A src_kind B N T_in ld_row ld_entry in_len out_len pos peak bad stream".split()
_STATS = ("pos peak bad B N T_in in_len out_len max_frames skip_max back_max stall_max end_slack min_focus stats focus dur flags "
          "stream").split()
_BASE = dict(src_kind=1, B=2, N=6, T_in=10, ld_row=10, ld_entry=60, max_frames=0, skip_max=1, back_max=1, stall_max=1, end_slack=1,
             min_focus=0.5)


def _args(params, **changes):
    """made-up, distinct, 16-byte-aligned pointers and a valid small shape, then `changes`"""
    vals = dict(_BASE)
    for i, name in enumerate(params):
        if name not in vals:
            vals[name] = 0x10000 * (i + 1)
    vals.update(changes)
    return [vals[name] for name in params]


def test_entry_points_reject_bad_arguments(lib):
    """Both entry points return T2S_EINVAL for a valid argument tuple with one rule broken.  The pointers are made up, so this runs
    only where there is no device (tests/test_align_kernels_gpu.py has the same refusals on real buffers); the valid tuple itself is
    never called."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only on a machine without a GPU")
    assert len(_ROWS) == len(_lib.SIGNATURES["t2s_align_rows"]) and len(_STATS) == len(_lib.SIGNATURES["t2s_align_stats"])
    bad_rows = [dict(A=None), dict(pos=None), dict(peak=None), dict(bad=None), dict(A=0x10002), dict(A=0x10001, src_kind=2),
                dict(in_len=0x80002), dict(out_len=0x90001), dict(pos=0xa0002), dict(peak=0xb0003), dict(src_kind=0), dict(src_kind=3),
                dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(T_in=0), dict(T_in=-9), dict(ld_row=9), dict(ld_entry=59),
                dict(ld_row=11), dict(B=65536, N=32768, ld_entry=1 << 40)]
    bad_stats = [dict(pos=None), dict(peak=None), dict(bad=None), dict(stats=None), dict(focus=None), dict(dur=None), dict(flags=None),
                 dict(pos=0x10002), dict(peak=0x20001), dict(in_len=0x70002), dict(out_len=0x80003), dict(stats=0xf0002),
                 dict(focus=0x100004), dict(dur=0x110002), dict(flags=0x120001), dict(B=0), dict(N=0), dict(T_in=0), dict(T_in=-1),
                 dict(B=65536, N=32768)]
    for ch in bad_rows:
        assert lib.t2s_align_rows(*_args(_ROWS, **ch)) == -1, "t2s_align_rows accepted %r" % (ch,)
    for ch in bad_stats:
        assert lib.t2s_align_stats(*_args(_STATS, **ch)) == -1, "t2s_align_stats accepted %r" % (ch,)
