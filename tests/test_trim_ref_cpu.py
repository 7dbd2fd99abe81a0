"""Silence trimming and peak rescaling where no GPU is needed: the float64 restatement of tests/trim_ref.py (librosa's formulas -
librosa itself is not a dependency and is not imported) in its two forms, known answers, the property of the GPU tests' seeded
clips that lets them compare bounds for equality, and the entry points' argument checks (which return before anything is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import trim_ref as R

MARGIN_DB = 1e-6


def _lib_loaded():
    from text2speech_amd import _lib
    return _lib, _lib.load()


def _both_forms(clip, fl, h, mode, top_db, r, floor=0.0):
    (b_db, margin) = R.trim_bounds(clip, fl, h, mode, top_db, r, floor, form="db", with_margin=True)
    b_rule = R.trim_bounds(clip, fl, h, mode, top_db, r, floor, form="rule")
    return b_db, b_rule, margin


def test_db_form_and_rule_agree_on_the_issue_trial_grid():
    """seeds x lengths 300 / 1025 / 4096 / 20000 x four frame shapes x top_db 23 / 40 / 60 x both pad modes x rescaling on and off"""
    worst = np.inf
    for seed in range(6):
        for n in (300, 1025, 4096, 20000):
            clip = R.clip_int16(seed, n)
            for fl, h in ((512, 128), (800, 200), (64, 16), (50, 20)):
                for mode in R.MODES:
                    if mode == "reflect" and n <= fl // 2:
                        continue
                    for top_db in (23, 40, 60):
                        for r in (None, 0.999):
                            b_db, b_rule, margin = _both_forms(clip, fl, h, mode, top_db, r)
                            assert b_db == b_rule, (seed, n, fl, h, mode, top_db, r)
                            worst = min(worst, margin)
    print("TRIM REF grid: closest frame to the threshold %.3e dB" % worst)
    assert worst >= MARGIN_DB


def test_gpu_test_clips_keep_their_distance_from_the_threshold():
    """every bounds comparison of the GPU tests: the two forms agree and no frame lies within 1e-6 dB of the threshold (float clips
    on their values as rounded to the source type)"""
    _, lib = _lib_loaded()
    tile = lib.t2s_trim_tile()
    worst, some_trimmed, some_whole = np.inf, 0, 0
    cases = [c + (0.0,) for c in R.kernel_cases(tile)] + R.surface_cases()
    for label, clip, fl, h, mode, top_db, r, floor in cases:
        b_db, b_rule, margin = _both_forms(clip, fl, h, mode, top_db, r, floor)
        assert b_db == b_rule, label
        assert margin >= MARGIN_DB, "%s: a frame %.3e dB from the threshold" % (label, margin)
        worst = min(worst, margin)
        some_trimmed += b_rule not in ((0, clip.size), (0, 0))
        some_whole += b_rule == (0, clip.size)
    print("TRIM REF GPU clips: %d comparisons, closest frame to the threshold %.3e dB; %d trimmed, %d whole"
          % (len(cases), worst, some_trimmed, some_whole))
    assert some_trimmed > len(cases) // 4 and some_whole > 0


def test_known_answers():
    zeros = np.zeros(3000, dtype=np.int16)
    for mode in R.MODES:
        for r in (None, 0.999):
            assert R.trim_bounds(zeros, 512, 128, mode, 23, r) == (0, 0)
            assert R.trim_bounds(zeros, 512, 128, mode, 23, r, form="db") == (0, 0)
    burst = R.burst_clip()
    for form in ("db", "rule"):
        assert R.trim_bounds(burst, 512, 128, "reflect", 23, None, form=form) == (0, 5000), "the floor: nothing is cut"
        assert R.trim_bounds(burst, 512, 128, "reflect", 23, 0.999, form=form) == (1792, 2432)
        assert R.trim_bounds(burst, 512, 128, "reflect", 100, 0.999, form=form) == (0, 5000)
    # a reflect clip of at most frame_length // 2 samples has no frames; a non-finite sample leaves no loud frame
    assert R.trim_bounds(np.full(256, 1000, dtype=np.int16), 512, 128, "reflect", 23) == (0, 0)
    assert R.trim_bounds(np.full(256, 1000, dtype=np.int16), 512, 128, "constant", 23) == (0, 256)
    x = R.clip_float(3, 3000, np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1500] = bad
        assert R.trim_bounds(y, 512, 128, "reflect", 23, 0.999) == (0, 0)
        assert R.trim_bounds(y, 512, 128, "reflect", 23, 0.999, form="db") == (0, 0)
    # frames: 1 + n // hop for an even frame length
    assert R.n_frames(5000, 512, 128) == 40 and R.frame_energies(burst, 512, 128, "reflect").size == 40
    assert R.n_frames(1, 50, 20) == 1 and R.n_frames(21, 50, 20) == 2


def test_energies_are_the_padded_sums():
    x = np.arange(1, 11, dtype=np.int16)                   # pad 2 reflect: 3 2 | 1 .. 10 | 9 8
    E = R.frame_energies(x, 4, 3, "reflect")
    xp = np.array([3, 2, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 9, 8], dtype=np.float64)
    assert E.tolist() == [float((xp[f * 3:f * 3 + 4] ** 2).sum()) for f in range(4)]
    E0 = R.frame_energies(x, 4, 3, "constant")
    xp[:2] = 0
    xp[-2:] = 0
    assert E0.tolist() == [float((xp[f * 3:f * 3 + 4] ** 2).sum()) for f in range(4)]
    xf = (x / 16.0).astype(np.float32)
    assert np.allclose(R.frame_energies(xf, 4, 3, "reflect"), E / 256.0, rtol=1e-15)


def test_rescale_formulas():
    for peak in (3, 1000, 20000, 32767, -32768):
        x = np.array([peak, -peak if peak != -32768 else 32767, 0, 1], dtype=np.int16)
        y = R.rescale(x, 0.999)
        assert y.dtype == np.int16 and y[0] == np.sign(peak) * np.rint(0.999 * 32768) and y[2] == 0
        if peak != -32768:
            assert y[1] == -y[0]
    assert np.rint(0.999 * 32768) == 32735
    x = R.clip_int16(5, 2000)
    assert np.array_equal(R.rescale(x, None), x) and np.array_equal(R.rescale(np.zeros(5, dtype=np.int16), 0.999), np.zeros(5))
    y = R.rescale(x, 0.999)
    assert int(np.abs(y.astype(np.int32)).max()) == 32735
    assert float(np.abs(y - x.astype(np.float64) * 0.999 * 32768 / np.abs(x.astype(np.float64)).max()).max()) <= 0.5 + 1e-9
    xf = R.clip_float(5, 2000, np.float32)
    yf = R.rescale(xf, 32767 / 32768, 0.01)
    assert yf.dtype == np.float32 and abs(float(np.abs(yf).max()) - 32767 / 32768) <= 2.0 ** -24
    quiet = (xf * np.float32(1e-3)).astype(np.float32)     # below the floor: the gain is rescaling_max / 0.01
    assert np.array_equal(R.rescale(quiet, 0.5, 0.01), (quiet.astype(np.float64) * (0.5 / 0.01)).astype(np.float32))
    # what the gather writes
    s, e = R.trim_bounds(x, 512, 128, "reflect", 23, 0.999)
    assert 0 < s < e < x.size and np.array_equal(R.rescale_trim(x, 512, 128, "reflect", 23, 0.999), y[s:e])


def test_the_python_surface_checks_its_arguments_without_a_device():
    from text2speech_amd import _lib, audio
    T2SError = _lib.T2SError
    for kw in (dict(frame_length=1), dict(frame_length=8193), dict(hop_length=0), dict(hop_length=513), dict(pad_mode="edge"),
               dict(top_db=-1), dict(top_db=float("nan")), dict(rescaling_max=0.0), dict(rescaling_max=float("inf")),
               dict(peak_floor=-0.1), dict(peak_floor=None)):
        with pytest.raises(T2SError):
            audio.Trimmer(**kw)
    tr = audio.Trimmer()
    assert (tr.frame_length, tr.hop_length, tr.top_db, tr.pad_mode, tr.rescaling_max, tr.peak_floor) == (512, 128, 23.0, "reflect", None, 0.0)
    assert tr.n_frames(5000) == 40 and tr.pad == 256
    with pytest.raises(RuntimeError, match="no CPU path"):
        tr.forward(torch.zeros(1, 3000))
    with pytest.raises(RuntimeError, match="no CPU path"):
        tr.trim_batch(torch.zeros(2, 3000), [3000, 100])


def test_entry_points_refuse_bad_arguments():
    """every T2S_EINVAL case returns before anything is launched, so the checks run here too (pointers are never followed)"""
    _, lib = _lib_loaded()
    assert lib.t2s_trim_tile() == 64
    P, Q, S, D = 0x1000, 0x2000, 0x3000, 0x100000            # fake, aligned, disjoint
    nan, inf = float("nan"), float("inf")

    def energy(src=P, kind=0, src_len=1000, table=Q, rows=1, fl=512, hop=128, mode=0, max_frames=8, en=S, en_len=8, stats=D):
        return lib.t2s_trim_energy(src, kind, src_len, table, rows, fl, hop, mode, max_frames, en, en_len, stats, None)

    def bounds(table=Q, rows=1, kind=0, src_len=1000, fl=512, hop=128, mode=0, max_frames=8, en=S, en_len=8, stats=D, top_db=23.0,
               rescale=1, r=0.999, floor=0.0, out=P):
        return lib.t2s_trim_bounds(table, rows, kind, src_len, fl, hop, mode, max_frames, en, en_len, stats, top_db, rescale, r, floor,
                                   out, None)

    def gather(src=P, kind=0, src_len=1000, table=Q, rows=1, bnd=S, stats=D, r=0.999, floor=0.0, dst=0x200000, dkind=0, dst_len=1000,
               max_out=1000, lens=None):
        return lib.t2s_trim_gather(src, kind, src_len, table, rows, bnd, stats, r, floor, dst, dkind, dst_len, max_out, lens, None)

    EINVAL = -1
    frames = [dict(fl=1), dict(fl=8193), dict(hop=0), dict(hop=513), dict(mode=2), dict(mode=-1), dict(max_frames=0),
              dict(max_frames=(1 << 40) + 1)]
    common = [dict(table=None), dict(rows=0), dict(rows=65536), dict(kind=3), dict(kind=-1), dict(src_len=0), dict(table=Q + 4)]
    for kw in frames + common + [dict(src=None), dict(stats=None), dict(en_len=0), dict(stats=D + 4), dict(en=S + 4)]:
        assert energy(**kw) == EINVAL, kw
    for kw in frames + common + [dict(en=None), dict(stats=None), dict(out=None), dict(en_len=0), dict(top_db=-1.0), dict(top_db=nan),
                                 dict(top_db=inf), dict(r=-0.5), dict(r=nan), dict(r=inf), dict(r=0.0), dict(floor=-1.0), dict(floor=nan),
                                 dict(floor=inf), dict(rescale=2), dict(out=P + 4)]:
        assert bounds(**kw) == EINVAL, kw
    for kw in common + [dict(src=None), dict(dst=None), dict(dst_len=0), dict(max_out=0), dict(max_out=(1 << 40) + 1), dict(dkind=1),
                        dict(kind=1, dkind=0), dict(kind=2, dkind=0), dict(dkind=2), dict(r=-1.0), dict(r=nan), dict(r=inf), dict(r=0.0),
                        dict(floor=-1.0), dict(floor=nan), dict(bnd=S + 4), dict(stats=D + 4),
                        dict(dst=P + 100), dict(dst=P), dict(src=0x200000 + 1998)]:            # in place / overlapping
        assert gather(**kw) == EINVAL, kw
