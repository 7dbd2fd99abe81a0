"""Restatement in float64 numpy of the silence trimming and peak rescaling the library computes (include/t2s_hip.h, t2s_trim_*).

librosa is not a dependency of this project and is not imported: this restates the formulas of librosa.effects.trim
(`non_silent = power_to_db(rms(y, frame_length, hop_length) ** 2, ref=np.max, top_db=None) > -top_db`, bounds = frames_to_samples
of the first and of the last + 1 non-silent frame, the end cut to the clip), librosa.feature.rms (centred frames: frame_length // 2
samples of padding at both ends, mode "reflect" before librosa 0.10 and "constant" from 0.10 on; rms^2 = mean of the squares) and
librosa.power_to_db (10 log10(max(amin, S)) - 10 log10(max(amin, ref)), amin = 1e-10), and the reference's
`wav / np.abs(wav).max() * rescaling_max` (datasets/kss.py:70) and save_wav's `32767 / max(0.01, max |wav|)` (utils/audio.py:14-17).

    pad = fl // 2;  n_frames = 1 + (n + 2 pad - fl) // h;  E_f = sum of the squares of padded samples f h .. f h + fl - 1
    peak_eff = max(max |x|, peak_floor);  g = rescaling_max / peak_eff with rescaling and peak_eff > 0, else 1 / 32768 (int16), 1
    loud_db:    10 log10(max(1e-10, g^2 E_f / fl)) - 10 log10(max(1e-10, g^2 E_max / fl)) > -top_db          (librosa's form)
    loud_rule:  max(E_f, F) > rho max(E_max, F),  rho = 10^(-top_db / 10),  F = 1e-10 fl / g^2              (the library's form)
    start = h f_first,  end = min(n, h (f_last + 1));  (0, 0) without a loud frame

One stated addition to librosa's rule: a clip of zeros (E_max = 0) has no loud frame and trims to (0, 0) - librosa's floor makes every
frame of it 0 dB below the reference and returns it whole - and so does a clip with a non-finite sample, which librosa's comparisons
give as well.

tests/test_trim_ref_cpu.py asserts that both forms give the same bounds and that no frame of the seeded clips defined here lies
within 1e-6 dB of the threshold, so the GPU tests compare bounds for equality and exempt nothing."""
import numpy as np

AMIN = 1e-10
FRAMES = ((512, 128), (64, 16), (50, 20))        # (frame_length, hop): the last has a hop that does not divide it and an odd pad
MODES = ("reflect", "constant")
# (top_db, rescaling_max) of the kernel tests
DECISIONS = ((23, None), (23, 0.999), (40, 0.999), (60, None))


def pad_signal(x, fl, mode):
    x = np.asarray(x)
    return np.pad(x.astype(np.float64), fl // 2, mode="reflect" if mode == "reflect" else "constant")


def n_frames(n, fl, h):
    return 1 + (n + 2 * (fl // 2) - fl) // h


def frame_energies(x, fl, h, mode):
    """float64 [n_frames]; int16 input: the exact integers (int64 sums); floats: sums in numpy.longdouble rounded once"""
    x = np.asarray(x)
    if mode == "reflect" and x.size <= fl // 2:
        return np.zeros(0)
    if x.dtype == np.int16:
        xp = np.pad(x.astype(np.int64), fl // 2, mode="reflect" if mode == "reflect" else "constant")
        sq = xp * xp
    else:
        sq = pad_signal(x, fl, mode).astype(np.longdouble) ** 2
    win = np.lib.stride_tricks.sliding_window_view(sq, fl)[::h]
    return win.sum(axis=1).astype(np.float64)


def peak_of(x):
    a = np.abs(np.asarray(x).astype(np.float64))
    if a.size == 0:
        return 0.0
    return float(a.max()) if np.isfinite(a).all() else float("inf")


def gain(x, rescaling_max, peak_floor=0.0):
    peak_eff = max(peak_of(x), peak_floor)
    if rescaling_max is not None and peak_eff > 0:
        return rescaling_max / peak_eff
    return 1.0 / 32768.0 if np.asarray(x).dtype == np.int16 else 1.0


def db_margins(E, g, fl, top_db):
    """(loud by librosa's dB form, distance of every frame from the threshold in dB)"""
    with np.errstate(invalid="ignore", over="ignore"):
        db = 10.0 * np.log10(np.maximum(AMIN, g * g * E / fl))
        ref = 10.0 * np.log10(np.maximum(AMIN, g * g * E.max() / fl))
        d = db - ref + top_db
    return d > 0, np.abs(d)


def loud_rule(E, g, fl, top_db):
    rho = 10.0 ** (-top_db / 10.0)
    F = AMIN * fl / (g * g)
    return np.maximum(E, F) > rho * max(float(E.max()), F)


def bounds_of(loud, n, h):
    idx = np.flatnonzero(loud)
    if idx.size == 0:
        return 0, 0
    return int(idx[0]) * h, min(n, (int(idx[-1]) + 1) * h)


def trim_bounds(x, fl, h, mode, top_db, rescaling_max=None, peak_floor=0.0, form="rule", with_margin=False):
    """(start, end) of one clip; with_margin also returns the smallest distance of a frame from the threshold in dB"""
    x = np.asarray(x)
    E = frame_energies(x, fl, h, mode)
    if E.size == 0 or not np.isfinite(x.astype(np.float64)).all() or E.max() == 0:       # (a clip of zeros: nothing is loud)
        return ((0, 0), np.inf) if with_margin else (0, 0)
    g = gain(x, rescaling_max, peak_floor)
    loud_db, margin = db_margins(E, g, fl, top_db)
    loud = loud_db if form == "db" else loud_rule(E, g, fl, top_db)
    b = bounds_of(loud, x.size, h)
    return (b, float(margin.min())) if with_margin else b


def to_int16(y):
    r = np.rint(np.where(np.isnan(y), 0.0, y))
    return np.clip(r, -32768, 32767).astype(np.int16)


def rescale(x, rescaling_max, peak_floor=0.0):
    """int16 -> int16: rint(x s), s = rescaling_max 32768 / peak_eff, saturated; floats -> float32: (float)(x (rescaling_max /
    peak_eff)); both with one division, one product and one rounding in float64.  None, or peak_eff = 0: the samples themselves
    (floats widened to float32)."""
    x = np.asarray(x)
    peak_eff = max(peak_of(x), peak_floor)
    if x.dtype == np.int16:
        if rescaling_max is None or not peak_eff > 0:
            return x.copy()
        return to_int16(x.astype(np.float64) * ((rescaling_max * 32768.0) / peak_eff))
    if rescaling_max is None or not peak_eff > 0:
        return x.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x.astype(np.float64) * (rescaling_max / peak_eff)).astype(np.float32)


def rescale_trim(x, fl, h, mode, top_db, rescaling_max, peak_floor=0.0):
    """the kept samples, rescaled: what the gather writes"""
    x = np.asarray(x)
    y = rescale(x, rescaling_max, peak_floor)
    if top_db is None:
        return y
    s, e = trim_bounds(x, fl, h, mode, top_db, rescaling_max, peak_floor)
    return y[s:e]


# ---- seeded clips -----------------------------------------------------------------------------------------------------------------------
def clip_int16(seed, n):
    """a quiet Gaussian lead and tail (sigma 30 LSB) around a ramped tone-plus-noise burst of several thousand LSB"""
    gen = np.random.RandomState(seed)
    lead, tail = int(n * gen.uniform(0.15, 0.35)), int(n * gen.uniform(0.15, 0.35))
    m = n - lead - tail
    x = gen.normal(0.0, 30.0, n)
    t = np.arange(m)
    ramp = np.minimum(1.0, np.minimum(t + 1, m - t) / max(1.0, 0.2 * m))
    x[lead:lead + m] += ramp * (6000.0 * np.sin(2 * np.pi * gen.uniform(0.01, 0.05) * t) + gen.normal(0.0, 1500.0, m))
    return np.clip(np.rint(x), -32767, 32767).astype(np.int16)


def clip_float(seed, n, dtype):
    """the same clip as floats in (-1, 1), rounded to the type: the factor fills the mantissas, so that sums of squares round"""
    return (clip_int16(seed, n).astype(np.float64) * (0.9173 / 32768.0)).astype(dtype)


def burst_clip():
    x = np.zeros(5000, dtype=np.int16)
    x[2000:2100] = 3
    return x


def lengths_for(fl, h, mode, tile):
    """the shortest clip of the mode, and the lengths that give tile - 1, tile, tile + 1 and 2 tile + 1 frames"""
    pad = fl // 2
    ns = [pad + 1] if mode == "reflect" else [1, 2]
    ns += [(f - 1) * h + fl - 2 * pad for f in (tile - 1, tile, tile + 1, 2 * tile + 1)]
    ns.append(ns[-2] + h - 1)                                  # the last length that still has tile + 1 frames
    for n in ns[-5:]:
        assert n > pad
    return ns


def seed_of(fl, h, mode, n):
    return 7919 * FRAMES.index((fl, h)) + 104729 * MODES.index(mode) + n % 9973


def kernel_cases(tile):
    """(label, clip, fl, h, mode, top_db, rescaling_max) of every bounds comparison of tests/test_trim_kernels_gpu.py"""
    cases = []
    for fl, h in FRAMES:
        for mode in MODES:
            for n in lengths_for(fl, h, mode, tile):
                seed = seed_of(fl, h, mode, n)
                for dtype in (np.int16, np.float32, np.float16):
                    clip = clip_int16(seed, n) if dtype == np.int16 else clip_float(seed, n, dtype)
                    for top_db, r in DECISIONS:
                        cases.append(("%s (%d, %d) %s n %d top_db %g rescaling %s" % (np.dtype(dtype).name, fl, h, mode, n, top_db, r),
                                      clip, fl, h, mode, top_db, r))
    dtypes = (np.int16, np.float32, np.float16)

    def as_type(seed, n, dtype):
        return clip_int16(seed, n) if dtype == np.int16 else clip_float(seed, n, dtype)
    extra = [("burst", burst_clip(), 512, 128, "reflect", 23, None), ("burst", burst_clip(), 512, 128, "reflect", 23, 0.999),
             ("burst", burst_clip(), 512, 128, "reflect", 100, 0.999)]
    for dtype in dtypes[1:]:
        for d in ((23, None), (23, 0.999)):
            extra.append(("beside non-finite clips", clip_float(11, 3000, dtype), 512, 128, "reflect") + d)
    for fl, h, mode in ((512, 128, "reflect"), (50, 20, "constant")):
        for q, n in enumerate(POOL_LENGTHS):
            if mode == "constant" or n > fl // 2:
                for dtype in dtypes:
                    for d in ((23, 0.999), (40, None)):
                        extra.append(("pool clip %d %s" % (q, np.dtype(dtype).name), as_type(600 + q, n, dtype), fl, h, mode) + d)
    for dtype in dtypes[:2]:
        extra.append(("dst_cap", as_type(9, 5000, dtype), 512, 128, "reflect", 23, 0.999))
    safe = clip_int16(12, 400)
    for first in (350, 367, 0):
        extra.append(("table values %d:" % first, safe[first:], 64, 16, "reflect", 23, None))
    extra.append(("refused calls", clip_int16(3, 500), 64, 16, "reflect", 23, 0.999))
    return cases + extra


POOL_LENGTHS = (700, 257, 3000, 1, 9000, 2049, 300)        # the clips of the kernel tests' pool


# ---- the Python surface's clips (tests/test_trim_gpu.py) --------------------------------------------------------------------------------
SURFACE_RATE = 44800
SURFACE_CLIP_LENGTHS = (3000, 700, 2049, 9000, 300)
SURFACE_DECISIONS = ((23, 0.999, 512, 128, "reflect"), (40, None, 64, 16, "constant"), (None, 0.999, 512, 128, "reflect"),
                     (23, 0.999, 50, 20, "constant"))          # (top_db, rescaling_max, fl, h, mode)
BATCH_LENGTHS = (4096, 1500, 2600, 900)
BATCH_TRIMMERS = ((23, None, 512, 128, "reflect", 0.0), (40, 0.999, 64, 16, "constant", 0.0), (None, 32767 / 32768, 512, 128, "reflect", 0.01),
                  (23, 0.5, 512, 128, "reflect", 0.0))         # ... and peak_floor


CHUNK_CLIP_LENGTHS = (40, 100, 64, 33)                     # repeated to more than 65535 clips: (23, 0.999) at (64, 16) constant


def chunk_clips():
    return [clip_int16(900 + q, n) for q, n in enumerate(CHUNK_CLIP_LENGTHS)]


def surface_clips():
    return [clip_int16(300 + q, n) for q, n in enumerate(SURFACE_CLIP_LENGTHS)]


def batch_rows(dtype=np.float32):
    return [clip_float(400 + q, n, dtype) for q, n in enumerate(BATCH_LENGTHS)]


def surface_cases():
    """(label, clip, fl, h, mode, top_db, rescaling_max, peak_floor) of every bounds comparison of tests/test_trim_gpu.py"""
    cases = []
    for top_db, r, fl, h, mode in SURFACE_DECISIONS:
        if top_db is not None:
            for q, c in enumerate(surface_clips()):
                cases.append(("pool clip %d" % q, c, fl, h, mode, top_db, r, 0.0))
    for top_db, r, fl, h, mode, floor in BATCH_TRIMMERS:
        if top_db is not None:
            for dtype in (np.float32, np.float16):
                for q, c in enumerate(batch_rows(dtype)):
                    cases.append(("batch row %d %s" % (q, np.dtype(dtype).name), c, fl, h, mode, top_db, r, floor))
    for q, c in enumerate(chunk_clips()):
        cases.append(("chunked pool clip %d" % q, c, 64, 16, "constant", 23, 0.999, 0.0))
    return cases
