"""The clips of tests/test_pool_chunks_gpu.py: a few distinct clips cycled to more than 65535, with clips that differ from their
neighbours at both ends and around the seam between two launches.  tests/test_far_util_cpu.py checks the arrangement and the
decision margins of these seeds."""
import numpy as np

import filter_ref
import limiter_ref
import loudness_ref
import resample_ref
import trim_ref

LIMIT_L, LIMIT_OS = 67, 4       # audio.Limiter's defaults at LIMIT_POOL_FS: look-ahead in samples, oversampling
CHUNK = 65535
N_CLIPS = CHUNK + 9
SEAM = (CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2)  # the last rows of the first launch and the first of the second


def cycle(n_base, n_special):
    """index of the distinct clip at each of the N_CLIPS places: the base clips in turn; special clips at both ends and at SEAM,
    each different from its neighbours"""
    idx = [k % n_base for k in range(N_CLIPS)]
    places = (0,) + SEAM + (N_CLIPS - 1,)
    for j, k in enumerate(places):
        idx[k] = n_base + j % n_special
    return idx


RESAMPLE_POOL_RATE, RESAMPLE_POOL_TARGETS = 44100, (44800, 16000)          # 64 / 63 up, 160 / 441 down


def resample_pool_clips():
    """(base, special)"""
    return trim_ref.chunk_clips(), [resample_ref.clip_int16(4700 + q, n) for q, n in enumerate((1501, 257, 700, 2049, 1, 300))]


LOUD_POOL_FS, LOUD_POOL_TARGET, LIMIT_POOL_TARGET = 4000, loudness_ref.POOL_TARGET, -8.0


def loud_pool_clips():
    """(base: too short to be measured, special: loudness_ref.pool_rows at 4 kHz - measured, silent and short ones)"""
    return trim_ref.chunk_clips(), [loudness_ref.clip(LOUD_POOL_FS, n, seed, "int16") for n, seed in loudness_ref.pool_rows(LOUD_POOL_FS)]


LIMIT_POOL_FS = 44800


def limit_pool_clips():
    L, os = LIMIT_L, LIMIT_OS
    sizes = [2 * limiter_ref.TILE + 1, 2, limiter_ref.TILE, 2 * L + 1, limiter_ref.TILE + 1, 1]
    return trim_ref.chunk_clips(), [limiter_ref.clip(n, limiter_ref.seed_of(n, L, os, "int16"), "int16", L) for n in sizes]


def limit_loud_pool_clips():
    """limit() behind a Loudness at LOUD_POOL_FS: steady rows whose gain pushes them over the ceiling, and a short one"""
    h = loudness_ref.hop(LOUD_POOL_FS)
    special = [loudness_ref.as_kind(loudness_ref.steady(s, LOUD_POOL_FS, n) * a, "int16")
               for n, s, a in ((25 * h + 5, 0, 0.3), (13 * h + 17, 1, 1.0), (900, 2, 1.0), (5 * h, 3, 0.5))]
    return trim_ref.chunk_clips(), special


FILTER_POOL_FS = 22050


def filter_pool_clips():
    gen = np.random.RandomState(4800)
    T = filter_ref.TILE
    special = [np.clip(4.0 * np.rint(1200.0 * gen.randn(n)), -32768, 32764).astype(np.int16) for n in (150, 400, 401, 1000, T + 1, 2 * T + 777)]
    loud = np.clip(np.rint(20000.0 * np.random.RandomState(4802).randn(700)), -32768, 32767).astype(np.int16)   # its output saturates
    return trim_ref.chunk_clips(), special[:2] + [loud] + special[2:]
