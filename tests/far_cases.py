"""The seeded rows and the shapes of tests/test_far_offsets_kernels_gpu.py: three clips per table-addressed entry point and two blocks
per row-strided one, the smallest that span two tiles of the kernel with a ragged tail, and the layouts they are placed at
(tests/far_util.py).  tests/test_far_util_cpu.py checks the layouts and the decision margins of these seeds."""
import numpy as np

import filter_ref
import limiter_ref
import loudness_ref
import resample_ref
import trim_ref
from far_util import CROSS_MIN, ITEMSIZE, NP_OF, layout

RESAMPLE_RATIOS = {"int16": (64, 63), "float16": (5, 14)}
TRIM = (64, 16, "constant", (23, 0.999))                    # frame_length, hop, pad_mode, (top_db, rescaling_max)
LOUD_FS = 8000
LIMIT_L, LIMIT_OS = 67, 4
SOS_SECTIONS = 2


def _three(n):
    """lengths of rows A, B, C around n: all different, all odd or even in turn"""
    return (n, n + 3, n + 10)


def resample_clips(kind, tile):
    up, down = RESAMPLE_RATIOS[kind]
    n = resample_ref.n_in_for(2 * tile + 77, up, down)
    if kind == "int16":
        return [resample_ref.clip_int16(4100 + q, m) for q, m in enumerate(_three(n))]
    return [np.random.RandomState(4200 + q).uniform(-1, 1, m).astype(NP_OF[kind]) for q, m in enumerate(_three(n))]


def trim_clips(kind, tile):
    fl, h = TRIM[0], TRIM[1]
    n = (2 * tile + 3) * h + 5                              # 2 tile + 4 frames
    return [trim_ref.clip_int16(4300 + q, m) if kind == "int16" else trim_ref.clip_float(4300 + q, m, NP_OF[kind])
            for q, m in enumerate(_three(n))]


def loud_clips(kind):
    n = 2 * loudness_ref.TILE + 133
    return [loudness_ref.clip(LOUD_FS, m, (0, 2, 4)[q], kind) for q, m in enumerate(_three(n))]


def limit_clips(kind):
    n = 2 * limiter_ref.TILE + 77
    return [limiter_ref.clip(m, 4400 + q, kind, LIMIT_L) for q, m in enumerate(_three(n))]


def sos_clips(kind):
    n = 2 * filter_ref.TILE + 777
    rng = np.random.RandomState(4500)
    if kind == "int16":
        return [np.clip(np.rint(5000.0 * rng.randn(m)), -32768, 32767).astype(np.int16) for m in _three(n)]
    return [(0.4 * rng.randn(m)).astype(NP_OF[kind]) for m in _three(n)]


TABLE_CASES = ("resample", "trim", "loud", "limit", "sos")
TABLE_KINDS = ("int16", "float16")
OUT_KIND = {"int16": "int16", "float16": "float32", "float32": "float32"}
PAD = 3                     # dst_cap = the row's output + PAD: +0 behind the samples, on the far side too


def table_clips(name, kind, resample_tile, trim_tile):
    """rows A, B, C of a table-addressed entry point"""
    if name == "resample":
        return resample_clips(kind, resample_tile)
    if name == "trim":
        return trim_clips(kind, trim_tile)
    return {"loud": loud_clips, "limit": limit_clips, "sos": sos_clips}[name](kind)


def table_out_counts(name, kind, clips):
    """the most samples each row's output holds"""
    if name != "resample":
        return [c.size for c in clips]
    u, d, _ = resample_ref.filter_ref(*RESAMPLE_RATIOS[kind])
    return [resample_ref.out_length(c.size, u, d) for c in clips]


def table_layouts(resample_tile, trim_tile):
    """(label, Layout) of every placement of the table-addressed cases: the far source, then the far destination"""
    found = []
    for name in TABLE_CASES:
        for kind in TABLE_KINDS:
            clips = table_clips(name, kind, resample_tile, trim_tile)
            found.append(("%s %s source" % (name, kind), layout(ITEMSIZE[kind], [c.size for c in clips])))
            found.append(("%s %s destination" % (name, kind),
                          layout(ITEMSIZE[OUT_KIND[kind]], [n + PAD for n in table_out_counts(name, kind, clips)])))
    return found


GATHER_N = 1600


def gather_layouts():
    return [("pcm16_gather pool", layout(2, [c.size for c in gather_clips()])),
            ("pcm16_gather rows", layout(4, [GATHER_N, GATHER_N, GATHER_N + 900]))]


# row-strided entry points: two blocks of `count` elements, the second far behind the first through the stride
PCM16_N = 2500
JOIN_N = 2 * 2048 + 77                                      # two tiles of t2s_join_tile() and a ragged tail
ALIGN = (8, 300, 303)                                       # N, T_in, ld_row of an entry: two workgroups of four rows
ALIGN_ROW_T = 2500                                          # ... and where ld_row carries the distance: two rows of this many columns
WARP = (3, 2 * 256 + 77, 2 * 256 + 78)                      # C, F, ld_row of an entry: two blocks of t2s_warp_block() and a tail
WARP_ROW_F = 1600
WARP_MAP = (1600, 40)                                       # F, T_in
WINDOW_GL = (8, 300)                                        # G, L of t2s_wg_audio_window: 2400 samples a row
WINDOW_OFF, WINDOW_PAD = 3, 5


def resample_rows(resample_tile):
    """(up, down, the rows' samples) of t2s_resample_batch / t2s_resample_window: f16 rows that give two tiles of outputs and a tail"""
    up, down = RESAMPLE_RATIOS["float16"]
    return up, down, resample_ref.n_in_for(2 * resample_tile + 77, up, down)


def strided_counts(resample_tile):
    """[(label, kind, elements of one block)] of every far placement of the row-strided cases"""
    up, down, n = resample_rows(resample_tile)
    n_out = resample_ref.out_length(n, up, down)
    N, T, ld_row = ALIGN
    C, F, ld_mel = WARP
    keep = WINDOW_GL[0] * WINDOW_GL[1]
    return [("pcm16 ldx", "float16", PCM16_N), ("resample_batch ldx", "float16", n), ("resample_batch ldo", "float32", n_out),
            ("join_gather ldx", "float16", JOIN_N), ("align_rows ld_entry", "float16", (N - 1) * ld_row + T),
            ("align_rows ld_row", "float16", ALIGN_ROW_T), ("warp_gather ld_entry", "float16", (C - 1) * ld_mel + F),
            ("warp_gather ld_row", "float16", WARP_ROW_F), ("warp_map ld_path", "int32", WARP_MAP[0]),
            ("wg_audio_window", "float32", WINDOW_OFF + keep + WINDOW_PAD),
            ("resample_window ldp", "float16", n), ("resample_window ldo", "float32", n_out),
            ("limit_window ldp", "float16", 2 * limiter_ref.TILE + 77), ("limit_window ldo", "float32", 2 * limiter_ref.TILE + 77),
            ("sos_window ldp", "float16", 2 * filter_ref.TILE + 777), ("sos_window ldo", "float32", 2 * filter_ref.TILE + 777)]


def pair_counts(count):
    """rows A, B, C of a strided case: the first block, and the second as the far row or as the straddling one"""
    return [count, count, max(count, CROSS_MIN)]


def strided_layouts(resample_tile):
    return [(label, layout(ITEMSIZE[kind], pair_counts(count))) for label, kind, count in strided_counts(resample_tile)]


def gather_clips():
    """t2s_pcm16_gather: int16 rows of a little more than one output row"""
    return [resample_ref.clip_int16(4600 + q, m, 32768) for q, m in enumerate(_three(1601))]
