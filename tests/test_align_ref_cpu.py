"""tests/align_ref.py - the numpy restatement of the alignment check (include/t2s_hip.h) - on hand-built matrices whose answers are
written out here, and the margin of the seeded inputs of tests/test_align_kernels_gpu.py: no row's two largest values are close."""
import math

import numpy as np
import pytest

import align_cases as C
import align_ref as R


def onehot(path, T_in, top=0.9, dtype=np.float32):
    """[1, N, T_in]: row t holds `top` at path[t] and (1 - top) / 8 elsewhere"""
    A = np.full((1, len(path), T_in), (1.0 - top) / 8, dtype=dtype)
    for t, j in enumerate(path):
        A[0, t, j] = top
    return A


def test_clean_diagonal():
    path = [0, 0, 1, 2, 2, 2, 3, 4, 5, 5]
    r = R.report(onehot(path, 6), **dict(R.OFF, skip_max=1, back_max=0, stall_max=3, end_slack=0, min_focus=0.5, max_frames=11))
    assert r.pos[0].tolist() == path and r.bad[0].tolist() == [0] * 10
    assert r.peak.dtype == np.float32 and (r.peak[0] == np.float32(0.9)).all()
    assert r.stats[0].tolist() == [10, 6, 1, 0, 3, 5, 6, 0]
    assert r.dur[0].tolist() == [2, 1, 3, 1, 1, 2]
    assert abs(r.focus[0] - float(np.float32(0.9))) < 1e-15
    assert r.flags[0] == 0


def test_one_skip_of_5():
    path = [0, 1, 2, 7, 8, 9]
    r = R.report(onehot(path, 10), **dict(R.OFF, skip_max=4))
    assert r.stats[0].tolist() == [6, 10, 5, 0, 1, 9, 6, 0]
    assert r.dur[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1, 1]
    assert r.flags[0] == R.SKIP
    assert R.report(onehot(path, 10), **dict(R.OFF, skip_max=5)).flags[0] == 0


def test_one_backward_jump_of_3():
    path = [0, 1, 2, 3, 4, 1, 2, 3, 4, 5]
    r = R.report(onehot(path, 6), **dict(R.OFF, back_max=2))
    assert r.stats[0].tolist() == [10, 6, 1, 3, 1, 5, 6, 0]
    assert r.dur[0].tolist() == [1, 2, 2, 2, 2, 1]
    assert r.flags[0] == R.BACK
    assert R.report(onehot(path, 6), **dict(R.OFF, back_max=3)).flags[0] == 0


def test_a_stall_of_9_across_positions():
    """two frames on symbol 1, nine on symbol 2, then on: the run is counted where it is, not from the path's start"""
    path = [0, 1, 1] + [2] * 9 + [3, 4]
    r = R.report(onehot(path, 5), **dict(R.OFF, stall_max=8))
    assert r.stats[0].tolist() == [14, 5, 1, 0, 9, 4, 5, 0]
    assert r.dur[0].tolist() == [1, 2, 9, 1, 1]
    assert r.flags[0] == R.STALL
    assert R.report(onehot(path, 5), **dict(R.OFF, stall_max=9)).flags[0] == 0
    # a symbol visited again later is a new run
    r2 = R.report(onehot([2, 2, 2, 1, 2, 2], 3), **R.OFF)
    assert r2.stats[0, 4] == 3 and r2.dur[0].tolist() == [0, 1, 5] and r2.stats[0, 6] == 2


def test_an_unfinished_end():
    path = [0, 1, 2, 3, 3, 4]
    A = onehot(path, 8)
    assert R.report(A, **dict(R.OFF, end_slack=2)).flags[0] == R.UNFINISHED         # 4 < 8 - 1 - 2
    assert R.report(A, **dict(R.OFF, end_slack=3)).flags[0] == 0                    # 4 < 4 is false
    assert R.report(A, **dict(R.OFF, end_slack=-1)).flags[0] == 0
    r = R.report(A, in_len=[5], **dict(R.OFF, end_slack=0))                         # five symbols: the end is reached
    assert r.flags[0] == 0 and r.stats[0].tolist() == [6, 5, 1, 0, 2, 4, 5, 0] and r.dur[0].tolist() == [1, 1, 1, 2, 1, 0, 0, 0]


def test_a_tie_goes_to_the_smaller_index():
    A = np.array([[[0.1, 0.4, 0.4, 0.1], [0.25, 0.25, 0.25, 0.25], [0.0, 0.0, 0.0, 1.0]]], dtype=np.float32)
    r = R.report(A, **R.OFF)
    assert r.pos[0].tolist() == [1, 0, 3]
    assert r.peak[0].tolist() == [np.float32(0.4), np.float32(0.25), 1.0]
    assert r.stats[0].tolist() == [3, 4, 3, 1, 1, 3, 3, 0]


def test_a_nan_row():
    A = onehot([0, 1, 2, 3], 4)
    A[0, 1, :] = np.nan                                         # a row of NaN: pos 0, peak -inf
    A[0, 2, 0] = np.nan                                         # one NaN: never chosen
    A[0, 3, 1] = np.inf                                         # an infinity is chosen and is not finite
    r = R.report(A, **R.OFF)
    assert r.pos[0].tolist() == [0, 0, 2, 1]
    assert r.peak[0, 1] == -np.inf and r.peak[0, 2] == np.float32(0.9) and r.peak[0, 3] == np.inf
    assert r.bad[0].tolist() == [0, 1, 1, 1]
    assert r.stats[0].tolist() == [4, 4, 2, 1, 2, 1, 3, 3]
    assert r.flags[0] == R.NONFINITE
    assert math.isnan(r.focus[0])                               # -inf + inf
    assert R.report(A, **dict(R.OFF, min_focus=0.1)).flags[0] == R.NONFINITE | R.DIFFUSE       # !(NaN >= 0.1)
    # a NaN behind the entry's symbols is not looked at
    B = onehot([0, 1], 4)
    B[0, :, 3] = np.nan
    assert R.report(B, in_len=[3], **R.OFF).flags[0] == 0


def test_no_frame_and_one_frame():
    A = onehot([2, 1, 0], 3)
    r = R.report(A, out_len=[0], **dict(R.OFF, skip_max=0, back_max=0, stall_max=0))
    assert r.pos[0].tolist() == [-1, -1, -1] and r.peak[0].tolist() == [0, 0, 0] and r.bad[0].tolist() == [0, 0, 0]
    assert r.stats[0].tolist() == [0, 3, 0, 0, 0, -1, 0, 0] and r.focus[0] == 0.0 and r.dur[0].tolist() == [0, 0, 0]
    assert r.flags[0] == R.EMPTY
    assert R.report(A, out_len=[0], **dict(R.OFF, end_slack=0)).flags[0] == R.EMPTY | R.UNFINISHED       # -1 < 3 - 1 - 0
    assert R.report(A, out_len=[0], **dict(R.OFF, min_focus=0.5)).flags[0] == R.EMPTY | R.DIFFUSE
    assert R.report(A, out_len=[-4], **R.OFF).stats[0, 0] == 0
    r = R.report(A, out_len=[1], **dict(R.OFF, skip_max=0, back_max=0, stall_max=0, end_slack=0, max_frames=1))
    assert r.pos[0].tolist() == [2, -1, -1]
    assert r.stats[0].tolist() == [1, 3, 0, 0, 1, 2, 1, 0] and r.dur[0].tolist() == [0, 0, 1]
    assert r.flags[0] == R.TRUNCATED | R.STALL
    assert R.report(A, out_len=[9], **R.OFF).stats[0, 0] == 3                       # beyond N: N


def test_one_symbol():
    A = onehot([0, 0, 0, 0], 1, top=0.5)
    r = R.report(A, **dict(R.OFF, end_slack=0, stall_max=4, min_focus=0.5))
    assert r.pos[0].tolist() == [0, 0, 0, 0] and r.stats[0].tolist() == [4, 1, 0, 0, 4, 0, 1, 0] and r.dur[0].tolist() == [4]
    assert r.focus[0] == 0.5 and r.flags[0] == 0
    # in_len below 1 is 1, beyond T_in is T_in
    wide = onehot([3, 3], 4)
    assert R.report(wide, in_len=[0], **R.OFF).pos[0].tolist() == [0, 0]
    assert R.report(wide, in_len=[-7], **R.OFF).stats[0, 1] == 1
    assert R.report(wide, in_len=[99], **R.OFF).pos[0].tolist() == [3, 3]


def test_thresholds_switch_their_own_bit_only():
    path = [0, 5, 2, 2, 2, 2, 3]                                # skip 5, back 3, stall 4, last 3 of 8, focus 0.9
    A = onehot(path, 8)
    base = dict(max_frames=8, skip_max=5, back_max=3, stall_max=4, end_slack=4, min_focus=0.89)
    assert R.report(A, **base).flags[0] == 0
    for name, value, bit in (("max_frames", 7, R.TRUNCATED), ("skip_max", 4, R.SKIP), ("back_max", 2, R.BACK),
                             ("stall_max", 3, R.STALL), ("end_slack", 3, R.UNFINISHED), ("min_focus", 0.91, R.DIFFUSE)):
        assert R.report(A, **dict(base, **{name: value})).flags[0] == bit, name
    assert R.report(A, **R.OFF).flags[0] == 0
    assert R.report(A, **dict(R.OFF, max_frames=-3)).flags[0] == 0


def test_focus_is_the_correctly_rounded_mean():
    rng = np.random.RandomState(3)
    peak = rng.uniform(0.1, 1.0, (1, 1000)).astype(np.float32)
    pos = np.zeros((1, 1000), dtype=np.int32)
    bad = np.zeros((1, 1000), dtype=np.uint8)
    _, focus, _, _ = R.stats(pos, peak, bad, 4, **R.OFF)
    from fractions import Fraction
    exact = sum(Fraction(float(v)) for v in peak[0]) / 1000
    assert abs(Fraction(focus[0]) - exact) <= Fraction(2.0 ** -53) * exact * 2       # two roundings: the sum's and the division's
    assert R.focus_bound(peak[0], 1000) >= 2.0 ** -53 * 1001 * 0.1


# the seeded inputs of tests/test_align_kernels_gpu.py (its CASES): the margin of every row, checked here on the CPU
@pytest.mark.parametrize("case", range(len(C.CASES)))
def test_seeded_inputs_keep_their_margin(case):
    c = C.CASES[case]
    gap = R.top2_gap(C.make(c), c.in_len, c.out_len)
    print("case %d %s: smallest relative gap between a row's two largest values %.4f" % (case, c, gap))
    assert gap > R.MARGIN


def test_block_edge_paths_keep_their_margin():
    for name, c, path, _ in C.edge_cases():
        gap = R.top2_gap(C.make(c, path), c.in_len, c.out_len)
        print("%s: smallest relative gap %.4f" % (name, gap))
        assert gap > R.MARGIN
