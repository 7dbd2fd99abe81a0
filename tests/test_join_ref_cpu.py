"""tests/join_ref.py, the numpy restatement of the join's definition, pinned on the CPU: the GPU tests compare the kernels with it bit
for bit, so what it computes is stated here independently of it."""
import numpy as np
import pytest

import join_ref as J


def _rows(sizes, seed=0, dtype=np.float32):
    rng = np.random.RandomState(seed)
    return [rng.uniform(-1, 1, s).astype(dtype) for s in sizes]


def test_no_fade_is_concatenate_with_zero_runs():
    rows = _rows([7, 5, 9, 4])
    lengths = [3, 5, 0, 4]
    for gaps, gap in ((None, 0), (None, 3), ([2, 0, 5], 0)):
        g = gaps if gaps is not None else [gap] * 3
        parts = []
        for p in range(4):
            parts.append(rows[p][:lengths[p]])
            if p < 3:
                parts.append(np.zeros(g[p], dtype=np.float32))
        want = np.concatenate(parts)
        dst, length, off = J.join(rows, lengths, gaps=gaps, gap=gap, fade=0)
        assert dst.dtype == np.float32 and dst.tobytes() == want.tobytes()
        assert length == want.size == off[4]
        assert off.dtype == np.int64
        assert off.tolist() == [0, 3 + g[0], 8 + g[0] + g[1], 8 + g[0] + g[1] + g[2], want.size]


def test_order_maps_position_to_row():
    rows = _rows([4, 6, 5])
    lengths = [4, 2, 5]
    dst, length, off = J.join(rows, lengths, order=[2, 0, 1], gap=1)
    want = np.concatenate([rows[2][:5], [0], rows[0][:4], [0], rows[1][:2]]).astype(np.float32)
    assert dst.tobytes() == want.tobytes() and off.tolist() == [0, 6, 11, 13]


@pytest.mark.parametrize("F", [1, 2, 8, 1000, 65536])
def test_ramp_is_strictly_increasing_inside_the_unit_interval(F):
    r = J.ramp(F)
    assert r.dtype == np.float32 and r.size == F
    assert r[0] > 0 and r[-1] < 1
    assert bool((np.diff(r.astype(np.float64)) > 0).all())
    k = np.arange(F, dtype=np.float64)
    assert r.tobytes() == np.float32((2 * k + 1) / (2.0 * F)).tobytes()          # one division in double, one rounding
    assert J.ramp(0).size == 0


def test_ramp_values():
    assert J.ramp(1).tolist() == [0.5]
    assert J.ramp(2).tolist() == [0.25, 0.75]
    assert J.ramp(8)[3] == np.float32(7.0 / 16.0)


def test_length_one_segment_gets_both_factors():
    x = np.array([0.7], dtype=np.float32)
    for F in (1, 3, 8):
        r0 = J.ramp(F)[0]
        y = J.fade_segment(x, F, True, True)
        assert y[0] == np.float32(np.float32(x[0] * r0) * r0)
        assert J.fade_segment(x, F, True, False)[0] == np.float32(x[0] * r0)
        assert J.fade_segment(x, F, False, False)[0] == x[0]


def test_short_segment_both_ramps_in_order():
    F = 8
    x = _rows([11], seed=3)[0]
    r = J.ramp(F)
    y = J.fade_segment(x, F, True, True)
    for i in range(11):
        v = x[i]
        if i < F:
            v = np.float32(v * r[i])
        if 10 - i < F:
            v = np.float32(v * r[10 - i])
        assert y[i] == v


def test_which_segments_get_which_ramp():
    F = 2
    rows = [np.ones(6, dtype=np.float32)] * 3
    dst, _, off = J.join(rows, [6, 6, 6], fade=F)
    r = J.ramp(F)
    first, mid, last = dst[0:6], dst[6:12], dst[12:18]
    assert first.tolist() == [1, 1, 1, 1, r[1], r[0]]
    assert mid.tolist() == [r[0], r[1], 1, 1, r[1], r[0]]
    assert last.tolist() == [r[0], r[1], 1, 1, 1, 1]
    dst, _, _ = J.join(rows, [6, 6, 6], fade=F, fade_ends=True)
    assert dst[0:6].tolist() == mid.tolist() and dst[12:18].tolist() == mid.tolist()
    one, _, _ = J.join(rows[:1], [6], fade=F)
    assert one.tolist() == [1] * 6                              # n = 1 without fade_ends: a copy


def test_offsets_unclipped_when_dst_cap_is_short():
    rows = _rows([10, 10, 10])
    full, total, off = J.join(rows, [10, 7, 10], gap=4)
    assert total == 35 and off.tolist() == [0, 14, 25, 35]
    for cap in (1, 13, 14, 20, 34, 35, 36, 50):
        dst, length, off_c = J.join(rows, [10, 7, 10], gap=4, dst_cap=cap)
        assert off_c.tolist() == off.tolist()
        assert length == min(35, cap) and dst.size == cap
        assert dst[:min(cap, 35)].tobytes() == full[:min(cap, 35)].tobytes()
        assert not dst[35:].any()


def test_out_of_range_lengths_are_clamped():
    rows = _rows([6, 9, 5])
    a = J.join(rows, [-5, 9 + 7, 5], gap=2, fade=2)
    b = J.join(rows, [0, 9, 5], gap=2, fade=2)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tolist() == b[2].tolist() == [0, 2, 13, 18]


def test_negative_gaps_count_as_zero_and_last_gap_is_ignored():
    rows = _rows([3, 3])
    _, total, off = J.join(rows, [3, 3], gaps=[-4])
    assert total == 6 and off.tolist() == [0, 3, 6]


def test_f16_rows_are_widened_exactly():
    rows = _rows([9, 12], dtype=np.float16)
    dst, _, _ = J.join(rows, [9, 12], fade=0)
    assert dst.tobytes() == np.concatenate(rows).astype(np.float32).tobytes()


def test_fill_marks_what_the_definition_leaves_to_the_zeros():
    rows = _rows([4, 4])
    dst, _, _ = J.join(rows, [2, 3], gap=3, dst_cap=12, fill=np.nan)
    assert np.isnan(dst).tolist() == [False] * 2 + [True] * 3 + [False] * 3 + [True] * 4
