"""tests/filter_ref.py - the float64 restatement the GPU tests compare csrc/sosfilt.hip with - pinned without a device: the
sequential form against a per-sample loop of the header's arithmetic and against scipy, the two emphasis designs against the
reference's lfilter calls, the chunked form against the whole-row parallel form bit for bit, audio.sos_table against matrix powers,
the stability refusals, and the CONDITIONS on the accuracy cases that keep the device bar honest: E, the reordering error in
double measured between the two references, leaves the bar's second term below a quarter of a float32 ulp at the row's peak, and
(int16 pools) leaves no sample - at most one in a thousand for the 20 Hz high-pass - so close to a half-integer that the reordering
may move its code."""
import numpy as np
import pytest
from scipy.signal import lfilter, sosfilt

import filter_ref as R
from text2speech_amd import _lib, audio

ROW_LENGTHS = (0, 1, 2, R.SEGMENT - 1, R.SEGMENT, R.SEGMENT + 1, R.TILE - 1, R.TILE, R.TILE + 1, 2 * R.TILE + 777)


def _loop(sos, v):
    """the header's arithmetic as a per-sample loop: transposed direct form II, section after section"""
    out = np.array(v, dtype=np.float64)
    for b0, b1, b2, _, a1, a2 in sos:
        s1 = s2 = 0.0
        for i in range(out.size):
            x = out[i]
            y = b0 * x + s1
            s1 = b1 * x - a1 * y + s2
            s2 = b2 * x - a2 * y
            out[i] = y
    return out


@pytest.mark.parametrize("case", sorted(R.ACCURACY_CASES))
def test_sequential_is_sosfilt_and_the_headers_loop(case):
    sos = R.ACCURACY_CASES[case]
    x = R.input_rows(3000)["mix_f32"].copy()
    x[[7, 1500]] = [np.nan, -np.inf]
    y, bad = R.sequential(sos, x)
    v = x.astype(np.float64)
    v[[7, 1500]] = 0.0
    assert bad == 2 and np.all(np.isfinite(y))
    assert np.array_equal(y, sosfilt(sos, v))
    assert np.max(np.abs(y - _loop(sos, v))) <= 1e-12 * np.max(np.abs(y))


def test_emphasis_designs_are_the_references_lfilter_calls():
    x = R.input_rows(5000)["noise_f32"].astype(np.float64)
    for k in (0.97, 0.9, 0.5):
        pre, de = audio.sos_preemphasis(k), audio.sos_deemphasis(k)
        assert pre.shape == de.shape == (1, 6) and pre.dtype == de.dtype == np.float64
        p = lfilter([1.0, -k], [1.0], x)                        # utils/audio.py:24-27
        d = lfilter([1.0], [1.0, -k], x)                        # utils/audio.py:30-33
        assert np.max(np.abs(sosfilt(pre, x) - p)) <= 1e-12 * np.max(np.abs(p))
        assert np.max(np.abs(sosfilt(de, x) - d)) <= 1e-12 * np.max(np.abs(d))
        assert np.max(np.abs(sosfilt(de, sosfilt(pre, x)) - x)) <= 1e-12 * np.max(np.abs(x))
    assert np.array_equal(audio.sos_preemphasis(0.97), R.ACCURACY_CASES["preemphasis_0.97"])
    assert np.array_equal(audio.sos_deemphasis(0.97), R.ACCURACY_CASES["deemphasis_0.97"])


def test_butter_designs_are_scipys():
    assert np.array_equal(audio.sos_butter(4, 80.0, "highpass", 44800), R.ACCURACY_CASES["highpass_80_o4_44800"])
    assert np.array_equal(audio.sos_butter(4, (300.0, 3400.0), "bandpass", 8000), R.ACCURACY_CASES["telephone_300_3400_o4_8000"])
    assert np.array_equal(audio.sos_butter(8, 3400.0, "lowpass", 44800), R.ACCURACY_CASES["lowpass_3400_o8_44800"])
    assert audio.sos_butter(8, 3400.0, "lowpass", 44800).shape == (4, 6)
    for n in (1, 2, 4, R.MAX_SECTIONS):
        assert audio._check_sos(R.sections_case(n)).shape == (n, 6)


@pytest.mark.parametrize("case", sorted(R.BIT_CASES))
def test_chunked_form_is_the_whole_row_bit_for_bit(case):
    sos = R.BIT_CASES[case]
    tab = audio.sos_table(sos, R.SEGMENT, R.LANES)
    base = R.input_rows(2 * R.TILE + 777)["mix_f32"]
    for L in ROW_LENGTHS + (300,):
        x = base[:L].copy()
        if L > 40:
            x[L // 3] = np.nan
        for dtype in (np.float32, np.float16):
            if dtype is np.float16 and L not in (300, 2 * R.TILE + 777):
                continue                                        # (on the host only the widening differs)
            xd = x.astype(dtype)
            whole, bad = R.parallel(sos, tab, xd)
            for name, cuts in R.cut_patterns(L).items():
                st, at, got = R.ParallelStream(sos, tab), 0, []
                for n in cuts:
                    got.append(st.push(xd[at:at + n]))
                    at += n
                    assert got[-1].size == n
                got = np.concatenate(got) if got else np.zeros(0)
                assert np.array_equal(got, whole), (L, dtype, name)
                assert st.nonfinite == bad


def test_parallel_form_is_the_sequential_form_to_rounding():
    for n in (1, 2, 4, R.MAX_SECTIONS):
        sos = R.sections_case(n)
        tab = audio.sos_table(sos, R.SEGMENT, R.LANES)
        x = R.input_rows(2 * R.TILE + 777)["noise_f32"]
        ref, _ = R.sequential(sos, x)
        par, _ = R.parallel(sos, tab, x)
        assert np.max(np.abs(par - ref)) <= 1e-11 * np.max(np.abs(ref)), n
        g = 32768.0
        assert np.max(np.abs(R.parallel(sos, tab, x, g)[0] - R.sequential(sos, x, g)[0])) <= 1e-11 * g * np.max(np.abs(ref))


@pytest.mark.parametrize("n", (1, 2, 4, R.MAX_SECTIONS))
def test_sos_table_against_direct_matrix_powers(n):
    """the table runs the recurrence; the product of the one-sample matrices is the same map up to the roundings of T products of
    a contraction: 1e-10 of the largest entry is three orders above that and six below any wrong entry"""
    sos = R.sections_case(n)
    tab = audio.sos_table(sos, R.SEGMENT, R.LANES)
    assert tab.shape == (R.TAB_DOUBLES,) and tab.dtype == np.float64
    d = 2 * n
    M = np.zeros((d, d))                                        # one sample with zero input on (s1, s2 of section 0, ...)
    feed = np.zeros(d)                                          # the input of the current section as a row over the state
    for j, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        assert tab[5 * j:5 * j + 5].tolist() == [b0, b1, b2, a1, a2]
        e1, e2 = np.eye(d)[2 * j], np.eye(d)[2 * j + 1]
        y = b0 * feed + e1
        M[2 * j] = b1 * feed - a1 * y + e2
        M[2 * j + 1] = b2 * feed - a2 * y
        feed = y
        Mj = np.array([[-a1, 1.0], [-a2, 0.0]])
        for k in range(8):
            want = np.linalg.matrix_power(Mj, R.SEGMENT << k)
            got = tab[R.TAB_POW + 32 * j + 4 * k:R.TAB_POW + 32 * j + 4 * k + 4].reshape(2, 2)
            assert np.max(np.abs(got - want)) <= 1e-10 * max(1.0, np.max(np.abs(want))), (j, k)
    want = np.linalg.matrix_power(M, R.TILE)
    got = tab[R.TAB_TILE:R.TAB_TILE + d * d].reshape(d, d)
    assert np.max(np.abs(got - want)) <= 1e-10 * max(1.0, np.max(np.abs(want)))
    assert not np.any(tab[5 * n:R.TAB_POW]) and not np.any(tab[R.TAB_TILE + d * d:])


def test_library_geometry_is_the_restatements():
    lib = _lib.load()
    assert (lib.t2s_sos_segment(), lib.t2s_sos_tile(), lib.t2s_sos_max_sections(), lib.t2s_sos_table_doubles()) == \
        (R.SEGMENT, R.TILE, R.MAX_SECTIONS, R.TAB_DOUBLES)
    assert audio.SOS_MAX_SECTIONS == R.MAX_SECTIONS and audio.SOS_TABLE_DOUBLES == R.TAB_DOUBLES
    assert lib.t2s_sos_window_carry(3) == 16 * 3 + 4 * R.TILE and lib.t2s_sos_window_carry(0) == -1
    assert lib.t2s_sos_scratch(3, R.TILE + 1, 4) == 3 * 2 * 8 and lib.t2s_sos_scratch(1, 0, 1) == -1


def test_stability_and_shape_refusals():
    ok = R.ACCURACY_CASES["highpass_80_o4_44800"]
    for label, sos in (("a pole on the circle", [[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]]),
                       ("a pole outside", [[1.0, 0.0, 0.0, 1.0, -2.1, 1.1]]),
                       ("a complex pair of radius 1", [[1.0, 0.0, 0.0, 1.0, -1.2, 1.0]]),
                       ("a complex pair outside", [[1.0, 0.0, 0.0, 1.0, 0.0, 1.0001]]),
                       ("a NaN", [[1.0, np.nan, 0.0, 1.0, 0.0, 0.0]]),
                       ("an infinity", [[np.inf, 0.0, 0.0, 1.0, 0.0, 0.0]]),
                       ("a0 = 2", [[2.0, 0.0, 0.0, 2.0, 0.0, 0.0]]),
                       ("a0 next to 1", [[1.0, 0.0, 0.0, np.nextafter(1.0, 2.0), 0.0, 0.0]]),
                       ("no section", np.zeros((0, 6))),
                       ("nine sections", np.tile(ok[:1], (9, 1))),
                       ("five columns", ok[:, :5]),
                       ("one dimension", ok[0]),
                       ("not numbers", [["a"] * 6])):
        with pytest.raises(_lib.T2SError):
            audio._check_sos(sos)
        with pytest.raises(_lib.T2SError):
            audio.SosFilter(sos)
    with pytest.raises(_lib.T2SError, match="radius"):
        audio.SosFilter([[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]])
    with pytest.raises(_lib.T2SError, match="a0 = 2"):
        audio.sos_table([[2.0, 0.0, 0.0, 2.0, 0.0, 0.0]], R.SEGMENT)
    assert audio.SosFilter(ok, device="cuda").n_sections == 2           # constructing needs no device


@pytest.mark.parametrize("case", sorted(R.ACCURACY_CASES))
def test_accuracy_cases_keep_the_bar_honest(case):
    """The condition on the accuracy cases (not a measurement of the device): the bar's second term, 16 max(E, 2^-50 G max|x|), stays
    below 2^-26 max|ref| on every input row, and for the int16 row no `ref` - at most one in a thousand for the 20 Hz high-pass -
    lies within that term of a half-integer."""
    for row in sorted(R.input_rows()):
        sos, x, ref, E, G, term = R.measure(case, row)
        peak = float(np.max(np.abs(ref)))
        print("%-28s %-10s E %.3e  G %.4f  second term / (2^-24 max|ref|) %.3e" % (case, row, E, G, term / (2.0 ** -24 * peak)))
        assert term < 2.0 ** -26 * peak, (case, row)
        if case == "preemphasis_0.97":
            assert E == 0.0                                     # a section without feedback has nothing to reorder
        if x.dtype == np.int16:
            share = float(np.mean(R.int16_exempt(ref, term)))
            print("%-28s %-10s exempt share %.3e" % (case, row, share))
            assert share <= 1e-3
            if case not in R.LOOSE_INT16:
                assert share == 0.0


def test_cut_patterns_cover_the_edges():
    pats = R.cut_patterns(2 * R.TILE + 777)
    assert set(pats) == {"one", "S-1", "S", "S+1", "T-1", "T", "T+1", "long", "random"}
    assert pats["random"][-1] == 0 and 0 in pats["random"][:-1] and max(pats["long"]) > 2 * R.TILE
    assert R.cut_patterns(300)["ones"] == [1] * 300
    assert list(R.cut_patterns(0)) == ["one"] and list(R.cut_patterns(1)) == ["one", "ones"]
