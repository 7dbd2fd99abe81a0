"""Sample-rate conversion where no GPU is needed: the restatement of tests/resample_ref.py against scipy.signal.resample_poly,
audio.resample_filter against scipy's firwin, the entry points' argument checks, and the property of the GPU tests' seeded inputs
that lets them compare int16 outputs for equality."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as R


def _lib_loaded():
    from text2speech_amd import _lib
    return _lib, _lib.load()


@pytest.mark.parametrize("up,down", [(2, 1), (1, 2), (3, 7), (64, 63), (5, 14), (160, 147)])
def test_restatement_equals_scipy(up, down):
    """float64 input of +-32768: equal lengths, values within 1e-9 absolute (measured 1.5e-11: the margin is between two references)"""
    from scipy.signal import resample_poly
    _, _, h = R.filter_ref(up, down)
    half = h.size // 2
    gen = np.random.RandomState(up * 1000 + down)
    worst = 0.0
    for n in (1, 2, 7, half // up + 1, 300, 1025):
        x = gen.uniform(-32768, 32768, n)
        want = resample_poly(x, up, down)
        got = R.resample_ref(x, up, down)
        assert got.shape == want.shape == (R.out_length(n, up, down),), (n, got.shape, want.shape)
        worst = max(worst, float(np.abs(got - want).max()))
    print("RESAMPLE REF %d/%d: worst |restatement - scipy| %.3e" % (up, down, worst))
    assert worst <= 1e-9


def test_filters_equal_firwin():
    from scipy.signal import firwin
    from text2speech_amd import audio
    for orig, new in ((1, 2), (2, 1), (7, 3), (63, 64), (14, 5), (44100, 48000), (44100, 44800), (44800, 16000), (44800, 8000)):
        up, down, h = audio.resample_filter(orig, new)
        rup, rdown, rh = R.filter_ref(new, orig)
        assert (up, down) == (rup, rdown) and h.dtype == np.float64
        n_taps = 20 * max(up, down) + 1
        want = firwin(n_taps, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        assert h.shape == want.shape
        assert float(np.abs(h - want).max()) <= 1e-14 and float(np.abs(rh - want).max()) <= 1e-14
    assert audio.resample_filter(44100, 44800)[:2] == (64, 63) and audio.resample_filter(44800, 8000)[:2] == (5, 28)
    assert audio.resample_filter(48000, 48000)[:2] == (1, 1)
    with pytest.raises(ValueError):
        audio.resample_filter(0, 16000)


def test_resampler_names_the_limit():
    from text2speech_amd import _lib, audio
    with pytest.raises(_lib.T2SError, match="512"):
        audio.Resampler(44100, 44101)
    with pytest.raises(_lib.T2SError, match="512"):
        audio.Resampler(513, 1)


def test_symbols_exported_and_declared():
    _lib, lib = _lib_loaded()
    for name in ("t2s_resample_tile", "t2s_resample_table", "t2s_resample_batch"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    sig = _lib.SIGNATURES["t2s_resample_table"]
    assert sig[2] is ctypes.c_long and sig[11] is ctypes.c_long and sig[12] is ctypes.c_long and len(sig) == 15
    assert _lib.SIGNATURES["t2s_resample_batch"][4] is ctypes.c_long and _lib.SIGNATURES["t2s_resample_batch"][12] is ctypes.c_long
    assert lib.t2s_abi_version() == 4
    tile = lib.t2s_resample_tile()
    assert tile >= 64 and tile % 64 == 0


def test_entry_points_refuse_before_any_launch():
    """Made-up pointers: every call here must return T2S_EINVAL (-1) without touching them.  Only where there is no device, as in
    tests/test_abi.py: a check that went missing would launch on those pointers."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only on a machine without a GPU")
    _, lib = _lib_loaded()
    SRC, TABLE, H, DST, LENS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def table(src=SRC, src_kind=0, src_len=1000, table=TABLE, n_rows=2, h=H, n_taps=41, up=2, down=1, dst=DST, dst_kind=0,
              dst_len=4000, max_out=2000, out_lengths=None):
        return lib.t2s_resample_table(src, src_kind, src_len, table, n_rows, h, n_taps, up, down, dst, dst_kind, dst_len, max_out,
                                      out_lengths, None)

    def batch(x=SRC, is_half=0, B=2, N=100, ldx=100, lengths=LENS, h=H, n_taps=41, up=2, down=1, out=DST, N_out=200, ldo=200,
              out_lengths=None):
        return lib.t2s_resample_batch(x, is_half, B, N, ldx, lengths, h, n_taps, up, down, out, N_out, ldo, out_lengths, None)

    assert table(src=None) == -1 and table(table=None) == -1 and table(h=None) == -1 and table(dst=None) == -1
    assert batch(x=None) == -1 and batch(h=None) == -1 and batch(out=None) == -1
    assert table(n_rows=0) == -1 and table(n_rows=-1) == -1 and table(n_rows=65536) == -1
    assert batch(B=0) == -1 and batch(B=-2) == -1 and batch(B=65536) == -1
    assert batch(N=0) == -1 and batch(N=-5) == -1 and batch(N_out=0) == -1 and batch(N_out=-1) == -1
    assert table(max_out=0) == -1 and table(max_out=-7) == -1
    assert table(src_len=0) == -1 and table(dst_len=0) == -1
    for f in (table, batch):
        assert f(up=0) == -1 and f(down=0) == -1 and f(up=-2) == -1 and f(down=-1) == -1
        assert f(up=4, down=2, n_taps=81) == -1 and f(up=6, down=9, n_taps=181) == -1, "gcd(up, down) != 1"
        assert f(up=513, down=1, n_taps=10261) == -1 and f(up=1, down=513, n_taps=10261) == -1, "max(up, down) > 512"
        assert f(n_taps=40) == -1 and f(n_taps=1) == -1 and f(n_taps=2) == -1 and f(n_taps=-3) == -1
        assert f(h=H + 4) == -1, "h not 8-byte aligned"
        assert f(up=1, down=1, n_taps=(1 << 20) + 1) == -1, "a filter whose phase table does not fit the LDS"
    assert batch(ldx=99) == -1 and batch(ldo=199) == -1
    assert table(src_kind=3) == -1 and table(src_kind=-1) == -1 and table(dst_kind=2) == -1 and table(dst_kind=-1) == -1


def test_gpu_inputs_have_no_reference_sample_near_a_half_integer():
    """The int16 comparisons of tests/test_resample_kernels_gpu.py are for equality with rint(reference): that is a fair demand of
    a kernel whose float64 sum differs from the reference in the last bits only while no reference sample lies within 1e-6 of
    k + 1/2.  If a seed ever gives one, change the seed."""
    _, lib = _lib_loaded()
    cases = R.int16_cases(lib.t2s_resample_tile())
    total = 0
    for label, up, down, clip in cases:
        y = R.resample_ref(clip, up, down)
        assert R.near_half_integer(y) == 0, label
        total += y.size
    print("RESAMPLE REF: %d cases, %d reference samples, none within 1e-6 of a half-integer" % (len(cases), total))
    sq = R.resample_ref(R.square_wave(900), 64, 63)
    assert sq.max() > 40000 and sq.min() < -40000, "the full-scale square wave overshoots the int16 range"
