"""The delivery entry points and audio.DeliveryStream without a device: every tuple t2s_resample_window, t2s_limit_window and
t2s_g711 refuse (made-up pointers, so only where there is no GPU: a check that went missing would launch on them), every
constructor and push argument DeliveryStream refuses, what it derives from its arguments, and synthesize_stream's own checks of
delivery=."""
import ctypes

import numpy as np
import pytest
import torch

from text2speech_amd import _lib, audio, streaming

T2SError = _lib.T2SError


def test_the_names_exist():
    lib = _lib.load()
    assert lib.t2s_abi_version() == 4
    for name in ("t2s_resample_window_carry", "t2s_resample_window_end", "t2s_resample_window", "t2s_limit_window_carry",
                 "t2s_limit_window_end", "t2s_limit_window", "t2s_g711"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.t2s_resample_window_end.restype is ctypes.c_long and lib.t2s_limit_window_end.restype is ctypes.c_long
    for name in ("DeliveryStream", "DELIVERY_ENCODINGS", "to_ulaw", "to_alaw"):
        assert name in audio.__all__
    assert audio.DELIVERY_ENCODINGS == ("f32", "pcm16", "ulaw", "alaw")
    header = open(_lib.HERE + "/../include/t2s_hip.h").read()
    for word in ("t2s_resample_window(", "t2s_limit_window(", "t2s_g711(", "mutes", "0xD5", "0x55", "8159", "32635", "132"):
        assert word in header


def test_entry_points_refuse_before_any_launch():
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only on a machine without a GPU")
    lib = _lib.load()
    CI, CO, PIECE, H, W, OUT, STATE, GAINS = (0x10000 * (i + 1) for i in range(8))

    def rs(carry_in=CI, carry_out=CO, piece=PIECE, is_half=0, B=2, n=100, ldp=100, K0=0, M0=0, final=0, h=H, n_taps=41, up=2, down=1,
           out=OUT, out_cap=400, ldo=400):
        return lib.t2s_resample_window(carry_in, carry_out, piece, is_half, B, n, ldp, K0, M0, final, h, n_taps, up, down, out, out_cap,
                                       ldo, None)

    def lm(carry_in=CI, carry_out=CO, piece=PIECE, is_half=0, B=2, n=500, ldp=500, N0=0, O0=0, final=0, gains=GAINS, h=H, n_taps=81, os=4,
           half_width=10, w=W, lookahead=16, ceiling=0.5, out=OUT, out_cap=500, ldo=500, state=STATE):
        return lib.t2s_limit_window(carry_in, carry_out, piece, is_half, B, n, ldp, N0, O0, final, gains, h, n_taps, os, half_width, w,
                                    lookahead, ceiling, out, out_cap, ldo, state, None)

    for f in (rs, lm):
        assert f(carry_in=None) == -1 and f(carry_out=None) == -1 and f(piece=None) == -1 and f(h=None) == -1 and f(out=None) == -1
        assert f(carry_out=CI) == -1 and f(carry_out=CI + 8) == -1, "the carries overlap"
        assert f(B=0) == -1 and f(B=-1) == -1 and f(B=65536) == -1
        assert f(n=-1) == -1 and f(n=2 ** 31) == -1 and f(ldp=99) == -1
        assert f(out_cap=10) == -1 and f(ldo=10) == -1 and f(ldo=-1) == -1
        assert f(h=H + 4) == -1 and f(carry_in=CI + 2) == -1 and f(carry_out=CO + 1) == -1 and f(out=OUT + 2) == -1
        assert f(piece=PIECE + 2) == -1 and f(piece=PIECE + 1, is_half=1) == -1
    assert rs(K0=-1) == -1 and rs(M0=-1) == -1 and rs(K0=2 ** 40) == -1 and rs(M0=2 ** 40 + 1) == -1
    assert rs(up=0) == -1 and rs(down=0) == -1 and rs(up=-2) == -1 and rs(up=4, down=2, n_taps=81) == -1
    assert rs(up=513, down=1, n_taps=10261) == -1 and rs(up=1, down=513, n_taps=10261) == -1
    assert rs(n_taps=40) == -1 and rs(n_taps=1) == -1 and rs(n_taps=-3) == -1 and rs(up=1, down=1, n_taps=(1 << 20) + 1) == -1
    assert rs(final=1, out_cap=199) == -1, "a final window owes ceil(K1 up / down) outputs"
    assert lm(N0=-1) == -1 and lm(O0=-1) == -1 and lm(N0=2 ** 40) == -1 and lm(O0=501) == -1, "O0 behind what the stream has seen"
    assert lm(w=None) == -1 and lm(state=None) == -1 and lm(w=W + 4) == -1 and lm(state=STATE + 4) == -1 and lm(gains=GAINS + 4) == -1
    assert lm(os=3) == -1 and lm(os=0) == -1 and lm(os=8) == -1 and lm(n_taps=80) == -1 and lm(os=2) == -1
    assert lm(half_width=0, n_taps=1) == -1 and lm(half_width=33, n_taps=265) == -1
    assert lm(lookahead=-1) == -1 and lm(lookahead=1025) == -1
    for c in (0.0, -0.5, float("nan"), float("inf"), 0.1):
        assert lm(ceiling=c) == -1, "the ceiling is a positive finite float32 value"
    assert lm(final=1, out_cap=499) == -1 and lm(out_cap=457) == -1
    PCM = 0x90000
    assert lib.t2s_g711(None, 10, 0, OUT, None) == -1 and lib.t2s_g711(PCM, 10, 0, None, None) == -1
    assert lib.t2s_g711(PCM, 0, 0, OUT, None) == -1 and lib.t2s_g711(PCM, -1, 1, OUT, None) == -1 and lib.t2s_g711(PCM + 1, 10, 0, OUT, None) == -1
    assert lib.t2s_g711(PCM, 10, 2, OUT, None) == -1 and lib.t2s_g711(PCM, 10, -1, OUT, None) == -1


def test_derived_attributes():
    d = audio.DeliveryStream(44800, 8000, encoding="ulaw")
    assert (d.src_rate, d.out_rate, d.up, d.down, d.n_taps) == (44800, 8000, 5, 28, 561)
    assert (d.resample_carry, d.limit_carry, d.latency, d.delivered, d.B) == (113, 0, 10, 0, None)
    lim = audio.Limiter(48000)
    d = audio.DeliveryStream(44800, 48000, limiter=lim, gain=2.0, encoding="pcm16")
    assert (d.up, d.down, d.n_taps, d.resample_carry, d.limit_carry) == (15, 14, 301, 21, 2 * lim.reach)
    assert d.latency == -(-150 // 14) + lim.reach and isinstance(d.latency, int)
    d = audio.DeliveryStream(44800, limiter=audio.Limiter(44800))
    assert (d.out_rate, d.up, d.down, d.resample_carry, d.latency) == (44800, 1, 1, 0, 144)
    assert audio.DeliveryStream(16000, 16000, encoding="alaw").latency == 0
    lib = _lib.load()
    for src, out in ((44800, 48000), (44800, 16000), (44800, 8000), (22050, 48000)):
        d = audio.DeliveryStream(src, out)
        assert d.resample_carry == lib.t2s_resample_window_carry(d.n_taps, d.up)
    assert audio.DeliveryStream(8000, limiter=audio.Limiter(8000)).limit_carry == lib.t2s_limit_window_carry(12, 10)


@pytest.mark.parametrize("args,kw,message", [
    ((0,), {}, "src_rate must be a positive integer"),
    ((44100.5,), {}, "src_rate must be a positive integer"),
    ((True,), {}, "src_rate must be a positive integer"),
    (("48k",), {}, "src_rate must be a positive integer"),
    ((44800, -1), {}, "out_rate must be a positive integer"),
    ((44800, 8000.5), {}, "out_rate must be a positive integer"),
    ((44800, 8000), dict(encoding="mp3"), "encoding must be one of f32, pcm16, ulaw, alaw, got 'mp3'"),
    ((44800, 8000), dict(encoding=None), "encoding must be one of"),
    ((44800,), {}, "nothing to do"),
    ((44800, 44800), {}, "nothing to do"),
    ((44800, 8000), dict(gain=2.0), "gain needs a limiter"),
    ((44800, 8000), dict(limiter="loud"), "limiter must be an audio.Limiter or None, got a str"),
    ((44800, 44101), {}, "is the ratio 44101 / 44800; max\\(up, down\\) may be at most 512"),
])
def test_refused_constructor_arguments(args, kw, message):
    with pytest.raises(T2SError, match="DeliveryStream: .*" + message):
        audio.DeliveryStream(*args, **kw)


def test_refused_limiters_and_gains():
    with pytest.raises(T2SError, match="the limiter was built for 44800 Hz, the delivery rate is 8000 Hz"):
        audio.DeliveryStream(44800, 8000, limiter=audio.Limiter(44800))
    lim = audio.Limiter(8000)
    for gain, message in ((float("nan"), "finite number"), ("2", "finite number"), (True, "finite number"),
                          (torch.ones(2), "must be float64 \\[B\\]"), (torch.ones(2, 1, dtype=torch.float64), "must be float64 \\[B\\]"),
                          (torch.ones(0, dtype=torch.float64), "must be float64 \\[B\\]")):
        with pytest.raises(T2SError, match="DeliveryStream: .*gain.*" + message):
            audio.DeliveryStream(44800, 8000, limiter=lim, gain=gain)
    audio.DeliveryStream(44800, 8000, limiter=lim, gain=0.5)
    audio.DeliveryStream(44800, 8000, limiter=lim, gain=torch.ones(3, dtype=torch.float64))
    assert lim._tables is None, "constructing needs no device"


def test_refused_pushes_and_no_cpu_path():
    d = audio.DeliveryStream(44800, 8000)
    for piece, message in ((np.zeros((1, 10), np.float32), "a piece must be a tensor \\[B, n\\], got a ndarray"),
                           (torch.zeros(10), "a piece must be a tensor \\[B, n\\], got \\(10,\\)"),
                           (torch.zeros(1, 1, 10), "a piece must be a tensor \\[B, n\\]"),
                           (torch.zeros(1, 10, dtype=torch.float64), "expected float32 or float16, got torch.float64"),
                           (torch.zeros(1, 10, dtype=torch.int16), "expected float32 or float16, got torch.int16")):
        with pytest.raises(T2SError, match="DeliveryStream.push: " + message):
            d.push(piece)
    with pytest.raises(RuntimeError, match="expected a tensor in HBM \\(cuda\\); there is no CPU path"):
        d.push(torch.zeros(1, 10))
    with pytest.raises(T2SError, match="there is no CPU path"):
        d.open(1, "cpu")
    with pytest.raises(T2SError, match="nothing has been pushed yet"):
        audio.DeliveryStream(8000, limiter=audio.Limiter(8000)).report()
    with pytest.raises(T2SError, match="the stream has no limiter"):
        d.report()
    assert d.B is None and d.delivered == 0
    for f in (audio.to_ulaw, audio.to_alaw):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            f(torch.zeros(4))


class _Eval:
    training = False


def test_synthesize_stream_checks_delivery_before_anything_runs():
    d = audio.DeliveryStream(44800, 8000)
    with pytest.raises(T2SError, match="delivery= and pcm16=True exclude each other"):
        streaming.synthesize_stream(_Eval(), _Eval(), None, seed=1, pcm16=True, delivery=d)
    with pytest.raises(T2SError, match="delivery must be an audio.DeliveryStream or a callable that makes one, got a int"):
        streaming.synthesize_stream(_Eval(), _Eval(), None, seed=1, delivery=3)
    with pytest.raises(T2SError, match="delivery\\(\\) returned a NoneType"):
        streaming.synthesize_stream(_Eval(), _Eval(), None, seed=1, delivery=lambda: None)
