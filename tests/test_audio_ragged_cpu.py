"""tests/audio_ragged_ref.py pinned on the CPU - equal lengths reproduce the unragged references exactly, shortening one entry changes no
element of another, the PCM reference is numpy's astype('int16') for in-range values - and, where there is no GPU, the argument
checks of the four entry points that take per-entry lengths: each refusal returns T2S_EINVAL before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import audio_ragged_ref as G
import tail_ref_util as R

N_FFT, HOP, T, B = 64, 16, 645, 3
C, F_ = N_FFT // 2 + 1, T // HOP + 1


@pytest.fixture(scope="module")
def ops():
    fwd, inv_t, win_sq = R.stft_operands(N_FFT, HOP, N_FFT, "hann")
    gen = torch.Generator().manual_seed(5)
    audio = torch.rand(B, T, generator=gen) - 0.5
    return dict(fwd=fwd, inv_t=inv_t, win_sq=win_sq, audio=audio)


def _magT(mag, ld):
    b, c, f = mag.shape
    out = torch.zeros(b * f, ld, dtype=mag.dtype)
    out[:, :c] = mag.transpose(1, 2).reshape(b * f, c)
    return out


def test_equal_lengths_are_the_unragged_references(ops):
    full = [T] * B
    want = R.stft_transform_ref(ops["audio"], ops["fwd"], N_FFT, HOP)
    got = G.stft_transform_ragged_ref(ops["audio"], full, ops["fwd"], N_FFT, HOP)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    _, mag, ph = want
    basis = torch.zeros(7, 48, dtype=torch.float64)
    basis[:, :C] = torch.rand(7, C, generator=torch.Generator().manual_seed(6)).double()
    magT = _magT(mag, 48)
    for clip in (1e-5, 0.0):
        assert torch.equal(G.mel_ragged_ref(magT, basis, B, F_, [F_] * B, clip), R.mel_ref(magT, basis, B, F_, clip))
    bias = torch.rand(C, generator=torch.Generator().manual_seed(7)) * 0.5
    for kw in (dict(), dict(bias=bias, strength=0.75)):
        assert torch.equal(G.stft_inverse_ragged_ref(mag, ph, [F_] * B, ops["inv_t"], N_FFT, HOP, ops["win_sq"], **kw),
                           R.stft_inverse_ref(mag, ph, ops["inv_t"], N_FFT, HOP, ops["win_sq"], **kw))


def test_shortening_one_entry_changes_no_other(ops):
    """... and the shortened entry is its own slice's result with zeros behind, whatever its padding holds (NaN here)."""
    audio = ops["audio"].clone()
    base = G.stft_transform_ragged_ref(audio, [T, T, T], ops["fwd"], N_FFT, HOP)
    audio[1, 127:] = float("nan")
    short = G.stft_transform_ragged_ref(audio, [T, 127, T], ops["fwd"], N_FFT, HOP)
    for s, w in zip(short, base):
        assert torch.equal(s[0], w[0]) and torch.equal(s[2], w[2])
        assert bool(torch.isfinite(s).all())
    ft, mag, ph = short
    assert G.frame_counts([T, 127, T], HOP) == [F_, 8, F_]
    assert float(mag[1, :, 8:].abs().max()) == 0.0 and float(ph[1, :, 8:].abs().max()) == 0.0 and float(ft[1, 8:].abs().max()) == 0.0
    alone = R.stft_transform_ref(ops["audio"][1:2, :127].contiguous(), ops["fwd"], N_FFT, HOP)
    assert torch.equal(mag[1, :, :8], alone[1][0]) and torch.equal(ph[1, :, :8], alone[2][0])
    # the padded-row transform differs from the entry alone in its last frames: the reflection is about another sample
    padded = R.stft_transform_ref(ops["audio"][1:2], ops["fwd"], N_FFT, HOP)[1][0, :, :8]
    assert float((padded[:, 7] - mag[1, :, 7]).abs().max()) > 1e-3
    assert float((padded[:, :5] - mag[1, :, :5]).abs().max()) < 1e-12           # (frames that end below sample 127)
    # inverse: frames behind the end hold NaN and do not reach a sample; the other entries keep every bit
    _, mag_f, ph_f = base
    mag_n, ph_n = mag_f.clone(), ph_f.clone()
    mag_n[1, :, 8:] = float("nan")
    ph_n[1, :, 8:] = float("nan")
    full = G.stft_inverse_ragged_ref(mag_f, ph_f, [F_] * B, ops["inv_t"], N_FFT, HOP, ops["win_sq"])
    rag = G.stft_inverse_ragged_ref(mag_n, ph_n, [F_, 8, F_], ops["inv_t"], N_FFT, HOP, ops["win_sq"])
    assert torch.equal(rag[0], full[0]) and torch.equal(rag[2], full[2])
    assert bool(torch.isfinite(rag).all()) and float(rag[1, HOP * 7:].abs().max()) == 0.0
    # A consistent spectrogram gives the signal back however many frames add to a sample, so the two agree to rounding here ...
    tail = slice(HOP * 7 - N_FFT // 2, HOP * 7)
    assert float((rag[1, tail] - full[1, tail]).abs().max()) < 1e-6
    assert float((rag[1, :HOP * 7 - N_FFT] - full[1, :HOP * 7 - N_FFT]).abs().max()) < 1e-12
    # ... but not once the denoiser's subtraction has changed it: the last n_fft / 2 valid samples then depend on which frames count
    bias = torch.full((C,), 0.5)
    full_b = G.stft_inverse_ragged_ref(mag_f, ph_f, [F_] * B, ops["inv_t"], N_FFT, HOP, ops["win_sq"], bias=bias, strength=1.0)
    rag_b = G.stft_inverse_ragged_ref(mag_n, ph_n, [F_, 8, F_], ops["inv_t"], N_FFT, HOP, ops["win_sq"], bias=bias, strength=1.0)
    assert float((rag_b[1, tail] - full_b[1, tail]).abs().max()) > 1e-3
    assert float((rag_b[1, :HOP * 7 - N_FFT] - full_b[1, :HOP * 7 - N_FFT]).abs().max()) < 1e-12
    assert torch.equal(rag_b[0], full_b[0]) and float(rag_b[1, HOP * 7:].abs().max()) == 0.0
    # mel: zeros, not log(clip), behind
    basis = torch.zeros(5, 48, dtype=torch.float64)
    basis[:, :C] = 0.01
    magT = _magT(mag_n, 48)
    mel = G.mel_ragged_ref(magT, basis, B, F_, [F_, 8, F_], 1e-5)
    assert bool(torch.isfinite(mel).all()) and float(mel[1, :, 8:].abs().max()) == 0.0
    assert torch.equal(mel[0], R.mel_ref(_magT(mag_f, 48), basis, B, F_, 1e-5)[0])


def test_pcm_reference():
    gen = np.random.RandomState(3)
    x = (gen.uniform(-1, 1, (3, 1001)) * (32767.0 / 32768.0)).astype(np.float32)
    x[0, :6] = [0.0, -0.0, 1.0 / 32768, -1.0 / 32768, 0.999969482421875, -0.999969482421875]
    assert np.abs(x).max() * 32768 < 32768
    want = (x * 32768).astype("int16")                  # the reference's own conversion, defined for in-range values
    assert np.array_equal(G.pcm16_ref(x), want)
    assert np.array_equal(G.pcm16_ref(torch.from_numpy(x)), want)
    h = x.astype(np.float16)
    h = np.clip(h, -0.99951171875, 0.99951171875)       # the largest fp16 below 1
    assert np.array_equal(G.pcm16_ref(torch.from_numpy(h)), (h.astype(np.float32) * 32768).astype("int16"))
    # truncation toward zero, saturation, NaN, lengths
    e = np.array([[100.5 / 32768, -100.5 / 32768, 1.0, -1.0, 3.0, -3.0, np.nan, np.inf, -np.inf, -32767.5 / 32768]], dtype=np.float32)
    assert G.pcm16_ref(e).tolist() == [[100, -100, 32767, -32768, 32767, -32768, 0, 32767, -32768, -32767]]
    assert G.pcm16_ref(e, [3]).tolist() == [[100, -100, 32767, 0, 0, 0, 0, 0, 0, 0]]
    assert G.pcm16_ref(e, [0]).tolist() == [[0] * 10]


# ---- argument checks of the entry points, with made-up device pointers: only where there is no device ---------------------------------
def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _addr(a):
    return ctypes.cast(a, ctypes.c_void_p)


def test_entry_points_refuse_before_any_launch():
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only on a machine without a GPU")
    from text2speech_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = [0x10000 * (i + 1) for i in range(12)]          # made-up, distinct, aligned
    DEVL = 0x900000                                     # the device copy of the lengths: never read on the host

    def tr(host, lengths=DEVL, Bn=2, Tn=T):
        return lib.t2s_stft_transform_ragged(P[0], Bn, Tn, lengths, None if host is None else _addr(host), P[1], N_FFT, HOP, P[2],
                                             R.ru(Tn + N_FFT, 4), P[3], P[4], P[5], P[6], 48, None)

    ok = _ints(T, 100)
    assert tr(ok, lengths=None) == -1, "NULL lengths"
    assert tr(None) == -1, "NULL lengths_host"
    assert tr(_ints(T, N_FFT // 2)) == -1, "a length of n_fft / 2"
    assert tr(_ints(N_FFT // 2, T)) == -1
    assert tr(_ints(T + 1, 100)) == -1, "a length above T"
    assert tr(_ints(T, 0)) == -1 and tr(_ints(-5, T)) == -1

    def mel(host, frames=DEVL, Fn=F_):
        return lib.t2s_mel_from_mag_ragged(P[0], 48, 2, Fn, frames, None if host is None else _addr(host), P[1], 80, 1e-5, P[2], None)

    assert mel(_ints(F_, 3), frames=None) == -1 and mel(None) == -1
    assert mel(_ints(F_, 0)) == -1, "a frame count of 0"
    assert mel(_ints(F_ + 1, 3)) == -1, "a frame count of F + 1"

    def inv(host, frames=DEVL, Fn=F_):
        return lib.t2s_stft_inverse_ragged(P[0], P[1], 2, Fn, frames, None if host is None else _addr(host), N_FFT, HOP, P[2], 80,
                                           None, 0.0, P[3], 1e-38, P[4], P[5], P[6], None)

    assert inv(_ints(F_, 3), frames=None) == -1 and inv(None) == -1
    assert inv(_ints(F_, 0)) == -1, "a frame count of 0"
    assert inv(_ints(1, F_)) == -1, "a frame count of 1"
    assert inv(_ints(F_, F_ + 1)) == -1, "a frame count of F + 1"
    # the partner's own rules still hold
    assert inv(_ints(2, 2), Fn=1) == -1
    assert tr(_ints(20, 20), Tn=N_FFT // 2) == -1
    # t2s_pcm16: lengths may be NULL, the rest may not
    assert lib.t2s_pcm16(None, 0, 1, 8, 8, None, P[1], None) == -1
    assert lib.t2s_pcm16(P[0], 0, 1, 8, 8, None, None, None) == -1
    assert lib.t2s_pcm16(P[0], 0, 0, 8, 8, None, P[1], None) == -1
    assert lib.t2s_pcm16(P[0], 0, 1, 0, 8, None, P[1], None) == -1
    assert lib.t2s_pcm16(P[0], 1, 2, 8, 7, None, P[1], None) == -1, "ldx below N"
