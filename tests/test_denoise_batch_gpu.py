"""The batch forms of the audio classes (text2speech_amd/audio.py): Denoiser.denoise_batch, STFT.transform_batch / inverse_batch,
TacotronSTFT.mel_spectrogram_batch and to_pcm16.  Every entry of a padded batch gets what it gets alone, bit for bit, and zeros behind
its end.  The audio padding holds 1e4 here (it would wreck a spectrum and trip the range assertion if it were read), the padding of
magnitude and phase handed to inverse_batch holds NaN."""
import os

import numpy as np
import pytest
import torch

from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = synth.WAVEGLOW_SMALL
PAD = 1e4
GOLDEN_BAR = 1e-3       # tests/test_audio_gpu.py::test_denoiser_and_griffin_lim_vs_reference_golden: rel-L2 against the reference's output


def _rel(a, b):
    """relative L2 error of a against b"""
    a = torch.as_tensor(a).double().cpu().flatten()
    b = torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _padded(clip, lengths, value=PAD):
    out = clip.clone()
    for b, n in enumerate(lengths):
        out[b, n:] = value
    return out


@pytest.fixture(scope="module")
def model():
    import text2speech_amd.glow as glow
    assert torch.cuda.is_available()
    _lib.load()
    m = glow.WaveGlow(**CFG)
    m.load_state_dict(synth.waveglow_state(CFG), strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def dn(model):
    from text2speech_amd.audio import Denoiser
    return Denoiser(model).to(DEV)


@pytest.fixture(scope="module")
def clip():
    """the clip of tests/golden/audio_denoise_gl.npz, built as tests/test_audio_gpu.py builds it"""
    gen = torch.Generator().manual_seed(44)
    return torch.rand(2, 4096, generator=gen) * 0.6 - 0.3


@pytest.mark.parametrize("key,strength", [("denoised_s01", 0.1), ("denoised_s10", 1.0)])
def test_golden_entry_0_and_short_entry_1(dn, clip, golden_dir, key, strength):
    """1. entry 0 (full length) against the reference's own Denoiser output; 2. entry 1 (2304 of 4096 samples) bit-equal to forward() of
    its slice, zeros behind, and different from forward() of the padded row in its last 512 samples."""
    g = np.load(os.path.join(golden_dir, "audio_denoise_gl.npz"))
    lengths = [4096, 2304]
    out, alen = dn.denoise_batch(_padded(clip, lengths).to(DEV), lengths, strength)
    assert tuple(out.shape) == (2, 1, 4096) and out.dtype == torch.float32
    assert alen.dtype == torch.int64 and alen.device == out.device and alen.cpu().tolist() == lengths
    e0 = _rel(out[0], g[key][0])
    print("denoise_batch strength %.1f: entry 0 vs the reference's output: rel-L2 %.3e (bar %.0e)" % (strength, e0, GOLDEN_BAR))
    assert e0 < GOLDEN_BAR
    solo = dn(clip[1:2, :2304].to(DEV), strength=strength)
    assert tuple(solo.shape) == (1, 1, 2304)
    assert torch.equal(out[1, 0, :2304].view(torch.int32), solo[0, 0].view(torch.int32)), _rel(out[1, 0, :2304], solo[0, 0])
    assert bool((out[1, 0, 2304:].view(torch.int32) == 0).all())
    # forward() on the row with its padding zeroed (the kindest padding): right up to where the end is felt, wrong in the last 512
    naive = dn(_padded(clip, lengths, 0.0).to(DEV), strength=strength)
    d = (naive[1, 0, :2304] - out[1, 0, :2304]).abs()
    print("forward() on the padded row vs denoise_batch, entry 1: worst |diff| in the last 512 samples %.3e, in front of them %.3e"
          % (float(d[-512:].max()), float(d[:-512].max())))
    assert float(d[-512:].max()) > 0.0
    # entry 0 is not touched by entry 1's being short
    full = dn(clip[0:1].to(DEV), strength=strength)
    assert torch.equal(out[0].view(torch.int32), full[0].view(torch.int32))


def _mel_and_noise(frames, seed):
    gen = torch.Generator().manual_seed(seed)
    B, F_ = len(frames), max(frames)
    L = F_ * 256 // CFG["n_group"]
    n_early = len([k for k in range(CFG["n_flows"]) if k % CFG["n_early_every"] == 0 and k > 0])
    n_rem = CFG["n_group"] - n_early * CFG["n_early_size"]
    mel = torch.randn(B, 80, F_, generator=gen)
    nf = torch.randn(B, n_rem, L, generator=gen)
    ne = [torch.randn(B, CFG["n_early_size"], L, generator=gen) for _ in range(n_early)]
    return mel.to(DEV), (nf.to(DEV), [t.to(DEV) for t in ne])


def _entry(frames, mel, noise, b):
    f, Lb = frames[b], frames[b] * 256 // CFG["n_group"]
    return mel[b:b + 1, :, :f].contiguous(), (noise[0][b:b + 1, :, :Lb].contiguous(), [t[b:b + 1, :, :Lb].contiguous() for t in noise[1]])


@pytest.mark.parametrize("half", [False, True])
def test_chain_infer_batch_denoise_pcm(half):
    """3. infer_batch -> denoise_batch(audio, audio_lengths) -> to_pcm16(..., lengths), both results passed on as returned, against
    infer -> Denoiser.forward -> to_pcm16 of every entry alone (its noise sliced to its columns).  half: the model .half() with float
    1x1 convolutions, so that float16 audio goes in."""
    import text2speech_amd.glow as glow
    from text2speech_amd.audio import Denoiser, to_pcm16
    _lib.load()
    m = glow.WaveGlow(**CFG)
    m.load_state_dict(synth.waveglow_state(CFG), strict=True)
    m = m.to(DEV).eval()
    den = Denoiser(m).to(DEV)                       # (the bias spectrum from the float model, for both)
    if half:
        m = m.half()
        for k in m.convinv:
            k.float()
        # infer() of a .half() model takes the fp16 chain by default and infer_batch() the split-bf16 planes: two arithmetics, whose
        # audio differs in the fourth digit.  The solo run is put on infer_batch's planes, so that the two are comparable at all.
        m._eng().infer_w16 = False
    frames = (12, 7, 3)
    mel, noise = _mel_and_noise(frames, seed=61)
    if half:
        mel = mel.half()
    audio, alen = m.infer_batch(mel, torch.tensor(frames), sigma=0.666, noise=noise)
    assert audio.dtype == (torch.float16 if half else torch.float32) and tuple(audio.shape) == (3, 256 * 12)
    den_audio, dlen = den.denoise_batch(audio, alen, 0.1)
    pcm = to_pcm16(den_audio, dlen)
    assert tuple(den_audio.shape) == (3, 1, 256 * 12) and den_audio.dtype == torch.float32
    assert dlen.dtype == torch.int64 and dlen.cpu().tolist() == [256 * f for f in frames]
    assert pcm.dtype == torch.int16 and pcm.shape == den_audio.shape
    for b, f in enumerate(frames):
        n = 256 * f
        mb, nb = _entry(frames, mel, noise, b)
        solo_audio = m.infer(mb, sigma=0.666, noise=nb)
        same_audio = torch.equal(solo_audio[0], audio[b, :n])
        want_den = den(solo_audio, strength=0.1)
        want = to_pcm16(want_den)
        # the stages this file is about, on the batch's own audio: bit-equal whatever infer_batch and infer make of each other
        stage = to_pcm16(den(audio[b:b + 1, :n], strength=0.1))
        assert torch.equal(pcm[b, 0, :n], stage[0, 0]), "entry %d: denoise_batch + to_pcm16 differ from forward + to_pcm16 on its slice" % b
        diff = int((pcm[b, 0, :n].int() - want[0, 0].int()).abs().max())
        print("chain %s entry %d (%d frames): infer_batch audio bit-equal to infer's: %s; worst PCM difference of the chain %d"
              % ("f16" if half else "f32", b, f, same_audio, diff))
        assert torch.equal(pcm[b, 0, :n], want[0, 0]), "entry %d: the chain differs from the solo chain (worst %d)" % (b, diff)
        assert bool((pcm[b, 0, n:] == 0).all()) and bool((den_audio[b, 0, n:].view(torch.int32) == 0).all())


def test_refusals(model, dn):
    """4. An entry too short for the reflect padding is refused by name before any launch; one case each of the other checks."""
    from text2speech_amd.audio import STFT, TacotronSTFT, to_pcm16
    T2SError = _lib.T2SError
    frames = (12, 2)
    mel, noise = _mel_and_noise(frames, seed=62)
    audio, alen = model.infer_batch(mel, torch.tensor(frames), sigma=0.666, noise=noise)
    seen = []
    real = _lib.call
    _lib.call = lambda name, *a: (seen.append(name), real(name, *a))[1]
    try:
        with pytest.raises(T2SError, match=r"denoise_batch: entry 1 has 512 samples, the minimum is 513"):
            dn.denoise_batch(audio, alen, 0.1)
        x = torch.zeros(2, 4096, device=DEV)
        with pytest.raises(T2SError, match=r"denoise_batch: lengths must be integers, got torch.float32"):
            dn.denoise_batch(x, torch.tensor([4096.0, 2304.0]))
        with pytest.raises(T2SError, match=r"denoise_batch: lengths has shape \(3,\), the batch holds 2"):
            dn.denoise_batch(x, [4096, 2304, 1024])
        with pytest.raises(T2SError, match=r"denoise_batch: entry 0 has 4097 samples, the padded batch holds 4096"):
            dn.denoise_batch(x, [4097, 2304])
        with pytest.raises(T2SError, match=r"denoise_batch: audio must be \[B, T\] or \[B, 1, T\]"):
            dn.denoise_batch(torch.zeros(2, 2, 4096, device=DEV), [4096, 2304])
        st = STFT(1024, 256, 1024).to(DEV)
        with pytest.raises(T2SError, match=r"transform_batch: entry 1 has 512 samples, the minimum is 513"):
            st.transform_batch(x, [4096, 512])
        mag = torch.zeros(2, 513, 17, device=DEV)
        with pytest.raises(T2SError, match=r"inverse_batch: entry 0 has 1 frames, the minimum is 2"):
            st.inverse_batch(mag, mag, torch.tensor([1, 17], device=DEV))
        with pytest.raises(T2SError, match=r"inverse_batch: entry 1 has 18 frames, the padded batch holds 17"):
            st.inverse_batch(mag, mag, [17, 18])
        with pytest.raises(T2SError, match=r"inverse_batch: magnitude and phase must both be"):
            st.inverse_batch(mag, mag[:, :, :16], [17, 17])
        with pytest.raises(T2SError, match=r"mel_spectrogram_batch: lengths must be integers, got torch.bool"):
            TacotronSTFT().to(DEV).mel_spectrogram_batch(x, torch.tensor([True, True]))
        with pytest.raises(T2SError, match=r"to_pcm16: entry 1 has 4097 samples, the padded batch holds 4096"):
            to_pcm16(x, [0, 4097])
        with pytest.raises(T2SError, match=r"to_pcm16: entry 0 has -1 samples, the minimum is 0"):
            to_pcm16(x, [-1, 5])
        with pytest.raises(RuntimeError, match="no CPU path"):
            to_pcm16(torch.zeros(2, 8))
    finally:
        _lib.call = real
    assert seen == [], "a refused call launched: %r" % seen


def test_mel_spectrogram_batch():
    """5. class defaults; clips of (4096, 2300, 600) samples; padding of 1e4."""
    from text2speech_amd.audio import TacotronSTFT
    _lib.load()
    ts = TacotronSTFT().to(DEV)
    lengths = [4096, 2300, 600]
    gen = torch.Generator().manual_seed(80)
    clean = torch.rand(3, 4096, generator=gen) * 1.9 - 0.95
    y = _padded(clean, lengths).to(DEV)
    mel, ml = ts.mel_spectrogram_batch(y, torch.tensor(lengths, device=DEV))
    assert tuple(mel.shape) == (3, 80, 17) and mel.dtype == torch.float32
    assert ml.dtype == torch.int64 and ml.device == mel.device and ml.cpu().tolist() == [1 + n // 256 for n in lengths] == [17, 9, 3]
    for b, n in enumerate(lengths):
        fb = 1 + n // 256
        solo = ts.mel_spectrogram(clean[b:b + 1, :n].to(DEV))
        assert tuple(solo.shape) == (1, 80, fb)
        assert torch.equal(mel[b, :, :fb].contiguous().view(torch.int32), solo[0].view(torch.int32)), (b, _rel(mel[b, :, :fb], solo[0]))
        assert bool((mel[b, :, fb:].contiguous().view(torch.int32) == 0).all()), "entry %d: a column behind its end is not +0" % b
    bad = y.clone()
    bad[1, 1000] = 1.5
    with pytest.raises(AssertionError, match="outside"):
        ts.mel_spectrogram_batch(bad, lengths)
    bad = y.clone()
    bad[2, 599] = -1.5                               # the last valid sample
    with pytest.raises(AssertionError, match="outside"):
        ts.mel_spectrogram_batch(bad, lengths)


def test_round_trip():
    """6. transform_batch -> inverse_batch per entry, bit-equal to transform -> inverse of the slice; NaN in the padding of the
    magnitude and phase handed to inverse_batch."""
    from text2speech_amd.audio import STFT
    _lib.load()
    st = STFT(1024, 256, 1024).to(DEV)
    lengths = [4096, 2300, 600]
    gen = torch.Generator().manual_seed(81)
    clean = torch.rand(3, 4096, generator=gen) - 0.5
    mag, ph, fl = st.transform_batch(_padded(clean, lengths).to(DEV), lengths)
    assert tuple(mag.shape) == tuple(ph.shape) == (3, 513, 17)
    assert fl.dtype == torch.int64 and fl.device == mag.device and fl.cpu().tolist() == [17, 9, 3]
    for b, f in enumerate(fl.cpu().tolist()):
        assert bool((mag[b, :, f:] == 0).all()) and bool((ph[b, :, f:] == 0).all())
    mag_n, ph_n = mag.clone(), ph.clone()
    for b, f in enumerate(fl.cpu().tolist()):
        mag_n[b, :, f:] = float("nan")
        ph_n[b, :, f:] = float("nan")
    out, alen = st.inverse_batch(mag_n, ph_n, fl)                  # the frame lengths as returned (on the device)
    assert tuple(out.shape) == (3, 1, 4096) and alen.dtype == torch.int64 and alen.cpu().tolist() == [4096, 2048, 512]
    for b, n in enumerate(lengths):
        m1, p1 = st.transform(clean[b:b + 1, :n].to(DEV))
        assert torch.equal(mag[b, :, :m1.size(2)], m1[0]) and torch.equal(ph[b, :, :m1.size(2)], p1[0])
        solo = st.inverse(m1, p1)
        nb = solo.size(2)
        assert nb == int(alen[b])
        assert torch.equal(out[b, 0, :nb].view(torch.int32), solo[0, 0].view(torch.int32)), (b, _rel(out[b, 0, :nb], solo[0, 0]))
        assert bool((out[b, 0, nb:].view(torch.int32) == 0).all())
        assert _rel(out[b, 0, 512:nb - 512], clean[b, 512:nb - 512]) < 1e-5 if nb > 1024 else True
