"""t2s_stft_transform, t2s_mel_from_mag and t2s_stft_inverse (csrc/audio_ops.hip, csrc/t2s_api_audio.hip) called directly, with operands
built as text2speech_amd.audio.STFT builds them, at the configurations the class tests never reach: the class defaults (800, 200, 800),
window=None, win_length < filter_length, a hop that does not divide n_fft, a hop past the window (window-sum-square 0), the minimum T,
8 and 9 frames (either side of the GEMV / matrix-core dispatcher), wider leading dimensions.  Every output is compared element by
element with a float64 strided contraction / overlap-add (tests/tail_ref_util.py); the contractions are exact f32, so the bound is
4 x the worst error of the same evaluation in torch float32 on the CPU (4: another summation order).  Waveform bounds are absolute -
scaled by the clip's peak, not by each sample - so the first and the last hop count.  Figures: profiles/tail_kernel_tests.md."""
import math

import numpy as np
import pytest
import torch

import tail_ref_util as R
from text2speech_amd import _lib
from wg_bwd_util import DEV, Guarded, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
TINY = float(np.finfo(np.float32).tiny)

# (n_fft, hop, win_length, window, T, B)
CASES = {
    "min-T": (64, 16, 64, "hann", 33, 1),                 # T = n_fft / 2 + 1: the reflect padding reads every sample; F = 3
    "F8": (64, 16, 64, "hann", 127, 1),                   # the last GEMV item count
    "F9": (64, 16, 64, "hann", 128, 1),                   # the first matrix-core one
    "ragged-T-B3": (64, 16, 64, "hann", 645, 3),          # T no multiple of hop, B > 1
    "hop-20-of-48": (48, 20, 48, "hann", 210, 2),         # 2 or 3 frames per sample; c = 25: ld_rc 64, ld_mt 32
    "class-defaults": (800, 200, 800, "hann", 2000, 1),   # c = 401
    "short-window": (64, 16, 32, "hann", 256, 2),         # centre-padded window
    "hop-past-window": (64, 48, 16, "hann", 480, 2),      # window-sum-square 0 in places
    "no-window": (64, 16, 64, None, 256, 2),              # win_sq == NULL
}


def _st():
    return _lib.current_stream()


def _p(t):
    if t is None:
        return None
    return _lib.ptr(t.t if isinstance(t, Guarded) else t)


def _bits(t):
    return (t.t if isinstance(t, Guarded) else t).view(torch.int32).clone()


def _elementwise(label, got, want, bound):
    got, want = R.f64(got), R.f64(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s: an element is not finite (never written?)" % label
    err = float((got - want).abs().max())
    print("PARITY %-58s worst |err| %.3e  bound %.3e  peak %.3e" % (label, err, bound, float(want.abs().max())))
    assert err <= bound, "%s: worst element-wise error %.3e > %.3e" % (label, err, bound)


def _audio(name):
    n_fft, hop, win, window, T, B = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    t = torch.arange(T).float()
    return 0.4 * torch.rand(B, T, generator=gen) - 0.2 + 0.5 * torch.sin(0.21 * t)[None] * torch.rand(B, 1, generator=gen)


def _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt, want=(True, True, True)):
    B, T = audio_d.shape
    c, F_ = n_fft // 2 + 1, T // hop + 1
    xp, ft = Guarded(B, ldp), Guarded(B, F_, 2 * c)                 # scratch: NaN before the call
    mag = Guarded(B, c, F_) if want[0] else None
    ph = Guarded(B, c, F_) if want[1] else None
    magT = Guarded(B * F_, ld_mt) if want[2] else None
    _lib.call("t2s_stft_transform", _p(audio_d), B, T, _p(fwd_d), n_fft, hop, _p(xp), ldp, _p(ft), _p(mag), _p(ph), _p(magT), ld_mt,
              _st())
    torch.cuda.synchronize()
    for g, name in ((xp, "xp"), (ft, "ft"), (mag, "mag"), (ph, "phase"), (magT, "magT")):
        if g is not None:
            g.assert_guards(name)
    return xp, ft, mag, ph, magT


@pytest.mark.parametrize("name", list(CASES))
def test_stft_transform(name):
    _lib.load()
    n_fft, hop, win, window, T, B = CASES[name]
    c, F_ = n_fft // 2 + 1, T // hop + 1
    audio = _audio(name)
    fwd, _, _ = R.stft_operands(n_fft, hop, win, window)
    (ft64, mag64, ph64), (e_ft, e_mag, _) = R.f32_floor(R.stft_transform_ref, audio, fwd, n_fft, hop)
    e_pol = R.stft_polar_floor(audio, fwd, n_fft, hop)
    audio_d, fwd_d = dev(audio), dev(fwd)
    ldp, ld_mt = R.ru(T + n_fft, 4) + 8, R.ru(c, 16)              # a wider xp than the minimum
    xp, ft, mag, ph, magT = _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt)
    assert torch.equal(xp.t[:, :T + n_fft].cpu(), R.reflect_pad(audio, n_fft)), "xp is not torch's reflect pad, bit for bit"
    assert bool(xp.untouched(xp.t[:, T + n_fft:]).all()), "xp: columns past T + n_fft were written"
    _elementwise(name + " ft", ft.t, ft64, 4 * e_ft)
    _elementwise(name + " mag", mag.t, mag64, 4 * e_mag)
    mc, ms = R.polar(mag.t, ph.t)
    _elementwise(name + " mag cos(phase)", mc, ft64[:, :, :c].transpose(1, 2), 4 * e_pol)
    _elementwise(name + " mag sin(phase)", ms, ft64[:, :, c:].transpose(1, 2), 4 * e_pol)
    # the phase itself where the magnitude is well above rounding: a perturbation d of (re, im) turns the angle by asin(|d| / mag), and
    # atan2f adds a few units in the last place of pi (2^-22)
    big = mag64 > 1e3 * 4 * e_ft
    assert int(big.sum()) > big.numel() // 4
    turn = R.angle_diff(ph.t, ph64)[big] - (1.01 * math.sqrt(2.0) * 4 * e_ft / mag64[big] + 4 * 2.0 ** -22)
    print("PARITY %-58s worst excess over the bound %.3e (of %d bins)" % (name + " phase", float(turn.max()), int(big.sum())))
    assert float(turn.max()) <= 0.0
    assert float(ph.t.abs().max()) <= math.pi + 2.0 ** -22
    # magT: the transpose of mag bit for bit, zero padding columns, at both leading dimensions
    for ld in (ld_mt, ld_mt + 16):
        mt = magT if ld == ld_mt else _transform(audio_d, fwd_d, n_fft, hop, ldp, ld)[4]
        v = mt.t.view(B, F_, ld)
        assert torch.equal(v[:, :, :c].transpose(1, 2).contiguous().view(torch.int32), _bits(mag)), ld
        assert bool((v[:, :, c:].view(torch.int32) == 0).all()), "magT: a padding column is not +0 (ld_mt %d)" % ld
    # each optional output NULL in turn: the others keep their bits
    full = [_bits(mag), _bits(ph), _bits(magT)]
    for skip in range(3):
        outs = _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt, want=tuple(i != skip for i in range(3)))[2:]
        for i in range(3):
            if i != skip:
                assert torch.equal(_bits(outs[i]), full[i]), (skip, i)
    # silence: magnitude and phase exactly zero
    _, ft0, mag0, ph0, magT0 = _transform(torch.zeros_like(audio_d), fwd_d, n_fft, hop, ldp, ld_mt)
    assert float(mag0.t.abs().max()) == 0.0 and float(ph0.t.abs().max()) == 0.0 and float(magT0.t.abs().max()) == 0.0


@pytest.mark.parametrize("F_", [1, 8, 9, 33])
@pytest.mark.parametrize("n_mel", [1, 17, 80])
def test_mel_from_mag(n_mel, F_):
    """B = 2, c = 33 bins in rows of 48.  Frames 0 of the second clip (and 2 .. 4 where there are as many) are silent: log(clip) there.
    The log-domain bound is absolute: 4 x the float32 evaluation's error plus one unit in the last place of an f32 logarithm below 16."""
    _lib.load()
    B, c, ld = 2, 33, 48
    gen = torch.Generator().manual_seed(1000 * n_mel + F_)
    mag = 10.0 ** (torch.rand(B, F_, c, generator=gen) * 5 - 4)
    mag[1, 0] = 0.0
    if F_ >= 5:
        mag[:, 2:5] = 0.0
    magT = torch.zeros(B * F_, ld)
    magT[:, :c] = mag.view(B * F_, c)
    basis = torch.zeros(n_mel, ld)
    basis[:, :c] = torch.rand(n_mel, c, generator=gen) * (torch.rand(n_mel, c, generator=gen) < 0.3).float() * 0.05
    basis[0, 0] = 0.01
    magT_d, basis_d = dev(magT), dev(basis)
    tag = "mel_from_mag n_mel %d F %d" % (n_mel, F_)

    def run(clip):
        mel = Guarded(B, n_mel, F_)
        _lib.call("t2s_mel_from_mag", _p(magT_d), ld, B, F_, _p(basis_d), n_mel, clip, _p(mel), _st())
        torch.cuda.synchronize()
        mel.assert_guards(tag)
        return mel

    want, e32 = R.f32_floor(R.mel_ref, magT, basis, B, F_, 1e-5)
    mel = run(1e-5)
    _elementwise(tag + " log", mel.t, want, 4 * e32 + 2.0 ** -20)
    silent = torch.zeros(B, F_, dtype=torch.bool)
    silent[1, 0] = True
    if F_ >= 5:
        silent[:, 2:5] = True
    floor = mel.t.cpu().transpose(1, 2)[silent]
    # the kernel takes the logarithm in double and rounds once: the f32 nearest to log of the f32 clip, bit for bit
    pin = torch.tensor(math.log(float(np.float32(1e-5))), dtype=torch.float32)
    assert bool((floor.view(torch.int32) == pin.view(torch.int32)).all()), "silent frames: %r, not %r" % (float(floor[0, 0]), float(pin))
    want_raw, e_raw = R.f32_floor(R.mel_ref, magT, basis, B, F_, 0.0)
    raw = run(0.0)
    _elementwise(tag + " raw product (clip 0)", raw.t, want_raw, 4 * e_raw)
    assert torch.equal(_bits(run(-1.0)), _bits(raw))
    assert float(raw.t.cpu().transpose(1, 2)[silent].abs().max()) == 0.0


def _inverse(mag_d, ph_d, inv_d, n_fft, hop, win_sq_d, bias_d=None, strength=0.0):
    B, c, F_ = mag_d.shape
    ld_rc = inv_d.size(1)
    rc, frames = Guarded(B * F_, ld_rc), Guarded(B, F_, n_fft)      # scratch: NaN before the call
    out = Guarded(B, hop * (F_ - 1))
    _lib.call("t2s_stft_inverse", _p(mag_d), _p(ph_d), B, F_, n_fft, hop, _p(inv_d), ld_rc, _p(bias_d), strength, _p(win_sq_d), TINY,
              _p(rc), _p(frames), _p(out), _st())
    torch.cuda.synchronize()
    for g, name in ((rc, "rc"), (frames, "frames"), (out, "out")):
        g.assert_guards(name)
    assert bool(torch.isfinite(rc.t).all()) and bool(torch.isfinite(frames.t).all()), "scratch not overwritten completely"
    assert float(rc.t[:, 2 * c:].abs().max()) == 0.0 if ld_rc > 2 * c else True
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_stft_inverse_of_a_transform(name):
    """The spectrogram of a clip (float32 on the CPU) back to a waveform, every sample against float64 overlap-add."""
    _lib.load()
    n_fft, hop, win, window, T, B = CASES[name]
    fwd, inv_t, win_sq = R.stft_operands(n_fft, hop, win, window)
    assert inv_t.size(1) == R.ru(n_fft + 2, 16)
    _, mag, ph = R.stft_transform_ref(_audio(name), fwd, n_fft, hop, dtype=torch.float32)
    want, e32 = R.f32_floor(R.stft_inverse_ref, mag, ph, inv_t, n_fft, hop, win_sq)
    out = _inverse(dev(mag), dev(ph), dev(inv_t), n_fft, hop, dev(win_sq) if win_sq is not None else None)
    _elementwise(name + " inverse (F %d)" % mag.size(2), out.t, want, 4 * e32)
    if name == "hop-past-window":
        ws = torch.zeros(n_fft + hop * (mag.size(2) - 1))
        for f in range(mag.size(2)):
            ws[f * hop:f * hop + n_fft] += win_sq
        ws = ws[n_fft // 2:n_fft // 2 + want.size(1)]
        assert bool((ws == 0).any()) and bool((ws > 0).any())          # both sides of the `wss > tiny` branch are in the output


@pytest.mark.parametrize("F_", [2, 8, 9, 33])
def test_stft_inverse_frame_counts_and_bias(F_):
    """(64, 16, 64, hann) with random magnitudes and phases at 2, 8, 9 and 33 frames (GEMV up to 8, matrix cores from 9), a wider ld_rc,
    and the denoiser's fused subtraction: strength 0 = no bias bit for bit, a strength that clamps every bin = silence, and one in
    between against the float64 clamp."""
    _lib.load()
    n_fft, hop, B, c = 64, 16, 2, 33
    gen = torch.Generator().manual_seed(F_)
    mag = torch.rand(B, c, F_, generator=gen) * 2.0
    ph = torch.rand(B, c, F_, generator=gen) * (2 * math.pi) - math.pi
    bias = torch.rand(c, generator=gen) + 0.1
    for ld_rc in (80, 96):
        _, inv_t, win_sq = R.stft_operands(n_fft, hop, n_fft, "hann", ld_rc=ld_rc)
        args = (dev(mag), dev(ph), dev(inv_t), n_fft, hop, dev(win_sq))
        tag = "inverse F %d ld_rc %d" % (F_, ld_rc)
        want, e32 = R.f32_floor(R.stft_inverse_ref, mag, ph, inv_t, n_fft, hop, win_sq)
        plain = _inverse(*args)
        _elementwise(tag, plain.t, want, 4 * e32)
        bias_d = dev(bias)
        assert torch.equal(_bits(_inverse(*args, bias_d=bias_d, strength=0.0)), _bits(plain)), "strength 0 is not the plain inverse"
        assert float(_inverse(*args, bias_d=bias_d, strength=1e6).t.abs().max()) == 0.0, "every bin clamped: not silence"
        want_b, e_b = R.f32_floor(R.stft_inverse_ref, mag, ph, inv_t, n_fft, hop, win_sq, bias=bias, strength=0.75)
        assert float((want_b - want).abs().max()) > 0.05 * float(want.abs().max())
        _elementwise(tag + " bias x 0.75", _inverse(*args, bias_d=bias_d, strength=0.75).t, want_b, 4 * e_b)


def test_audio_refusals():
    """T2S_EINVAL with nothing written."""
    lib = _lib.load()
    n_fft, hop, T, B = 64, 16, 128, 1
    c, F_ = 33, 9
    fwd, inv_t, win_sq = [dev(t) for t in R.stft_operands(n_fft, hop, n_fft, "hann")]
    audio = torch.zeros(B, 8192, device=DEV)
    outs = [Guarded(B, 8192 + 4112), Guarded(B, 600, 2 * c), Guarded(B, c, 600), Guarded(B, c, 600), Guarded(B * 600, 48)]
    before = [_bits(g) for g in outs]

    def tr(T=T, n_fft=n_fft, hop=hop, ldp=None, ld_mt=48, basis=fwd):
        ldp = R.ru(T + n_fft, 4) if ldp is None else ldp
        return lib.t2s_stft_transform(_p(audio), B, T, _p(basis), n_fft, hop, _p(outs[0]), ldp, _p(outs[1]), _p(outs[2]), _p(outs[3]),
                                      _p(outs[4]), ld_mt, _st())

    for kw in (dict(T=n_fft // 2), dict(n_fft=72), dict(hop=18), dict(ldp=T + n_fft - 4),
               dict(ldp=T + n_fft + 2), dict(ld_mt=32), dict(ld_mt=40)):
        assert tr(**kw) == EINVAL, kw
    # n_fft > 4096 on its own: T = 8192 > n_fft / 2, ldp = T + n_fft, no magT (so no ld_mt rule), buffers sized for n_fft = 4112;
    # the same call at n_fft = 4096 is accepted, so nothing else refuses
    big_basis = torch.zeros(2 * 2057 * 4112, device=DEV)
    big_xp, big_ft = Guarded(B, 8192 + 4112), Guarded(B, 8192 // 16 + 1, 2 * 2057)

    def limit(n):
        return lib.t2s_stft_transform(_p(audio), B, 8192, _p(big_basis), n, 16, _p(big_xp), 8192 + n, _p(big_ft), None, None, None, 0, _st())

    assert limit(4112) == EINVAL
    torch.cuda.synchronize()
    assert bool(big_xp.untouched(big_xp.t).all()) and bool(big_ft.untouched(big_ft.t).all()), "a refused call wrote"
    assert limit(4096) == 0
    torch.cuda.synchronize()
    big_xp.assert_guards("xp at n_fft 4096")
    big_ft.assert_guards("ft at n_fft 4096")
    assert float(big_ft.t.flatten()[:513 * 4098].abs().max()) == 0.0 and bool(big_ft.untouched(big_ft.t.flatten()[513 * 4098:]).all())
    mag, ph = torch.ones(B, c, F_, device=DEV), torch.zeros(B, c, F_, device=DEV)
    iouts = [Guarded(B * F_, 80), Guarded(B, F_, n_fft), Guarded(B, hop * (F_ - 1))]
    ibefore = [_bits(g) for g in iouts]

    def inv(F=F_, ld_rc=80):
        return lib.t2s_stft_inverse(_p(mag), _p(ph), B, F, n_fft, hop, _p(inv_t), ld_rc, None, 0.0, _p(win_sq), TINY, _p(iouts[0]),
                                    _p(iouts[1]), _p(iouts[2]), _st())

    for kw in (dict(F=1), dict(ld_rc=64), dict(ld_rc=48)):
        assert inv(**kw) == EINVAL, kw
    # the batch index is a grid y / z dimension: B = 65536 is refused, not left to fail at the launch
    big_B = 65536
    assert lib.t2s_stft_transform(_p(audio), big_B, T, _p(fwd), n_fft, hop, _p(outs[0]), R.ru(T + n_fft, 4), _p(outs[1]), _p(outs[2]),
                                  _p(outs[3]), _p(outs[4]), 48, _st()) == EINVAL
    assert lib.t2s_stft_inverse(_p(mag), _p(ph), big_B, F_, n_fft, hop, _p(inv_t), 80, None, 0.0, _p(win_sq), TINY, _p(iouts[0]),
                                _p(iouts[1]), _p(iouts[2]), _st()) == EINVAL
    # t2s_mel_from_mag: rows of no columns
    basis, mel = torch.zeros(17, 48, device=DEV), Guarded(B, 17, F_)
    outs.append(mel)
    before.append(_bits(mel))
    assert lib.t2s_mel_from_mag(_p(outs[4]), 0, B, F_, _p(basis), 17, 1e-5, _p(mel), _st()) == EINVAL
    # the partners that take lengths refuse a NULL device array and a NULL host copy
    ld, lh = torch.full((B,), T, dtype=torch.int32, device=DEV), torch.full((B,), T, dtype=torch.int32)
    fd, fh = torch.full((B,), F_, dtype=torch.int32, device=DEV), torch.full((B,), F_, dtype=torch.int32)
    for d, h in ((None, lh), (ld, None)):
        assert lib.t2s_stft_transform_ragged(_p(audio), B, T, _p(d), _p(h), _p(fwd), n_fft, hop, _p(outs[0]), R.ru(T + n_fft, 4),
                                             _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(outs[4]), 48, _st()) == EINVAL
    for d, h in ((None, fh), (fd, None)):
        assert lib.t2s_mel_from_mag_ragged(_p(outs[4]), 48, B, F_, _p(d), _p(h), _p(basis), 17, 1e-5, _p(mel), _st()) == EINVAL
        assert lib.t2s_stft_inverse_ragged(_p(mag), _p(ph), B, F_, _p(d), _p(h), n_fft, hop, _p(inv_t), 80, None, 0.0, _p(win_sq), TINY,
                                           _p(iouts[0]), _p(iouts[1]), _p(iouts[2]), _st()) == EINVAL
    torch.cuda.synchronize()
    for g, b in zip(outs + iouts, before + ibefore):
        assert torch.equal(_bits(g), b), "a refused call wrote"
    assert tr() == 0 and inv() == 0                                   # the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert not torch.equal(_bits(iouts[2]), ibefore[2])
