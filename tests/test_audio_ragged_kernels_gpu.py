"""t2s_stft_transform_ragged, t2s_mel_from_mag_ragged, t2s_stft_inverse_ragged and t2s_pcm16 (csrc/audio_ops.hip, csrc/t2s_api_audio.hip)
called directly on guarded buffers.  The promise under test: every entry of a padded batch gets, BIT FOR BIT, what its unragged partner
entry point gives it alone (same leading dimensions), whatever the padding holds - the audio padding is NaN here, and so are the frames
behind an entry's end that the inverse is handed - and +0 behind its end.  The same outputs against the float64 per-entry references
of tests/audio_ragged_ref.py, with the bound of tests/test_audio_kernels_gpu.py: 4 x the float32 CPU floor (R.f32_floor).

Lengths sit at the minimum T (n_fft / 2 + 1), at 8 and 9 frames (the last item count of the GEMV path, the first of the matrix cores:
the contractions are launched per entry at the entry's own item count, which is what keeps the bits) and at T, no multiple of the hop;
each case runs in two entry orders, so that the short entry is first and last in memory.  Figures: profiles/audio_ragged_tests.md."""
import numpy as np
import pytest
import torch

import audio_ragged_ref as G
import tail_ref_util as R
from text2speech_amd import _lib
from wg_bwd_util import DEV, Guarded, dev

pytestmark = pytest.mark.gpu
TINY = float(np.finfo(np.float32).tiny)
NAN = float("nan")

# name -> (n_fft, hop, win_length, window, lengths: the minimum, 8 frames, 9 frames, T)
CASES = {
    "64-16": (64, 16, 64, "hann", (33, 127, 128, 645)),
    "48-20": (48, 20, 48, "hann", (25, 159, 160, 215)),
    "64-48-wss0": (64, 48, 16, "hann", (33, 383, 384, 485)),          # window-sum-square 0 in places; the minimum is 1 frame
    "64-16-nowin": (64, 16, 64, None, (33, 127, 128, 645)),
    "1024-256": (1024, 256, 1024, "hann", (768, 2304, 4096)),         # the Denoiser's defaults: 4, 10 and 17 frames
}
RUNS = [(n, o) for n in CASES for o in ((0, 1) if n != "1024-256" else (0,))]


def _st():
    return _lib.current_stream()


def _p(t):
    if t is None:
        return None
    return _lib.ptr(t.t if isinstance(t, Guarded) else t)


def _bits(t):
    return (t.t if isinstance(t, Guarded) else t).contiguous().view(torch.int32).cpu()


def _same(label, got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    n = int((g != w).sum())
    assert n == 0, "%s: %d of %d elements differ in their bits" % (label, n, g.numel())


def _zeros(label, t):
    if t.numel():
        assert bool((_bits(t) == 0).all()), "%s: an element behind the entry's end is not +0" % label


def _elementwise(label, got, want, bound):
    got, want = R.f64(got), R.f64(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s: an element is not finite" % label
    err = float((got - want).abs().max())
    print("PARITY %-64s worst |err| %.3e  bound %.3e  peak %.3e" % (label, err, bound, float(want.abs().max())))
    assert err <= bound, "%s: worst element-wise error %.3e > %.3e" % (label, err, bound)


def _lens(values):
    h = torch.tensor(list(values), dtype=torch.int32)
    return h.to(DEV), h


def _case(name, order):
    n_fft, hop, win, window, lengths = CASES[name]
    lengths = list(lengths[::-1] if order else lengths)
    T = max(lengths)
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    t = torch.arange(T).float()
    clean = 0.4 * torch.rand(len(lengths), T, generator=gen) - 0.2 + 0.5 * torch.sin(0.21 * t)[None] * torch.rand(len(lengths), 1,
                                                                                                              generator=gen)
    if order:
        clean = clean.flip(0)                      # the same clip for the same length in both orders
    return n_fft, hop, win, window, lengths, T, clean


def _pad(clean, lengths, value):
    out = clean.clone()
    for b, n in enumerate(lengths):
        out[b, n:] = value
    return out


# ---- the entry points on guarded buffers --------------------------------------------------------------------------------------------
def _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt, lengths=None, want=(True, True, True)):
    """t2s_stft_transform (lengths None) or its ragged partner: (mag, phase, magT) Guarded; guards checked."""
    B, T = audio_d.shape
    c, F_ = n_fft // 2 + 1, T // hop + 1
    xp, ft = Guarded(B, ldp), Guarded(B, F_, 2 * c)
    mag = Guarded(B, c, F_) if want[0] else None
    ph = Guarded(B, c, F_) if want[1] else None
    magT = Guarded(B * F_, ld_mt) if want[2] else None
    if lengths is None:
        _lib.call("t2s_stft_transform", _p(audio_d), B, T, _p(fwd_d), n_fft, hop, _p(xp), ldp, _p(ft), _p(mag), _p(ph), _p(magT), ld_mt,
                  _st())
    else:
        ld, lh = _lens(lengths)
        _lib.call("t2s_stft_transform_ragged", _p(audio_d), B, T, _p(ld), _p(lh), _p(fwd_d), n_fft, hop, _p(xp), ldp, _p(ft), _p(mag),
                  _p(ph), _p(magT), ld_mt, _st())
    torch.cuda.synchronize()
    for g, nm in ((xp, "xp"), (ft, "ft"), (mag, "mag"), (ph, "phase"), (magT, "magT")):
        if g is not None:
            g.assert_guards(nm)
    return mag, ph, magT


def _inverse(mag_d, ph_d, inv_d, n_fft, hop, win_sq_d, frames=None, bias_d=None, strength=0.0):
    B, c, F_ = mag_d.shape
    ld_rc = inv_d.size(1)
    rc, fb, out = Guarded(B * F_, ld_rc), Guarded(B, F_, n_fft), Guarded(B, hop * (F_ - 1))
    if frames is None:
        _lib.call("t2s_stft_inverse", _p(mag_d), _p(ph_d), B, F_, n_fft, hop, _p(inv_d), ld_rc, _p(bias_d), strength, _p(win_sq_d), TINY,
                  _p(rc), _p(fb), _p(out), _st())
    else:
        fd, fh = _lens(frames)
        _lib.call("t2s_stft_inverse_ragged", _p(mag_d), _p(ph_d), B, F_, _p(fd), _p(fh), n_fft, hop, _p(inv_d), ld_rc, _p(bias_d),
                  strength, _p(win_sq_d), TINY, _p(rc), _p(fb), _p(out), _st())
    torch.cuda.synchronize()
    for g, nm in ((rc, "rc"), (fb, "frames"), (out, "out")):
        g.assert_guards(nm)
    return out


def _mel(magT_d, ld, B, F_, basis_d, n_mel, clip, frames=None):
    mel = Guarded(B, n_mel, F_)
    if frames is None:
        _lib.call("t2s_mel_from_mag", _p(magT_d), ld, B, F_, _p(basis_d), n_mel, clip, _p(mel), _st())
    else:
        fd, fh = _lens(frames)
        _lib.call("t2s_mel_from_mag_ragged", _p(magT_d), ld, B, F_, _p(fd), _p(fh), _p(basis_d), n_mel, clip, _p(mel), _st())
    torch.cuda.synchronize()
    mel.assert_guards("mel")
    return mel


# ---- transform ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", RUNS)
def test_stft_transform_ragged(name, order):
    _lib.load()
    n_fft, hop, win, window, lengths, T, clean = _case(name, order)
    B, c, F_ = len(lengths), n_fft // 2 + 1, T // hop + 1
    fr = G.frame_counts(lengths, hop)
    fwd, _, _ = R.stft_operands(n_fft, hop, win, window)
    fwd_d = dev(fwd)
    ldp, ld_mt = R.ru(T + n_fft, 4), R.ru(c, 16)
    audio_d = dev(_pad(clean, lengths, NAN))
    mag, ph, magT = _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt, lengths)
    tag = "%s order %d" % (name, order)
    mt = magT.t.view(B, F_, ld_mt)
    # 1. bit equality with the partner on the entry alone; 3. +0 behind
    zero_row = dev(_pad(clean, lengths, 0.0))
    pm, pp, _ = _transform(zero_row, fwd_d, n_fft, hop, ldp, ld_mt)              # what the padded row would have given
    for b, (n, fb) in enumerate(zip(lengths, fr)):
        sm, sp, smt = _transform(dev(clean[b:b + 1, :n]), fwd_d, n_fft, hop, ldp, ld_mt)
        _same(tag + " mag entry %d" % b, mag.t[b, :, :fb], sm.t[0])
        _same(tag + " phase entry %d" % b, ph.t[b, :, :fb], sp.t[0])
        _same(tag + " magT entry %d" % b, mt[b, :fb], smt.t)
        _same(tag + " last frame of entry %d" % b, mag.t[b, :, fb - 1], sm.t[0, :, fb - 1])
        _zeros(tag + " mag %d" % b, mag.t[b, :, fb:])
        _zeros(tag + " phase %d" % b, ph.t[b, :, fb:])
        _zeros(tag + " magT %d" % b, mt[b, fb:])
        if n < T:
            d = float((pm.t[b, :, fb - 1] - mag.t[b, :, fb - 1]).abs().max())
            print("BITES  %-64s padded-row transform, last frame of entry %d (len %d): worst |diff| %.3e" % (tag, b, n, d))
            if win == n_fft and (fb - 1) * hop + n_fft // 2 > n:          # (a centre-padded window may end in front of the entry's end)
                assert d > 0.0
    # 2. against float64
    (ft64, mag64, ph64), (e_ft, e_mag, _) = R.f32_floor(G.stft_transform_ragged_ref, clean, lengths, fwd, n_fft, hop)
    _, mag32, ph32 = G.stft_transform_ragged_ref(clean, lengths, fwd, n_fft, hop, dtype=torch.float32)
    mc32, ms32 = R.polar(mag32, ph32)
    re64, im64 = ft64[:, :, :c].transpose(1, 2), ft64[:, :, c:].transpose(1, 2)
    e_pol = max(float((mc32 - re64).abs().max()), float((ms32 - im64).abs().max()))
    _elementwise(tag + " mag", mag.t, mag64, 4 * e_mag)
    mc, ms = R.polar(mag.t, ph.t)
    _elementwise(tag + " mag cos(phase)", mc, re64, 4 * e_pol)
    _elementwise(tag + " mag sin(phase)", ms, im64, 4 * e_pol)
    if order:
        return
    # 6. optional outputs NULL one at a time: the others keep their bits
    full = [_bits(mag), _bits(ph), _bits(magT)]
    for skip in range(3):
        outs = _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt, lengths, want=tuple(i != skip for i in range(3)))
        for i in range(3):
            if i != skip:
                assert torch.equal(_bits(outs[i]), full[i]), (skip, i)
    # 5. all lengths equal to T: the partner's bits for the whole batch
    clean_d = dev(clean)
    for got, want in zip(_transform(clean_d, fwd_d, n_fft, hop, ldp, ld_mt, [T] * B), _transform(clean_d, fwd_d, n_fft, hop, ldp, ld_mt)):
        _same(tag + " equal lengths", got, want)


# ---- mel ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n_mel", [17, 80])
def test_mel_from_mag_ragged(n_mel, order):
    """c = 33 bins in rows of 48, frames (1, 8, 9, 41) of 41; rows behind an entry's end hold NaN.  Frame 0 of the 9-frame entry is
    silent: log(clip) there, while the columns behind every end are +0."""
    _lib.load()
    c, ld, F_ = 33, 48, 41
    frames = [1, 8, 9, 41][::-1] if order else [1, 8, 9, 41]
    B = len(frames)
    gen = torch.Generator().manual_seed(1000 * n_mel + 7)
    mag = 10.0 ** (torch.rand(B, F_, c, generator=gen) * 5 - 4)
    if order:
        mag = mag.flip(0)
    mag[frames.index(9), 0] = 0.0
    magT = torch.zeros(B, F_, ld)
    magT[:, :, :c] = mag
    clean = magT.clone()
    for b, fb in enumerate(frames):
        magT[b, fb:] = NAN
    basis = torch.zeros(n_mel, ld)
    basis[:, :c] = torch.rand(n_mel, c, generator=gen) * (torch.rand(n_mel, c, generator=gen) < 0.3).float() * 0.05
    basis[0, 0] = 0.01
    magT_d, basis_d = dev(magT.view(B * F_, ld)), dev(basis)
    tag = "mel ragged n_mel %d order %d" % (n_mel, order)
    for clip in (1e-5, 0.0):
        mel = _mel(magT_d, ld, B, F_, basis_d, n_mel, clip, frames)
        for b, fb in enumerate(frames):
            solo = _mel(dev(clean[b, :fb]), ld, 1, fb, basis_d, n_mel, clip)
            _same(tag + " clip %g entry %d" % (clip, b), mel.t[b, :, :fb], solo.t[0])
            _zeros(tag + " entry %d" % b, mel.t[b, :, fb:])
        want, e32 = R.f32_floor(G.mel_ragged_ref, clean.view(B * F_, ld), basis, B, F_, frames, clip)
        _elementwise(tag + " clip %g" % clip, mel.t, want, 4 * e32 + (2.0 ** -20 if clip > 0 else 0.0))
        if clip > 0:
            pin = torch.tensor(float(np.log(np.float64(np.float32(1e-5)))), dtype=torch.float32)
            assert bool((mel.t[frames.index(9), :, 0].cpu().view(torch.int32) == pin.view(torch.int32)).all()), "the silent frame"
        full = _mel(dev(clean.view(B * F_, ld)), ld, B, F_, basis_d, n_mel, clip)
        _same(tag + " equal lengths, clip %g" % clip, _mel(dev(clean.view(B * F_, ld)), ld, B, F_, basis_d, n_mel, clip, [F_] * B), full)


# ---- inverse ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", RUNS)
def test_stft_inverse_ragged(name, order):
    """The float32 spectrogram of every entry alone (CPU) in a padded batch whose frames behind each end are NaN, back to waveforms:
    plain, and with the denoiser's bias at strength 0.1 and 1.0 (the clamp bites: asserted)."""
    _lib.load()
    n_fft, hop, win, window, lengths, T, clean = _case(name, order)
    B, c, F_ = len(lengths), n_fft // 2 + 1, T // hop + 1
    fr = [max(f, 2) for f in G.frame_counts(lengths, hop)]         # (hop 48: the minimum length is one frame; the inverse needs two)
    fwd, inv_t, win_sq = R.stft_operands(n_fft, hop, win, window)
    lens2 = [max(n, hop * (f - 1)) for n, f in zip(lengths, fr)]
    _, mag, ph = G.stft_transform_ragged_ref(clean, lens2, fwd, n_fft, hop, dtype=torch.float32)
    _, mag_row, ph_row = R.stft_transform_ref(_pad(clean, lens2, 0.0), fwd, n_fft, hop, dtype=torch.float32)   # the padded row's own
    mag_n, ph_n = mag.clone(), ph.clone()
    for b, fb in enumerate(fr):
        mag_n[b, :, fb:] = NAN
        ph_n[b, :, fb:] = NAN
    gen = torch.Generator().manual_seed(11)
    bias = (torch.rand(c, generator=gen) + 0.1) * float(mag.mean())
    inv_d, ws_d = dev(inv_t), (dev(win_sq) if win_sq is not None else None)
    mag_d, ph_d, bias_d = dev(mag_n), dev(ph_n), dev(bias)
    for strength in (None, 0.1, 1.0):
        kw = {} if strength is None else dict(bias=bias, strength=strength)
        dkw = {} if strength is None else dict(bias_d=bias_d, strength=strength)
        tag = "%s order %d inverse%s" % (name, order, "" if strength is None else " bias x %.1f" % strength)
        if strength == 1.0:
            cl = mag[fr.index(F_)] - bias.view(c, 1) < 0
            assert bool(cl.any()) and not bool(cl.all()), "the clamp does not bite"
        out = _inverse(mag_d, ph_d, inv_d, n_fft, hop, ws_d, frames=fr, **dkw)
        row = _inverse(dev(mag_row), dev(ph_row), inv_d, n_fft, hop, ws_d, **dkw)      # Denoiser.forward's way with the padded row
        for b, fb in enumerate(fr):
            nb = hop * (fb - 1)
            solo = _inverse(dev(mag[b:b + 1, :, :fb]), dev(ph[b:b + 1, :, :fb]), inv_d, n_fft, hop, ws_d, **dkw)
            _same(tag + " entry %d" % b, out.t[b, :nb], solo.t[0])
            _same(tag + " last n_fft/2 samples of entry %d" % b, out.t[b, max(nb - n_fft // 2, 0):nb], solo.t[0, max(nb - n_fft // 2, 0):])
            _zeros(tag + " entry %d" % b, out.t[b, nb:])
            if fb < F_:
                tail = slice(max(nb - n_fft // 2, 0), nb)
                d = float((row.t[b, tail] - out.t[b, tail]).abs().max())
                print("BITES  %-64s padded-row processing, last n_fft/2 samples of entry %d (%d frames): worst |diff| %.3e"
                      % (tag, b, fb, d))
                if win == n_fft:                   # (a window shorter than the hop: every sample has one frame, either way)
                    assert d > 0.0
        want, e32 = R.f32_floor(G.stft_inverse_ragged_ref, mag, ph, fr, inv_t, n_fft, hop, win_sq, **kw)
        _elementwise(tag, out.t, want, 4 * e32)
        if not order:
            _same(tag + " equal lengths", _inverse(dev(mag_row), dev(ph_row), inv_d, n_fft, hop, ws_d, frames=[F_] * B, **dkw), row)


# ---- a whole batch with and without lengths -----------------------------------------------------------------------------------------
# (n_fft, hop, window, T): 8 frames (the GEMV path), 41 frames (matrix cores), a hop that does not divide n_fft, no window
FULL = {"64-16-F8": (64, 16, "hann", 127), "64-16-F41": (64, 16, "hann", 645), "48-20": (48, 20, "hann", 215),
        "64-16-nowin": (64, 16, None, 645)}


@pytest.mark.parametrize("name", list(FULL))
def test_full_lengths_are_the_plain_call(name):
    """One plain call on a batch of 3 against one ragged call on the same batch with every length T (every frame count F): the same
    kernels without and with the lengths pointer at the same item counts, so mag, phase, magT, the waveform of the inverse (plain
    and with the denoiser's bias) and the mel (log and raw) are the same bits."""
    _lib.load()
    n_fft, hop, window, T = FULL[name]
    B, c, F_ = 3, n_fft // 2 + 1, T // hop + 1
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    audio = 0.4 * torch.rand(B, T, generator=gen) - 0.2 + 0.5 * torch.sin(0.21 * torch.arange(T).float())[None] * torch.rand(
        B, 1, generator=gen)
    fwd, inv_t, win_sq = R.stft_operands(n_fft, hop, n_fft, window)
    audio_d, fwd_d, inv_d = dev(audio), dev(fwd), dev(inv_t)
    ws_d = dev(win_sq) if win_sq is not None else None
    ldp, ld_mt = R.ru(T + n_fft, 4), R.ru(c, 16)
    mag, ph, magT = _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt)
    assert float(mag.t.abs().max()) > 0.0
    for nm, got, want in zip(("mag", "phase", "magT"), _transform(audio_d, fwd_d, n_fft, hop, ldp, ld_mt, [T] * B), (mag, ph, magT)):
        _same("%s %s" % (name, nm), got, want)
    bias_d = dev((torch.rand(c, generator=gen) + 0.1) * float(mag.t.mean()))
    for dkw in ({}, dict(bias_d=bias_d, strength=1.0)):
        want = _inverse(mag.t, ph.t, inv_d, n_fft, hop, ws_d, **dkw)
        assert float(want.t.abs().max()) > 0.0
        _same("%s inverse %s" % (name, sorted(dkw)), _inverse(mag.t, ph.t, inv_d, n_fft, hop, ws_d, frames=[F_] * B, **dkw), want)
    n_mel = 17
    basis = torch.zeros(n_mel, ld_mt)
    basis[:, :c] = torch.rand(n_mel, c, generator=gen) * (torch.rand(n_mel, c, generator=gen) < 0.3).float() * 0.05
    basis_d = dev(basis)
    for clip in (1e-5, 0.0):
        _same("%s mel clip %g" % (name, clip), _mel(magT.t, ld_mt, B, F_, basis_d, n_mel, clip, [F_] * B),
              _mel(magT.t, ld_mt, B, F_, basis_d, n_mel, clip))


# ---- PCM ----------------------------------------------------------------------------------------------------------------------------
PCM_GUARD, PCM_SENTINEL = 63, 0x7A5A          # an odd guard: the output starts at an odd element


def _specials(np_dtype):
    one = np_dtype(100.0 / 32768)
    v = [0.0, -0.0, 1.0 / 32768, -1.0 / 32768, one, np.nextafter(one, np_dtype(0)), np.nextafter(one, np_dtype(1)),
         -one, -np.nextafter(one, np_dtype(0)), -np.nextafter(one, np_dtype(1)), 0.999969482421875, -0.999969482421875, 1.0, -1.0,
         3.0, -3.0, NAN, float("inf"), float("-inf")]
    return np.array(v, dtype=np_dtype)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_pcm16(B, half):
    """Exact against tests/audio_ragged_ref.pcm16_ref.  The special values stand at the first and at the last elements of every row
    (rotated, so that each is first and last somewhere); rows of odd N and odd ldx; lengths 0, 1, N - 1, N."""
    lib = _lib.load()
    np_dtype = np.float16 if half else np.float32
    sp = _specials(np_dtype)
    assert G.pcm16_ref(sp[None, 4:7]).tolist() == [[100, 99, 100]]              # just below / above an integer
    gen = np.random.RandomState(17 + B + 2 * half)
    case = 0
    for N in (1, 255, 256, 257, 1023):
        for ldx in (N, N + 1):
            for lengths in (None, [0, 1, N - 1][:B] if B == 3 else [N - 1], [N] * B, [1] * B, [0] * B):
                case += 1
                x = np.full((B, ldx), NAN, dtype=np_dtype)
                x[:, :N] = (gen.uniform(-1.0, 1.0, (B, N)) * 0.999).astype(np_dtype)
                for b in range(B):
                    r = np.roll(sp, case + 5 * b)
                    k = min(len(r), N)
                    x[b, :k] = r[:k]
                    if N > 2 * len(r):
                        x[b, N - len(r):N] = np.roll(r, 3)
                want = G.pcm16_ref(x[:, :N], lengths)
                xin = x.copy()
                if lengths is not None:
                    for b, n in enumerate(lengths):
                        xin[b, n:N] = 0.5                 # what a read behind the end would show as 16384
                x_d = torch.from_numpy(xin).to(DEV)
                raw = torch.full((B * N + 2 * PCM_GUARD,), PCM_SENTINEL, dtype=torch.int16, device=DEV)
                out = raw[PCM_GUARD:PCM_GUARD + B * N]
                ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
                rc = lib.t2s_pcm16(_p(x_d), int(half), B, N, ldx, _p(ld), out.data_ptr(), _st())
                assert rc == 0
                torch.cuda.synchronize()
                assert bool((raw[:PCM_GUARD] == PCM_SENTINEL).all()) and bool((raw[PCM_GUARD + B * N:] == PCM_SENTINEL).all()), \
                    "t2s_pcm16 wrote outside its output (N %d ldx %d)" % (N, ldx)
                got = out.view(B, N).cpu().numpy()
                bad = np.argwhere(got != want)
                assert bad.size == 0, "N %d ldx %d lengths %r: first mismatch at %r: x %r got %d want %d" % (
                    N, ldx, lengths, bad[0].tolist(), float(x[tuple(bad[0])]), got[tuple(bad[0])], want[tuple(bad[0])])
    print("PCM    B %d %s: %d cases exact" % (B, "f16" if half else "f32", case))
