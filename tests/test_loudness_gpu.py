"""audio.Loudness, PcmPool.loudness / normalize_loudness and longform.normalize_long on the device against the float64 restatement of
tests/loudness_ref.py: padded float32 / float16 batches, every row against the row alone, the serving chain
denoise_batch -> trim_batch -> normalize_batch -> resample_batch -> to_pcm16 without a synchronising call and on a caller's stream,
an int16 pool, and long-form results.  tests/test_loudness_ref_cpu.py asserts the margins that make equal counts a fair demand."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as R
import stream_util as SU
from text2speech_amd import _lib, audio as A, longform as L, synth
from text2speech_amd.data import PcmPool

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 2.6e-13
# f32 rounding of the normalised samples is 6e-8 relative, 5e-7 dB; gate decisions of the steady rows do not change with the gain
AGAIN_DB = 1e-5


def _padded(clips, dtype, stride_extra=0):
    """the clips as rows of a padded batch (a view of wider rows with stride_extra), NaN and 1e4 behind every length"""
    N = max(c.size for c in clips)
    wide = torch.full((len(clips), N + stride_extra), 1e4, dtype=dtype, device=DEV)
    wide[:, ::2] = float("nan")
    for b, c in enumerate(clips):
        wide[b, :c.size] = torch.from_numpy(c).to(DEV)
    return wide[:, :N], torch.tensor([c.size for c in clips], dtype=torch.int32, device=DEV)


def _check_report(rep, clips, fs, target=-23.0, limit=None):
    ms, lufs, peak, gain, blocks, flags = (t.cpu().numpy() for t in rep)
    for b, c in enumerate(clips):
        want = R.measure(c, fs, target, limit)
        assert (int(blocks[b]), int(flags[b])) == (want["J"], want["flags"]) and peak[b] == want["peak"], b
        if want["flags"] & (R.SHORT | R.SILENT):
            assert ms[b] == 0.0 and gain[b] == 1.0 and lufs[b] == -math.inf
        else:
            assert abs(ms[b] - want["ms"]) <= BAR * want["ms"] and abs(gain[b] - want["g"]) <= BAR * want["g"], b
            assert abs(lufs[b] - want["lufs"]) <= 4.35 * BAR + 1e-13
    return gain


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("fs", [8000, 44800])
def test_measure_and_normalize_padded_batches(fs, dtype):
    kind = "float32" if dtype == torch.float32 else "float16"
    clips = [R.as_kind(R.steady(seed, fs, n), kind) for n, seed in R.steady_rows(fs)]
    x, lens = _padded(clips, dtype, stride_extra=5)
    ld = A.Loudness(fs, -23.0)
    rep = ld.measure_batch(x, lens)
    assert all(t.is_cuda for t in rep) and rep.gain.dtype == torch.float64 and rep.flags.dtype == torch.int32
    gain = _check_report(rep, clips, fs)
    out, out_lens = ld.normalize_batch(x, lens)
    assert out_lens is lens and out.dtype == torch.float32 and tuple(out.shape) == tuple(x.shape)
    again = ld.measure_batch(out, lens)
    measured = 0
    for b, c in enumerate(clips):
        want = R.apply_float(c, float(gain[b]))
        assert out[b, :c.size].cpu().numpy().tobytes() == want.tobytes(), "row %d: the bits of (float)((double)x g)" % b
        assert bool((out[b, c.size:].view(torch.int32) == 0).all()), "+0 behind the length"
        solo = ld.forward(x[b, :c.size])
        assert solo.shape == (c.size,) and torch.equal(solo.view(torch.int32), out[b, :c.size].view(torch.int32)), "row %d alone" % b
        if int(rep.flags[b]) == 0:
            measured += 1
            assert abs(float(again.lufs[b]) + 23.0) < AGAIN_DB, "row %d measures %.7f LUFS after normalising" % (b, float(again.lufs[b]))
            assert int(again.blocks[b]) == int(rep.blocks[b])
        else:
            assert want.tobytes() == c.astype(np.float32).tobytes()
    assert measured >= 3
    # [B, 1, N], whole rows, a solo [1, N]
    o3, _ = ld.normalize_batch(x.contiguous()[:, None, :], lens)
    assert tuple(o3.shape) == (len(clips), 1, x.size(1)) and torch.equal(o3[:, 0].view(torch.int32), out.view(torch.int32))
    whole = torch.from_numpy(clips[0]).to(DEV)[None]
    assert torch.equal(ld(whole).view(torch.int32), out[0:1, :clips[0].size].view(torch.int32))


def test_peak_limit_and_refusals_on_the_device():
    fs = 44100
    clip = R.click_row(fs)
    ld = A.Loudness(fs, -3.0, peak_limit=0.9)
    x = torch.from_numpy(clip).to(DEV)
    rep = ld.measure_batch(x)
    _check_report(rep, [clip], fs, -3.0, 0.9)
    assert int(rep.flags[0]) == A.LOUD_FLAG_PEAK and float(ld(x).abs().max()) <= 0.9 * (1 + 2.0 ** -24)
    with pytest.raises(_lib.T2SError):
        ld.measure_batch(x.to(torch.float64))
    with pytest.raises(_lib.T2SError):
        ld.normalize_batch(x[None].repeat(2, 1), torch.tensor([5, 6, 7]))


def _chain(den_audio, dlen, tr, ld, rs):
    cut, clen = tr.trim_batch(den_audio, dlen)
    lev, llen = ld.normalize_batch(cut, clen)
    out, olen = rs.resample_batch(lev, llen)
    return cut, clen, lev, out, olen, A.to_pcm16(out)           # (zeros behind olen already; with lengths it would read them back)


def test_chain_denoise_trim_normalize_resample_pcm():
    """every pair of results passed on as returned, against the same stages on every entry's own slice; the batch's calls behind
    the denoiser make no synchronising call; and the same chain on a caller's stream whose input becomes true behind a gate"""
    import text2speech_amd.glow as glow
    cfg = synth.WAVEGLOW_SMALL
    m = glow.WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg), strict=True)
    m = m.to(DEV).eval()
    den = A.Denoiser(m).to(DEV)
    tr, ld, rs = A.Trimmer(top_db=60), A.Loudness(44800, -23.0, peak_limit=0.98), A.Resampler(44800, 48000, device=DEV)
    frames = (100, 85, 30)                                      # 0.57 s, 0.49 s and 0.17 s: the last is too short to measure
    mel, _ = synth.waveglow_inputs(len(frames), 256 * (max(frames) - 1), seed=61)
    wav, alen = m.infer_batch(mel.to(DEV), torch.tensor(frames), sigma=0.666, seeds=[3, 4, 5])
    wav = wav * (0.25 / wav.abs().amax())
    den_audio, dlen = den.denoise_batch(wav, alen, 0.1)
    _chain(den_audio, dlen, tr, ld, rs)                         # (warm: the first calls load the kernels)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cut, clen, lev, out, olen, pcm = _chain(den_audio, dlen, tr, ld, rs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rep = ld.measure_batch(cut, clen)
    flags = rep.flags.cpu().tolist()
    assert flags[2] & A.LOUD_FLAG_SHORT and not flags[0] & 11 and not flags[1] & 11, flags
    assert float(rep.gain[0]) != 1.0
    for b, f in enumerate(frames):
        n = 256 * f
        solo_cut = tr.forward(den(wav[b:b + 1, :n], strength=0.1))
        k = solo_cut.size(-1)
        assert int(clen[b]) == k > 0
        solo_lev = ld.forward(solo_cut)
        assert torch.equal(lev[b, 0, :k].view(torch.int32), solo_lev[0, 0].view(torch.int32)), "entry %d: levelled" % b
        solo = rs.forward(solo_lev)
        v = solo.size(-1)
        assert int(olen[b]) == v and torch.equal(out[b, 0, :v].view(torch.int32), solo[0, 0].view(torch.int32)), "entry %d" % b
        assert torch.equal(pcm[b, 0, :v], A.to_pcm16(solo)[0, 0]) and bool((pcm[b, 0, v:] == 0).all())
    # ---- on a caller's stream: the input is a decoy until a gate on that stream has drained ----
    true, true_l = den_audio.clone(), dlen.clone()
    decoy, decoy_l = (den_audio * 0.37).flip(0).contiguous(), dlen.flip(0).contiguous()
    buf, buf_l = true.clone(), true_l.clone()

    def call():
        return [t.clone() for t in _chain(buf, buf_l, tr, ld, rs)[2:]]
    ref, ms = SU.timed(call)
    buf.copy_(decoy)
    buf_l.copy_(decoy_l)
    dec = call()
    torch.cuda.synchronize()
    assert not all(torch.equal(a, b) for a, b in zip(dec, ref)), "the decoy input gives the true result - the test could not fail"
    n = SU.gate_matmuls(ms)
    SU.log("trim -> normalize -> resample -> pcm16", ms, n)
    S = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(S):
        call()
    S.synchronize()
    gate = SU.behind_gate(S, [buf, buf_l], [true, true_l], n)
    with torch.cuda.stream(S):
        got = call()
        gate.check()
    S.synchronize()
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(got, ref)), "the chain on a caller's stream differs from the default-stream run"


@pytest.mark.parametrize("fs", [8000, 44100])
def test_pool_loudness_and_normalize_loudness(fs):
    clips = [R.clip(fs, n, seed, "int16") for n, seed in R.pool_rows(fs)]
    pool = PcmPool(clips, fs)
    rep = pool.loudness(R.POOL_TARGET)
    _check_report(rep, clips, fs, R.POOL_TARGET, None)
    want = [R.measure(c, fs, R.POOL_TARGET, R.POOL_PEAK_LIMIT) for c in clips]
    short = [q for q, w in enumerate(want) if w["flags"] & R.SHORT]
    silent = [q for q, w in enumerate(want) if w["flags"] & R.SILENT]
    assert short and silent
    with pytest.raises(_lib.T2SError) as e:
        pool.normalize_loudness(R.POOL_TARGET)
    assert str(short) in str(e.value) and str(silent) in str(e.value)
    out = pool.normalize_loudness(R.POOL_TARGET, R.POOL_PEAK_LIMIT, allow_unmeasured=True)
    assert out.pcm.dtype == torch.int16 and torch.equal(out.lengths, pool.lengths) and out.sampling_rate == fs
    got = out.pcm.cpu().numpy()
    for q, (c, w) in enumerate(zip(clips, want)):
        o = int(pool.offsets[q])
        assert np.array_equal(got[o:o + c.size], R.apply_int16(c, w["g"])), "clip %d" % q
    loud = PcmPool([c for q, c in enumerate(clips) if q not in short + silent], fs)
    lev = loud.normalize_loudness(R.POOL_TARGET)                # nothing to refuse
    assert lev.pcm.numel() == loud.pcm.numel()


def _same_but_audio(a, b):
    return all(getattr(a, f) is getattr(b, f) for f in a._fields if f != "audio")


def test_normalize_long_on_joined_random_rows():
    fs = 8000
    gen = torch.Generator().manual_seed(7)
    rows = (torch.randn(3, 9000, generator=gen) * 0.1).to(DEV)
    lens = torch.tensor([9000, 4000, 7777], dtype=torch.int32, device=DEV)
    audio, length, offsets = A.join_batches([(rows, lens)], pause=80, fade=16)
    ld = A.Loudness(fs, -20.0)
    for r in (L.LongForm(audio, length, offsets, ["a", "b", "c"], torch.zeros(3, dtype=torch.bool, device=DEV)),
              L.LongFormTimed(audio, length, offsets, ["a", "b", "c"], None, torch.zeros(3, 1, 2, dtype=torch.int64, device=DEV))):
        out = L.normalize_long(r, ld)
        assert type(out) is type(r) and _same_but_audio(out, r) and out.audio is not r.audio
        want, _ = ld.normalize_batch(r.audio, r.length)
        assert torch.equal(out.audio.view(torch.int32), want.view(torch.int32))
        rep = ld.measure_batch(out.audio, out.length)
        assert int(rep.flags[0]) == 0 and abs(float(rep.lufs[0]) + 20.0) < AGAIN_DB
    with pytest.raises(_lib.T2SError, match="pcm16=False"):
        L.normalize_long(r._replace(audio=A.to_pcm16(audio)), ld)


def test_normalize_long_on_a_synthesized_result():
    import longform_util as U
    t, w = U.tacotron(), U.waveglow()
    thr, _ = U.pick_threshold(U.solo_gate_probs(t, U.seeds()))
    try:
        U.set_decoder(t, thr, U.N_STEPS)
        r = L.synthesize_long(t, w, chunks=U.CHUNKS, seed=U.SEED, sigma=U.SIGMA, pause_ms=2.0, fade_ms=0.5)
    finally:
        U.restore_decoder(t)
    ld = A.Loudness(L.SAMPLING_RATE, -23.0, peak_limit=0.99)
    out = L.normalize_long(r, ld)
    want, _ = ld.normalize_batch(r.audio, r.length)
    assert isinstance(out, L.LongForm) and _same_but_audio(out, r)
    assert torch.equal(out.audio.view(torch.int32), want.view(torch.int32))
    n = int(r.length)
    assert bool((out.audio[0, n:].view(torch.int32) == 0).all())
