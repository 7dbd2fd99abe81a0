"""audio.Limiter, Loudness.normalize_limit_batch, PcmPool.true_peak / limit and longform.limit_long on the device against the float64
restatement of tests/limiter_ref.py: padded float32 / float16 batches, every row against the row alone, the serving chain
infer_batch -> denoise_batch -> trim_batch -> resample_batch -> normalize_limit_batch -> to_pcm16 without a synchronising call and on
a caller's stream, an int16 pool, and long-form results.  tests/test_limiter_ref_cpu.py asserts the margins that make equal counts
and equal int16 samples a fair demand."""
import numpy as np
import pytest
import torch

import limiter_ref as R
import loudness_ref as LR
import stream_util as SU
from text2speech_amd import _lib, audio as A, longform as LF, synth
from text2speech_amd.data import PcmPool

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 44800                      # lookahead_ms = 1.5 is 67 samples here, one of limiter_ref's look-aheads
C = R.ceiling(-1.0)
AGAIN_DB = 1e-5                 # float32 rounding of the samples is 6e-8 relative, 5e-7 dB (tests/test_loudness_gpu.py)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _padded(clips, dtype, stride_extra=0):
    """the clips as rows of a padded batch (a view of wider rows with stride_extra), NaN and 1e4 behind every length"""
    N = max(c.size for c in clips)
    wide = torch.full((len(clips), N + stride_extra), 1e4, dtype=dtype, device=DEV)
    wide[:, ::2] = float("nan")
    for b, c in enumerate(clips):
        wide[b, :c.size] = torch.from_numpy(c).to(DEV)
    return wide[:, :N], torch.tensor([c.size for c in clips], dtype=torch.int32, device=DEV)


def _check_report(rep, clips, L, os, gains=None):
    tp, sp, smin, limited, flags = (t.cpu().numpy() for t in rep)
    for b, c in enumerate(clips):
        ref = R.reference(c, C, L, os, 1.0 if gains is None else float(gains[b]))
        b_p, b_s = R.bounds(ref, L, os)
        assert (int(limited[b]), int(flags[b])) == ref.counts and sp[b] == ref.stats[1], b
        assert abs(tp[b] - ref.stats[0]) <= b_p.max() and abs(smin[b] - ref.stats[2]) <= b_s, b


def _check_samples(out, c, L, os, g=1.0):
    ref = R.reference(c, C, L, os, g)
    _, b_s = R.bounds(ref, L, os)
    tol = 2.0 ** -24 * np.abs(ref.o) + np.abs(ref.u) * b_s + 2.0 ** -52 * np.abs(ref.o) + 2.0 ** -149
    assert (np.abs(out.astype(np.float64) - ref.o) <= tol).all() and np.abs(out).max() <= np.float32(C)
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_limit_batch_entries_are_forward_on_the_entry_alone(dtype):
    kind = "float32" if dtype == torch.float32 else "float16"
    lim = A.Limiter(FS)
    L, os = lim.lookahead, lim.oversample
    assert (L, os, lim.reach, lim.ceiling) == (67, 4, 2 * 67 + 10, C)
    sizes = [2 * R.TILE + 1, 2 * L + 1, R.TILE + 1, 2]
    clips = [R.clip(n, R.seed_of(n, L, os, kind), kind, L) for n in sizes]
    for order in ([0, 1, 2, 3], [3, 2, 0, 1]):
        rows = [clips[q] for q in order]
        x, lens = _padded(rows, dtype, stride_extra=5)
        rep = lim.true_peak_batch(x, lens)
        assert all(t.is_cuda for t in rep) and rep.true_peak.dtype == torch.float64 and rep.flags.dtype == torch.int32
        _check_report(rep, rows, L, os)
        out, out_lens = lim.limit_batch(x, lens)
        assert out_lens is lens and out.dtype == torch.float32 and tuple(out.shape) == tuple(x.shape)
        for b, c in enumerate(rows):
            ref = _check_samples(out[b, :c.size].cpu().numpy(), c, L, os)
            assert ref.counts[0] > 0 or c.size <= 2
            assert bool((out[b, c.size:].view(torch.int32) == 0).all()), "+0 behind the length"
            solo = lim.forward(x[b, :c.size])
            assert solo.shape == (c.size,) and torch.equal(_bits(solo), _bits(out[b, :c.size])), "row %d alone" % b
    # [B, 1, N], whole rows, a solo [1, N], a host sequence of lengths
    o3, _ = lim.limit_batch(x.contiguous()[:, None, :], lens.tolist())
    assert tuple(o3.shape) == (len(clips), 1, x.size(1)) and torch.equal(_bits(o3[:, 0]), _bits(out))
    whole = torch.from_numpy(rows[0]).to(DEV)[None]
    assert torch.equal(_bits(lim(whole)), _bits(out[0:1, :rows[0].size]))
    # a gain per row, as a strided view: entry b is the entry alone with its own gain
    table = torch.tensor([[0, 0, 0, 3.0], [0, 0, 0, 1.0], [0, 0, 0, 8.0], [0, 0, 0, 0.0]], dtype=torch.float64, device=DEV)
    gain = table[:, 3]
    assert not gain.is_contiguous()
    _check_report(lim.true_peak_batch(x, lens, gain), rows, L, os, gain.tolist())
    outg, _ = lim.limit_batch(x, lens, gain)
    for b, c in enumerate(rows):
        _check_samples(outg[b, :c.size].cpu().numpy(), c, L, os, float(gain[b]))
        solo, _ = lim.limit_batch(x[b:b + 1, :c.size], None, gain[b:b + 1])
        assert torch.equal(_bits(solo[0]), _bits(outg[b, :c.size]))


def test_a_ceiling_above_every_peak_returns_the_inputs_bits():
    lim = A.Limiter(FS, ceiling_db=0.0)
    assert lim.ceiling == 1.0
    for kind, dtype in (("float32", torch.float32), ("float16", torch.float16)):
        clips = [(R.clip(n, n, kind, 67).astype(np.float64) * 0.5).astype(np.float32 if kind == "float32" else np.float16)
                 for n in (3000, 1024, 77)]
        x, lens = _padded(clips, dtype, stride_extra=3)
        rep = lim.true_peak_batch(x, lens)
        assert rep.limited.tolist() == [0, 0, 0] and rep.flags.tolist() == [0, 0, 0] and rep.min_gain.tolist() == [1.0, 1.0, 1.0]
        assert float(rep.true_peak.max()) <= 1.0
        out, _ = lim.limit_batch(x, lens)
        for b, c in enumerate(clips):
            assert out[b, :c.size].cpu().numpy().tobytes() == c.astype(np.float32).tobytes()
            assert bool((out[b, c.size:].view(torch.int32) == 0).all())


def _transient_row(fs):
    x = (LR.steady(0, fs, 25 * LR.hop(fs) + 5) * 0.2).astype(np.float32)
    x[9000] = 0.9
    return x


def test_normalize_limit_batch_is_measure_then_limit_and_keeps_the_loudness():
    fs, target = 8000, -16.0
    ld, ldp, lim = A.Loudness(fs, target), A.Loudness(fs, target, peak_limit=C), A.Limiter(fs)
    L, os = lim.lookahead, lim.oversample
    assert L == 12
    quiet = (0.01 * np.sin(2 * np.pi * 997.0 / fs * np.arange(13 * LR.hop(fs) + 17))).astype(np.float32)   # no crest to limit
    short = R.clip(900, 5, "float32", L)                        # too short to measure: gain 1, limited all the same
    clips = [_transient_row(fs), quiet, short]
    x, lens = _padded(clips, torch.float32, stride_extra=1)
    rep = ld.measure_batch(x, lens)
    out, out_lens = ld.normalize_limit_batch(x, lens, lim)
    assert out_lens is lens
    want, _ = lim.limit_batch(x, lens, gain=rep.gain)
    assert torch.equal(_bits(out), _bits(want))
    tp = lim.true_peak_batch(x, lens, rep.gain)
    plain, _ = ld.normalize_batch(x, lens)
    gains = rep.gain.cpu().numpy()
    assert tp.limited.tolist()[1] == 0 and tp.limited.tolist()[0] > 0 and tp.limited.tolist()[2] > 0 and gains[2] == 1.0
    assert torch.equal(_bits(out[1]), _bits(plain[1])), "a row with nothing over the ceiling is normalize_batch's"
    for b, c in enumerate(clips):
        _check_samples(out[b, :c.size].cpu().numpy(), c, L, os, float(gains[b]))
    # ---- the transient row: limited, it keeps its loudness; with a peak limit the whole row is turned down ----
    c0 = clips[0]
    g_ref = LR.measure(c0, fs, target)["g"]
    d_lim = abs(LR.measure(R.limit(c0, C, L, os, g=g_ref).out, fs, target)["lufs"] - target)
    g_pk = LR.measure(c0, fs, target, C)
    d_pk = abs(LR.measure(LR.apply_float(c0, g_pk["g"]), fs, target)["lufs"] - target)
    assert g_pk["flags"] & LR.PEAK and d_lim + 4 * AGAIN_DB < d_pk, "the input does not show the difference"
    pk, _ = ldp.normalize_batch(x, lens)
    got_lim = abs(float(ld.measure_batch(out, lens).lufs[0]) - target)
    got_pk = abs(float(ld.measure_batch(pk, lens).lufs[0]) - target)
    print("LIMITER loudness kept: off target by %.6f dB limited (reference %.6f), by %.4f dB with peak_limit (reference %.4f)"
          % (got_lim, d_lim, got_pk, d_pk))
    assert got_lim <= d_lim + AGAIN_DB and got_pk >= d_pk - AGAIN_DB and got_lim < got_pk
    with pytest.raises(_lib.T2SError, match="44800 Hz"):
        ld.normalize_limit_batch(x, lens, A.Limiter(44800))
    with pytest.raises(_lib.T2SError, match="audio.Limiter"):
        ld.normalize_limit_batch(x, lens, ld)


def _chain(den_audio, dlen, tr, rs, ld, lim):
    cut, clen = tr.trim_batch(den_audio, dlen)
    res, rlen = rs.resample_batch(cut, clen)
    out, olen = ld.normalize_limit_batch(res, rlen, lim)
    return res, rlen, out, A.to_pcm16(out)                      # (zeros behind olen already; with lengths it would read them back)


def test_chain_denoise_trim_resample_normalize_limit_pcm():
    """every pair of results passed on as returned, against the same stages on every entry's own slice; the batch's calls behind
    the denoiser make no synchronising call; and the same chain on a caller's stream whose input becomes true behind a gate"""
    import text2speech_amd.glow as glow
    cfg = synth.WAVEGLOW_SMALL
    m = glow.WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg), strict=True)
    m = m.to(DEV).eval()
    den = A.Denoiser(m).to(DEV)
    tr, rs = A.Trimmer(top_db=60), A.Resampler(44800, 48000, device=DEV)
    ld, lim = A.Loudness(48000, -8.0), A.Limiter(48000)         # a loud target: the limiter has work
    frames = (100, 85, 30)                                      # 0.57 s, 0.49 s and 0.17 s: the last is too short to measure
    mel, _ = synth.waveglow_inputs(len(frames), 256 * (max(frames) - 1), seed=61)
    wav, alen = m.infer_batch(mel.to(DEV), torch.tensor(frames), sigma=0.666, seeds=[3, 4, 5])
    wav = wav * (0.25 / wav.abs().amax())
    den_audio, dlen = den.denoise_batch(wav, alen, 0.1)
    _chain(den_audio, dlen, tr, rs, ld, lim)                    # (warm: the first calls load the kernels and upload the tables)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res, rlen, out, pcm = _chain(den_audio, dlen, tr, rs, ld, lim)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    tp = lim.true_peak_batch(res, rlen, ld.measure_batch(res, rlen).gain)
    assert tp.limited.tolist()[0] > 0 and tp.limited.tolist()[1] > 0 and not any(f & 8 for f in tp.flags.tolist()), tp
    top = int(np.rint(32768.0 * lim.ceiling))
    assert int(pcm.to(torch.int32).abs().max()) <= top and float(out.abs().max()) <= lim.ceiling
    for b, f in enumerate(frames):
        n = 256 * f
        solo_res = rs.forward(tr.forward(den(wav[b:b + 1, :n], strength=0.1)))
        v = solo_res.size(-1)
        assert int(rlen[b]) == v > 0
        solo, _ = ld.normalize_limit_batch(solo_res, None, lim)
        assert torch.equal(_bits(out[b, 0, :v]), _bits(solo[0, 0])), "entry %d" % b
        assert bool((out[b, 0, v:].view(torch.int32) == 0).all())
        assert torch.equal(pcm[b, 0, :v], A.to_pcm16(solo)[0, 0]) and bool((pcm[b, 0, v:] == 0).all())
    # ---- on a caller's stream: the input is a decoy until a gate on that stream has drained ----
    true, true_l = den_audio.clone(), dlen.clone()
    decoy, decoy_l = (den_audio * 0.37).flip(0).contiguous(), dlen.flip(0).contiguous()
    buf, buf_l = true.clone(), true_l.clone()

    def call():
        return [t.clone() for t in _chain(buf, buf_l, tr, rs, ld, lim)[2:]]
    ref, ms = SU.timed(call)
    buf.copy_(decoy)
    buf_l.copy_(decoy_l)
    dec = call()
    torch.cuda.synchronize()
    assert not all(torch.equal(a, b) for a, b in zip(dec, ref)), "the decoy input gives the true result - the test could not fail"
    n = SU.gate_matmuls(ms)
    SU.log("trim -> resample -> normalize + limit -> pcm16", ms, n)
    S = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(S):
        call()
    S.synchronize()
    gate = SU.behind_gate(S, [buf, buf_l], [true, true_l], n)
    with torch.cuda.stream(S):
        got = call()
        gate.check()
    S.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, ref)), "the chain on a caller's stream differs from the default-stream run"


def test_pool_true_peak_and_limit():
    L, os = 67, 4
    lim = A.Limiter(FS)
    sizes = [2 * R.TILE + 1, 2, R.TILE, 2 * L + 1, R.TILE + 1, 1]
    clips = [R.clip(n, R.seed_of(n, L, os, "int16"), "int16", L) for n in sizes]
    pool = PcmPool(clips, FS)
    _check_report(pool.true_peak(lim), clips, L, os)
    out = pool.limit(lim)
    assert out.pcm.dtype == torch.int16 and torch.equal(out.lengths, pool.lengths) and out.sampling_rate == FS and out is not pool
    got = out.pcm.cpu().numpy()
    top = np.rint(32768.0 * C)
    for q, c in enumerate(clips):
        o = int(pool.offsets[q])
        assert np.array_equal(got[o:o + c.size], R.reference(c, C, L, os, 1.0).out), "clip %d" % q
    assert np.abs(got.astype(np.int64)).max() <= top
    # with a loudness target first: the reference is fed the gain the device measured (its own test bounds that)
    fs = 8000
    lim8, ld = A.Limiter(fs), A.Loudness(fs, -8.0)
    clips = [LR.as_kind(LR.steady(s, fs, n) * a, "int16") for n, s, a in ((25 * LR.hop(fs) + 5, 0, 0.3), (13 * LR.hop(fs) + 17, 1, 1.0), (900, 2, 1.0))]
    pool = PcmPool(clips, fs)
    gains = pool.loudness(-8.0).gain.cpu().numpy()
    out = pool.limit(lim8, ld)
    got = out.pcm.cpu().numpy()
    limited = 0
    assert gains[2] == 1.0 and gains[0] > 1.5 and torch.equal(out.lengths, pool.lengths)
    for q, c in enumerate(clips):
        o = int(pool.offsets[q])
        ref = R.limit(c, C, lim8.lookahead, 4, g=float(gains[q]))
        v = 32768.0 * ref.o
        assert float(np.abs(v - np.floor(v) - 0.5).min()) > 1e-6, "clip %d: the input cannot ask for equal samples" % q
        assert np.array_equal(got[o:o + c.size], ref.out), "clip %d" % q
        limited += ref.counts[0]
    assert limited > 100
    with pytest.raises(_lib.T2SError, match="8000 Hz"):
        pool.limit(lim)
    with pytest.raises(_lib.T2SError, match="audio.Limiter"):
        pool.true_peak(ld)


def _same_but_audio(a, b):
    return all(getattr(a, f) is getattr(b, f) for f in a._fields if f != "audio")


def test_limit_long_on_joined_random_rows():
    fs = 8000
    gen = torch.Generator().manual_seed(7)
    rows = (torch.randn(3, 9000, generator=gen) * 0.35).to(DEV)
    lens = torch.tensor([9000, 4000, 7777], dtype=torch.int32, device=DEV)
    audio, length, offsets = A.join_batches([(rows, lens)], pause=80, fade=16)
    lim, ld = A.Limiter(fs), A.Loudness(fs, -14.0)
    for r in (LF.LongForm(audio, length, offsets, ["a", "b", "c"], torch.zeros(3, dtype=torch.bool, device=DEV)),
              LF.LongFormTimed(audio, length, offsets, ["a", "b", "c"], None, torch.zeros(3, 1, 2, dtype=torch.int64, device=DEV))):
        out = LF.limit_long(r, lim)
        assert type(out) is type(r) and _same_but_audio(out, r) and out.audio is not r.audio
        want, _ = lim.limit_batch(r.audio, r.length)
        assert torch.equal(_bits(out.audio), _bits(want)) and not torch.equal(_bits(want), _bits(r.audio))
        assert float(out.audio.abs().max()) <= lim.ceiling
        n = int(r.length)
        _check_samples(out.audio.reshape(-1)[:n].cpu().numpy(), r.audio.reshape(-1)[:n].cpu().numpy(), lim.lookahead, 4)
        both = LF.limit_long(r, lim, ld)
        want, _ = ld.normalize_limit_batch(r.audio, r.length, lim)
        assert _same_but_audio(both, r) and torch.equal(_bits(both.audio), _bits(want))
    with pytest.raises(_lib.T2SError, match="pcm16=False"):
        LF.limit_long(r._replace(audio=A.to_pcm16(audio)), lim)
    with pytest.raises(_lib.T2SError, match="LongForm"):
        LF.limit_long((audio, length), lim)
