"""Silence trimming and peak rescaling behind the Python surface: PcmPool.rescale_trim against a pool built from the host output of
tests/trim_ref.py (librosa's formulas restated; tests/test_trim_ref_cpu.py asserts that no frame of these seeded clips lies within
1e-6 dB of the threshold), training batches on the trimmed pool, audio.Trimmer, and the serving chain
infer_batch -> denoise_batch -> trim_batch -> resample_batch -> to_pcm16 against the same chain on every entry alone."""
import numpy as np
import pytest
import torch

import trim_ref as R
from text2speech_amd import _lib, audio, data, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = synth.WAVEGLOW_SMALL
T2SError = _lib.T2SError

_HOST = {}


def _host_trimmed(decision):
    """the reference's output for the surface clips under one decision, computed once"""
    if decision not in _HOST:
        top_db, r, fl, h, mode = decision
        _HOST[decision] = [R.rescale_trim(c, fl, h, mode, top_db, r) for c in R.surface_clips()]
    return _HOST[decision]


# ---- PcmPool ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decision", R.SURFACE_DECISIONS)
def test_pool_rescale_trim_equals_the_host_trimmed_pool(decision):
    top_db, r, fl, h, mode = decision
    clips = R.surface_clips()
    pool = data.PcmPool(clips, R.SURFACE_RATE, DEV)
    out = pool.rescale_trim(r, top_db, fl, h, mode)
    want = data.PcmPool(_host_trimmed(decision), R.SURFACE_RATE, DEV)
    assert out is not pool and out.sampling_rate == R.SURFACE_RATE and len(out) == len(pool)
    assert out.pcm.dtype == torch.int16 and out.pcm.is_cuda and out.lengths.dtype == torch.int64
    assert out.lengths.tolist() == want.lengths.tolist() and out.offsets.tolist() == want.offsets.tolist()
    assert torch.equal(out.pcm, want.pcm)
    if top_db is not None:
        assert int(out.lengths.sum()) < int(pool.lengths.sum()), "something is cut"
    else:
        assert out.lengths.tolist() == pool.lengths.tolist()
    assert torch.equal(pool.pcm.cpu(), torch.from_numpy(np.concatenate(clips))), "the source pool is untouched"


def test_pool_rescale_trim_with_neither_half_is_an_equal_pool():
    pool = data.PcmPool(R.surface_clips(), R.SURFACE_RATE, DEV)
    same = pool.rescale_trim()
    assert same is not pool and same.pcm.data_ptr() != pool.pcm.data_ptr() and torch.equal(same.pcm, pool.pcm)
    assert same.lengths.tolist() == pool.lengths.tolist() and same.offsets.tolist() == pool.offsets.tolist()


def test_pool_rescale_trim_reads_back_once():
    """rescaling alone reads nothing back; with top_db the one read is the [n_clips, 2] cut points"""
    pool = data.PcmPool(R.surface_clips(), R.SURFACE_RATE, DEV)
    pool.rescale_trim(0.999)                                # (warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = pool.rescale_trim(0.999)
        with pytest.raises(RuntimeError, match="synchroniz"):
            pool.rescale_trim(0.999, 23)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out.pcm.cpu(), torch.from_numpy(np.concatenate([R.rescale(c, 0.999) for c in R.surface_clips()])))


def test_training_batches_on_the_trimmed_pool_equal_those_on_the_host_trimmed_pool():
    decision = R.SURFACE_DECISIONS[0]
    top_db, r, fl, h, mode = decision
    got = data.PcmPool(R.surface_clips(), R.SURFACE_RATE, DEV).rescale_trim(r, top_db, fl, h, mode)
    want = data.PcmPool(_host_trimmed(decision), R.SURFACE_RATE, DEV)
    stft = dict(filter_length=64, hop_length=16, win_length=64, sampling_rate=R.SURFACE_RATE, mel_fmin=0.0, mel_fmax=8000.0)
    idx, starts = [0, 2, 3, 4], [100, 0, 7, 0]
    a = data.Mel2SampBatch(got, 400, n_mel_channels=8, **stft)(idx, starts=starts)
    b = data.Mel2SampBatch(want, 400, n_mel_channels=8, **stft)(idx, starts=starts)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    seqs = [[3, 4, 5], [6], [7, 8], [9, 10, 11, 12], [13, 14]]
    xa, ya = data.TextMelBatch(got, seqs, 1, 64, 16, 64, 8, R.SURFACE_RATE, 0.0, 8000.0)([0, 1, 3, 4])
    xb, yb = data.TextMelBatch(want, seqs, 1, 64, 16, 64, 8, R.SURFACE_RATE, 0.0, 8000.0)([0, 1, 3, 4])
    assert torch.equal(ya[0].view(torch.int32), yb[0].view(torch.int32)) and torch.equal(ya[1], yb[1])
    assert torch.equal(xa[0], xb[0]) and torch.equal(xa[5], xb[5]) and xa[3] == xb[3]
    assert xa[5].tolist() == [1 + int(got.lengths[i]) // 16 for i in (3, 0, 4, 1)]


def test_pool_errors_name_the_clips():
    clips = R.surface_clips()
    zeros = np.zeros(900, dtype=np.int16)
    pool = data.PcmPool([clips[0], zeros, clips[1], zeros], R.SURFACE_RATE, DEV)
    with pytest.raises(T2SError, match=r"clips \[1, 3\] trim to nothing"):
        pool.rescale_trim(0.999, 23)
    with pytest.raises(T2SError, match=r"clips \[1, 3\] trim to nothing"):
        pool.rescale_trim(None, 40, 64, 16, "constant")
    assert len(pool.rescale_trim(0.999)) == 4, "rescaling alone keeps a clip of zeros as it is"
    short = data.PcmPool([clips[0], clips[1][:256], clips[2], clips[1][:100], clips[1][:257]], R.SURFACE_RATE, DEV)
    with pytest.raises(T2SError, match=r"clips \[1, 3\] have at most frame_length // 2 = 256 samples"):
        short.rescale_trim(0.999, 23)
    assert len(short.rescale_trim(0.999, 23, pad_mode="constant")) == 5
    assert len(short.rescale_trim(0.999, 23, 64, 16)) == 5
    for kw in (dict(top_db=-1), dict(rescaling_max=0.0), dict(frame_length=1), dict(hop_length=0), dict(pad_mode="edge")):
        with pytest.raises(T2SError):
            pool.rescale_trim(**kw)


def test_pool_of_more_than_65535_clips_goes_in_chunks():
    base = R.chunk_clips()
    want = [R.rescale_trim(c, 64, 16, "constant", 23, 0.999) for c in base]
    n = 65535 + 9
    pool = data.PcmPool([base[k % 4] for k in range(n)], R.SURFACE_RATE, DEV)
    out = pool.rescale_trim(0.999, 23, 64, 16, "constant")
    assert len(out) == n and out.lengths.tolist() == [want[k % 4].size for k in range(n)]
    assert torch.equal(out.pcm.cpu(), torch.from_numpy(np.concatenate([want[k % 4] for k in range(n)])))
    only = pool.rescale_trim(0.999, None)
    assert torch.equal(only.pcm.cpu(), torch.from_numpy(np.concatenate([R.rescale(base[k % 4], 0.999) for k in range(n)])))


def test_resample_then_rescale_trim_runs():
    clips = R.surface_clips()
    pool = data.PcmPool(clips, 44100, DEV).resample(44800)
    out = pool.rescale_trim(0.999, 23)
    assert out.sampling_rate == 44800 and len(out) == len(pool)
    assert bool((out.lengths <= pool.lengths).all()) and bool((out.lengths > 0).all()) and out.pcm.numel() == int(out.lengths.sum())
    # against the reference on the resampled samples
    src = pool.pcm.cpu().numpy()
    got = out.pcm.cpu().numpy()
    for q in range(len(pool)):
        o, n = int(pool.offsets[q]), int(pool.lengths[q])
        (s, e), margin = R.trim_bounds(src[o:o + n], 512, 128, "reflect", 23, 0.999, with_margin=True)
        assert margin >= 1e-6, "clip %d: a frame %.2e dB from the threshold" % (q, margin)
        assert int(out.lengths[q]) == e - s
        assert np.array_equal(got[int(out.offsets[q]):int(out.offsets[q]) + e - s], R.rescale(src[o:o + n], 0.999)[s:e])


# ---- Trimmer ------------------------------------------------------------------------------------------------------------------------------
def _trimmer(t):
    top_db, r, fl, h, mode, floor = t
    return audio.Trimmer(fl, h, top_db, mode, r, floor)


@pytest.mark.parametrize("t", R.BATCH_TRIMMERS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_trimmer_forward_equals_the_reference(t, dtype):
    top_db, r, fl, h, mode, floor = t
    tr = _trimmer(t)
    np_dtype = np.float32 if dtype == torch.float32 else np.float16
    for x in R.batch_rows(np_dtype):
        want = R.rescale_trim(x, fl, h, mode, top_db, r, floor)
        xd = torch.from_numpy(x).to(DEV)
        y1 = tr.forward(xd)
        y2 = tr(xd[None, :])
        y3 = tr(xd[None, None, :])
        assert y1.dtype == torch.float32 and tuple(y1.shape) == (want.size,) and tuple(y2.shape) == (1, want.size)
        assert tuple(y3.shape) == (1, 1, want.size)
        assert y1.cpu().numpy().tobytes() == want.tobytes()
        assert torch.equal(y2[0].view(torch.int32), y1.view(torch.int32)) and torch.equal(y3[0, 0].view(torch.int32), y1.view(torch.int32))
        if top_db is not None:
            s, e = R.trim_bounds(x, fl, h, mode, top_db, r, floor)
            bs, be = tr.bounds_batch(xd[None, :], [x.size])
            assert bs.dtype == be.dtype == torch.int64 and bs.is_cuda and (int(bs[0]), int(be[0])) == (s, e)


def test_save_wav_normalisation():
    """Trimmer(top_db=None, rescaling_max=32767 / 32768, peak_floor=0.01) then to_pcm16 is utils/audio.py:14-17: the peak becomes
    32767, and a clip quieter than the floor is raised by 1 / 0.01 only"""
    tr = audio.Trimmer(top_db=None, rescaling_max=32767 / 32768, peak_floor=0.01)
    x = R.batch_rows()[1]
    xd = torch.from_numpy(x).to(DEV)
    y = tr(xd)
    assert tuple(y.shape) == (x.size,) and y.cpu().numpy().tobytes() == R.rescale(x, 32767 / 32768, 0.01).tobytes()
    assert int(audio.to_pcm16(y).abs().max()) in (32766, 32767)
    quiet = (x * np.float32(1e-3)).astype(np.float32)
    yq = tr(torch.from_numpy(quiet).to(DEV))
    assert yq.cpu().numpy().tobytes() == (quiet.astype(np.float64) * ((32767 / 32768) / 0.01)).astype(np.float32).tobytes()


def _padded(rows, order, width, dtype, junk=True):
    x = torch.full((len(order), width), 1e4, dtype=dtype, device=DEV)
    if junk:
        x[:, ::2] = float("nan")                            # NaN and 1e4 behind every entry's end
    for k, q in enumerate(order):
        x[k, :rows[q].size] = torch.from_numpy(rows[q]).to(DEV)
    return x


@pytest.mark.parametrize("t", R.BATCH_TRIMMERS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_trim_batch_entries_equal_forward_alone(t, dtype):
    tr = _trimmer(t)
    np_dtype = np.float32 if dtype == torch.float32 else np.float16
    rows = R.batch_rows(np_dtype)
    solo = [tr.forward(torch.from_numpy(x).to(DEV)) for x in rows]
    width = max(R.BATCH_LENGTHS) + 3
    for order in ((0, 1, 2, 3), (3, 1, 0, 2)):
        x = _padded(rows, order, width, dtype)
        lens = torch.tensor([rows[q].size for q in order], device=DEV)
        tr.trim_batch(x, lens)                              # (warm)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out, out_lens = tr.trim_batch(x, lens)
            out3, out_lens3 = tr.trim_batch(x[:, None, :], lens)
            bs, be = tr.bounds_batch(x, lens)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert tuple(out.shape) == (4, width) and out.dtype == torch.float32 and tuple(out3.shape) == (4, 1, width)
        assert out_lens.dtype == torch.int32 and out_lens.is_cuda and tuple(out_lens.shape) == (4,)
        assert torch.equal(out3[:, 0].view(torch.int32), out.view(torch.int32)) and torch.equal(out_lens3, out_lens)
        assert torch.equal((be - bs).to(torch.int32), out_lens)
        for k, q in enumerate(order):
            v = solo[q].numel()
            assert int(out_lens[k]) == v
            assert torch.equal(out[k, :v].view(torch.int32), solo[q].view(torch.int32)), "entry %d differs from the entry alone" % q
            assert bool((out[k, v:].view(torch.int32) == 0).all()), "zeros behind entry %d" % q
    # host lengths and a sequence give the same
    a, al = tr.trim_batch(x, lens.cpu())
    b, bl = tr.trim_batch(x, [rows[q].size for q in order])
    assert torch.equal(a.view(torch.int32), out.view(torch.int32)) and torch.equal(b.view(torch.int32), out.view(torch.int32))
    assert torch.equal(al, out_lens) and torch.equal(bl, out_lens)


def test_trim_batch_entry_that_trims_to_nothing():
    tr = audio.Trimmer(rescaling_max=0.999)
    rows = R.batch_rows()
    x = _padded(rows, (0, 1, 2, 3), 4100, torch.float32, junk=False)
    x[1, :1500] = 0.0                                       # an entry of zeros
    x[2, 700] = float("nan")                                # an entry with a non-finite sample
    lens = torch.tensor([4096, 1500, 2600, 0], device=DEV)  # ... and an empty one
    out, out_lens = tr.trim_batch(x, lens)
    solo = tr(x[0, :4096])
    assert out_lens.tolist() == [solo.numel(), 0, 0, 0] and solo.numel() > 0
    assert torch.equal(out[0, :solo.numel()].view(torch.int32), solo.view(torch.int32))
    assert bool((out[1:].view(torch.int32) == 0).all()) and bool((out[0, solo.numel():].view(torch.int32) == 0).all())
    assert tuple(tr(x[1, :1500]).shape) == (0,)
    # lengths beyond the row are clamped on the device
    out2, out_lens2 = tr.trim_batch(x[:1], torch.tensor([1 << 40], device=DEV))
    full = tr(x[0])
    assert int(out_lens2[0]) == full.numel() and torch.equal(out2[0, :full.numel()].view(torch.int32), full.view(torch.int32))


def test_trimmer_refusals():
    tr = audio.Trimmer()
    seen = []
    real = _lib.call
    _lib.call = lambda name, *a: (seen.append(name), real(name, *a))[1]
    try:
        x = torch.zeros(2, 3000, device=DEV)
        with pytest.raises(T2SError, match="float32 or float16"):
            tr.trim_batch(x.to(torch.int16), [3000, 3000])
        with pytest.raises(T2SError, match=r"audio must be \[B, T\] or \[B, 1, T\]"):
            tr.trim_batch(x[0], [3000])
        with pytest.raises(T2SError, match="one clip"):
            tr.forward(x)
        with pytest.raises(T2SError, match=r"lengths has shape \(3,\), the batch holds 2"):
            tr.trim_batch(x, [100, 50, 3])
        with pytest.raises(T2SError, match="lengths must be integers"):
            tr.trim_batch(x, torch.tensor([100.0, 50.0]))
        with pytest.raises(T2SError, match=r"\[N\], \[B, N\] or \[B, 1, N\]"):
            tr.bounds_batch(torch.zeros(2, 2, 100, device=DEV), [100, 100])
    finally:
        _lib.call = real
    assert seen == [], "a refused call launched: %r" % seen


# ---- the serving chain --------------------------------------------------------------------------------------------------------------------
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


def test_chain_infer_denoise_trim_resample_pcm():
    """infer_batch -> denoise_batch -> trim_batch -> resample_batch -> to_pcm16, every pair of results passed on as returned, against
    the same stages on every entry's own slice; the trim and resample calls of the batch make no synchronising call.  A silent
    tail is appended to each entry's vocoder output so that the trim has something to cut."""
    import text2speech_amd.glow as glow
    m = glow.WaveGlow(**CFG)
    m.load_state_dict(synth.waveglow_state(CFG), strict=True)
    m = m.to(DEV).eval()
    den = audio.Denoiser(m).to(DEV)
    tr = audio.Trimmer(top_db=23, rescaling_max=0.999)
    rs = audio.Resampler(44800, 48000, device=DEV)
    frames = (12, 7, 3)
    mel, noise = _mel_and_noise(frames, seed=61)
    wav, alen = m.infer_batch(mel, torch.tensor(frames), sigma=0.666, noise=noise)
    for b, f in enumerate(frames):                          # the last third of every entry: near silence
        n = 256 * f
        wav[b, n - n // 3:n] *= 1e-4
    den_audio, dlen = den.denoise_batch(wav, alen, 0.1)
    rs.resample_batch(*tr.trim_batch(den_audio, dlen))      # (warm: the first calls load the kernels)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cut, clen = tr.trim_batch(den_audio, dlen)
        out, olen = rs.resample_batch(cut, clen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pcm = audio.to_pcm16(out, olen)
    assert tuple(cut.shape) == tuple(den_audio.shape) and clen.dtype == torch.int32
    assert tuple(out.shape) == (3, 1, rs.out_length(256 * 12)) and olen.dtype == torch.int64
    some_cut = False
    for b, f in enumerate(frames):
        n = 256 * f
        solo_cut = tr.forward(den(wav[b:b + 1, :n], strength=0.1))
        k = solo_cut.size(-1)
        some_cut |= 0 < k < n
        assert int(clen[b]) == k and torch.equal(cut[b, 0, :k].view(torch.int32), solo_cut[0, 0].view(torch.int32))
        solo = rs.forward(solo_cut)
        v = solo.size(-1)
        assert int(olen[b]) == v == rs.out_length(k)
        assert torch.equal(out[b, 0, :v].view(torch.int32), solo[0, 0].view(torch.int32)), "entry %d differs from the entry alone" % b
        assert bool((out[b, 0, v:].view(torch.int32) == 0).all())
        assert torch.equal(pcm[b, 0, :v], audio.to_pcm16(solo)[0, 0]) and bool((pcm[b, 0, v:] == 0).all())
    assert some_cut, "the trim cut nothing"
