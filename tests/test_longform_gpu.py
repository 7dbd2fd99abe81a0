"""Long-form synthesis on the device (text2speech_amd/longform.py, audio.join_batches): synthesize_long against its parts, against the
solo chains of its chunks, across groupings, with a chunk that never stops, without read-backs, on a caller's stream, and for
.half() models.

synth.tacotron_state with synth.TACOTRON_HPARAMS and the 64-channel stress WaveGlow of tests/test_streaming_gpu.py; five chunks of
3 - 9 symbols, 40 decoder steps at most, the gate threshold chosen from the solo gate trajectories (tests/longform_util.py) so that
the chunks stop at different steps.  SOLO_BAR is the project's call-against-call bar, 1e-4 rel-L2; every figure is printed before it
is asserted (profiles/longform_tests.md records them)."""
import numpy as np
import pytest
import torch

import join_ref as J
import longform_util as U
import stream_util as SU
import streaming_ref as R
from text2speech_amd import _lib, audio as A, longform as L

pytestmark = pytest.mark.gpu

DEV = U.DEV
SOLO_BAR = R.SOLO_BAR
STRIDE = 256
RATE = 44800
PAUSE_MS, FADE_MS = 2.0, 0.5                        # 90 and 22 samples at 44 800 Hz


@pytest.fixture(scope="module")
def case():
    """the models, the chunks' seeds, the gate threshold and the stop steps it gives: computed once"""
    assert torch.cuda.is_available()
    _lib.load()
    t, w = U.tacotron(), U.waveglow()
    seeds = U.seeds()
    probs = U.solo_gate_probs(t, seeds)
    thr, stops = U.pick_threshold(probs)
    print("long-form case: gate threshold %.6f, stop steps %s" % (thr, stops))
    return dict(t=t, w=w, seeds=seeds, probs=probs, thr=thr, frames=[s + 1 for s in stops], den=A.Denoiser(w),
                tr=A.Trimmer(top_db=23), rs=A.Resampler(RATE, 48000, device=DEV))


def _long(case, thr=None, **kw):
    kw.setdefault("pause_ms", PAUSE_MS)
    kw.setdefault("fade_ms", FADE_MS)
    kw.setdefault("chunks", U.CHUNKS)
    if "seeds" not in kw:
        kw.setdefault("seed", U.SEED)
    try:
        U.set_decoder(case["t"], case["thr"] if thr is None else thr, U.N_STEPS)
        return L.synthesize_long(case["t"], case["w"], sigma=U.SIGMA, **kw)
    finally:
        U.restore_decoder(case["t"])


def _groups(case, batch_size, sort_by_length=True):
    """the batched calls of synthesize_long made by hand, group by group -> ([(mel_post, frames on the device, seeds)], order)"""
    ids = U.chunk_ids()
    n_ids = [i.size(1) for i in ids]
    groups, order = L._plan(n_ids, batch_size, sort_by_length)
    out = []
    try:
        U.set_decoder(case["t"], case["thr"], U.N_STEPS)
        for g in groups:
            padded = torch.zeros(len(g), max(n_ids[c] for c in g), dtype=torch.int64)
            for b, c in enumerate(g):
                padded[b, :n_ids[c]] = ids[c][0]
            s = [case["seeds"][c] for c in g]
            res = case["t"].inference_batch(padded.to(DEV), torch.tensor([n_ids[c] for c in g]), seeds=s)
            out.append((res[1], res[4], s))
    finally:
        U.restore_decoder(case["t"])
    return out, order


def _segments(r, lens=None):
    """the chunks' samples out of a LongForm result (host float32 arrays); lens: their lengths where no pause tells them apart"""
    off = r.offsets.cpu().tolist()
    a = r.audio[0].cpu().numpy()
    n = len(off) - 1
    return [a[off[i]:off[i] + (lens[i] if lens is not None else off[i + 1] - off[i])] for i in range(n)]


def test_it_is_its_parts(case):
    den, tr, rs = case["den"], case["tr"], case["rs"]
    got = _long(case, batch_size=2, denoiser=den, strength=0.1, trimmer=tr, resampler=rs, pcm16=True)
    groups, order = _groups(case, 2)
    assert len(groups) == 3
    batches, flags = [], []
    for mel_post, frames, s in groups:
        wav, wl = case["w"].infer_batch(mel_post, frames, sigma=U.SIGMA, seeds=s)
        wav, wl = den.denoise_batch(wav, wl, 0.1)
        batches.append(tr.trim_batch(wav, wl))
        flags.append(frames == U.N_STEPS)
    pause, fade = L.ms_to_samples(PAUSE_MS, RATE), L.ms_to_samples(FADE_MS, RATE)
    assert (pause, fade) == (90, 22)
    audio, length, offsets = A.join_batches(batches, order=order, pause=pause, fade=fade)
    audio2, length2 = rs.resample_batch(audio, length)
    pcm = A.to_pcm16(audio2, length2)
    print("long-form: %d chunks, %d joined samples at %d Hz, %d at 48000 Hz, offsets %s"
          % (len(U.CHUNKS), int(length), RATE, int(length2), offsets.tolist()))
    assert got.audio.dtype == torch.int16 and tuple(got.audio.shape) == tuple(pcm.shape) and torch.equal(got.audio, pcm)
    assert torch.equal(got.length, length2) and torch.equal(got.offsets, offsets)
    assert got.truncated.dtype == torch.bool and got.truncated.tolist() == torch.cat(flags)[order].tolist() == [False] * 5
    assert got.chunks == U.CHUNKS
    assert 0 < int(length) <= sum(STRIDE * f for f in case["frames"]) + 4 * pause


@pytest.mark.parametrize("denoise", [False, True])
def test_chunks_equal_their_solo_chains(case, denoise):
    t, w, den = case["t"], case["w"], case["den"]
    kw = dict(denoiser=den, strength=0.1) if denoise else {}
    got = _long(case, batch_size=2, fade_ms=0, **kw)
    off = got.offsets.cpu().tolist()
    pause = L.ms_to_samples(PAUSE_MS, RATE)
    solo = []
    try:
        U.set_decoder(t, case["thr"], U.N_STEPS)
        for ids, s in zip(U.chunk_ids(), case["seeds"]):
            a = w.infer(t.inference(ids.to(DEV), None, seed=s)[1], sigma=U.SIGMA, seed=s)
            solo.append((den(a, 0.1)[:, 0] if denoise else a)[0].cpu().numpy())
    finally:
        U.restore_decoder(t)
    lens = [x.size for x in solo]
    want_lens = [(STRIDE * f // 256) * 256 for f in case["frames"]]
    assert lens == want_lens and len(set(lens)) >= 2
    assert off == [sum(lens[:i]) + i * pause for i in range(5)] + [sum(lens) + 4 * pause], "the lengths differ from the solo chains'"
    assert int(got.length) == off[5] and got.truncated.tolist() == [False] * 5
    segs = _segments(got, lens)
    worst = 0.0
    for i, (g, s) in enumerate(zip(segs, solo)):
        e = R.rel(g, s)
        worst = max(worst, e)
        print("long-form chunk %d (%d samples)%s vs its solo chain: rel %.2e, bit-equal %s"
              % (i, s.size, " denoised" if denoise else "", e, bool(np.array_equal(g, s))))
    print("long-form vs solo chains%s: worst rel %.2e" % (" denoised" if denoise else "", worst))
    assert worst < SOLO_BAR
    a = got.audio[0].cpu().numpy()
    for i in range(4):
        assert not a[off[i] + lens[i]:off[i + 1]].any(), "the pause behind chunk %d" % i
    assert not a[off[5]:].any(), "the tail"
    # with a fade the utterance is join_ref of the same rows, bit for bit
    fade = L.ms_to_samples(FADE_MS, RATE)
    faded = _long(case, batch_size=2, **kw)
    want, total, want_off = J.join(segs, lens, gap=pause, fade=fade, dst_cap=faded.audio.size(1))
    assert faded.offsets.cpu().tolist() == want_off.tolist() == off and int(faded.length) == total
    assert faded.audio[0].cpu().numpy().tobytes() == want.tobytes()
    assert not np.array_equal(want, a), "the fade changes nothing: the comparison could not fail"


def test_grouping_does_not_matter(case):
    ref = _long(case, batch_size=5, sort_by_length=False)
    n = int(ref.length)
    worst = 0.0
    for bs in (1, 2, 5):
        for sort in (True, False):
            got = _long(case, batch_size=bs, sort_by_length=sort)
            assert torch.equal(got.length, ref.length) and torch.equal(got.offsets, ref.offsets), (bs, sort)
            assert got.truncated.tolist() == ref.truncated.tolist()
            e = R.rel(got.audio[0, :n], ref.audio[0, :n])
            worst = max(worst, e)
            print("long-form batch_size %d sort %-5s vs one unsorted batch: rel %.2e, bit-equal %s"
                  % (bs, sort, e, bool(torch.equal(got.audio[0, :n], ref.audio[0, :n]))))
            assert not bool(got.audio[0, n:].any())
    assert worst < SOLO_BAR
    # explicit seeds are chunk_seeds' where they are the same values
    again = _long(case, batch_size=5, sort_by_length=False, seeds=case["seeds"])
    assert torch.equal(again.audio, ref.audio)


def test_truncation_is_flagged(case, capfd):
    thr, stops, late = U.pick_truncating_threshold(case["probs"])
    print("long-form truncation: gate threshold %.6f, stop steps %s, chunk %d never stops" % (thr, stops, late))
    got = _long(case, thr=thr, batch_size=2)
    assert "Reached max decoder steps" in capfd.readouterr().err
    assert got.truncated.tolist() == [i == late for i in range(5)]
    off = got.offsets.cpu().tolist()
    pause = L.ms_to_samples(PAUSE_MS, RATE)
    assert off[late + 1] - off[late] - (pause if late < 4 else 0) == STRIDE * U.N_STEPS


def test_no_read_back_behind_inference_batch(case):
    """From inference_batch's results on - the mel, and the output lengths read to the host once, as synthesize_long reads them -
    the whole chain runs with synchronising calls made an error."""
    den, tr, rs, w = case["den"], case["tr"], case["rs"], case["w"]
    (mel_post, frames_d, s), = _groups(case, 5)[0]
    seeds_d = torch.tensor(s, dtype=torch.int64).to(DEV)
    frames = frames_d.cpu()

    def chain():
        wav, wl = w.infer_batch(mel_post, frames, sigma=U.SIGMA, seeds=seeds_d)
        wav, wl = den.denoise_batch(wav, frames * STRIDE, 0.1)
        cut, cl = tr.trim_batch(wav, wl)
        audio, length, offsets = A.join_batches([(cut, cl)], order=[4, 2, 0, 1, 3], pause=90, fade=22)
        audio2, length2 = rs.resample_batch(audio, length)
        return A.to_pcm16(audio2), length2, offsets
    want = chain()                                          # (warm: the first calls load the kernels and pack the weights)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = chain()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(g, x) for g, x in zip(got, want))


def test_join_batches_on_a_callers_stream():
    """join_batches on a stream S whose inputs become true only behind a gate on S, and a consumer on S."""
    gen = torch.Generator().manual_seed(45)
    true = (torch.rand(3, 4096, generator=gen) - 0.5).to(DEV)
    decoy = (torch.rand(3, 4096, generator=gen) - 0.5).to(DEV)
    true_l, decoy_l = torch.tensor([4096, 1500, 3001]).to(DEV), torch.tensor([100, 4096, 7]).to(DEV)
    half = (torch.rand(2, 1000, generator=gen) - 0.5).half().to(DEV)
    buf, buf_l = decoy.clone(), decoy_l.clone()

    def call():
        return A.join_batches([(buf, buf_l), (half, [1000, 333])], order=[2, 4, 0, 1, 3], pauses=[5, 0, 7, 90], fade=8)

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    def fill(a, l):
        buf.copy_(a, non_blocking=True)
        buf_l.copy_(l, non_blocking=True)
    name = "join_batches, two batches, device lengths"
    fill(true, true_l)
    call()
    ref, ms = SU.timed(lambda: [x.clone() for x in call()])
    fill(decoy, decoy_l)
    dec = [x.clone() for x in call()]
    torch.cuda.synchronize()
    assert not same(dec, ref), "the decoy input gives the true result - the test could not fail"
    n = SU.gate_matmuls(ms)
    SU.log(name, ms, n)
    S = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(S):                              # (fills S's pool of the caching allocator, as before_after does)
        call()
    S.synchronize()
    gate = SU.behind_gate(S, [buf, buf_l], [true, true_l], n)       # the decoy until the gate has drained
    with torch.cuda.stream(S):
        out = call()
        gate.check()                                        # nothing waited for the host: the gate is still running
        got = [x.clone() for x in out]                      # the consumer, on S
    S.synchronize()
    assert same(got, ref), "join_batches on a caller's stream differs from the default-stream run"
    again = [x.clone() for x in call()]
    torch.cuda.synchronize()
    assert same(again, ref)
    assert int(ref[1]) == 4096 + 1500 + 3001 + 1000 + 333 + 102


def test_join_batches_results_and_device_checks():
    x = torch.full((3, 1, 50), 1e4, device=DEV)
    x[:, :, ::2] = float("nan")
    rows = [np.linspace(-1, 1, n).astype(np.float32) for n in (50, 20, 0)]
    for b, r in enumerate(rows):
        x[b, 0, :r.size] = torch.from_numpy(r).to(DEV)
    lens = [50, 20, 0]
    for lengths in (lens, torch.tensor(lens), torch.tensor(lens, dtype=torch.int32).to(DEV), torch.tensor(lens).to(DEV)):
        audio, length, offsets = A.join_batch(x, lengths, order=[1, 2, 0], pause=4, fade=3, fade_ends=True)
        want, total, off = J.join([np.pad(r, (0, 50 - r.size)) for r in rows], lens, order=[1, 2, 0], gap=4, fade=3, fade_ends=True,
                                  dst_cap=158)
        assert tuple(audio.shape) == (1, 158) and audio.dtype == torch.float32 and audio.is_cuda
        assert length.dtype == torch.int32 and tuple(length.shape) == (1,) and int(length) == total == 78
        assert offsets.dtype == torch.int64 and offsets.tolist() == off.tolist()
        assert audio[0].cpu().numpy().tobytes() == want.tobytes()
    # a view of wider rows goes in as it is; a transposed one is copied
    wide = torch.zeros(2, 70, device=DEV)
    wide[:, :50] = x[:2, 0].nan_to_num(0.0, posinf=0.0).clamp(-1, 1)
    a1 = A.join_batch(wide[:, :50], [50, 20], pause=1)[0]
    a2 = A.join_batch(wide[:, :50].t().contiguous().t(), [50, 20], pause=1)[0]
    assert torch.equal(a1, a2) and a1.size(1) == 101
    with pytest.raises(_lib.T2SError, match="lengths live on"):
        A.join_batch(x, torch.tensor(lens).to("cuda:1" if torch.cuda.device_count() > 1 else "meta"))         # not the audio's device
    with pytest.raises(_lib.T2SError, match="float32 or float16"):
        A.join_batch(x.double(), lens)


def test_refusals_launch_nothing(case, monkeypatch):
    t, w = case["t"], case["w"]
    calls = []
    monkeypatch.setattr(_lib, "call", lambda *a, **k: calls.append(a[0]))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    T2SError = _lib.T2SError
    with pytest.raises(T2SError, match="seed"):
        L.synthesize_long(t, w, "가. 나.")
    with pytest.raises(T2SError, match="exactly one"):
        L.synthesize_long(t, w, "가. 나.", chunks=["가."], seed=1)
    with pytest.raises(T2SError, match="nothing to say"):
        L.synthesize_long(t, w, " \n ", seed=1)
    t.train()
    try:
        with pytest.raises(T2SError, match="eval mode"):
            L.synthesize_long(t, w, "가. 나.", seed=1)
    finally:
        t.eval()
    w.train()
    try:
        with pytest.raises(T2SError, match="eval mode"):
            L.synthesize_long(t, w, "가. 나.", seed=1)
    finally:
        w.eval()
    assert calls == [] and torch.cuda.memory_allocated(DEV) == before


def test_half_vocoder_output_joins_bit_equal(case):
    """a .half() WaveGlow's infer_batch returns float16: joined, every sample is its exact widening (times the ramps in float32)"""
    wh = U.waveglow(half=True)
    (mel_post, frames_d, s), = _groups(case, 5)[0]
    wav, wl = wh.infer_batch(mel_post.half(), frames_d, sigma=U.SIGMA, seeds=s)
    assert wav.dtype == torch.float16
    rows = [r for r in wav.cpu().numpy()]
    lens = wl.cpu().tolist()
    assert lens == [STRIDE * f for f in frames_d.cpu().tolist()] and len(set(lens)) >= 2
    for fade in (0, 22):
        audio, length, offsets = A.join_batches([(wav, wl)], order=[3, 1, 4, 0, 2], pause=90, fade=fade)
        want, total, off = J.join(rows, lens, order=[3, 1, 4, 0, 2], gap=90, fade=fade, dst_cap=audio.size(1))
        assert int(length) == total and offsets.tolist() == off.tolist()
        assert audio[0].cpu().numpy().tobytes() == want.tobytes()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
