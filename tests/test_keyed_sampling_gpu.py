"""Per-utterance seeds (text2speech_amd/sampling.py, csrc/sampling.hip): with ``seed=`` / ``seeds=`` an entry draws the same prenet
masks and the same vocoder noise alone and in any batch, so the batching promise - entry b of a batch gets what it gets alone -
holds for a caller who injects no draws by hand.

Vocoder: synth.WAVEGLOW_SMALL and mels of (12, 7, 3) frames, the shapes and the bar (SOLO_BAR, 1e-4 relative L2 against the solo HIP
run) of tests/test_waveglow_infer_batch_gpu.py.  Tacotron: texts of (48, 31, 17) symbols, 60 steps and a gate threshold picked with
a margin from the solo trajectories, as tests/test_batch_inference_gpu.py does, and its bound for that batch size (1e-4 at <= 4
items)."""
import pytest
import torch

import test_batch_inference_gpu as BI
import test_waveglow_infer_batch_gpu as IB
from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = IB.DEV
CFG = IB.CFG
SIGMA = IB.SIGMA
SOLO_BAR = IB.SOLO_BAR
FRAMES = (12, 7, 3)
SEEDS = (11, 2 ** 62 + 5, 0)
TEXTS = (48, 31, 17)
STEPS = 60
TACO_BAR = 1e-4         # tests/test_batch_inference_gpu.py: batch against solo at <= 4 items
_rel = IB._rel


def _cols(frames):
    return IB._cols(CFG, frames)


def _mels(frames, seed):
    """[B, 80, F] N(0, 1) everywhere, the padding included"""
    return torch.randn(len(frames), 80, max(frames), generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.fixture(scope="module")
def wg():
    assert torch.cuda.is_available()
    _lib.load()
    return IB._build(CFG)


@pytest.fixture(scope="module")
def mel():
    return _mels(FRAMES, seed=153)


@pytest.fixture(scope="module")
def batch_audio(wg, mel):
    audio, alen = wg.infer_batch(mel, torch.tensor(FRAMES), sigma=SIGMA, seeds=SEEDS)
    torch.cuda.synchronize()
    return audio, alen


# ---------------------------------------------------------------------------------------------------------------- vocoder
def test_vocoder_noise_bridge(wg, mel, batch_audio):
    """infer(seed=s) is bit for bit infer(noise=draw_noise([s], L)); the same for the batch; draw_noise's layout is noise='s."""
    for b, f in enumerate(FRAMES):
        mb = mel[b:b + 1, :, :f].contiguous()
        noise = wg.draw_noise([SEEDS[b]], _cols(f))
        assert tuple(noise[0].shape) == (1, wg.n_remaining_channels, _cols(f)) and len(noise[1]) == 2
        assert all(tuple(t.shape) == (1, wg.n_early_size, _cols(f)) for t in noise[1])
        assert bool(torch.isfinite(noise[0]).all()) and 0.8 < float(noise[0].std()) < 1.2
        seeded = wg.infer(mb, sigma=SIGMA, seed=SEEDS[b])
        assert torch.equal(seeded, wg.infer(mb, sigma=SIGMA, noise=noise)), (b, _rel(seeded, wg.infer(mb, sigma=SIGMA, noise=noise)))
    audio, _ = batch_audio
    injected, _ = wg.infer_batch(mel, list(FRAMES), sigma=SIGMA, noise=wg.draw_noise(SEEDS, _cols(max(FRAMES))))
    assert torch.equal(audio, injected)


def test_vocoder_batch_against_solo(wg, mel, batch_audio):
    audio, alen = batch_audio
    solo = [wg.infer(mel[b:b + 1, :, :f].contiguous(), sigma=SIGMA, seed=SEEDS[b])[0] for b, f in enumerate(FRAMES)]
    print("infer_batch(seeds=) bit-equal to infer(seed=): %s" % [bool(torch.equal(audio[b, :256 * f], solo[b])) for b, f in enumerate(FRAMES)])
    IB._check_against("infer_batch(seeds=) vs solo infer(seed=)", audio, alen, FRAMES, solo, SOLO_BAR)
    assert all(float(s.abs().max()) > 0 for s in solo)


def test_vocoder_regrouping(wg, mel, batch_audio):
    """Entries 1 and 2 in a second batch: other places, another neighbour, a longer padded length and other values in the padding."""
    audio, _ = batch_audio
    frames2 = (3, 16, 7)
    mel2 = _mels(frames2, seed=154)
    mel2[0, :, :3] = mel[2, :, :3]
    mel2[2, :, :7] = mel[1, :, :7]
    audio2, _ = wg.infer_batch(mel2, list(frames2), sigma=SIGMA, seeds=[SEEDS[2], 99, SEEDS[1]])
    for b2, b, f in ((0, 2, 3), (2, 1, 7)):
        got, want = audio2[b2, :256 * f], audio[b, :256 * f]
        print("regrouped entry of %d frames: rel %.2e, bit-equal %s" % (f, _rel(got, want), bool(torch.equal(got, want))))
        assert _rel(got, want) < SOLO_BAR
        assert bool((audio2[b2, 256 * f:] == 0).all())
    # the draws themselves do not know the batch: entry 1's noise at either place, either length
    z1 = wg.draw_noise(SEEDS, _cols(12))
    z2 = wg.draw_noise([SEEDS[2], 99, SEEDS[1]], _cols(16))
    for a, b_ in zip([z1[0]] + z1[1], [z2[0]] + z2[1]):
        assert torch.equal(a[1, :, :_cols(7)], b_[2, :, :_cols(7)]) and torch.equal(a[2, :, :_cols(3)], b_[0, :, :_cols(3)])


def test_vocoder_repeat_and_seed_change(wg, mel, batch_audio):
    audio, _ = batch_audio
    torch.manual_seed(1)
    again, _ = wg.infer_batch(mel, list(FRAMES), sigma=SIGMA, seeds=torch.tensor(SEEDS, dtype=torch.int64))             # host tensor
    torch.manual_seed(2)
    third, _ = wg.infer_batch(mel, list(FRAMES), sigma=SIGMA, seeds=torch.tensor(SEEDS, dtype=torch.int64, device=DEV))  # device tensor
    assert torch.equal(audio, again) and torch.equal(audio, third)
    other, _ = wg.infer_batch(mel, list(FRAMES), sigma=SIGMA, seeds=[s + 1 for s in SEEDS])
    for b, f in enumerate(FRAMES):
        assert _rel(other[b, :256 * f], audio[b, :256 * f]) > 0.1, b
    # unseeded calls still draw from torch's generator at the padded shape: two of them differ
    u1, _ = wg.infer_batch(mel, list(FRAMES), sigma=SIGMA)
    u2, _ = wg.infer_batch(mel, list(FRAMES), sigma=SIGMA)
    assert not torch.equal(u1, u2)


def test_vocoder_per_entry_sigma(wg, mel):
    sig = torch.tensor([0.666, 0.5, 1.0])
    audio, alen = wg.infer_batch(mel, list(FRAMES), sigma=sig.to(DEV), seeds=SEEDS)
    solo = [wg.infer(mel[b:b + 1, :, :f].contiguous(), sigma=float(sig[b]), seed=SEEDS[b])[0] for b, f in enumerate(FRAMES)]
    IB._check_against("infer_batch(seeds=, sigma=[B]) vs solo infer(seed=, sigma_b)", audio, alen, FRAMES, solo, SOLO_BAR)
    host, _ = wg.infer_batch(mel, list(FRAMES), sigma=sig, seeds=SEEDS)
    assert torch.equal(host, audio)


def test_vocoder_fp16_batch_chain(mel):
    """The same on the opt-in fp16 chain of a .half() model: bridge, batch against solo (infer_w16 = True), repeat."""
    m = IB._build(CFG)
    m.half()
    for c in m.convinv:
        c.float()
    eng = m._eng()
    eng.infer_batch_w16 = True
    audio, alen = m.infer_batch(mel, list(FRAMES), sigma=SIGMA, seeds=SEEDS)
    assert eng.last_infer_batch_w16 is True and eng.last_infer_w16 is True
    again, _ = m.infer_batch(mel, list(FRAMES), sigma=SIGMA, seeds=SEEDS)
    injected, _ = m.infer_batch(mel, list(FRAMES), sigma=SIGMA, noise=m.draw_noise(SEEDS, _cols(max(FRAMES))))
    assert torch.equal(audio, again) and torch.equal(audio, injected)
    eng.infer_batch_w16, eng.infer_w16 = False, True
    solo = []
    for b, f in enumerate(FRAMES):
        mb = mel[b:b + 1, :, :f].contiguous()
        solo.append(m.infer(mb, sigma=SIGMA, seed=SEEDS[b])[0])
        assert eng.last_infer_w16 is True and eng.last_infer_batch_w16 is False
        assert torch.equal(solo[b], m.infer(mb, sigma=SIGMA, noise=m.draw_noise([SEEDS[b]], _cols(f)))[0])
    print("fp16 chain: infer_batch(seeds=) bit-equal to infer(seed=): %s"
          % [bool(torch.equal(audio[b, :256 * f], solo[b])) for b, f in enumerate(FRAMES)])
    IB._check_against("fp16 chain: infer_batch(seeds=) vs solo infer(seed=)", audio, alen, FRAMES, solo, SOLO_BAR)


def test_vocoder_refusals(monkeypatch, wg, mel):
    launched = []
    noise = wg.draw_noise(SEEDS, _cols(max(FRAMES)))
    monkeypatch.setattr(_lib, "call", lambda fn, *a: launched.append(fn))
    T2SError = _lib.T2SError
    sig = torch.tensor([0.666, 0.5, 1.0], device=DEV)
    batch = dict(spect=mel, lengths=list(FRAMES), sigma=SIGMA)
    for kind, extra in [(T2SError, dict(noise=noise, seeds=SEEDS)), (T2SError, dict(sigma=sig)), (T2SError, dict(sigma=sig, noise=noise)),
                        (ValueError, dict(seeds=[1, -2, 3])), (ValueError, dict(seeds=torch.tensor([1, -2, 3]))),
                        (ValueError, dict(seeds=[1, 2])), (ValueError, dict(seeds=[1, 2, 3, 4])), (ValueError, dict(seeds=[1, 2, 2 ** 63])),
                        (ValueError, dict(seeds=torch.tensor([1, 2], device=DEV))), (ValueError, dict(seeds=[1.5, 2, 3])),
                        (ValueError, dict(seeds=torch.tensor([1, 2, 3], dtype=torch.int32))),
                        (ValueError, dict(seeds=SEEDS, sigma=torch.tensor([0.5, 0.5]))), (ValueError, dict(seeds=SEEDS, sigma=-1.0)),
                        (ValueError, dict(seeds=SEEDS, sigma=torch.tensor([0.5, float("nan"), 1.0])))]:
        with pytest.raises(kind):
            wg.infer_batch(**dict(batch, **extra))
    solo = mel[:1]
    with pytest.raises(T2SError):
        wg.infer(solo, sigma=SIGMA, noise=(noise[0][:1], [t[:1] for t in noise[1]]), seed=3)
    with pytest.raises(T2SError):
        wg.infer(solo, sigma=sig[:1])
    with pytest.raises(ValueError):
        wg.infer(solo, sigma=SIGMA, seed=-1)
    with pytest.raises(ValueError):
        wg.draw_noise([1, -1], 8)
    with pytest.raises(ValueError):
        wg.draw_noise([], 8)
    assert launched == []


# --------------------------------------------------------------------------------------------------------------- Tacotron
@pytest.fixture(scope="module")
def taco():
    assert torch.cuda.is_available()
    _lib.load()
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(BI.HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    return m.to(DEV).eval()


def _solo_taco(taco, ids, b, seed):
    """(outputs, the mask buffer the call read) of text b alone under `seed`, no masks injected"""
    out = taco.inference(ids[b:b + 1, :TEXTS[b]].contiguous(), seed=seed)
    return out, taco._eng().last_prenet_masks


@pytest.fixture(scope="module")
def taco_case(taco):
    """ids (padding holds random symbols), the gate threshold picked from the solo trajectories under SEEDS, the batch's outputs and
    masks and every solo run's at that threshold: computed once, read only"""
    ids = torch.randint(2, 80, (len(TEXTS), max(TEXTS)), generator=torch.Generator().manual_seed(len(TEXTS) * 7 + TEXTS[0])).to(DEV)
    try:
        BI._set_decoder(taco, 2.0, STEPS)
        probs = [torch.sigmoid(_solo_taco(taco, ids, b, SEEDS[b])[0][2][0, :, 0].double().cpu()) for b in range(len(TEXTS))]
        thr, stops = BI._pick_threshold(probs)
        BI._set_decoder(taco, thr, STEPS)
        torch.manual_seed(5)
        batch = taco.inference_batch(ids, torch.tensor(TEXTS), seeds=SEEDS)
        batch_masks = taco._eng().last_prenet_masks
        torch.manual_seed(6)
        solo = [_solo_taco(taco, ids, b, SEEDS[b]) for b in range(len(TEXTS))]
    finally:
        BI._restore_decoder(taco)
    want = [min(s + 1, STEPS) for s in stops]
    print("gate threshold %.6f, output lengths %s" % (thr, want))
    return dict(ids=ids, thr=thr, want=want, batch=batch, batch_masks=batch_masks, solo=solo, probs=probs)


def test_tacotron_batch_against_solo(taco_case):
    c = taco_case
    mel, post, gate, align, olen = c["batch"]
    assert len(set(c["want"])) >= 2
    assert olen.cpu().tolist() == c["want"] == [int(s[0][0].size(2)) for s in c["solo"]]          # the same stop steps
    assert tuple(c["batch_masks"].shape) == (STEPS, len(TEXTS), 2, 256) and c["batch_masks"].dtype == torch.uint8
    for b, L in enumerate(TEXTS):
        out, masks = c["solo"][b]
        assert tuple(masks.shape) == (STEPS, 1, 2, 256)
        assert torch.equal(c["batch_masks"][:, b], masks[:, 0]), "entry %d drew other masks in the batch than alone" % b
        assert 0.45 < float(masks.float().mean()) < 0.55
        f = c["want"][b]
        got = (mel[b:b + 1, :, :f], post[b:b + 1, :, :f], gate[b:b + 1, :f])
        for name, g, s in zip(("mel", "mel_post", "gate"), got, out):
            assert tuple(g.shape) == tuple(s.shape), (b, name)
            print("inference_batch(seeds=) vs inference(seed=) entry %d %s: rel %.2e" % (b, name, _rel(g, s)))
            assert _rel(g, s) < TACO_BAR, (b, name, _rel(g, s))
    assert not torch.equal(c["batch_masks"][:, 0], c["batch_masks"][:, 1])


def test_tacotron_regrouping(taco, taco_case):
    """Entries 1 and 2 regrouped and reordered, beside another text and under a longer padding: the same masks, the same stop step."""
    c = taco_case
    ids2 = torch.randint(2, 80, (3, 53), generator=torch.Generator().manual_seed(77)).to(DEV)
    ids2[0, :TEXTS[2]] = c["ids"][2, :TEXTS[2]]
    ids2[2, :TEXTS[1]] = c["ids"][1, :TEXTS[1]]
    try:
        BI._set_decoder(taco, c["thr"], STEPS)
        out = taco.inference_batch(ids2, [TEXTS[2], 53, TEXTS[1]], seeds=torch.tensor([SEEDS[2], 4242, SEEDS[1]], device=DEV))
        masks = taco._eng().last_prenet_masks
    finally:
        BI._restore_decoder(taco)
    olen = out[4].cpu().tolist()
    for b2, b in ((0, 2), (2, 1)):
        assert torch.equal(masks[:, b2], c["batch_masks"][:, b]), (b2, b)
        assert olen[b2] == c["want"][b], (olen, c["want"])
        f = c["want"][b]
        assert _rel(out[1][b2:b2 + 1, :, :f], c["solo"][b][0][1]) < TACO_BAR          # mel_post against the solo run, as above


def test_tacotron_refusals(monkeypatch, taco, taco_case):
    ids = taco_case["ids"]
    masks = torch.ones(STEPS, 3, 2, 256, dtype=torch.uint8)
    launched = []
    monkeypatch.setattr(_lib, "call", lambda fn, *a: launched.append(fn))
    with pytest.raises(_lib.T2SError):
        taco.inference(ids[:1], prenet_masks=masks[:, :1], seed=3)
    with pytest.raises(_lib.T2SError):
        taco.inference_batch(ids, list(TEXTS), prenet_masks=masks, seeds=SEEDS)
    for bad in ([1, 2], [1, 2, 3, 4], [1, -1, 3], [1, 2, 2 ** 63], torch.tensor([1, -1, 3]), torch.tensor([1, 2], device=DEV), [0.5, 1, 2]):
        with pytest.raises((ValueError, _lib.T2SError)):
            taco.inference_batch(ids, list(TEXTS), seeds=bad)
    for bad in (-1, 2 ** 63, 1.5):
        with pytest.raises((ValueError, _lib.T2SError)):
            taco.inference(ids[:1], seed=bad)
    assert launched == []


# ------------------------------------------------------------------------------------------------------------------ chain
def _chain_threshold(probs, margin=1e-4, min_frames=3):
    """A gate threshold for the chain, whose denoiser needs more than 512 samples (3 frames) of every entry: from the solo
    trajectories as tests/test_batch_inference_gpu.py::_pick_threshold picks (half-way inside a gap wider than 2 margin of the values
    the entries meet up to their stop steps), every entry giving at least min_frames frames, as many different lengths as can be
    had.  Without such a gap: 2.0, which no sigmoid passes - every entry then runs all its steps."""
    vals = sorted({float(v) for p in probs for v in p})
    best, best_key = 2.0, 0
    for lo, hi in zip(vals, vals[1:]):
        mid = 0.5 * (lo + hi)
        stops = [BI._stops(p, mid) for p in probs]
        if min(stops) + 1 < min_frames:
            continue
        near = torch.cat([p[:s + 1] for p, s in zip(probs, stops)])
        below, above = near[near < mid], near[near > mid]
        if below.numel() == 0 or above.numel() == 0 or float(above.min()) - float(below.max()) <= 2 * margin:
            continue
        if len(set(stops)) > best_key:
            best, best_key = 0.5 * (float(below.max()) + float(above.min())), len(set(stops))
    return best


def test_chain_text_to_pcm(taco, wg, taco_case):
    """inference_batch(seeds=S) -> infer_batch(seeds=S) -> denoise_batch -> to_pcm16, every result passed on as returned, against each
    entry's solo chain on the batch's own mel_post slice with the same seed."""
    from text2speech_amd.audio import Denoiser, to_pcm16
    try:
        BI._set_decoder(taco, _chain_threshold(taco_case["probs"]), STEPS)
        _, post, _, _, olen = taco.inference_batch(taco_case["ids"], list(TEXTS), seeds=SEEDS)
    finally:
        BI._restore_decoder(taco)
    frames = olen.cpu().tolist()
    print("chain: output lengths %s" % frames)
    assert min(frames) >= 3
    den = Denoiser(wg).to(DEV)
    audio, alen = wg.infer_batch(post, olen, sigma=SIGMA, seeds=SEEDS)
    den_audio, dlen = den.denoise_batch(audio, alen, 0.1)
    pcm = to_pcm16(den_audio, dlen)
    assert pcm.dtype == torch.int16 and tuple(pcm.shape) == (len(frames), 1, 256 * max(frames))
    solo = []
    for b, f in enumerate(frames):
        n = 256 * f
        a = wg.infer(post[b:b + 1, :, :f].contiguous(), sigma=SIGMA, seed=SEEDS[b])
        solo.append(a[0])
        same = bool(torch.equal(a[0], audio[b, :n]))
        want = to_pcm16(den(a, strength=0.1))
        diff = int((pcm[b, 0, :n].int() - want[0, 0].int()).abs().max())
        print("chain entry %d (%d frames): audio bit-equal %s, rel %.2e; worst PCM difference %d" % (b, f, same, _rel(audio[b, :n], a[0]), diff))
        if same:
            assert torch.equal(pcm[b, 0, :n], want[0, 0]), "entry %d: equal audio, different PCM (worst %d)" % (b, diff)
        assert bool((pcm[b, 0, n:] == 0).all())
    IB._check_against("chain: infer_batch(seeds=) on inference_batch(seeds=)'s mel_post vs solo infer(seed=)", audio, alen, frames, solo, SOLO_BAR)
