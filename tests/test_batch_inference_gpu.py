"""Batched inference of texts of different lengths (Tacotron.inference_batch): every entry of a batch computes what the same text
computes alone, through each free-running decode form, against the solo HIP run and the CPU oracle."""
import copy

import pytest
import torch

from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP = synth.TACOTRON_HPARAMS


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available()
    _lib.load()
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    return m.to(DEV).eval()


def _set_decoder(model, thr, n):
    model.decoder.gate_threshold, model.decoder.max_decoder_steps = thr, n


def _restore_decoder(model):
    _set_decoder(model, HP["gate_threshold"], HP["max_decoder_steps"])


def _ragged(seed, lengths, n):
    """Padded ids whose padding holds random symbols too (the batch must not read them), and prenet masks [n, B, 2, 256]."""
    gen = torch.Generator().manual_seed(seed)
    B, T = len(lengths), max(lengths)
    ids = torch.randint(2, 80, (B, T), generator=gen)
    masks = (torch.rand(n, B, 2, 256, generator=gen) < 0.5).to(torch.uint8)
    return ids, masks


def _stops(p, thr):
    above = (p > thr).nonzero()
    return int(above[0]) if above.numel() else p.numel()


def _pick_threshold(probs, margin=1e-4):
    """A gate threshold from the solo sigmoid(gate) trajectories at which at least two entries stop at different steps, as few
    as can be had after one or two frames, with every entry's sigmoid(gate) more than `margin` away from it up to and including
    its stop step.  Between two neighbouring values of all trajectories the stop steps do not change; the threshold then goes
    half-way between the nearest values that the entries' prefixes hold."""
    vals = sorted({float(v) for p in probs for v in p})
    best, best_key = None, None
    for lo, hi in zip(vals, vals[1:]):
        mid = 0.5 * (lo + hi)
        stops = [_stops(p, mid) for p in probs]
        near = torch.cat([p[:s + 1] for p, s in zip(probs, stops)])
        below, above = near[near < mid], near[near > mid]
        if below.numel() == 0 or above.numel() == 0:
            continue
        lo2, hi2 = float(below.max()), float(above.min())
        if hi2 - lo2 <= 2 * margin:
            continue
        key = (len(set(stops)) >= 2, sum(s >= 2 for s in stops), len(set(stops)), sum(s < p.numel() for p, s in zip(probs, stops)))
        if best_key is None or key > best_key:
            best, best_key = (0.5 * (lo2 + hi2), stops), key
    assert best is not None and best_key[0], ("no gate threshold separates the entries' stop steps",
                                                    [[round(float(v), 5) for v in p[:12]] for p in probs])
    return best


def _solo(model, ids, L, masks, b):
    return model.inference(ids[b:b + 1, :L].to(DEV), None, prenet_masks=masks[:, b:b + 1])


@pytest.mark.parametrize("lengths,n,solo_bound", [
    ((48, 31, 17), 60, 1e-4),                           # streamed gate partials (<= 4 items): the solo run's decode form
    ((40, 33, 27, 21, 12, 5), 60, 1e-3),                # one-workgroup attention, 5-8 items
    ((50, 47, 44, 40, 35, 31, 26, 20, 13, 7), 50, 1e-3),     # matrix-core cells, one-launch attention (9+ items)
    ((600, 350), 40, 1e-3),                             # past 512 positions: the three-launch attention
])
def test_batch_matches_solo_runs_and_oracle(model, lengths, n, solo_bound):
    from oracle import tacotron_oracle as O
    ids, masks = _ragged(len(lengths) * 7 + lengths[0], lengths, n)
    B = len(lengths)
    sd = synth.tacotron_state()
    try:
        _set_decoder(model, 2.0, n)
        probs = [torch.sigmoid(_solo(model, ids, L, masks, b)[2][0, :, 0].double().cpu()) for b, L in enumerate(lengths)]
        thr, stops = _pick_threshold(probs)
        _set_decoder(model, thr, n)
        lens = torch.tensor(lengths)
        if B == 6:
            lens = lens.to(DEV)                         # lengths on the device: read back once
        mel, post, gate, align, olen = model.inference_batch(ids.to(DEV), lens, prenet_masks=masks)
        solo = [_solo(model, ids, L, masks, b) for b, L in enumerate(lengths)]
    finally:
        _restore_decoder(model)
    model._eng().check_lstm_xbuf()
    want = [min(s + 1, n) for s in stops]
    print("gate threshold %.6f, output lengths %s" % (thr, want))
    assert len(set(want)) >= 2
    assert olen.dtype == torch.int64 and olen.device == mel.device
    assert olen.cpu().tolist() == want == [int(s[0].size(2)) for s in solo]
    N = max(want)
    assert tuple(mel.shape) == tuple(post.shape) == (B, 80, N)
    assert tuple(gate.shape) == (B, N, 1) and tuple(align.shape) == (B, N, max(lengths))
    for b, L in enumerate(lengths):
        f = want[b]
        got = (mel[b:b + 1, :, :f], post[b:b + 1, :, :f], gate[b:b + 1, :f], align[b:b + 1, :f, :L])
        with torch.no_grad():
            orc = O.tacotron_inference(sd, HP, ids[b:b + 1, :L], n, masks[:, b:b + 1].float(), gate_threshold=thr)
        for name, g, s, o in zip(("mel", "mel_post", "gate", "align"), got, solo[b], orc):
            assert tuple(g.shape) == tuple(s.shape) == tuple(o.shape), (b, name)
            assert _rel(g, s) < solo_bound, (b, name, _rel(g, s))
            assert _rel(g, o) < 1e-3, (b, name, _rel(g, o))
        # padding: exactly what parse_output writes, and nothing of the other entries' positions
        assert bool((mel[b, :, f:] == 0).all()) and bool((post[b, :, f:] == 0).all())
        assert bool((gate[b, f:] == 1e3).all())
        assert bool((align[b, f:] == 0).all()) and bool((align[b, :, L:] == 0).all())


def test_full_lengths_equal_inference_bitwise(model):
    n, T = 30, 24
    ids, masks = _ragged(5, (T, T, T), n)
    try:
        _set_decoder(model, 2.0, n)
        want = model.inference(ids.to(DEV), None, prenet_masks=masks)
        got = model.inference_batch(ids.to(DEV), [T, T, T], prenet_masks=masks)
    finally:
        _restore_decoder(model)
    assert got[4].cpu().tolist() == [n, n, n]
    for name, g, w in zip(("mel", "mel_post", "gate", "align"), got[:4], want):
        assert torch.equal(g, w), name


def test_argument_checks_and_half_outputs(model):
    ids, masks = _ragged(9, (12, 7), 8)
    ids = ids.to(DEV)
    for bad in ([12], [12, 7, 3], [0, 7], [12, 13], [12.0, 7.0]):
        with pytest.raises(_lib.T2SError):
            model.inference_batch(ids, bad, prenet_masks=masks)
    model.train()
    try:
        with pytest.raises(_lib.T2SError):
            model.inference_batch(ids, [12, 7], prenet_masks=masks)
    finally:
        model.eval()
    half = copy.deepcopy(model).half()
    try:
        _set_decoder(half, 2.0, 8)
        out = half.inference_batch(ids, torch.tensor([12, 7]), prenet_masks=masks)
    finally:
        _restore_decoder(half)
    assert [o.dtype for o in out] == [torch.float16] * 4 + [torch.int64]
    assert out[4].cpu().tolist() == [8, 8] and bool(torch.isfinite(out[1]).all())


def test_batch_then_vocoded_per_entry_matches_solo_pipeline(model):
    """Three sentences through inference_batch, each vocoded alone from its own frames (WaveGlow.infer, injected noise), against
    the solo text-to-audio pipeline."""
    from text2speech_amd.glow import WaveGlow
    from text2speech_amd.text import text_to_sequence
    texts = ["존경하는 국민 여러분, 2017년 9월 12일입니다.", "안녕하세요.", "오늘은 날씨가 맑고 따뜻합니다."]
    seqs = [torch.as_tensor(text_to_sequence(t)).long() for t in texts]
    lengths = [int(s.numel()) for s in seqs]
    ids = torch.zeros(3, max(lengths), dtype=torch.long)
    for b, s in enumerate(seqs):
        ids[b, :lengths[b]] = s
    n = 40
    gen = torch.Generator().manual_seed(29)
    masks = (torch.rand(n, 3, 2, 256, generator=gen) < 0.5).to(torch.uint8)
    cfg = synth.WAVEGLOW_SMALL
    wg = WaveGlow(**cfg)
    wg.load_state_dict(synth.waveglow_state(cfg))
    wg = wg.to(DEV).eval()
    try:
        _set_decoder(model, 2.0, n)
        _, post, _, _, olen = model.inference_batch(ids.to(DEV), lengths, prenet_masks=masks)
        solo = [_solo(model, ids, L, masks, b)[1] for b, L in enumerate(lengths)]
    finally:
        _restore_decoder(model)
    for b in range(3):
        f = int(olen[b])
        Lz = f * 256 // 8
        nf = torch.randn(1, 4, Lz, generator=gen)
        ne = [torch.randn(1, 2, Lz, generator=gen) for _ in range(2)]
        audio = wg.infer(post[b:b + 1, :, :f], sigma=0.666, noise=(nf, ne))
        want = wg.infer(solo[b], sigma=0.666, noise=(nf, ne))
        assert tuple(audio.shape) == tuple(want.shape) == (1, f * 256)
        assert _rel(audio, want) < 1e-3, (b, _rel(audio, want))
