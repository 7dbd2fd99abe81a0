"""WaveGlow.infer_batch: every entry of a padded batch of mels of different lengths gives the audio it gives
alone - against the CPU oracle of the entry alone, against the solo HIP run, whatever the padding holds, on each engine path, after
a longer call on the same workspace, and fed by Tacotron.inference_batch as it returns.

synth.WAVEGLOW_SMALL: 64 channels, 8 layers (dilations to 128 columns), 32 columns per mel frame.  The 3-frame entry (96 columns) is
shorter than the two largest dilations, the 7-frame entry (224) than the largest: their last layers read past their own end from
nearly every column."""
import collections

import pytest
import torch

from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG = synth.WAVEGLOW_SMALL
FRAMES = (12, 3, 7, 12)
SIGMA = 0.666
ORACLE_BAR = 1e-3       # rel-L2 and max-rel: tests/test_waveglow_gpu.py::test_infer_small_vs_golden
SOLO_BAR = 1e-4         # rel-L2 against the solo HIP run: what tests/test_waveglow_gpu.py holds split-bf16 to
PARTNERS = ("t2s_wg_start", "t2s_wg_start_window", "t2s_wg_res_only", "t2s_wg_res_only_start", "t2s_wg_flow_boundary")


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _maxrel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _build(cfg, sd=None):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg) if sd is None else sd, strict=True)
    return m.to(DEV).eval()


def _cols(cfg, frames):
    return frames * 256 // cfg["n_group"]


def _inputs(cfg, frames, seed):
    """(mel [B, 80, F], (final, [early draws])) at the padded shape, N(0, 1) everywhere: the padding holds values, not zeros"""
    gen = torch.Generator().manual_seed(seed)
    B, F_ = len(frames), max(frames)
    L = _cols(cfg, F_)
    n_early = len([k for k in range(cfg["n_flows"]) if k % cfg["n_early_every"] == 0 and k > 0])
    n_rem = cfg["n_group"] - n_early * cfg["n_early_size"]
    mel = torch.randn(B, 80, F_, generator=gen)
    nf = torch.randn(B, n_rem, L, generator=gen)
    ne = [torch.randn(B, cfg["n_early_size"], L, generator=gen) for _ in range(n_early)]
    return mel, (nf, ne)


def _zero_padding(cfg, frames, mel, noise):
    mel, nf, ne = mel.clone(), noise[0].clone(), [t.clone() for t in noise[1]]
    for b, f in enumerate(frames):
        mel[b, :, f:] = 0
        for t in [nf] + ne:
            t[b, :, _cols(cfg, f):] = 0
    return mel, (nf, ne)


def _entry(cfg, frames, mel, noise, b):
    """entry b alone: its frames, its columns of every draw"""
    f, Lb = frames[b], _cols(cfg, frames[b])
    return mel[b:b + 1, :, :f].contiguous(), (noise[0][b:b + 1, :, :Lb].contiguous(), [t[b:b + 1, :, :Lb].contiguous() for t in noise[1]])


def _oracle(cfg, sd, frames, mel, noise):
    from oracle import waveglow_oracle as O
    out = []
    with torch.no_grad():
        for b in range(len(frames)):
            mb, (nf, ne) = _entry(cfg, frames, mel, noise, b)
            out.append(O.waveglow_infer(sd, cfg, mb, nf, ne, sigma=SIGMA)[0])
    return out


def _to_dev(mel, noise):
    return mel.to(DEV), (noise[0].to(DEV), [t.to(DEV) for t in noise[1]])


def _check_against(label, audio, alen, frames, want, rel_bar, max_bar=None):
    """valid samples of every entry against want[b] (figures printed first), zero tails, audio_lengths"""
    assert tuple(audio.shape) == (len(frames), 256 * max(frames))
    assert alen.dtype == torch.int64 and alen.device == audio.device and alen.cpu().tolist() == [256 * f for f in frames]
    errs = [(_rel(audio[b, :256 * f], want[b]), _maxrel(audio[b, :256 * f], want[b])) for b, f in enumerate(frames)]
    print("%s: frames %s rel %s max %s" % (label, list(frames), ["%.2e" % e[0] for e in errs], ["%.2e" % e[1] for e in errs]))
    assert bool(torch.isfinite(audio).all())
    for b, f in enumerate(frames):
        assert tuple(want[b].shape) == (256 * f,)
        assert bool((audio[b, 256 * f:] == 0).all()), "%s: entry %d's tail is not zero" % (label, b)
        assert errs[b][0] < rel_bar, (label, b, errs[b])
        if max_bar is not None:
            assert errs[b][1] < max_bar, (label, b, errs[b])


@pytest.fixture(scope="module")
def case():
    """the model, the inputs of tests 1 - 4 on the host and the device, the oracle's audio of every entry alone: computed once"""
    assert torch.cuda.is_available()
    _lib.load()
    sd = synth.waveglow_state(CFG)
    m = _build(CFG, sd)
    mel, noise = _inputs(CFG, FRAMES, seed=53)
    want = _oracle(CFG, sd, FRAMES, mel, noise)
    return dict(m=m, sd=sd, mel=mel, noise=noise, want=want, dev=_to_dev(mel, noise))


@pytest.fixture(scope="module")
def batch_audio(case):
    mel, noise = case["dev"]
    audio, alen = case["m"].infer_batch(mel, torch.tensor(FRAMES), sigma=SIGMA, noise=noise)
    torch.cuda.synchronize()
    return audio, alen


def test_against_the_oracle(case, batch_audio):
    """1. Every entry's valid samples against oracle.waveglow_infer of that entry alone (noise sliced), the mel and noise padding
    holding N(0, 1) values; zero tails; audio_lengths.  infer() on the padded batch misses this bar by 50x and more on the two short
    entries (8.3e-2 and 5.0e-2 on the oracle itself, padding zeroed): asserted below on the device, so that the bar is known to
    tell the two apart."""
    audio, alen = batch_audio
    _check_against("infer_batch vs oracle", audio, alen, FRAMES, case["want"], ORACLE_BAR, ORACLE_BAR)
    mel, noise = _to_dev(*_zero_padding(CFG, FRAMES, case["mel"], case["noise"]))
    naive = case["m"].infer(mel, sigma=SIGMA, noise=noise)
    errs = [_rel(naive[b, :256 * f], case["want"][b]) for b, f in enumerate(FRAMES)]
    print("infer() on the padded batch (padding zeroed) vs oracle: rel %s" % ["%.2e" % e for e in errs])
    assert errs[1] > 10 * ORACLE_BAR and errs[2] > 10 * ORACLE_BAR
    assert errs[0] < ORACLE_BAR and errs[3] < ORACLE_BAR


def test_against_the_solo_run(case, batch_audio):
    """2. Every entry against m.infer of it alone: rel-L2 < 1e-4.  Measured on MI355X: 0.0 for all four entries - at these shapes the
    batch and the solo runs take the same tile height, and the valid columns see the same operands in the same order."""
    audio, alen = batch_audio
    mel, noise = case["dev"]
    solo = []
    for b in range(len(FRAMES)):
        mb, nb = _entry(CFG, FRAMES, mel, noise, b)
        solo.append(case["m"].infer(mb, sigma=SIGMA, noise=nb)[0])
    _check_against("infer_batch vs solo infer", audio, alen, FRAMES, solo, SOLO_BAR)


def test_padding_independence(case, batch_audio):
    """3. The same call with all padding zeroed gives bit-equal valid samples (two identical infer calls are bit-identical: asserted
    first, the property this test and the next rest on)."""
    m = case["m"]
    mel, noise = case["dev"]
    a1, a2 = m.infer(mel, sigma=SIGMA, noise=noise), m.infer(mel, sigma=SIGMA, noise=noise)
    assert torch.equal(a1, a2), "two identical infer calls differ: rel %.2e" % _rel(a1, a2)
    audio, _ = batch_audio
    mel0, noise0 = _to_dev(*_zero_padding(CFG, FRAMES, case["mel"], case["noise"]))
    audio0, _ = m.infer_batch(mel0, torch.tensor(FRAMES), sigma=SIGMA, noise=noise0)
    for b, f in enumerate(FRAMES):
        assert torch.equal(audio[b, :256 * f], audio0[b, :256 * f]), (b, _rel(audio[b, :256 * f], audio0[b, :256 * f]))
    assert torch.equal(audio, audio0)           # the tails are zeros either way


def test_equal_lengths_are_infer(case):
    """4. lengths == F everywhere: bit for bit infer() on the same inputs - the masked kernels do the unmasked kernels' arithmetic
    where nothing is masked.  Lengths on the device here (one read-back)."""
    m = case["m"]
    mel, noise = case["dev"]
    want = m.infer(mel, sigma=SIGMA, noise=noise)
    assert torch.equal(want, m.infer(mel, sigma=SIGMA, noise=noise))
    F_ = max(FRAMES)
    audio, alen = m.infer_batch(mel, torch.full((len(FRAMES),), F_, dtype=torch.int64, device=DEV), sigma=SIGMA, noise=noise)
    assert alen.cpu().tolist() == [256 * F_] * len(FRAMES)
    assert torch.equal(audio, want), _rel(audio, want)


def test_stale_workspace():
    """5. One model, frames (12, 12, 12) and then (12, 5, 9) at the same padded shape: the second result against the oracle as in
    test 1.  The X and window planes still hold the first call's rows past the short entries' ends; a writer that skipped the masked
    rows instead of zeroing them would leave them to the dilated taps."""
    sd = synth.waveglow_state(CFG)
    m = _build(CFG, sd)
    frames = (12, 5, 9)
    mel1, noise1 = _inputs(CFG, (12, 12, 12), seed=71)
    mel2, noise2 = _inputs(CFG, frames, seed=72)
    mel, noise = _to_dev(mel1, noise1)
    a1, _ = m.infer_batch(mel, [12, 12, 12], sigma=SIGMA, noise=noise)
    assert bool(torch.isfinite(a1).all())
    ws = m._eng().ws
    mel, noise = _to_dev(mel2, noise2)
    audio, alen = m.infer_batch(mel, list(frames), sigma=SIGMA, noise=noise)
    assert m._eng().ws is ws and len(ws) == 1           # the same resident workspace
    _check_against("second, ragged call vs oracle", audio, alen, frames, _oracle(CFG, sd, frames, mel2, noise2), ORACLE_BAR, ORACLE_BAR)


CFG4 = dict(CFG, n_flows=4)
# (start_fold, boundary) and the _ragged entry points a call takes on each path: F flows, N layers
_PATHS = {
    "default": ({}, (True, True), lambda F, N: dict(t2s_wg_flow_boundary_ragged=F, t2s_wg_start_ragged=0,
                                                    t2s_wg_res_only_start_ragged=F, t2s_wg_res_only_ragged=F * (N - 2))),
    "boundary-off": ({"T2S_FLOW_BOUNDARY": "0"}, (True, False), lambda F, N: dict(t2s_wg_flow_boundary_ragged=0, t2s_wg_start_ragged=F,
                                                                                  t2s_wg_res_only_start_ragged=0, t2s_wg_res_only_ragged=F * (N - 1))),
    "fold-off": ({"T2S_START_FOLD": "0"}, (False, False), lambda F, N: dict(t2s_wg_flow_boundary_ragged=0, t2s_wg_start_ragged=F,
                                                                            t2s_wg_res_only_start_ragged=0, t2s_wg_res_only_ragged=F * (N - 1))),
}


@pytest.fixture(scope="module")
def case4():
    sd = synth.waveglow_state(CFG4)
    mel, noise = _inputs(CFG4, FRAMES, seed=54)
    return dict(sd=sd, mel=mel, noise=noise, want=_oracle(CFG4, sd, FRAMES, mel, noise))


@pytest.mark.parametrize("name", list(_PATHS))
def test_each_engine_path(monkeypatch, case4, name):
    """6. Test 1's check with n_flows = 4 on each path a no-grad call can take (fresh model, environment as the path's switch), and
    the launches counted at the C ABI as tests/test_engine_paths_gpu.py counts them: T2S_COND_COMPOSE=1 is set and must not be
    read; no t2s_zero_plane_rows; none of the partner entry points; in total at most infer()'s launches + 2."""
    env, (start_fold, boundary), ragged = _PATHS[name]
    for var in ("T2S_START_FOLD", "T2S_FLOW_BOUNDARY"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("T2S_COND_COMPOSE", "1")
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    m = _build(CFG4, case4["sd"])
    eng = m._eng()
    F, N = m.n_flows, m.WN[0].n_layers
    mel, noise = _to_dev(case4["mel"], case4["noise"])
    audio, alen = m.infer_batch(mel, list(FRAMES), sigma=SIGMA, noise=noise)          # (packs the weights, inverts the 1x1s)
    assert eng.last_path == (start_fold, boundary, None)
    _check_against("path %s vs oracle" % name, audio, alen, FRAMES, case4["want"], ORACLE_BAR, ORACLE_BAR)

    seen = collections.Counter()
    real_call = _lib.call

    def counting_call(fn, *args):
        seen[fn] += 1
        return real_call(fn, *args)
    monkeypatch.setattr(_lib, "call", counting_call)
    audio2, _ = m.infer_batch(mel, list(FRAMES), sigma=SIGMA, noise=noise)
    torch.cuda.synchronize()
    batch = collections.Counter(seen)
    seen.clear()
    monkeypatch.delenv("T2S_COND_COMPOSE")
    m.infer(mel, sigma=SIGMA, noise=noise)
    torch.cuda.synchronize()
    plain = collections.Counter(seen)
    print("path %s: infer_batch %d launches, infer %d; %r" % (name, sum(batch.values()), sum(plain.values()), dict(batch)))
    assert torch.equal(audio2, audio)
    assert batch["t2s_zero_plane_rows"] == 0
    assert not any(batch[p] for p in PARTNERS), batch
    assert {k: batch[k] for k in ragged(F, N)} == ragged(F, N)
    assert not any(k.endswith("_ragged") for k in plain), plain
    assert sum(batch.values()) <= sum(plain.values()) + 2
    assert batch["t2s_wg_in_melwin_gate_fold"] == 0 and batch["t2s_wg_upsample_squeeze"] == 1


def test_hand_over_from_tacotron():
    """7. Tacotron.inference_batch on three short texts (synthetic weights, 12 decoder steps at most, the gate threshold placed in
    a gap - wider than 2e-4 - of the entries' own gate values at which they stop at as many different frames as can be had), its
    mel_post and output_lengths fed to infer_batch as they are; every entry against infer() on its own frames at the bar of
    test 2."""
    from text2speech_amd.tacotron import Tacotron
    hp = synth.TACOTRON_HPARAMS
    taco = Tacotron(hp, 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state(), strict=True)
    taco = taco.to(DEV).eval()
    n, lengths = 12, (23, 9, 16)
    gen = torch.Generator().manual_seed(88)
    ids = torch.randint(2, 80, (3, max(lengths)), generator=gen).to(DEV)
    masks = (torch.rand(n, 3, 2, 256, generator=gen) < 0.5).to(torch.uint8)
    taco.decoder.max_decoder_steps, taco.decoder.gate_threshold = n, 2.0
    gate = taco.inference_batch(ids, lengths, prenet_masks=masks)[2]
    probs = torch.sigmoid(gate[:, :, 0].double().cpu())                       # [3, n]: nobody stopped
    vals = sorted(set(probs.flatten().tolist()))
    gaps = []
    for lo, hi in zip(vals, vals[1:]):
        stops = [int((p > 0.5 * (lo + hi)).nonzero()[0]) if bool((p > 0.5 * (lo + hi)).any()) else n for p in probs]
        if len(set(stops)) >= 2 and hi - lo > 2e-4:
            gaps.append((len(set(stops)), sum(s >= 2 for s in stops), hi - lo, 0.5 * (lo + hi)))
    assert gaps, "no gate threshold separates the entries' stop steps"
    taco.decoder.gate_threshold = max(gaps)[3]
    _, post, _, _, olen = taco.inference_batch(ids, lengths, prenet_masks=masks)
    frames = olen.cpu().tolist()
    print("output lengths %s at gate threshold %.6f" % (frames, taco.decoder.gate_threshold))
    assert len(set(frames)) >= 2 and max(frames) == post.size(2)

    m = _build(CFG)
    _, noise = _inputs(CFG, frames, seed=89)
    noise = _to_dev(post, noise)[1]
    audio, alen = m.infer_batch(post, olen, sigma=SIGMA, noise=noise)
    solo = []
    for b in range(3):
        mb, nb = _entry(CFG, frames, post, noise, b)
        solo.append(m.infer(mb, sigma=SIGMA, noise=nb)[0])
    _check_against("Tacotron.inference_batch -> infer_batch vs solo infer", audio, alen, frames, solo, SOLO_BAR)


def test_refusals(monkeypatch, case):
    """8. Bad lengths, a noise tuple of the wrong shape and host tensors raise T2SError (or ValueError) before anything is launched."""
    m = case["m"]
    mel, noise = case["dev"]
    F_, B = max(FRAMES), len(FRAMES)
    launched = []
    monkeypatch.setattr(_lib, "call", lambda fn, *a: launched.append(fn))
    short = (noise[0][:, :, :-1], noise[1])
    bad = [
        dict(lengths=[12, 0, 7, 12]), dict(lengths=[12, 3, 7, F_ + 1]), dict(lengths=[12, 3, 7]), dict(lengths=[12, 3, 7, 12, 12]),
        dict(lengths=torch.tensor([12.0, 3.0, 7.0, 12.0])), dict(lengths=torch.tensor([12, 3, 7, 12], device=DEV).float()),
        dict(lengths=torch.tensor([[12, 3, 7, 12]])),
        dict(noise=short), dict(noise=(noise[0], noise[1][:1])), dict(noise=(noise[0][:B - 1], noise[1])),
        dict(noise=(noise[0], [noise[1][0], noise[1][1][:, :1]])), dict(noise=noise[0]),
        dict(spect=case["mel"]),
    ]
    for ch in bad:
        a = dict(spect=mel, lengths=list(FRAMES), sigma=SIGMA, noise=noise)
        a.update(ch)
        with pytest.raises((_lib.T2SError, ValueError)):
            m.infer_batch(**a)
    assert launched == []
