"""WaveGlow.infer_batch of a .half() model on the fp16 chain (engine switch infer_batch_w16, the _h16_ragged entry points, whose
GEMMs skip the column tiles behind an entry's end): every entry of a padded batch gives the audio it gives alone.

synth.WAVEGLOW_SMALL, .half() with the 1x1 convolutions put back to float as the reference's inference script does, frames
(12, 3, 7, 12), sigma 0.666: 384 columns, two column tiles per entry.  Entries 1 (96 columns) and 2 (224) skip their second tile
in every gate and residual GEMM, and are shorter than the largest dilations as well.  Helpers and bars are those of
tests/test_waveglow_infer_batch_gpu.py (the split-bf16 infer_batch) and tests/test_infer_w16_gpu.py (the fp16 chain of infer: the
oracle runs on the fp16-ROUNDED EFFECTIVE weights, in float64 on the CPU)."""
import pytest
import torch

import test_infer_w16_gpu as HW
import test_waveglow_infer_batch_gpu as IB
from oracle import waveglow_oracle as WO
from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = IB.DEV
CFG = IB.CFG
FRAMES = IB.FRAMES
SIGMA = IB.SIGMA
ORACLE_BAR = 1e-3       # rel-L2 and max-rel against the oracle: tests/test_infer_w16_gpu.py's bar for the fp16 chain
SOLO_BAR = IB.SOLO_BAR  # rel-L2 against the solo HIP run: tests/test_waveglow_infer_batch_gpu.py::test_against_the_solo_run
CFG48 = dict(CFG, WN_config=dict(CFG["WN_config"], n_channels=48))


def _half(cfg, sd=None):
    m = IB._build(cfg, sd)
    m.half()
    for c in m.convinv:
        c.float()
    return m


def _oracle16(cfg, m, frames, mel, noise):
    """float64 audio of every entry alone on the fp16-rounded effective weights of the .half() model m, built as
    tests/test_infer_w16_gpu.py builds its oracle (_w16_state) - but from the parameters m HOLDS, widened to f32.  They are that
    file's _half_rounded(sd) except for the 1x1 convolutions: .half() rounds their weights to fp16 as well before .float() widens
    them again, and the oracle has to invert the matrices the model inverts (left unrounded they move the oracle's audio by 6.5e-4
    norm-relative and 9.4e-4 max-relative at 48 channels and 3 frames - more than every other difference here taken together)."""
    sd16 = {k: v.double() for k, v in HW._w16_state({k: v.detach().float().cpu() for k, v in m.state_dict().items()}).items()}
    out = []
    with torch.no_grad():
        for b in range(len(frames)):
            mb, (nf, ne) = IB._entry(cfg, frames, mel, noise, b)
            out.append(WO.waveglow_infer(sd16, cfg, mb.double(), nf.double(), [t.double() for t in ne], sigma=SIGMA)[0])
    return out


def _batch(m, mel, lengths, noise, switch=True):
    eng = m._eng()
    eng.infer_batch_w16 = switch
    try:
        audio, alen = m.infer_batch(mel, lengths, sigma=SIGMA, noise=noise)
    finally:
        eng.infer_batch_w16 = False
    torch.cuda.synchronize()
    return audio, alen


def _solo16(m, mel, noise):
    eng = m._eng()
    eng.infer_w16 = True
    try:
        out = m.infer(mel, sigma=SIGMA, noise=noise)
    finally:
        eng.infer_w16 = None
    assert eng.last_infer_w16 is True and eng.last_infer_batch_w16 is False
    return out


@pytest.fixture(scope="module")
def case():
    """the half model, the inputs on the host and the device, the oracle's audio of every entry alone: computed once"""
    assert torch.cuda.is_available()
    _lib.load()
    sd = synth.waveglow_state(CFG)
    m = _half(CFG, sd)
    mel, noise = IB._inputs(CFG, FRAMES, seed=53)
    return dict(m=m, sd=sd, mel=mel, noise=noise, want=_oracle16(CFG, m, FRAMES, mel, noise), dev=IB._to_dev(mel, noise))


@pytest.fixture(scope="module")
def batch_audio(case):
    mel, noise = case["dev"]
    audio, alen = _batch(case["m"], mel, torch.tensor(FRAMES), noise)
    assert case["m"]._eng().last_infer_batch_w16 is True and case["m"]._eng().last_infer_w16 is True
    return audio, alen


def test_against_the_oracle(case, batch_audio):
    """1. Every entry's valid samples against the float64 oracle of that entry alone, the mel and noise padding holding N(0, 1)
    values; zero tails; int64 audio lengths on the device; the chain is the plain one.  Measured on MI355X: rel-L2 6.1e-5 to 6.9e-5,
    max-rel 6.4e-5 to 8.5e-5 over the four entries (48 channels, test 6: 5.6e-5 to 6.0e-5 and 7.8e-5 to 9.4e-5)."""
    audio, alen = batch_audio
    eng = case["m"]._eng()
    assert eng.last_path == (False, False, None)
    assert audio.dtype == torch.float32
    assert _lib.load().t2s_wg_gate_tile_rows(len(FRAMES), 64, 384) == 128
    IB._check_against("infer_batch (fp16 chain) vs oracle", audio, alen, FRAMES, case["want"], ORACLE_BAR, ORACLE_BAR)


def test_against_the_solo_run(case, batch_audio):
    """2. Every entry against m.infer of it alone with infer_w16 = True: rel-L2 < 1e-4.  Measured on MI355X: 0.0 for all four
    entries - batch and solo runs take the 128-row gate tiles here, and the valid columns see the same operands in the same order."""
    audio, alen = batch_audio
    mel, noise = case["dev"]
    solo = []
    for b in range(len(FRAMES)):
        mb, nb = IB._entry(CFG, FRAMES, mel, noise, b)
        solo.append(_solo16(case["m"], mb, nb)[0])
    IB._check_against("infer_batch (fp16 chain) vs solo infer (fp16 chain)", audio, alen, FRAMES, solo, SOLO_BAR)


def test_padding_independence(case, batch_audio):
    """3. Bit-equal valid samples whether the padding holds N(0, 1) values, zeros, or mel frames of 1e4 - which overflow the fp16
    conditioning planes behind the entries' ends and must neither reach a valid sample nor have the result refused: the check
    for non-finite audio runs after the tails are zeroed."""
    m = case["m"]
    audio, _ = batch_audio
    mel0, noise0 = IB._to_dev(*IB._zero_padding(CFG, FRAMES, case["mel"], case["noise"]))
    audio0, _ = _batch(m, mel0, torch.tensor(FRAMES), noise0)
    big = case["mel"].clone()
    for b, f in enumerate(FRAMES):
        big[b, :, f:] = 1e4
    audio_big, _ = _batch(m, big.to(DEV), torch.tensor(FRAMES), case["dev"][1])
    for b, f in enumerate(FRAMES):
        assert torch.equal(audio[b, :256 * f], audio0[b, :256 * f]), (b, IB._rel(audio[b, :256 * f], audio0[b, :256 * f]))
        assert torch.equal(audio[b, :256 * f], audio_big[b, :256 * f]), (b, IB._rel(audio[b, :256 * f], audio_big[b, :256 * f]))
    assert torch.equal(audio, audio0) and torch.equal(audio, audio_big)         # the tails are zeros either way


def test_equal_lengths_are_infer(case):
    """4. lengths == F everywhere: bit for bit infer() on the fp16 chain - no tile is skipped and the masked kernels do the unmasked
    kernels' arithmetic."""
    m = case["m"]
    mel, noise = case["dev"]
    want = _solo16(m, mel, noise)
    F_ = max(FRAMES)
    audio, alen = _batch(m, mel, torch.full((len(FRAMES),), F_, dtype=torch.int64, device=DEV), noise)
    assert m._eng().last_infer_batch_w16 is True
    assert alen.cpu().tolist() == [256 * F_] * len(FRAMES)
    assert torch.equal(audio, want), IB._rel(audio, want)


def test_stale_workspace():
    """5. One model: a split-bf16 infer_batch at frames (12, 12, 12) leaves bf16 bit patterns in every row of the shared planes;
    then the fp16 chain at (12, 5, 9) on the same workspace, against the oracle as in test 1.  The skipped tiles' acts columns keep
    those patterns (nothing reads them); the X rows past an entry's end must have been stored as zeros."""
    sd = synth.waveglow_state(CFG)
    m = _half(CFG, sd)
    frames = (12, 5, 9)
    mel1, noise1 = IB._inputs(CFG, (12, 12, 12), seed=71)
    mel2, noise2 = IB._inputs(CFG, frames, seed=72)
    mel, noise = IB._to_dev(mel1, noise1)
    a1, _ = _batch(m, mel, [12, 12, 12], noise, switch=False)
    assert m._eng().last_infer_batch_w16 is False and m._eng().last_infer_w16 is False and bool(torch.isfinite(a1).all())
    ws = m._eng().ws
    mel, noise = IB._to_dev(mel2, noise2)
    audio, alen = _batch(m, mel, list(frames), noise)
    assert m._eng().last_infer_batch_w16 is True
    assert m._eng().ws is ws and len(ws) == 1           # the same resident workspace
    IB._check_against("fp16 chain after a split-bf16 call vs oracle", audio, alen, frames,
                      _oracle16(CFG, m, frames, mel2, noise2), ORACLE_BAR, ORACLE_BAR)


def test_48_channels_on_256_row_tiles():
    """6. A half model at 48 channels: the gate GEMM is the 256-row ping-pong kernel, the residual rows are in identity order."""
    sd = synth.waveglow_state(CFG48)
    m = _half(CFG48, sd)
    assert _lib.load().t2s_wg_gate_tile_rows(len(FRAMES), 48, 384) == 256
    mel, noise = IB._inputs(CFG48, FRAMES, seed=55)
    mel_d, noise_d = IB._to_dev(mel, noise)
    audio, alen = _batch(m, mel_d, torch.tensor(FRAMES), noise_d)
    assert m._eng().last_infer_batch_w16 is True
    IB._check_against("C = 48 (256-row tiles) vs oracle", audio, alen, FRAMES, _oracle16(CFG48, m, FRAMES, mel, noise),
                      ORACLE_BAR, ORACLE_BAR)


def test_switch_semantics(case):
    """7. The default leaves infer_batch where it was; True on a model that cannot take the chain raises T2SError naming the
    switch before anything is packed."""
    mel, noise = case["dev"]
    m = case["m"]
    assert m._eng().infer_batch_w16 is False
    m.infer_batch(mel, list(FRAMES), sigma=SIGMA, noise=noise)
    assert m._eng().last_infer_batch_w16 is False and m._eng().last_infer_w16 is False
    _batch(m, mel, list(FRAMES), noise, switch=None)          # reserved: treated as False
    assert m._eng().last_infer_batch_w16 is False and m._eng().last_infer_w16 is False

    f32 = IB._build(CFG)
    mixed = _half(CFG)
    mixed.WN[5].cond_layers[2].float()
    cfg24 = dict(CFG, WN_config=dict(CFG["WN_config"], n_channels=24))
    c24 = _half(cfg24)
    for name, mm in (("f32", f32), ("mixed dtypes", mixed), ("n_channels = 24", c24)):
        ok, why = mm._eng().w16_batch_eligible()
        assert ok is False and why, name
        with pytest.raises(_lib.T2SError, match="infer_batch_w16"):
            _batch(mm, mel, list(FRAMES), noise)
        assert mm._eng().packed16 is None, name


def test_hand_over_from_tacotron():
    """8. Tacotron.inference_batch of a .half() model (synthetic weights, 12 decoder steps at most, the gate threshold placed as
    tests/test_waveglow_infer_batch_gpu.py::test_hand_over_from_tacotron places it), its fp16 mel_post and output_lengths fed to
    infer_batch as they are: both fp16 paths ran, and every entry equals infer() on the fp16 chain of its own frames at the bar of
    test 2."""
    from text2speech_amd.tacotron import Tacotron
    hp = synth.TACOTRON_HPARAMS
    taco = Tacotron(hp, 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state(), strict=True)
    taco = taco.to(DEV).eval().half()
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
    assert taco._eng().last_decode_w16 is True
    frames = olen.cpu().tolist()
    print("output lengths %s at gate threshold %.6f" % (frames, taco.decoder.gate_threshold))
    assert post.dtype == torch.float16 and len(set(frames)) >= 2 and max(frames) == post.size(2)

    m = _half(CFG)
    _, noise = IB._inputs(CFG, frames, seed=89)
    noise = IB._to_dev(post, noise)[1]
    audio, alen = _batch(m, post, olen, noise)
    assert m._eng().last_infer_batch_w16 is True and audio.dtype == torch.float16
    solo = []
    for b in range(3):
        mb, nb = IB._entry(CFG, frames, post, noise, b)
        solo.append(_solo16(m, mb, nb)[0])
    IB._check_against("half Tacotron.inference_batch -> infer_batch vs solo infer, fp16 chain", audio, alen, frames, solo, SOLO_BAR)
