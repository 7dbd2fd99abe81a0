"""Streaming synthesis on the device (text2speech_amd/streaming.py): WaveGlow.infer_window / infer_stream
against the float64 oracle's whole run and against infer(seed=); Tacotron.inference_stream against inference(seed=);
streaming.synthesize_stream against its parts.

synth.WAVEGLOW_SMALL with the stress weights, 260 frames: the exact halo (99, 96) is cut by the utterance's start in the first
window, by neither end in the middle one, by its end in the last.  ORACLE_BAR / SOLO_BAR are the project's bars
(tests/test_waveglow_infer_batch_gpu.py); every figure is printed before it is asserted, and whether a window came out bit-equal to
the whole call's slice is recorded, not asserted: the GEMMs tile two lengths differently."""
import collections

import pytest
import torch

import streaming_ref as R
from text2speech_amd import _lib, streaming, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG, F, SIGMA = R.CFG, R.F, R.SIGMA
SEED, SEED2 = 20240611, 977
HP = synth.TACOTRON_HPARAMS


def _waveglow(sd, half=False):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**CFG)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    if half:            # as the reference's inference script: .half() with the 1x1 convolutions put back to float
        m.half()
        for c in m.convinv:
            c.float()
    return m


@pytest.fixture(scope="module")
def case():
    """the stress model, a mel of 260 frames, the keyed draws of SEED, infer(seed=)'s audio and the oracle's: computed once"""
    assert torch.cuda.is_available()
    _lib.load()
    sd = synth.waveglow_state(CFG, **R.STRESS)
    m = _waveglow(sd)
    gen = torch.Generator().manual_seed(97)
    mel = torch.randn(1, 80, F, generator=gen)
    nf, ne = m.draw_noise([SEED], R.cols(CFG, F))
    from oracle import waveglow_oracle as O
    with torch.no_grad():
        want = O.waveglow_infer(R.double_state(sd), CFG, mel.double(), nf.double().cpu(), [t.double().cpu() for t in ne], sigma=SIGMA)[0]
    mel_d = mel.to(DEV)
    whole = m.infer(mel_d, sigma=SIGMA, seed=SEED)
    torch.cuda.synchronize()
    print("infer(seed=) vs oracle, 260 frames: rel %.2e max %.2e" % (R.rel(whole[0], want), R.maxrel(whole[0], want)))
    return dict(sd=sd, m=m, mel=mel_d, want=want, whole=whole)


def _final(f1):
    return f1 == F


@pytest.mark.parametrize("f0,f1", R.WINDOWS)
def test_infer_window_against_oracle_and_infer(case, f0, f1):
    m = case["m"]
    got = m.infer_window(case["mel"], f0, f1, sigma=SIGMA, seed=SEED, final=_final(f1))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 256 * (f1 - f0)) and got.dtype == torch.float32
    want, solo = case["want"][256 * f0:256 * f1], case["whole"][0, 256 * f0:256 * f1]
    e = (R.rel(got[0], want), R.maxrel(got[0], want), R.rel(got[0], solo))
    print("infer_window [%d, %d): vs oracle rel %.2e max %.2e; vs infer(seed=) rel %.2e, bit-equal %s"
          % (f0, f1, e[0], e[1], e[2], bool(torch.equal(got[0], solo))))
    assert e[0] < R.ORACLE_BAR and e[1] < R.ORACLE_BAR
    assert e[2] < R.SOLO_BAR
    # the same window with a 2-frame halo is a wrong window, and the bar says so
    short = m.infer_window(case["mel"], f0, f1, sigma=SIGMA, seed=SEED, final=_final(f1), halo=(2, 2))
    es = R.rel(short[0], want)
    print("infer_window [%d, %d) with halo (2, 2): vs oracle rel %.2e" % (f0, f1, es))
    assert es > 10 * R.ORACLE_BAR


def test_infer_window_arguments(case):
    m, mel = case["m"], case["mel"]
    T2SError = _lib.T2SError
    with pytest.raises(T2SError):
        m.infer_window(mel, 0, 32, sigma=SIGMA)                              # no seed
    with pytest.raises(TypeError):
        m.infer_window(mel, 0, 32, sigma=SIGMA, seed=SEED, noise=None)       # there is no noise=
    with pytest.raises(T2SError):
        m.infer_window(mel[:, :, :100], 0, 32, sigma=SIGMA, seed=SEED)       # 32 + 96 > 100 frames known, not final
    with pytest.raises(T2SError):
        m.infer_window(mel, 40, 40, sigma=SIGMA, seed=SEED)
    with pytest.raises(T2SError):
        m.infer_window(mel, 250, 261, sigma=SIGMA, seed=SEED, final=True)
    with pytest.raises(T2SError):
        m.infer_window(mel.cpu(), 0, 32, sigma=SIGMA, seed=SEED)
    # out / out_offset: the samples land in the caller's row, off any 16-byte boundary, and nothing else is written
    out = torch.full((1, 256 * 8 + 7), 7.0, device=DEV)
    got = m.infer_window(mel, 110, 118, sigma=SIGMA, seed=SEED, out=out, out_offset=3)
    own = m.infer_window(mel, 110, 118, sigma=SIGMA, seed=SEED)
    assert got.data_ptr() == out.data_ptr() + 12 and torch.equal(got, own)
    assert bool((out[:, :3] == 7.0).all()) and bool((out[:, 3 + 2048:] == 7.0).all())
    with pytest.raises(T2SError):
        m.infer_window(mel, 110, 118, sigma=SIGMA, seed=SEED, out=out, out_offset=8)


def test_infer_window_batch_of_two_seeds(case):
    m = case["m"]
    mel2 = torch.cat([case["mel"], case["mel"].flip(2)], 0).contiguous()
    whole = m.infer(mel2, sigma=SIGMA, seed=[SEED, SEED2])
    for f0, f1 in R.WINDOWS:
        got = m.infer_window(mel2, f0, f1, sigma=SIGMA, seed=[SEED, SEED2], final=_final(f1))
        assert tuple(got.shape) == (2, 256 * (f1 - f0))
        e = [R.rel(got[b], whole[b, 256 * f0:256 * f1]) for b in range(2)]
        eo = R.rel(got[0], case["want"][256 * f0:256 * f1])
        print("infer_window B = 2 [%d, %d): vs infer(seed=[..]) rel %s, bit-equal %s; entry 0 vs oracle rel %.2e"
              % (f0, f1, ["%.2e" % x for x in e], bool(torch.equal(got, whole[:, 256 * f0:256 * f1])), eo))
        assert max(e) < R.SOLO_BAR and eo < R.ORACLE_BAR
    assert R.rel(whole[0], case["whole"][0]) < R.SOLO_BAR           # entry 0 is the solo utterance under its seed


def test_infer_window_half_model(case):
    """a .half() copy takes infer's fp16 chain for its windows too"""
    m = _waveglow(case["sd"], half=True)
    whole = m.infer(case["mel"], sigma=SIGMA, seed=SEED)
    assert m._eng().last_infer_w16 is True
    for f0, f1 in R.WINDOWS:
        got = m.infer_window(case["mel"], f0, f1, sigma=SIGMA, seed=SEED, final=_final(f1))
        assert m._eng().last_infer_w16 is True
        e = R.rel(got[0], whole[0, 256 * f0:256 * f1])
        print("infer_window .half() [%d, %d): vs infer(seed=) rel %.2e, bit-equal %s" % (f0, f1, e, bool(torch.equal(got[0], whole[0, 256 * f0:256 * f1]))))
        assert e < R.SOLO_BAR


def _pieces(mel, n=64):
    Fm = mel.size(2)
    return [(mel[:, :, a:min(Fm, a + n)], a + n >= Fm) for a in range(0, Fm, n)]


@pytest.mark.parametrize("frames,first,window", [(1, 32, 128), (33, 32, 128), (260, 32, 128), (260, 8, 16)])
def test_infer_stream(case, monkeypatch, frames, first, window):
    m, eng = case["m"], case["m"]._eng()
    mel = case["mel"][:, :, :frames].contiguous()
    want = m.infer(mel, sigma=SIGMA, seed=SEED)
    lens = torch.tensor([12, 7])
    mel_b = case["mel"][:, :, :12].repeat(2, 1, 1).contiguous()
    want_b, _ = m.infer_batch(mel_b, lens, sigma=SIGMA, seeds=[SEED, SEED2])

    seen = collections.Counter()
    real_call = _lib.call

    def counting_call(name, *args):
        seen[name] += 1
        return real_call(name, *args)
    monkeypatch.setattr(_lib, "call", counting_call)

    out, between = [], None
    for i, a in enumerate(m.infer_stream(_pieces(mel), sigma=SIGMA, seed=SEED, first_frames=first, window_frames=window)):
        out.append(a)
        if i == 0:      # another call between two windows: its own workspace shape, and the stream's stay what they were
            between, _ = m.infer_batch(mel_b, lens, sigma=SIGMA, seeds=[SEED, SEED2])
    n_windows = len(out)
    got = torch.cat(out, 1)
    packs = {k: v for k, v in seen.items() if "pack" in k or "endfold_weights" in k or "startfold" in k}
    monkeypatch.setattr(_lib, "call", real_call)
    e = R.rel(got[0], want[0])
    print("infer_stream F = %d (first %d, window %d): %d windows, vs infer rel %.2e, bit-equal %s; pack launches %r; noise_at %d, audio_window %d"
          % (frames, first, window, n_windows, e, bool(torch.equal(got, want)), packs, seen["t2s_wg_noise_keyed_at"], seen["t2s_wg_audio_window"]))
    assert tuple(got.shape) == (1, 256 * frames)
    assert e < R.SOLO_BAR
    assert not packs, "a window repacked the weights"
    assert seen["t2s_wg_noise_keyed_at"] == seen["t2s_wg_audio_window"] == n_windows
    assert torch.equal(between, want_b), "infer_batch between two windows"
    again = torch.cat(list(m.infer_stream(_pieces(mel), sigma=SIGMA, seed=SEED, first_frames=first, window_frames=window)), 1)
    assert torch.equal(again, got), "a second stream is not bit-equal to the first"
    assert torch.equal(m.infer(mel, sigma=SIGMA, seed=SEED), want), "infer after the stream"
    assert len(eng.ws) == 1, "the engine keeps one shape resident, as before"


def test_infer_stream_arguments(case):
    m, mel = case["m"], case["mel"]
    with pytest.raises(_lib.T2SError):
        m.infer_stream(_pieces(mel), sigma=SIGMA)                    # a seed is required, and said before the first piece
    with pytest.raises(_lib.T2SError):
        list(m.infer_stream([(mel[:, :, :64], False)], sigma=SIGMA, seed=SEED))         # no piece flagged last


# ---------------------------------------------------------------------------------------------------------------- Tacotron
N_STEPS = 150       # max_decoder_steps of these tests: chunks of 64 end at 64, 128 and 150


def _set_decoder(model, thr, n):
    model.decoder.gate_threshold, model.decoder.max_decoder_steps = thr, n


def _pick_stop(model, margin=1e-4):
    """(ids, threshold, stop step): the way tests/test_batch_inference_gpu.py makes the stop fire - a threshold picked from the
    sigmoid(gate) trajectory of a run that never stops, half-way between a step's value and the largest one before it and more
    than `margin` away from both, so the run stops at that step and at none before.  The synthetic weights' trajectories mostly
    fall, so a dozen texts of different lengths are tried and the step nearest to 100 is taken: a stop inside a later chunk where
    one can be had."""
    best = None
    for k in range(12):
        ids = torch.randint(2, 80, (1, 9 + 7 * k), generator=torch.Generator().manual_seed(11 + k)).to(DEV)
        p = torch.sigmoid(model.inference(ids, None, seed=SEED)[2][0, :, 0].double().cpu())
        run_max = float(p[0])
        for s in range(1, p.numel()):
            v = float(p[s])
            if v - run_max > 2 * margin and (best is None or abs(s - 100) < abs(best[2] - 100)):
                best = (ids, 0.5 * (v + run_max), s)
            run_max = max(run_max, v)
    assert best is not None, "no step of any gate trajectory exceeds all before it"
    return best


@pytest.fixture(scope="module")
def taco():
    """the model, and a text with the gate threshold at which it stops at a known step: picked once"""
    assert torch.cuda.is_available()
    _lib.load()
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    m = m.to(DEV).eval()
    try:
        _set_decoder(m, 2.0, N_STEPS)
        ids, thr, stop = _pick_stop(m)
    finally:
        _set_decoder(m, HP["gate_threshold"], HP["max_decoder_steps"])
    print("stop case: %d symbols, gate threshold %.6f, stop step %d" % (ids.size(1), thr, stop))
    return dict(m=m, ids=ids, thr=thr, stop=stop)


def _cat_stream(pieces):
    assert [p[4] for p in pieces] == [False] * (len(pieces) - 1) + [True]
    return [torch.cat([p[i] for p in pieces], 2 if i < 2 else 1) for i in range(4)]


@pytest.mark.parametrize("stop", [True, False])
@pytest.mark.parametrize("chunk", [16, 64])
def test_inference_stream_equals_inference(taco, capfd, stop, chunk):
    model, ids = taco["m"], taco["ids"]
    try:
        thr, s = (taco["thr"], taco["stop"]) if stop else (2.0, N_STEPS - 1)
        _set_decoder(model, thr, N_STEPS)
        capfd.readouterr()
        want = model.inference(ids, None, seed=SEED)
        warn_want = "Reached max decoder steps" in capfd.readouterr().err
        pieces = list(model.inference_stream(ids, None, seed=SEED, chunk=chunk))
        warn_got = "Reached max decoder steps" in capfd.readouterr().err
    finally:
        _set_decoder(model, HP["gate_threshold"], HP["max_decoder_steps"])
    model._eng().check_lstm_xbuf()
    got = _cat_stream(pieces)
    n = want[0].size(2)
    e_post = R.rel(got[1], want[1])
    print("inference_stream chunk %d, %s: %d frames in %d pieces (threshold %.6f); mel_post rel %.2e, bit-equal %s"
          % (chunk, "stop" if stop else "no stop", n, len(pieces), thr, e_post, bool(torch.equal(got[1], want[1]))))
    assert n == s + 1 and warn_want == (not stop) and warn_got == warn_want
    for name, g, w in zip(("mel", "mel_post", "gate", "align"), got, want):
        assert tuple(g.shape) == tuple(w.shape), name
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert e_post < 1e-4                    # the batch-against-solo bar of tests/test_batch_inference_gpu.py
    # mel_post lags mel by the postnet's reach, 10 frames, until the last piece
    lag = [sum(p[0].size(2) for p in pieces[:i + 1]) - sum(p[1].size(2) for p in pieces[:i + 1]) for i in range(len(pieces))]
    assert lag[-1] == 0 and all(x == 10 for x in lag[:-1]), lag


def test_inference_stream_arguments(taco):
    model, ids = taco["m"], taco["ids"]
    with pytest.raises(_lib.T2SError):
        model.inference_stream(ids.repeat(2, 1), None, seed=SEED)            # B = 1
    with pytest.raises(ValueError):
        model.inference_stream(ids, None, seed=-1)
    model.train()
    try:
        with pytest.raises(_lib.T2SError):
            model.inference_stream(ids, None, seed=SEED)
    finally:
        model.eval()


# ---------------------------------------------------------------------------------------------------------------- the chain
@pytest.fixture(scope="module")
def chain(taco, case):
    """the streamed mel_post pieces of one text that stops inside a later chunk, and infer_stream's audio of them"""
    model, ids = taco["m"], taco["ids"]
    thr, s = taco["thr"], taco["stop"]
    try:
        _set_decoder(model, thr, N_STEPS)
        pieces = [(p[1], p[4]) for p in model.inference_stream(ids, None, seed=SEED)]
    finally:
        _set_decoder(model, HP["gate_threshold"], HP["max_decoder_steps"])
    return dict(thr=thr, frames=s + 1, pieces=pieces)


def _synth(taco, case, chain, **kw):
    model, ids = taco["m"], taco["ids"]
    try:
        _set_decoder(model, chain["thr"], N_STEPS)
        return list(streaming.synthesize_stream(model, case["m"], ids, seed=SEED, sigma=SIGMA, **kw))
    finally:
        _set_decoder(model, HP["gate_threshold"], HP["max_decoder_steps"])


def test_synthesize_stream_is_its_parts(taco, case, chain):
    kw = dict(first_frames=16, window_frames=32, halo=(24, 24))
    want = list(case["m"].infer_stream(chain["pieces"], sigma=SIGMA, seed=SEED, **kw))
    got = _synth(taco, case, chain, **kw)
    print("synthesize_stream: %d frames, %d audio pieces of %s samples" % (chain["frames"], len(got), [int(a.size(1)) for a in got]))
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert sum(a.size(1) for a in got) == 256 * chain["frames"]
    from text2speech_amd import audio as A
    pcm = _synth(taco, case, chain, pcm16=True, **kw)
    assert all(p.dtype == torch.int16 and torch.equal(p, A.to_pcm16(a)) for p, a in zip(pcm, got)) and len(pcm) == len(got)


def test_synthesize_stream_with_denoiser(taco, case, chain):
    from text2speech_amd.audio import Denoiser
    den = Denoiser(case["m"])
    kw = dict(first_frames=16, window_frames=32)
    plain = torch.cat(list(case["m"].infer_stream(chain["pieces"], sigma=SIGMA, seed=SEED, **kw)), 1)
    want = den(plain, 0.1)[:, 0]
    got = torch.cat(_synth(taco, case, chain, denoiser=den, strength=0.1, **kw), 1)
    e = R.rel(got, want)
    print("synthesize_stream with a Denoiser: %d samples, vs Denoiser.forward of the whole streamed audio rel %.2e, bit-equal %s"
          % (got.size(1), e, bool(torch.equal(got, want))))
    assert tuple(got.shape) == tuple(want.shape) == (1, 256 * chain["frames"])
    assert e < R.SOLO_BAR


def test_synthesize_stream_arguments(taco, case):
    model, ids = taco["m"], taco["ids"]
    with pytest.raises(_lib.T2SError):
        streaming.synthesize_stream(model, case["m"], ids)                   # a seed is required
    model.train()
    try:
        with pytest.raises(_lib.T2SError):
            streaming.synthesize_stream(model, case["m"], ids, seed=SEED)
    finally:
        model.eval()
