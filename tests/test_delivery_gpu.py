"""audio.DeliveryStream, to_ulaw / to_alaw and streaming.synthesize_stream(delivery=) on the device.

The invariant is equality of bits: whatever the piece lengths, the concatenation of what push() returns is
enc(limiter.limit_batch(Resampler(src, out).forward(whole), gain=gain)[0]) computed by the whole-row calls, and report() after the
last push is limiter.true_peak_batch's of the resampled row.  No stored sample exceeds the ceiling and no int16 code
trunc(32768 ceiling).  synthesize_stream(delivery=) on the small models of tests/test_streaming_gpu.py gives the chain applied to
the plain stream's concatenation; delivery=None issues the launches the call issued before."""
import numpy as np
import pytest
import torch

import delivery_ref as D
import stream_util as SU
import streaming_ref as R
from text2speech_amd import _lib, audio, streaming, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SRC = 44800
RATES = (48000, 16000, 8000, 44800)
N = 6200
ENC = {"f32": lambda x: x, "pcm16": audio.to_pcm16, "ulaw": audio.to_ulaw, "alaw": audio.to_alaw}
DTYPE = {"f32": torch.float32, "pcm16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


def _rows(B, n, seed, dtype=torch.float32):
    x = np.stack([D.row(n, seed + b, peaks=(0, 3, 700, 1024, 2047, 2048, 3000, n - 2, n - 1)) for b in range(B)])
    return torch.from_numpy(x).to(DEV).to(dtype)


def _cuts(n, C):
    cuts = []
    for c in D.piece_cycle(C):
        cuts.append(min(c, n - sum(cuts)))
    return cuts + [n - sum(cuts)]


def _whole(x, rate, limiter, gain, encoding):
    y = audio.Resampler(SRC, rate, device=DEV).forward(x) if rate != SRC else x
    if limiter is not None:
        g = torch.full((x.size(0),), float(gain), dtype=torch.float64, device=DEV) if isinstance(gain, float) else gain
        y = limiter.limit_batch(y, gain=g)[0]
    return ENC[encoding](y)


def _stream(ds, x, cuts, flush=False):
    outs, pos, total = [], 0, x.size(1)
    for q, c in enumerate(cuts):
        last = q == len(cuts) - 1 and not flush
        outs.append(ds.push(x[:, pos:pos + c], last))
        pos += c
        owed = -(-pos * ds.up // ds.down) - ds.delivered
        assert 0 <= owed <= ds.latency and (not last or owed == 0), "a push holds back at most `latency` delivery samples"
    if flush:
        outs.append(ds.push(x[:, total:], True))
    assert pos == total and ds.delivered == sum(o.size(1) for o in outs) == -(-total * ds.up // ds.down)
    return outs


@pytest.mark.parametrize("encoding", audio.DELIVERY_ENCODINGS)
@pytest.mark.parametrize("rate", RATES)
def test_the_stream_is_the_whole_chain(rate, encoding):
    B = 2
    limiter = audio.Limiter(rate, device=DEV)
    gain = 4.0 if rate in (48000, 8000) else torch.tensor([3.0, 5.0], dtype=torch.float64).to(DEV)       # (downsampling takes the peaks' tops off)
    half = rate == 16000 and encoding in ("f32", "ulaw")
    x = _rows(B, N, rate // 1000 + len(encoding), torch.float16 if half else torch.float32)
    want = _whole(x, rate, limiter, gain, encoding)
    ds = audio.DeliveryStream(SRC, rate, limiter=limiter, gain=gain, encoding=encoding)
    C = ds.resample_carry if rate != SRC else ds.limit_carry
    outs = _stream(ds, x, _cuts(N, C), flush=encoding == "pcm16")
    assert all(o.dtype == DTYPE[encoding] and o.size(0) == B and o.is_cuda for o in outs) and any(o.size(1) == 0 for o in outs)
    got = torch.cat(outs, 1)
    assert got.shape == want.shape and torch.equal(got, want)
    c = limiter.ceiling
    if encoding == "f32":
        assert float(got.abs().max()) <= c
    elif encoding == "pcm16":
        assert int(got.to(torch.int32).abs().max()) <= int(32768 * c)
    # the running state is the whole row's report
    y = audio.Resampler(SRC, rate, device=DEV).forward(x) if rate != SRC else x
    g = torch.full((B,), gain, dtype=torch.float64, device=DEV) if isinstance(gain, float) else gain
    rep, run = limiter.true_peak_batch(y, gain=g), ds.report()
    for a, b in zip(run, rep):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert bool((run.limited > 0).all()) and run.flags.tolist() == [audio.LIMIT_FLAG_LIMITED] * B
    with pytest.raises(_lib.T2SError, match="behind the one flagged last"):
        ds.push(x[:, :5])


@pytest.mark.parametrize("rate,encoding", [(8000, "ulaw"), (48000, "pcm16"), (16000, "f32"), (44800, "alaw")])
def test_a_stream_without_a_limiter(rate, encoding):
    x = _rows(3, 3000, 5, torch.float16 if rate == 16000 else torch.float32)
    x = x * 0.5 if rate == 16000 else x
    want = _whole(x, rate, None, None, encoding)
    ds = audio.DeliveryStream(SRC, rate, encoding=encoding)
    got = torch.cat(_stream(ds, x, _cuts(3000, max(ds.resample_carry, 9)), flush=True), 1)
    assert torch.equal(got, want) and got.dtype == DTYPE[encoding]
    with pytest.raises(_lib.T2SError, match="no limiter"):
        ds.report()


def test_one_sample_pushes_and_a_strided_piece():
    limiter = audio.Limiter(16000, lookahead_ms=0.5, device=DEV)
    wide = _rows(2, 2 * 400 + 1, 77)
    x = wide[:, 1::2]                                           # stride 2 inside a row: packed by the stream
    want = _whole(x.contiguous(), 16000, limiter, 2.0, "pcm16")
    ds = audio.DeliveryStream(SRC, 16000, limiter=limiter, gain=2.0, encoding="pcm16")
    outs = [ds.push(x[:, i:i + 1], i == 399) for i in range(400)]
    assert torch.equal(torch.cat(outs, 1), want)
    ds = audio.DeliveryStream(SRC, 16000, limiter=limiter, gain=2.0, encoding="pcm16")
    assert torch.equal(ds.push(x, True), want)
    ds = audio.DeliveryStream(SRC, 16000, limiter=limiter, gain=2.0, encoding="pcm16").open(2, "cuda")     # (no index: the current device)
    assert torch.equal(ds.push(x, True), want)
    with pytest.raises(_lib.T2SError, match="opened for 2 rows"):
        audio.DeliveryStream(SRC, 16000).open(2, DEV).push(x[:1])


def test_the_encoders():
    codes = np.arange(-32768, 32768, dtype=np.int64)
    x = torch.from_numpy((codes / 32768.0).astype(np.float32)).to(DEV).view(4, -1)
    assert torch.equal(audio.to_pcm16(x).view(-1).cpu(), torch.from_numpy(codes.astype(np.int16)))
    for f, ref in ((audio.to_ulaw, D.ulaw), (audio.to_alaw, D.alaw)):
        got = f(x)
        assert got.dtype == torch.uint8 and got.shape == x.shape
        assert got.view(-1).cpu().numpy().tobytes() == ref(codes.astype(np.int16)).tobytes()
    y = torch.from_numpy(D.row(1001, 4)).to(DEV) * 1.4
    for name in ("pcm16", "ulaw", "alaw"):
        assert ENC[name](y).cpu().numpy().tobytes() == D.ENCODERS[name](y.cpu().numpy()).tobytes()
    lens = [5, 0, 16384, 7]
    got = audio.to_ulaw(x, lens)
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n], audio.to_ulaw(x)[b, :n]) and bool((got[b, n:] == 0xFF).all()), "silence behind a row's end"


def test_a_sample_that_is_not_finite_mutes():
    limiter = audio.Limiter(SRC, device=DEV)
    x = _rows(2, 3000, 21)
    x[1, 1500] = float("nan")
    ds = audio.DeliveryStream(SRC, limiter=limiter)
    got = torch.cat(_stream(ds, x, [1000, 600, 1400]), 1)
    rep = ds.report()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= limiter.ceiling and float(got[1, 1500]) == 0.0
    assert rep.flags.tolist() == [audio.LIMIT_FLAG_LIMITED, audio.LIMIT_FLAG_LIMITED | audio.LIMIT_FLAG_NONFINITE]
    assert torch.equal(got[0], limiter.limit_batch(x[:1])[0][0]), "the row next to it is untouched by that"
    reach = limiter.reach
    clean = x.clone()
    clean[1, 1500] = 0
    want = limiter.limit_batch(clean)[0]
    assert torch.equal(got[1, :1500 - reach], want[1, :1500 - reach]) and torch.equal(got[1, 1501 + reach:], want[1, 1501 + reach:])


def _one_stream(x, rate=8000, encoding="ulaw", opened=True):
    limiter = audio.Limiter(rate, device=DEV)
    ds = audio.DeliveryStream(SRC, rate, limiter=limiter, gain=4.0, encoding=encoding)
    if opened:
        ds.open(x.size(0), DEV)
    return ds


def test_nothing_is_read_back():
    x = _rows(2, 5000, 31)
    cuts = [0, 1, 1023, 2000, 1976]
    want = _whole(x, 8000, audio.Limiter(8000, device=DEV), 4.0, "ulaw")
    torch.cat(_stream(_one_stream(x), x, cuts), 1)        # (warm: the first calls load the kernels and upload the tables)
    ds = _one_stream(x)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = _stream(ds, x, cuts)
        rep = ds.report()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(torch.cat(outs, 1), want) and bool((rep.limited > 0).all())


def test_on_a_callers_stream():
    """the pieces become true only behind a gate on the stream S the pushes are made on, and a consumer on
    S reads what they return"""
    true = _rows(2, 5000, 41)
    cuts = [1500, 0, 2000, 1500]
    want = _whole(true, 48000, audio.Limiter(48000, device=DEV), 4.0, "pcm16")
    buf = torch.zeros_like(true)
    S = torch.cuda.Stream(DEV)
    with torch.cuda.stream(S):
        warm = _one_stream(buf, 48000, "pcm16")
        _, ms = SU.timed(lambda: _stream(warm, buf, cuts))
        ds = _one_stream(buf, 48000, "pcm16")                   # (opened in front of the gate: the tables' upload blocks)
    n = SU.gate_matmuls(ms, DEV)
    torch.cuda.synchronize()
    gate = SU.behind_gate(S, buf, true, n)
    with torch.cuda.stream(S):
        seen = torch.cat(_stream(ds, buf, cuts), 1).clone()
    gate.check()
    SU.log("DeliveryStream.push", ms, n)
    torch.cuda.synchronize()
    assert torch.equal(seen, want)


# ---- synthesize_stream(delivery=) -------------------------------------------------------------------------------------------------------
N_STEPS = 150
HP = synth.TACOTRON_HPARAMS
SEED = 20240611
KW = dict(first_frames=16, window_frames=32, halo=(24, 24))


def _waveglow(sd, half=False):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**R.CFG)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    if half:
        m.half()
        for c in m.convinv:
            c.float()
    return m


@pytest.fixture(scope="module")
def models():
    """the small models of tests/test_streaming_gpu.py; the decoder runs to max_decoder_steps = 150 frames"""
    from text2speech_amd.tacotron import Tacotron
    taco = Tacotron(HP, 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state(), strict=True)
    taco = taco.to(DEV).eval()
    sd = synth.waveglow_state(R.CFG, **R.STRESS)
    ids = torch.randint(2, 80, (1, 23), generator=torch.Generator().manual_seed(11)).to(DEV)
    return dict(taco=taco, wg=_waveglow(sd), wg16=_waveglow(sd, half=True), ids=ids)


def _synth(models, wg="wg", **kw):
    taco = models["taco"]
    taco.decoder.gate_threshold, taco.decoder.max_decoder_steps = 2.0, N_STEPS
    try:
        args = dict(KW)
        args.update(kw)
        return list(streaming.synthesize_stream(taco, models[wg], models["ids"], seed=SEED, sigma=R.SIGMA, **args))
    finally:
        taco.decoder.gate_threshold, taco.decoder.max_decoder_steps = HP["gate_threshold"], HP["max_decoder_steps"]


@pytest.mark.parametrize("wg,denoise,rate,encoding", [("wg", False, 8000, "ulaw"), ("wg", True, 48000, "pcm16"), ("wg16", False, 16000, "f32"),
                                                      ("wg", True, 44800, "alaw")])
def test_synthesize_stream_with_delivery(models, capfd, wg, denoise, rate, encoding):
    den = audio.Denoiser(models[wg]) if denoise else None
    kw = dict(denoiser=den, strength=0.1) if denoise else {}
    plain = torch.cat(_synth(models, wg, **kw), 1)
    assert plain.size(1) == 256 * N_STEPS
    peak = float(_whole(plain, rate, None, None, "f32").float().abs().max())
    limiter = audio.Limiter(rate, device=DEV)
    gain = 1.5 * limiter.ceiling / peak                         # the caller's number: the tallest delivered sample goes over the ceiling
    made = []

    def make():
        made.append(audio.DeliveryStream(SRC, rate, limiter=limiter, gain=gain, encoding=encoding))
        return made[-1]
    got = _synth(models, wg, delivery=make if denoise else make(), **kw)
    capfd.readouterr()
    want = _whole(plain, rate, limiter, gain, encoding)
    assert len(made) == 1 and all(o.size(1) > 0 and o.dtype == DTYPE[encoding] for o in got) and len(got) > 2
    assert torch.equal(torch.cat(got, 1), want)
    rep = made[0].report()
    print("synthesize_stream(delivery=) %s -> %d Hz %s: %d pieces of %s samples; %d samples limited, min gain %.4f"
          % (plain.dtype, rate, encoding, len(got), [int(o.size(1)) for o in got], int(rep.limited[0]), float(rep.min_gain[0])))
    assert int(rep.limited[0]) > 0 and made[0].delivered == want.size(1)
    if encoding == "pcm16":
        assert int(want.to(torch.int32).abs().max()) <= int(32768 * limiter.ceiling)
    if encoding == "f32":
        assert float(want.abs().max()) <= limiter.ceiling


def test_delivery_none_issues_the_launches_it_issued_before(models, monkeypatch, capfd):
    names, real = [], _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    _synth(models)                                              # (warm: the first call packs the vocoder's weights)
    monkeypatch.setattr(_lib, "call", call)
    plain = _synth(models)
    n_plain = list(names)
    del names[:]
    none = _synth(models, delivery=None)
    n_none = list(names)
    del names[:]
    ds = audio.DeliveryStream(SRC, 8000, limiter=audio.Limiter(8000, device=DEV), encoding="ulaw")
    with_d = _synth(models, delivery=ds)
    n_with = list(names)
    capfd.readouterr()
    own = ("t2s_resample_window", "t2s_limit_window", "t2s_pcm16", "t2s_g711")
    assert n_plain and n_none == n_plain and all(torch.equal(a, b) for a, b in zip(none, plain))
    assert not any(n in own for n in n_plain) and [n for n in n_with if n not in own] == n_plain
    assert n_with.count("t2s_resample_window") == n_with.count("t2s_limit_window") == len(plain)
    assert n_with.count("t2s_g711") == len(with_d) <= len(plain)
    with pytest.raises(_lib.T2SError, match="exclude each other"):
        _synth(models, delivery=audio.DeliveryStream(SRC, 8000), pcm16=True)
