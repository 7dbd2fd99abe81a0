"""audio.SosFilter / FilterStream, PcmPool.filter, DeliveryStream(pre_filter=, post_filter=), synthesize_stream(delivery=) with
filters and longform.filter_long on the device.

The invariant is equality of bits: an entry of a batch is its own forward(); the pieces of a stream are the whole row; a
DeliveryStream's concatenated pushes are

    enc(limiter.limit_batch(post.forward(Resampler(src, out).forward(pre.forward(whole))), gain=gain)[0])

computed by the whole-row calls.  Against scipy the device is held to the bar of tests/test_filter_kernels_gpu.py (E measured on the
CPU, tests/filter_ref.py).  A stream built without filters issues the launches it issued before."""
import random

import numpy as np
import pytest
import torch

import delivery_ref as D
import filter_ref as R
import stream_util as SU
import streaming_ref as SR
from text2speech_amd import _lib, audio, data, longform as L, streaming, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SRC = 44800
T = R.TILE
ENC = {"f32": lambda x: x, "pcm16": audio.to_pcm16, "ulaw": audio.to_ulaw, "alaw": audio.to_alaw}


def _filt(case, rate=None):
    return audio.SosFilter(R.BIT_CASES[case], rate, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _rows(B, n, seed, dtype=torch.float32):
    x = np.stack([D.row(n, seed + b, peaks=(0, 3, 700, 1024, 2047, 2048, 3000, n - 2, n - 1)) for b in range(B)])
    return torch.from_numpy(x).to(DEV).to(dtype)


# ---- SosFilter / FilterStream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("f32", "f16"))
def test_filter_batch_is_every_entrys_forward(dtype):
    f = _filt("telephone_300_3400_o4_8000", 8000)
    lens = [2 * T + 777, 0, T, 333]
    N = max(lens)
    wide = torch.full((4, N + 7), float("nan"), dtype=dtype, device=DEV)
    rows = _rows(4, N, 5, dtype)
    x = wide[:, :N]                                             # strided rows, NaN behind every length
    for b, n in enumerate(lens):
        x[b, :n] = rows[b, :n]
    gain = torch.tensor([1.0, 1.0, 0.5, 32768.0], dtype=torch.float64, device=DEV)
    for g in (None, gain):
        out, rep = f.filter_batch(x, lens, g)
        assert out.shape == x.shape and out.dtype == torch.float32
        assert rep.nonfinite.tolist() == [0] * 4 and rep.clipped.tolist() == [0] * 4
        for b, n in enumerate(lens):
            assert not bool(out[b, n:].view(torch.int32).any()), "+0 behind the length"
            if n:
                solo, _ = f.filter_batch(rows[b, :n].clone(), None, None if g is None else g[b:b + 1])
                assert torch.equal(_bits(out[b, :n]), _bits(solo))
                if g is None:
                    assert torch.equal(_bits(f.forward(rows[b, :n].clone())), _bits(solo)) and torch.equal(_bits(f(rows[b:b + 1, :n])[0]), _bits(solo))
    assert torch.equal(_bits(f.filter_batch(x, lens, 0.5)[0][2]), _bits(f.filter_batch(x, lens, gain)[0][2]))
    # against scipy, under the kernel tests' bar
    xr = rows[0].cpu().numpy()
    sos = R.BIT_CASES["telephone_300_3400_o4_8000"]
    ref, _ = R.sequential(sos, xr)
    par, _ = R.parallel(sos, f.table(), xr)
    term = R.second_term(float(np.max(np.abs(par - ref))), R.impulse_l1(sos), float(np.max(np.abs(xr.astype(np.float64)))))
    got = f.filter_batch(x, lens)[0][0].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref) <= R.bar(ref, 0.0, 0.0, 0.0) + term)
    bad = rows[:1].clone()
    bad[0, [3, T, T + 1]] = float("inf")
    out, rep = f.filter_batch(bad)
    assert rep.nonfinite.tolist() == [3] and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("case", ("deemphasis_0.97", "highpass_5_o2_48000", "lowpass_3400_o8_44800"))
def test_filter_stream_is_forward(case):
    f = _filt(case)
    for B, n, dtype in ((2, 2 * T + 777, torch.float32), (1, T + 9, torch.float16)):
        x = _rows(B, n, 17, dtype)
        x[0, n // 2] = float("nan")
        want, rep = f.filter_batch(x)
        for name, cuts in R.cut_patterns(n, seed=3).items():
            st, at, outs = f.stream(), 0, []
            for q, c in enumerate(cuts):
                wide = torch.zeros(B, c + 3, dtype=dtype, device=DEV)
                wide[:, :c] = x[:, at:at + c]
                outs.append(st.push(wide[:, :c], last=q == len(cuts) - 1))
                at += c
                assert outs[-1].shape == (B, c) and outs[-1].dtype == torch.float32
            assert torch.equal(_bits(torch.cat(outs, 1)), _bits(want)), (case, name)
            assert torch.equal(st.report().nonfinite, rep.nonfinite) and st.position == n
            with pytest.raises(_lib.T2SError, match="flagged last"):
                st.push(x[:, :1])


# ---- PcmPool.filter -----------------------------------------------------------------------------------------------------------------
def test_pool_filter_and_training_batches_on_it():
    fs = 22050
    gen = np.random.RandomState(5)
    lens = [150, 400, 401, 1000, T + 1, 2 * T + 777]
    clips = [np.clip(4.0 * np.rint(1200.0 * gen.randn(n)), -32768, 32764).astype(np.int16) for n in lens]
    pool = data.PcmPool(clips, fs, DEV)
    sos = audio.sos_butter(4, 80.0, "highpass", fs)
    f = audio.SosFilter(sos, fs, device=DEV)
    out = pool.filter(f)
    assert out is not pool and out.pcm.dtype == torch.int16 and out.sampling_rate == fs
    assert torch.equal(out.lengths, pool.lengths) and torch.equal(out.offsets, pool.offsets)
    assert out.nonfinite.tolist() == [0] * len(lens)
    host, pcm = [], out.pcm.cpu().numpy()
    tab = f.table()
    for i, c in enumerate(clips):
        ref, _ = R.sequential(sos, c)
        par, _ = R.parallel(sos, tab, c)
        term = R.second_term(float(np.max(np.abs(par - ref))), R.impulse_l1(sos), float(np.max(np.abs(c.astype(np.float64)))))
        want, clipped = R.round16(ref)
        got = pcm[int(pool.offsets[i]):int(pool.offsets[i]) + lens[i]]
        diff = got.astype(np.int64) - want.astype(np.int64)
        exempt = R.int16_exempt(ref, term)
        assert np.all(diff[~exempt] == 0) and np.all(np.abs(diff) <= 1) and float(np.mean(exempt)) <= 1e-3, i
        assert int(out.clipped[i]) == clipped
        host.append(got.copy())
    # a clip's bits do not depend on its place in the pool
    back = data.PcmPool(clips[::-1], fs, DEV).filter(f)
    for i in range(len(lens)):
        j = len(lens) - 1 - i
        assert torch.equal(back.pcm[int(back.offsets[j]):int(back.offsets[j]) + lens[i]], out.pcm[int(out.offsets[i]):int(out.offsets[i]) + lens[i]])
    # training batches built on the filtered pool are those built on a pool of the same clips uploaded from the host
    stft = dict(filter_length=64, hop_length=16, win_length=64, sampling_rate=fs, mel_fmin=0.0, mel_fmax=8000.0)
    idx = [3, 0, 5, 4, 1]
    a = data.Mel2SampBatch(out, 400, rng=random.Random(7), n_mel_channels=8, **stft)(idx)
    b = data.Mel2SampBatch(data.PcmPool(host, fs, DEV), 400, rng=random.Random(7), n_mel_channels=8, **stft)(idx)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[0]).all())
    with pytest.raises(_lib.T2SError, match="designed for"):
        pool.filter(audio.SosFilter(sos, 8000, device=DEV))
    with pytest.raises(_lib.T2SError, match="SosFilter"):
        pool.filter(sos)


# ---- DeliveryStream -------------------------------------------------------------------------------------------------------------------
def _whole(x, rate, pre, post, limiter, gain, encoding):
    y = x if pre is None else pre.forward(x)
    y = audio.Resampler(SRC, rate, device=DEV).forward(y) if rate != SRC else y
    y = y if post is None else post.forward(y)
    if limiter is not None:
        g = None if gain is None else torch.full((x.size(0),), float(gain), dtype=torch.float64, device=DEV)
        y = limiter.limit_batch(y, gain=g)[0]
    return ENC[encoding](y)


def _push_all(ds, x, cuts):
    outs, pos = [], 0
    for q, c in enumerate(cuts):
        outs.append(ds.push(x[:, pos:pos + c], q == len(cuts) - 1))
        pos += c
    assert pos == x.size(1)
    return torch.cat(outs, 1)


def _setups():
    """name -> (out_rate, pre, post, with a limiter, gain, encoding)"""
    return {
        "pre only": (SRC, "deemphasis_0.97", None, False, None, "f32"),
        "post only": (16000, None, "highpass_80_o4_44800", False, None, "pcm16"),
        "both": (48000, "deemphasis_0.97", "peaking_q8_1000_44800", True, 2.0, "f32"),
        "telephone": (8000, None, "telephone_300_3400_o4_8000", True, 3.0, "ulaw"),
        "deemphasis to 48k int16": (48000, "deemphasis_0.97", None, True, 1.5, "pcm16"),
    }


def _make(setup, B=None):
    rate, pre, post, lim, gain, enc = setup
    pre = None if pre is None else _filt(pre, SRC)
    post = None if post is None else _filt(post, rate if post.startswith("telephone") else None)
    limiter = audio.Limiter(rate, device=DEV) if lim else None
    ds = audio.DeliveryStream(SRC, rate, limiter=limiter, gain=gain, encoding=enc, pre_filter=pre, post_filter=post)
    if B is not None:
        ds.open(B, DEV)
    return ds, (rate, pre, post, limiter, gain, enc)


@pytest.mark.parametrize("name", sorted(_setups()))
def test_delivery_stream_with_filters_is_the_whole_chain(name):
    setup = _setups()[name]
    n = 2 * T + 1500
    x = _rows(2, n, 23, torch.float16 if name == "both" else torch.float32)
    ds, parts = _make(setup)
    want = _whole(x, *parts)
    got = _push_all(ds, x, D.cuts_for(n, T))
    assert got.dtype == want.dtype and torch.equal(got, want), name
    # a causal filter holds nothing back: the latency is that of the same stream without filters
    stages = parts[0] != SRC or parts[3] is not None or parts[5] != "f32"
    assert ds.latency == (audio.DeliveryStream(SRC, parts[0], limiter=parts[3], gain=parts[4], encoding=parts[5]).latency if stages else 0)
    pre_rep, post_rep = ds.filter_report()
    assert (pre_rep is None) == (parts[1] is None) and (post_rep is None) == (parts[2] is None)
    for rep in (pre_rep, post_rep):
        assert rep is None or rep.nonfinite.tolist() == [0, 0]
    # other cuts, one sample at a time at the start and an empty final flush: the same bits
    ds2, _ = _make(setup)
    again = _push_all(ds2, x, [1] * 40 + [0, 777, n - 817 - 5000, 5000, 0])
    assert torch.equal(again, want), name


def test_delivery_stream_refusals_and_the_unfiltered_message():
    with pytest.raises(_lib.T2SError) as e:
        audio.DeliveryStream(SRC)
    assert str(e.value) == "DeliveryStream: nothing to do - ask for another rate, a limiter or an encoding"
    assert audio.DeliveryStream(SRC, pre_filter=_filt("deemphasis_0.97")).latency == 0
    with pytest.raises(_lib.T2SError, match="pre_filter was designed for"):
        audio.DeliveryStream(SRC, 8000, pre_filter=_filt("deemphasis_0.97", 8000))
    with pytest.raises(_lib.T2SError, match="post_filter was designed for"):
        audio.DeliveryStream(SRC, 8000, post_filter=_filt("deemphasis_0.97", SRC))
    with pytest.raises(_lib.T2SError, match="post_filter must be an audio.SosFilter"):
        audio.DeliveryStream(SRC, 8000, post_filter=R.BIT_CASES["deemphasis_0.97"])


def test_nothing_is_read_back_and_on_a_callers_stream():
    setup = _setups()["telephone"]
    x = _rows(2, 9000, 31)
    cuts = [0, 1, 1023, 4000, 3976]
    ds, parts = _make(setup, 2)
    want = _whole(x, *parts)
    _push_all(ds, x, cuts)                                      # (warm: the first calls load the kernels and upload the tables)
    ds, _ = _make(setup, 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _push_all(ds, x, cuts)
        ds.filter_report()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, want)
    # the pieces become true only behind a gate on the stream S the pushes are made on
    buf = torch.zeros_like(x)
    S = torch.cuda.Stream(DEV)
    with torch.cuda.stream(S):
        warm, _ = _make(setup, 2)
        _, ms = SU.timed(lambda: _push_all(warm, buf, cuts))
        ds, _ = _make(setup, 2)
    n = SU.gate_matmuls(ms, DEV)
    torch.cuda.synchronize()
    gate = SU.behind_gate(S, buf, x, n)
    with torch.cuda.stream(S):
        seen = _push_all(ds, buf, cuts).clone()
    gate.check()
    SU.log("DeliveryStream.push with filters", ms, n)
    torch.cuda.synchronize()
    assert torch.equal(seen, want)


# ---- synthesize_stream(delivery=) -------------------------------------------------------------------------------------------------------
N_STEPS = 150
HP = synth.TACOTRON_HPARAMS
SEED = 20240611
KW = dict(first_frames=16, window_frames=32, halo=(24, 24))


def _waveglow(sd, half=False):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**SR.CFG)
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
    sd = synth.waveglow_state(SR.CFG, **SR.STRESS)
    ids = torch.randint(2, 80, (1, 23), generator=torch.Generator().manual_seed(11)).to(DEV)
    return dict(taco=taco, wg=_waveglow(sd), wg16=_waveglow(sd, half=True), ids=ids)


def _synth(models, wg="wg", **kw):
    taco = models["taco"]
    taco.decoder.gate_threshold, taco.decoder.max_decoder_steps = 2.0, N_STEPS
    try:
        args = dict(KW)
        args.update(kw)
        return list(streaming.synthesize_stream(taco, models[wg], models["ids"], seed=SEED, sigma=SR.SIGMA, **args))
    finally:
        taco.decoder.gate_threshold, taco.decoder.max_decoder_steps = HP["gate_threshold"], HP["max_decoder_steps"]


@pytest.mark.parametrize("wg,name", [("wg", "telephone"), ("wg16", "deemphasis to 48k int16"), ("wg16", "pre only")])
def test_synthesize_stream_with_filtered_delivery(models, capfd, wg, name):
    plain = torch.cat(_synth(models, wg), 1)
    assert plain.size(1) == 256 * N_STEPS
    ds, parts = _make(_setups()[name])
    got = _synth(models, wg, delivery=ds)
    capfd.readouterr()
    want = _whole(plain, *parts)
    assert len(got) > 2 and torch.equal(torch.cat(got, 1), want)
    assert ds.delivered == want.size(1)


def test_a_stream_without_filters_issues_the_launches_it_issued_before(models, monkeypatch, capfd):
    names, real = [], _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    own = ("t2s_sos_window", "t2s_sos_filter")
    _synth(models)                                              # (warm: the first call packs the vocoder's weights)
    monkeypatch.setattr(_lib, "call", call)
    plain = _synth(models, delivery=audio.DeliveryStream(SRC, 8000, limiter=audio.Limiter(8000, device=DEV), encoding="ulaw"))
    n_plain = list(names)
    del names[:]
    none = _synth(models, delivery=audio.DeliveryStream(SRC, 8000, limiter=audio.Limiter(8000, device=DEV), encoding="ulaw",
                                                        pre_filter=None, post_filter=None))
    n_none = list(names)
    del names[:]
    ds, _ = _make(_setups()["telephone"])
    with_f = _synth(models, delivery=ds)
    n_with = list(names)
    del names[:]
    x = _rows(1, 3000, 3)
    a = audio.DeliveryStream(SRC, 8000, encoding="pcm16")
    a.push(x[:, :1700])
    a.push(x[:, 1700:], True)
    n_push = list(names)
    capfd.readouterr()
    assert n_plain and n_none == n_plain and all(torch.equal(p, q) for p, q in zip(none, plain))
    assert not any(n in own for n in n_plain) and [n for n in n_with if n not in own] == n_plain
    assert 1 <= n_with.count("t2s_sos_window") <= n_with.count("t2s_resample_window") and len(with_f) == len(plain)
    assert n_push == ["t2s_resample_window", "t2s_pcm16"] * 2        # a push without filters: the parent's two calls, nothing else


# ---- longform.filter_long -----------------------------------------------------------------------------------------------------------------
def _same_but_audio(a, b):
    return all(getattr(a, f) is getattr(b, f) for f in a._fields if f != "audio")


def test_filter_long_on_joined_rows():
    gen = torch.Generator().manual_seed(7)
    rows = (torch.randn(3, 9000, generator=gen) * 0.1).to(DEV)
    lens = torch.tensor([9000, 4000, 7777], dtype=torch.int32, device=DEV)
    joined, length, offsets = audio.join_batches([(rows, lens)], pause=80, fade=16)
    f = _filt("highpass_80_o4_44800", SRC)
    for r in (L.LongForm(joined, length, offsets, ["a", "b", "c"], torch.zeros(3, dtype=torch.bool, device=DEV)),
              L.LongFormTimed(joined, length, offsets, ["a", "b", "c"], None, torch.zeros(3, 1, 2, dtype=torch.int64, device=DEV))):
        out = L.filter_long(r, f)
        assert type(out) is type(r) and _same_but_audio(out, r) and out.audio is not r.audio
        want, _ = f.filter_batch(r.audio, r.length)
        assert torch.equal(_bits(out.audio), _bits(want))
        n = int(r.length)
        assert not bool(out.audio[0, n:].view(torch.int32).any())
        assert torch.equal(_bits(out.audio[0, :n]), _bits(f.forward(r.audio[0, :n].clone())))
    with pytest.raises(_lib.T2SError, match="pcm16=False"):
        L.filter_long(r._replace(audio=audio.to_pcm16(joined)), f)
    with pytest.raises(_lib.T2SError, match="SosFilter"):
        L.filter_long(r, None)
    with pytest.raises(_lib.T2SError, match="LongForm"):
        L.filter_long(joined, f)
