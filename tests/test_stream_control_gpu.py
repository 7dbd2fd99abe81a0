"""streaming.synthesize_stream(control=) on the device, on the small models of tests/test_streaming_gpu.py (its helpers are restated
here): the speaking rate, the symbol timestamps and the alignment watchdog inside a stream.

control=None issues the launches of the call without it; a StreamControl with nothing set, and speed=1.0, give the plain stream's
audio bit for bit; speed=0.8 gives stride warped_length(F, 0.8) samples within SOLO_BAR (1e-4 rel-L2, the project's bar between two
HIP calls) of infer(warp_mel(inference(...).mel_post, 0.8).mel, seed=); spans() and report() equal the whole-utterance calls; the
watchdog ends the stream at the piece the restatement names.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import align_ref as AR
import stream_ctl_ref as SC
import streaming_ref as R
import warp_ref as W
from text2speech_amd import _lib, alignment, audio, rate as RT, streaming, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SRC = 44800
N_STEPS = 150               # max_decoder_steps of these tests: decode chunks of 64 end at 64, 128 and 150
HP = synth.TACOTRON_HPARAMS
SEED = 20240611
SIGMA = R.SIGMA
SHORT = dict(first_frames=16, window_frames=32, halo=(24, 24))      # stream against stream: any halo, as long as both use it
EXACT = dict(first_frames=16, window_frames=32)                      # stream against infer(): the vocoder's own reach
OWN = ("t2s_align_window", "t2s_warp_window_map", "t2s_warp_window_gather", "t2s_warp_spans")
NEVER = alignment.AlignmentCheck(skip_max=10 ** 6, back_max=10 ** 6, stall_max=10 ** 6, end_slack=10 ** 6, min_focus=0.0)


def _waveglow(sd, half=False):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**R.CFG)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    if half:            # as the reference's inference script: .half() with the 1x1 convolutions put back to float
        m.half()
        for c in m.convinv:
            c.float()
    return m


def _set_decoder(model, thr, n):
    model.decoder.gate_threshold, model.decoder.max_decoder_steps = thr, n


def _pick_stop(model, margin=1e-4):
    """(ids, threshold, stop step): tests/test_streaming_gpu.py's way of making the stop fire at a known step - a threshold half-way
    between a step's sigmoid(gate) and the largest one before it, more than `margin` from both; a dozen texts are tried and the
    step nearest to 100 is taken."""
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


class Case:
    """one text under one gate threshold: the whole call's outputs and the streamed pieces, computed once and left unchanged"""

    def __init__(self, taco, ids, thr):
        self.taco, self.ids, self.thr = taco, ids, thr
        with self:
            self.mel, self.mel_post, self.gate, self.align = taco.inference(ids, None, seed=SEED)
            self.pieces = list(taco.inference_stream(ids, None, seed=SEED))
        self.F, self.T = self.mel_post.size(2), self.align.size(2)
        self.streamed = torch.cat([p[1] for p in self.pieces], 2)
        assert torch.equal(torch.cat([p[3] for p in self.pieces], 1), self.align)

    def __enter__(self):
        _set_decoder(self.taco, self.thr, N_STEPS)

    def __exit__(self, *exc):
        _set_decoder(self.taco, HP["gate_threshold"], HP["max_decoder_steps"])

    def synth(self, wg, **kw):
        with self:
            return list(streaming.synthesize_stream(self.taco, wg, self.ids, seed=SEED, sigma=SIGMA, **kw))


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available()
    _lib.load()
    from text2speech_amd.tacotron import Tacotron
    taco = Tacotron(HP, 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state(), strict=True)
    taco = taco.to(DEV).eval()
    sd = synth.waveglow_state(R.CFG, **R.STRESS)
    try:
        _set_decoder(taco, 2.0, N_STEPS)
        ids, thr, stop = _pick_stop(taco)
    finally:
        _set_decoder(taco, HP["gate_threshold"], HP["max_decoder_steps"])
    stopped = Case(taco, ids, thr)                              # stops at a picked step
    full = Case(taco, torch.randint(2, 80, (1, 23), generator=torch.Generator().manual_seed(11)).to(DEV), 2.0)   # three pieces, to the cap
    print("stop case: %d symbols, threshold %.6f, %d frames in %d pieces; full case: %d frames in %d pieces"
          % (ids.size(1), thr, stopped.F, len(stopped.pieces), full.F, len(full.pieces)))
    assert stopped.F == stop + 1 and full.F == N_STEPS and len(full.pieces) == 3
    return dict(taco=taco, wg=_waveglow(sd), wg16=_waveglow(sd, half=True), stopped=stopped, full=full)


def test_control_none_issues_the_launches_it_issued_before(models, monkeypatch, capfd):
    case, wg = models["full"], models["wg"]
    names, real = [], _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    case.synth(wg, **SHORT)                                     # (warm: the first call packs the vocoder's weights)
    monkeypatch.setattr(_lib, "call", call)
    plain = case.synth(wg, **SHORT)
    n_plain = list(names)
    del names[:]
    none = case.synth(wg, control=None, **SHORT)
    n_none = list(names)
    del names[:]
    ctl = streaming.StreamControl(speed=1.0, check=NEVER, timestamps=True)
    with_c = case.synth(wg, control=ctl, **SHORT)
    n_with = list(names)
    capfd.readouterr()
    assert n_plain and n_none == n_plain and all(torch.equal(a, b) for a, b in zip(none, plain))
    assert not any(n in OWN for n in n_plain) and [n for n in n_with if n not in OWN] == n_plain
    assert n_with.count("t2s_align_window") == len(case.pieces)
    assert n_with.count("t2s_warp_window_map") == n_with.count("t2s_warp_window_gather") == sum(1 for p in case.pieces if p[1].size(2))
    assert len(with_c) == len(plain) and all(torch.equal(a, b) for a, b in zip(with_c, plain))
    assert (ctl.frames_in, ctl.frames_out, ctl.aborted) == (case.F, case.F, False)


@pytest.mark.parametrize("which", ["stopped", "full"])
def test_a_control_with_nothing_set_and_speed_one_are_the_plain_stream(models, capfd, which):
    case, wg = models[which], models["wg"]
    plain = case.synth(wg, **SHORT)
    made = []

    def make():
        made.append(streaming.StreamControl())
        return made[-1]
    empty = case.synth(wg, control=make, **SHORT)
    one = streaming.StreamControl(speed=1.0)
    at_one = case.synth(wg, control=one, **SHORT)
    capfd.readouterr()
    assert len(made) == 1 and len(empty) == len(at_one) == len(plain)
    assert all(torch.equal(a, b) for a, b in zip(empty, plain)) and all(torch.equal(a, b) for a, b in zip(at_one, plain))
    assert sum(a.size(1) for a in plain) == 256 * case.F
    for ctl in (made[0], one):
        assert (ctl.frames_in, ctl.frames_out, ctl.flags, ctl.aborted) == (case.F, case.F, 0, False)
    with pytest.raises(_lib.T2SError, match="one utterance"):
        case.synth(wg, control=one, **SHORT)
    with pytest.raises(_lib.T2SError, match="StreamControl"):
        case.synth(wg, control=dict(speed=1.0), **SHORT)
    with pytest.raises(_lib.T2SError, match="returned"):
        case.synth(wg, control=lambda: 0.8, **SHORT)


def _reference(case, wg, warped_mel, den):
    out = wg.infer(warped_mel, sigma=SIGMA, seed=SEED)
    return den(out, 0.1)[:, 0] if den is not None else out


@pytest.mark.parametrize("wg,denoise,deliver", [("wg", False, False), ("wg", True, False), ("wg", False, True), ("wg16", False, False)])
def test_speed_inside_the_stream(models, capfd, wg, denoise, deliver):
    case, m = models["stopped"], models[wg]
    den = audio.Denoiser(m) if denoise else None
    kw = dict(denoiser=den, strength=0.1) if denoise else {}
    length = RT.warped_length(case.F, 0.8)
    want = _reference(case, m, RT.warp_mel(case.mel_post, None, 0.8).mel, den)
    own = _reference(case, m, RT.warp_mel(case.streamed, None, 0.8).mel, den)       # (the streamed mel_post: inference_stream's rounding)
    ctl = streaming.StreamControl(speed=0.8)
    if deliver:
        # 8 kHz mu-law: the encoding is pointwise, so the mu-law stream must be to_ulaw of the float stream bit for bit, and the
        # float stream meets the bar against the whole chain
        got = torch.cat(case.synth(m, control=ctl, delivery=audio.DeliveryStream(SRC, 8000, encoding="f32"), **EXACT, **kw), 1)
        codes = torch.cat(case.synth(m, control=streaming.StreamControl(speed=0.8), delivery=audio.DeliveryStream(SRC, 8000, encoding="ulaw"),
                                     **EXACT, **kw), 1)
        res = audio.Resampler(SRC, 8000, device=DEV)
        want, own = res.forward(want), res.forward(own)
        assert codes.dtype == torch.uint8 and torch.equal(codes, audio.to_ulaw(got))
        n_want = -(-256 * length * 8000 // SRC)
    else:
        got = torch.cat(case.synth(m, control=ctl, **EXACT, **kw), 1)
        n_want = 256 * length
    capfd.readouterr()
    e, e_own = R.rel(got[0].float(), want[0].float()), R.rel(got[0].float(), own[0].float())
    print("speed=0.8 in the stream (%s%s%s): %d -> %d frames, %d samples; vs infer(warp_mel(inference().mel_post)) rel %.2e; vs the "
          "same chain on the streamed mel_post rel %.2e" % (wg, ", denoiser" if denoise else "", ", 8 kHz delivery" if deliver else "",
                                                            case.F, length, got.size(1), e, e_own))
    assert (ctl.frames_in, ctl.frames_out) == (case.F, length)
    assert got.size(1) == n_want == want.size(1)
    assert e < R.SOLO_BAR


def test_a_rate_changed_while_the_stream_runs(models, capfd):
    case, wg = models["full"], models["wg"]
    ctl = streaming.StreamControl(speed=0.8)
    got, switch = [], None
    with case:
        for k, a in enumerate(streaming.synthesize_stream(case.taco, wg, case.ids, seed=SEED, sigma=SIGMA, control=ctl, **EXACT)):
            got.append(a)
            if k == 0:      # the first audio needs first_frames + 96 warped frames: two mel pieces are in, the third comes at 1.25
                ctl.speed = 1.25
                switch = ctl.frames_in
    capfd.readouterr()
    assert switch == sum(p[1].size(2) for p in case.pieces[:2]) < case.F
    index = (torch.arange(case.F) >= switch).to(torch.int32).view(1, -1).to(DEV)
    warped = RT.warp_mel(case.mel_post, None, 1.0, path=index, symbol_rates=torch.tensor([[0.8, 1.25]], device=DEV))
    length = int(warped.lengths[0])
    want = wg.infer(warped.mel[:, :, :length].contiguous(), sigma=SIGMA, seed=SEED)
    got = torch.cat(got, 1)
    e = R.rel(got[0], want[0])
    print("rate 0.8 -> 1.25 at source frame %d of %d: %d output frames; vs infer(warp_mel(path=, symbol_rates=)) rel %.2e"
          % (switch, case.F, length, e))
    assert ctl.frames_out == length and got.size(1) == 256 * length == want.size(1)
    assert e < R.SOLO_BAR


def _host_spans(path, n, T, s, hop, ratio, total):
    c = np.arange(n + 1, dtype=np.int64) * s
    return W.spans(c, W.first_last(path[:n], n, T, T), n, T, hop, ratio=ratio, total=total)


def test_timestamps_and_the_report(models, capfd):
    case, wg = models["full"], models["wg"]
    check = alignment.AlignmentCheck()
    ctl = streaming.StreamControl(speed=0.8, check=check, on_fail="flag", timestamps=True)
    ratio, s = (80, 441), RT.stretch_q(0.8)
    checked = 0
    with case:
        for a in streaming.synthesize_stream(case.taco, wg, case.ids, seed=SEED, sigma=SIGMA, control=ctl, **SHORT):
            n = ctl.frames_in
            got = ctl.spans(ratio)
            path = ctl.path[0].cpu().numpy()
            assert path.size >= n and got.dtype == torch.int64 and tuple(got.shape) == (1, case.T, 2)
            assert (got[0].cpu().numpy() == _host_spans(path, n, case.T, s, 256, ratio, None)).all(), n
            checked += 1
    capfd.readouterr()
    whole = alignment.alignment_report(case.align, check=check.with_max_frames(N_STEPS))
    length = RT.warped_length(case.F, 0.8)
    total = -(-256 * length * ratio[0] // ratio[1])
    warped = RT.warp_mel(case.mel_post, None, 0.8, path=whole.path, n_symbols=case.T)
    want = RT.symbol_spans(warped, None, None, None, 256, ratio=ratio, total=total)
    got = ctl.spans(ratio, total)
    rep = ctl.report()
    print("timestamps: %d symbols, spans checked after %d pieces; flags %d, stats %s" % (case.T, checked, ctl.flags, rep.stats[0].tolist()))
    assert torch.equal(got, want) and int(got.max()) <= total
    assert torch.equal(ctl.path, whole.path)
    for a, b in zip(rep, whole):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert ctl.flags == int(whole.flags[0]) and not ctl.aborted and ctl.frames_in == case.F


def _stall_after_each_piece(case):
    """the restatement's longest stall and flags after every alignment piece of the full run"""
    ref = SC.AlignChunks(1, case.T, None, **AR.OFF)
    return [int(ref.push(p[3].float().cpu().numpy(), p[4]).stats[0, 4]) for p in case.pieces]


@pytest.mark.parametrize("on_fail", ["stop", "flag"])
def test_the_watchdog(models, capfd, on_fail):
    case, wg, taco = models["full"], models["wg"], models["taco"]
    stalls = _stall_after_each_piece(case)
    k = 1 if stalls[1] > stalls[0] else 0                       # the piece in which the threshold is first exceeded
    stall_max = stalls[k] - 1
    assert stall_max >= 0 and (k == 0 or stalls[0] <= stall_max)
    check = alignment.AlignmentCheck(skip_max=-1, back_max=-1, stall_max=stall_max, end_slack=-1, min_focus=0.0, max_frames=10 ** 6)
    thr = dict(AR.OFF, stall_max=stall_max, max_frames=10 ** 6)
    ref = SC.AlignChunks(1, case.T, None, **thr)
    flags = [int(ref.push(p[3].float().cpu().numpy(), p[4]).flags[0]) for p in case.pieces]
    assert flags[k] == AR.STALL and (k == 0 or flags[0] == 0)
    with case:
        before = taco.inference(case.ids, None, seed=SEED)
    ctl = streaming.StreamControl(check=check, on_fail=on_fail)
    got = case.synth(wg, control=ctl, **SHORT)
    with case:
        after = taco.inference(case.ids, None, seed=SEED)
    taco._eng().check_lstm_xbuf()
    capfd.readouterr()
    print("watchdog (%s): longest stall after each piece %s, stall_max %d trips in piece %d; %d frames in, %d out, flags %d, aborted %s"
          % (on_fail, stalls, stall_max, k, ctl.frames_in, ctl.frames_out, ctl.flags, ctl.aborted))
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "an inference after the stream differs from the one before it"
    if on_fail == "flag":
        assert not ctl.aborted and ctl.frames_in == ctl.frames_out == case.F and ctl.flags == flags[-1] and ctl.flags & AR.STALL
        assert all(torch.equal(a, b) for a, b in zip(got, case.synth(wg, **SHORT)))
        return
    kept = sum(p[1].size(2) for p in case.pieces[:k + 1])
    assert ctl.aborted and ctl.frames_in == ctl.frames_out == kept < case.F and ctl.flags == flags[k]
    assert sum(a.size(1) for a in got) == 256 * kept
    cut = [(p[1], False) for p in case.pieces[:k + 1]] + [(case.pieces[0][1][:, :, :0], True)]
    want = list(wg.infer_stream(cut, sigma=SIGMA, seed=SEED, **SHORT))
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    # ... and what was delivered ends as an utterance ends
    ds = audio.DeliveryStream(SRC, 8000, encoding="ulaw")
    out = case.synth(wg, control=streaming.StreamControl(check=check), delivery=ds, **SHORT)
    capfd.readouterr()
    assert ds._ended and sum(o.size(1) for o in out) == ds.delivered == -(-256 * kept * 8000 // SRC)
    assert torch.equal(torch.cat(out, 1), audio.to_ulaw(audio.Resampler(SRC, 8000, device=DEV).forward(torch.cat(want, 1))))


def test_the_pushes_do_not_wait_and_run_on_a_callers_stream():
    B, C, F, T = 1, 80, 200, 31
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, F, generator=g).to(DEV)
    A = torch.from_numpy(AR.random_alignments(B, F, T, np.float16, 4)).to(DEV)
    check = alignment.AlignmentCheck(stall_max=1)
    cuts = [(0, 64), (64, 128), (128, 128), (128, 200)]

    def run():
        al = alignment.AlignmentStream(check, T, F, DEV)
        ws = RT.WarpStream(C, F, torch.float32, DEV, 0.8, path=al.path, n_symbols=T)
        out = []
        torch.cuda.set_sync_debug_mode("error")
        try:
            for a, b in cuts:
                al.push(A[:, a:b], b == F)
                out.append(ws.push(x[:, :, a:b], b == F))
                al.poll()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return al, ws, out
    al, ws, out = run()
    torch.cuda.synchronize()
    want = RT.warp_mel(x, None, 0.8)
    whole = alignment.alignment_report(A, check=check.with_max_frames(F))
    assert torch.equal(torch.cat(out, 2), want.mel) and torch.equal(ws.cum, want.cum)
    flags, stats = al.poll()
    assert torch.equal(flags, whole.flags.cpu()) and torch.equal(stats, whole.stats.cpu()) and int(flags[0]) & alignment.STALL
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        al2, ws2, out2 = run()
        rep = al2.report()
    side.synchronize()
    assert torch.equal(torch.cat(out2, 2), want.mel) and torch.equal(ws2.first_last, ws.first_last)
    for a, b in zip(rep, whole):
        assert torch.equal(a, b)
