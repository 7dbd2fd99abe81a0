"""The stream contract of INTEGRATION.md section 4 at the model level: every call here is issued on a caller's stream of its own,
never only on the default one.

(a) before: the true input reaches its buffer behind a gate on the caller's stream S (tests/stream_util.py); a call that did not
    wait for everything enqueued on S - on a helper stream, say - computes from the decoy the buffer held.
(b) after: the result is read with a copy enqueued on S and S.synchronize() alone, and the default-stream reference is re-run
    afterwards on the same object, which shows the run on S left workspaces and carried state usable.
(c) across streams: the weights become true behind a gate on stream A (their versions change on the host at once), the call is
    issued on A and at once on B; B's call finds the cache keyed as current and must wait for A on the device.

Reference: the same call on the default stream with the same seeds, synchronised.  Keyed draws and given seeds make every inference
path here deterministic, so results are compared with torch.equal (two runs are asserted bit-equal in tests/test_infer_w16_gpu.py,
tests/test_keyed_sampling_gpu.py and tests/test_streaming_gpu.py).  Every test asserts first that its decoy's result differs from
the true one, and that its gate was still running at the moment the docstring of the helper names.

Calls that block the host until S drains cannot have the gate checked after they return: infer of a .half() model (the fp16 range
check reads the audio back), infer_batch (the lengths are uploaded by a blocking copy) and Tacotron's inference (the stop poll).
For them the gate is checked right before the call."""
import time

import pytest
import torch

import stream_util as SU
from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA = 0.666
CFG = synth.WAVEGLOW_SMALL
CFG48 = dict(CFG, WN_config=dict(CFG["WN_config"], n_channels=48))
# the short model of tests/test_waveglow_train_gpu.py (_short_cfg): 4 flows of 4 layers keep a whole training step, the longest call
# here, at a few hundred launches - its gate stays far below the cap of half a second, whatever the host's pace
CFG_SHORT = dict(CFG, n_flows=4, n_early_every=2, WN_config=dict(n_layers=4, n_channels=64, kernel_size=3))
HP = synth.TACOTRON_HPARAMS
T_IN, N_STEPS = 16, 8


# ---------------------------------------------------------------------------------------------------------------- helpers
def _flat(out):
    if torch.is_tensor(out):
        return [out]
    res = []
    for o in out:
        res += _flat(o)
    return res


def _clone(out):
    """copies enqueued on the current stream"""
    return [t.detach().clone() for t in _flat(out)]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _fill(bufs, values):
    for b, v in zip(_flat(bufs), _flat(values)):
        b.copy_(v, non_blocking=True)


def _reference(name, call, buf, true, decoy, same):
    """(reference result, milliseconds of the call): default stream, warm; asserts that the decoy leads somewhere else."""
    _fill(buf, true)
    call()                                  # warm: packs, workspaces and job tables exist from here on
    ref, ms = SU.timed(lambda: _clone(call()))
    _fill(buf, decoy)
    dec = _clone(call())
    torch.cuda.synchronize()
    assert not same(dec, ref), "%s: the decoy input gives the true result - the test could not fail" % name
    return ref, ms


def before_after(name, call, buf, true, decoy, host_syncs=False, same=None):
    """(a) and (b) for call(), which reads the device tensor(s) `buf`, on a stream S of the test's own.  host_syncs: the call blocks the host until its stream
    drains, so the gate is checked right before it and not right after.  same(got, ref): torch.equal of every output unless the
    path accumulates with atomics and the test brings the bar of that path's own test."""
    same = same or _same
    ref, ms = _reference(name, call, buf, true, decoy, same)
    n = SU.gate_matmuls(ms)
    SU.log(name, ms, n)
    S = torch.cuda.Stream(device=DEV)
    # The caching allocator keeps a pool per stream, and on a new stream every temporary of the call is a device allocation of its
    # own: a training step was seen to take three times its usual host time that way, which the duration measured above does not
    # hold.  So the call runs once on S, ungated and on the decoy, and once more on the default stream: the gated run below finds
    # S's pool filled and still arrives on another stream than the object's last call.
    with torch.cuda.stream(S):
        call()
    S.synchronize()
    call()
    torch.cuda.synchronize()
    gate = SU.behind_gate(S, buf, true, n)          # buf holds the decoy until the gate has drained
    t0 = time.perf_counter()
    with torch.cuda.stream(S):
        if host_syncs:
            gate.check()
        out = call()
        running = gate.still_running()
        print("stream-contract %-46s issued on S in %.3f ms, gate still running: %s" % (name, (time.perf_counter() - t0) * 1e3, running))
        if not host_syncs:
            gate.check()
        got = _clone(out)
    S.synchronize()
    assert same(got, ref), "%s on a caller's stream differs from the default-stream run" % name
    again = _clone(call())                          # (b) the default stream again, same object
    torch.cuda.synchronize()
    assert same(again, ref), "%s on the default stream after the run on a caller's stream" % name


def _params(m):
    return [p.detach().clone() for p in m.parameters()]


def _set_params(m, values):
    """in place: the versions change on the host at once, the copies run on the current stream"""
    with torch.no_grad():
        for p, v in zip(m.parameters(), values):
            p.copy_(v, non_blocking=True)


def across(name, m, call, true_w, decoy_w, second=None, check="after B"):
    """(c) call() on stream A behind gated weights, then second() (default: the same call) on stream B at once.  check: where A's
    gate must still be running - "after B" (neither call blocks the host), "before B" (B's call blocks the host until B, and with
    the contract A, has drained) or "before A" (A's call blocks the host already)."""
    second = second or call
    _set_params(m, true_w)
    call()
    ref, ms = SU.timed(lambda: _clone(call()))
    ref2 = _clone(second())
    _set_params(m, decoy_w)
    dec = _clone(second())                          # warm, completely, under the decoy weights' versions
    torch.cuda.synchronize()
    assert not _same(dec, ref2), "%s: the decoy weights give the true result - the test could not fail" % name
    n = SU.gate_matmuls(2 * ms)                     # two calls are enqueued while it runs
    SU.log(name, 2 * ms, n)
    A, B = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    gate = SU.Gate(A, n)
    with torch.cuda.stream(A):
        _set_params(m, true_w)
        if check == "before A":
            gate.check()
        got_a = _clone(call())
    if check == "before B":
        gate.check()
    with torch.cuda.stream(B):
        got_b = _clone(second())
    if check == "after B":
        gate.check()                                # A's gate outlived the enqueueing of both calls
    A.synchronize()
    B.synchronize()
    assert _same(got_a, ref), "%s: the call on stream A" % name
    assert _same(got_b, ref2), "%s: the call on stream B read what A had not finished" % name


# ---------------------------------------------------------------------------------------------------------------- WaveGlow
def _waveglow(cfg, seed=1234, half=False):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg, seed=seed), strict=True)
    m = m.to(DEV).eval()
    if half:            # as the reference's inference script: .half() with the 1x1 convolutions put back to float
        m.half()
        for c in m.convinv:
            c.float()
    return m


def _mels(B, frames, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 80, frames, generator=gen).to(DEV), torch.randn(B, 80, frames, generator=gen).to(DEV)


def _seeds(B):
    return torch.arange(11, 11 + B, dtype=torch.int64).to(DEV)          # on the device: used as they are, no upload per call


@pytest.fixture(scope="module")
def wg():
    assert torch.cuda.is_available()
    _lib.load()
    return _waveglow(CFG)


@pytest.fixture(scope="module")
def wg_half():
    return _waveglow(CFG, half=True)


@pytest.fixture(scope="module")
def wg48_half():
    return _waveglow(CFG48, half=True)


def test_infer_f32(wg):
    true, decoy = _mels(2, 12, 1)
    buf, seeds = decoy.clone(), _seeds(2)
    before_after("WaveGlow.infer f32 B=2 F=12", lambda: wg.infer(buf, sigma=SIGMA, seed=seeds), buf, true, decoy)
    assert wg._eng().last_infer_w16 is False


@pytest.mark.parametrize("which", ["C64", "C48"])
def test_infer_half(which, wg_half, wg48_half):
    m = wg_half if which == "C64" else wg48_half
    true, decoy = _mels(1, 12, 2)
    buf, seeds = decoy.clone(), _seeds(1)
    before_after("WaveGlow.infer .half() %s B=1 F=12" % which, lambda: m.infer(buf, sigma=SIGMA, seed=seeds), buf, true, decoy,
                 host_syncs=True)
    assert m._eng().last_infer_w16 is True


def test_infer_batch_f32(wg):
    true, decoy = _mels(3, 10, 3)
    buf, seeds, lengths = decoy.clone(), _seeds(3), torch.tensor([10, 4, 7])
    before_after("WaveGlow.infer_batch f32 lengths 10/4/7", lambda: wg.infer_batch(buf, lengths, sigma=SIGMA, seeds=seeds), buf, true,
                 decoy, host_syncs=True)


def test_infer_batch_fp16_chain(wg_half):
    true, decoy = _mels(3, 10, 4)
    buf, seeds, lengths = decoy.clone(), _seeds(3), torch.tensor([10, 4, 7])
    eng = wg_half._eng()
    eng.infer_batch_w16 = True
    try:
        before_after("WaveGlow.infer_batch fp16 chain lengths 10/4/7",
                     lambda: wg_half.infer_batch(buf, lengths, sigma=SIGMA, seeds=seeds), buf, true, decoy, host_syncs=True)
        assert eng.last_infer_batch_w16 is True
    finally:
        eng.infer_batch_w16 = False


def test_forward_no_grad(wg):
    """the no-grad forward runs its input side on the "side" stream and its weight pack on the "pack" stream: both behind S"""
    true, decoy = _mels(2, 9, 5)
    gen = torch.Generator().manual_seed(6)
    audio = (torch.rand(2, 8 * 256, generator=gen) - 0.5).to(DEV)
    buf = decoy.clone()

    def call():
        with torch.no_grad():
            return wg((buf, audio))
    before_after("WaveGlow.forward no_grad B=2 T=2048", call, buf, true, decoy)


def test_forward_no_grad_gated_weights(wg):
    """(a) for the "pack" stream: the weights become true behind the gate, and the forced pack on the pack stream must see them"""
    mel, _ = _mels(2, 9, 7)
    gen = torch.Generator().manual_seed(8)
    audio = (torch.rand(2, 8 * 256, generator=gen) - 0.5).to(DEV)
    true_w, decoy_w = _params(wg), _params(_waveglow(CFG, seed=99))

    def call():
        with torch.no_grad():
            return wg((mel, audio))
    try:
        ref, ms = SU.timed(lambda: _clone(call()))
        _set_params(wg, decoy_w)
        dec = _clone(call())
        torch.cuda.synchronize()
        assert not _same(dec, ref)
        n = SU.gate_matmuls(ms)
        SU.log("WaveGlow.forward no_grad, gated weights", ms, n)
        S = torch.cuda.Stream(device=DEV)
        gate = SU.Gate(S, n)
        with torch.cuda.stream(S):
            _set_params(wg, true_w)
            got = _clone(call())
            gate.check()
        S.synchronize()
        assert _same(got, ref)
    finally:
        _set_params(wg, true_w)
        torch.cuda.synchronize()


def test_across_streams_infer(wg):
    """the `packed` slot: A repacks behind the gate, B finds the cache keyed as current"""
    mel, _ = _mels(1, 12, 9)
    seeds = _seeds(1)
    true_w, decoy_w = _params(wg), _params(_waveglow(CFG, seed=99))
    try:
        across("across streams: WaveGlow.infer f32", wg, lambda: wg.infer(mel, sigma=SIGMA, seed=seeds), true_w, decoy_w)
    finally:
        _set_params(wg, true_w)
        torch.cuda.synchronize()


def test_half_repack_blocks_the_host_two_streams_agree(wg_half, monkeypatch):
    """NOT a stale-read test.  A .half() model's repack blocks the host: the f32 copies of its parameters are new tensors, so the
    pack's job table is uploaded again, by a blocking copy on A.  B's call is then issued behind a drained A, and the gate can only
    be checked before A's call: this case shows (a) for the gated weights on the `packed16` slot and that the calls on A and B
    agree.  What orders a read of `packed16` on B behind A is the engine's StreamOrder, the same wait the f32 case above and the
    alternating case below exercise; for this slot alone it stands on reading.  (T2S_F16_GUARD=0, the switch of the timing runs,
    drops the other blocking step, the read-back of the fp16 range check.)"""
    monkeypatch.setenv("T2S_F16_GUARD", "0")
    m = wg_half
    mel, _ = _mels(1, 12, 9)
    seeds = _seeds(1)
    true_w, decoy_w = _params(m), _params(_waveglow(CFG, seed=99, half=True))
    try:
        across("gated weights, infer half on A then B (A blocks)", m, lambda: m.infer(mel, sigma=SIGMA, seed=seeds), true_w, decoy_w,
               check="before A")
    finally:
        _set_params(m, true_w)
        torch.cuda.synchronize()


def test_across_streams_infer_then_infer_batch(wg):
    """infer on A packs the true weights behind the gate; infer_batch on B takes the same `packed` slot from the cache.  (infer_batch
    as A's call would drain A on the host - its lengths upload blocks - and leave B nothing to run ahead of.)"""
    mel, _ = _mels(3, 10, 10)
    seeds, lengths = _seeds(3), torch.tensor([10, 4, 7])
    true_w, decoy_w = _params(wg), _params(_waveglow(CFG, seed=99))
    try:
        across("across streams: infer on A, infer_batch on B", wg, lambda: wg.infer(mel, sigma=SIGMA, seed=seeds), true_w, decoy_w,
               second=lambda: wg.infer_batch(mel, lengths, sigma=SIGMA, seeds=seeds), check="before B")
    finally:
        _set_params(wg, true_w)
        torch.cuda.synchronize()


def test_across_streams_adam_step_then_infer():
    """FusedAdam.step on A behind a gate, infer on B: B's pack must read the stepped parameters.  The reference is an identically
    built model and optimizer on the default stream.  No clipping here: the plain table kernel is elementwise, so the stepped
    weights - and the audio - are bit-equal between two runs."""
    from text2speech_amd.optim import FusedAdam
    mel, _ = _mels(1, 12, 11)
    seeds = _seeds(1)
    models = [_waveglow(CFG), _waveglow(CFG)]
    opts = []
    for m in models:
        gen = torch.Generator().manual_seed(12)
        for p in m.parameters():
            p.grad = (torch.randn(p.shape, generator=gen) * 0.1).to(DEV)
        opt = FusedAdam(m.parameters(), lr=0.0)
        opt.step()                                      # warm: job tables and moments exist; lr = 0 leaves the weights alone
        opt.param_groups[0]["lr"] = 1e-2
        opts.append(opt)
    ref_m, m = models
    call = lambda mm: mm.infer(mel, sigma=SIGMA, seed=seeds)
    call(ref_m)
    opts[0].step()
    ref, ms = SU.timed(lambda: _clone(call(ref_m)))
    dec = _clone(call(m))                               # warm under the weights before the step: the decoy
    torch.cuda.synchronize()
    assert not _same(dec, ref)
    n = SU.gate_matmuls(ms)
    SU.log("across streams: FusedAdam.step on A, infer on B", ms, n)
    A, B = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    gate = SU.Gate(A, n)
    with torch.cuda.stream(A):
        opts[1].step()
    with torch.cuda.stream(B):
        got = _clone(call(m))
    gate.check()
    B.synchronize()
    A.synchronize()
    assert _same(got, ref), "infer on stream B did not see the parameters FusedAdam.step wrote on stream A"


@pytest.mark.parametrize("half", [False, True], ids=["f32-packed", "half-packed16"])
def test_alternating_streams_share_the_workspace(half, wg, wg_half, monkeypatch):
    """unchanged weights, two inputs: infer on A behind a gate, infer on B at once - both on the engine's one resident workspace, B
    reading the cached `packed` / `packed16` planes while A is still busy.  (.half(): T2S_F16_GUARD=0 drops the read-back of the
    fp16 range check, which would drain A on the host; the launches are the same.)"""
    monkeypatch.setenv("T2S_F16_GUARD", "0")
    wg = wg_half if half else wg
    mel1, mel2 = _mels(1, 12, 13)
    seeds = _seeds(1)
    call = lambda mel: wg.infer(mel, sigma=SIGMA, seed=seeds)
    call(mel1)
    ref1, ms = SU.timed(lambda: _clone(call(mel1)))
    ref2 = _clone(call(mel2))
    torch.cuda.synchronize()
    assert not _same(ref1, ref2)
    n = SU.gate_matmuls(2 * ms)
    SU.log("alternating streams, one workspace%s" % (" (.half())" if half else ""), 2 * ms, n)
    A, B = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    gate = SU.Gate(A, n)
    with torch.cuda.stream(A):
        got1 = _clone(call(mel1))
    with torch.cuda.stream(B):
        got2 = _clone(call(mel2))
    gate.check()
    A.synchronize()
    B.synchronize()
    assert _same(got1, ref1), "the call on stream A"
    assert _same(got2, ref2), "the call on stream B"
    assert wg._eng().last_infer_w16 is half


# ---------------------------------------------------------------------------------------------------------------- Tacotron
def _tacotron(seed=4321, half=False):
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(seed=seed), strict=True)
    m = m.to(DEV).eval()
    if half:
        m.half()
    m.decoder.gate_threshold, m.decoder.max_decoder_steps = 2.0, N_STEPS      # never stops by itself: N_STEPS frames
    return m


def _ids(B, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(2, 80, (B, T_IN), generator=gen).to(DEV), torch.randint(2, 80, (B, T_IN), generator=gen).to(DEV)


@pytest.fixture(scope="module")
def taco():
    assert torch.cuda.is_available()
    _lib.load()
    return _tacotron()


def test_tacotron_inference(taco):
    true, decoy = _ids(1, 21)
    buf = decoy.clone()
    before_after("Tacotron2.inference B=1 T_in=16, 8 steps", lambda: taco.inference(buf, seed=5), buf, true, decoy, host_syncs=True)


def test_tacotron_inference_batch(taco):
    true, decoy = _ids(3, 22)
    buf, seeds, lengths = decoy.clone(), _seeds(3), torch.tensor([16, 9, 12])
    before_after("Tacotron2.inference_batch lengths 16/9/12", lambda: taco.inference_batch(buf, lengths, seeds=seeds), buf, true,
                 decoy, host_syncs=True)


def test_tacotron_half_decode():
    m = _tacotron(half=True)
    true, decoy = _ids(1, 23)
    buf = decoy.clone()
    before_after("Tacotron2.inference .half() (w16 decode)", lambda: m.inference(buf, seed=5), buf, true, decoy, host_syncs=True)
    assert m._eng().last_decode_w16 is True


def test_across_streams_tacotron_prepare(taco):
    """prepare() on A folds and packs the true weights behind the gate and re-keys the cache on the host; inference on B finds the
    cache current.  (inference as A's call would drain A at its first stop poll.)  B's inference blocks the host until B - and
    with the contract A - has drained, so the gate is checked after prepare() returns, right before B's call."""
    ids, _ = _ids(1, 24)
    true_w, decoy_w = _params(taco), _params(_tacotron(seed=99))
    eng = taco._eng()
    call = lambda: taco.inference(ids, seed=5)

    def whole():        # what is enqueued while the gate runs: the weights, prepare() and the inference
        _set_params(taco, true_w)
        eng.prepare(torch.device(DEV))
        return _clone(call())
    try:
        whole()
        ref, ms = SU.timed(whole)
        _set_params(taco, decoy_w)
        dec = _clone(call())
        torch.cuda.synchronize()
        assert not _same(dec, ref)
        n = SU.gate_matmuls(ms)
        SU.log("across streams: prepare on A, Tacotron2.inference on B", ms, n)
        A, B = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
        gate = SU.Gate(A, n)
        with torch.cuda.stream(A):
            _set_params(taco, true_w)
            eng.prepare(torch.device(DEV))
        gate.check()
        with torch.cuda.stream(B):
            got = _clone(call())
        B.synchronize()
        A.synchronize()
        assert _same(got, ref), "inference on stream B read prepared weights that stream A had not written yet"
    finally:
        _set_params(taco, true_w)
        torch.cuda.synchronize()


def test_synthesize_stream_keyed(taco, wg):
    """text to audio pieces on one caller's stream: Tacotron's chunks, the stop polls and the vocoder's windows"""
    from text2speech_amd import streaming
    true, decoy = _ids(1, 25)
    buf = decoy.clone()
    call = lambda: list(streaming.synthesize_stream(taco, wg, buf, seed=77, sigma=SIGMA, first_frames=16, window_frames=32, halo=(24, 24)))
    before_after("synthesize_stream, 8 frames", call, buf, true, decoy, host_syncs=True)


# ---------------------------------------------------------------------------------------------------------- training steps
def _step_same(loss_bar):
    """outputs [loss, gradients ..., parameters after the step ...]: the loss at its own test's bar (its partial sums are added with
    atomics); everything else bit for bit - both backward passes are asserted bitwise reproducible in
    tests/test_waveglow_train_gpu.py and tests/test_tacotron_train_gpu.py, the gradient norm adds its partials in a fixed order
     and the Adam kernel is elementwise."""
    def same(a, b):
        if len(a) != len(b) or abs(float(a[0]) - float(b[0])) > loss_bar * max(1.0, abs(float(b[0]))):
            return False
        return all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    return same


def _waveglow_step_case():
    from text2speech_amd.glow import WaveGlowLoss
    from text2speech_amd.optim import FusedAdam
    m = _waveglow(CFG_SHORT).train()
    mel, audio = synth.waveglow_inputs(2, 2048, seed=32)
    mel2, _ = synth.waveglow_inputs(2, 2048, seed=33)
    mel, mel2, audio = mel.to(DEV), mel2.to(DEV), audio.to(DEV)
    params = list(m.parameters())
    w0 = _params(m)
    opt = FusedAdam(params, lr=1e-3, max_grad_norm=1.0)
    crit = WaveGlowLoss(1.0)
    src = [w.clone() for w in w0]           # what a step starts from: the weights variant puts these behind the gate
    buf = mel.clone()

    def call():
        _set_params(m, src)
        for p in params:
            st = opt.state.get(p)
            if st and "exp_avg" in st:
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        opt.param_groups[0]["step"] = 0
        m.zero_grad(set_to_none=False)      # in place: the optimizer's job table keeps its pointers and is not uploaded again
        loss = crit(m((buf, audio)))
        loss.backward()
        grads = [p.grad for p in params]
        opt.step()
        return [loss.detach()] + grads + [p.detach() for p in params]
    return m, call, buf, mel, mel2, src, w0


def test_waveglow_training_step_gated_input():
    """loss, backward and a clipped FusedAdam.step on a caller's stream: the "pack" stream of the training forward, the "bwd_side"
    stream of the backward and autograd's own thread all sit behind the gate.  Loss bar: 1e-4, tests/test_waveglow_train_gpu.py."""
    m, call, buf, mel, mel2, src, w0 = _waveglow_step_case()
    before_after("WaveGlow training step, gated mel", call, buf, mel, mel2, same=_step_same(1e-4))


def test_waveglow_training_step_gated_weights():
    m, call, buf, mel, mel2, src, w0 = _waveglow_step_case()
    decoy_w = _params(_waveglow(CFG_SHORT, seed=99))
    buf.copy_(mel)
    before_after("WaveGlow training step, gated weights", call, src, w0, decoy_w, same=_step_same(1e-4))


def _tacotron_step_case():
    from text2speech_amd.optim import FusedAdam
    from text2speech_amd.tacotron import Tacotron, Tacotron2Loss
    B, T_in, T_out = 3, 16, 10
    gen = torch.Generator().manual_seed(8)
    in_len = torch.tensor([T_in - i for i in range(B)])
    out_len = torch.tensor([T_out - i for i in range(B)])
    text, text2 = torch.randint(2, 80, (B, T_in), generator=gen), torch.randint(2, 80, (B, T_in), generator=gen)
    mel_t = torch.randn(B, 80, T_out, generator=gen)
    gate_t = torch.zeros(B, T_out)
    for b in range(B):
        text[b, in_len[b]:] = 0
        text2[b, in_len[b]:] = 0
        mel_t[b, :, out_len[b]:] = 0
        gate_t[b, out_len[b] - 1:] = 1
    bern = lambda *s: (torch.rand(*s, generator=gen) < 0.5).to(torch.uint8).to(DEV)
    tm = {"enc": [bern(B, 512, T_in) for _ in range(3)], "att": bern(T_out, B, 1024), "dec": bern(T_out, B, 1024),
          "post": [bern(B, 512, T_out) for _ in range(4)] + [bern(B, 80, T_out)]}
    pm = bern(T_out + 1, B, 2, 256)
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    m = m.to(DEV).train()
    params = list(m.parameters())
    w0, b0 = _params(m), [b.detach().clone() for b in m.buffers()]
    src = [w.clone() for w in w0]
    opt = FusedAdam(params, lr=1e-3, max_grad_norm=1.0)
    crit = Tacotron2Loss()
    text, text2, mel_t, gate_t = text.to(DEV), text2.to(DEV), mel_t.to(DEV), gate_t.to(DEV)
    in_len_d, out_len_d, spk = in_len.to(DEV), out_len.to(DEV), torch.zeros(B, device=DEV)
    buf = text.clone()

    def call():
        _set_params(m, src)
        with torch.no_grad():
            for b, v in zip(m.buffers(), b0):       # BatchNorm running statistics back to the start
                b.copy_(v)
        for p in params:
            st = opt.state.get(p)
            if st and "exp_avg" in st:
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        opt.param_groups[0]["step"] = 0
        m.zero_grad(set_to_none=False)      # in place: the optimizer's job table keeps its pointers and is not uploaded again
        out = m((buf, in_len_d, mel_t, T_in, spk, out_len_d), prenet_masks=pm, train_masks=tm)
        loss = crit(out, (mel_t, gate_t))
        loss.backward()
        with_grad = [p for p in params if p.grad is not None]
        grads = [p.grad for p in with_grad]
        opt.step()
        return [loss.detach()] + grads + [p.detach() for p in params]
    return m, call, buf, text, text2, src, w0


def test_tacotron_training_step_gated_input():
    """teacher-forced forward (decoder cells on the library's helper stream), Tacotron2Loss, the BPTT on its helper streams, the
    encoder's backward side stream and a clipped FusedAdam.step.  Loss bar: 2e-4, tests/test_tacotron_train_gpu.py."""
    m, call, buf, text, text2, src, w0 = _tacotron_step_case()
    before_after("Tacotron training step, gated text", call, buf, text, text2, same=_step_same(2e-4))


def test_tacotron_training_step_gated_weights():
    m, call, buf, text, text2, src, w0 = _tacotron_step_case()
    decoy_w = _params(_tacotron(seed=99))
    before_after("Tacotron training step, gated weights", call, src, w0, decoy_w, same=_step_same(2e-4))


# ---------------------------------------------------------------------------------------------------------- audio front end
def _audio(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, T, generator=gen) - 0.5) * 1.6).to(DEV), ((torch.rand(B, T, generator=gen) - 0.5) * 1.6).to(DEV)


def test_stft_transform_and_inverse():
    from text2speech_amd.audio import STFT
    stft = STFT(1024, 256, 1024).to(DEV)
    true, decoy = _audio(2, 4096, 41)
    buf = decoy.clone()

    def call():
        mag, ph = stft.transform(buf)
        return mag, ph, stft.inverse(mag, ph)
    before_after("STFT.transform + inverse B=2 T=4096", call, buf, true, decoy)


def test_mel_spectrogram():
    from text2speech_amd.audio import TacotronSTFT
    ts = TacotronSTFT().to(DEV)
    true, decoy = _audio(2, 4096, 42)
    buf = decoy.clone()
    before_after("TacotronSTFT.mel_spectrogram B=2 T=4096", lambda: ts.mel_spectrogram(buf), buf, true, decoy, host_syncs=True)


def test_ragged_stft_and_mel():
    from text2speech_amd.audio import TacotronSTFT
    ts = TacotronSTFT().to(DEV)
    true, decoy = _audio(3, 4096, 43)
    buf, lengths = decoy.clone(), torch.tensor([4096, 1500, 3001])

    def call():
        mag, ph, fl = ts.stft_fn.transform_batch(buf, lengths)
        audio, alen = ts.stft_fn.inverse_batch(mag, ph, fl)
        mel, ml = ts.mel_spectrogram_batch(buf, lengths)
        return mag, ph, audio, alen, mel, ml
    before_after("ragged transform / inverse / mel, lengths 4096/1500/3001", call, buf, true, decoy, host_syncs=True)


def test_resample_and_trim_batches():
    """resample_batch and trim_batch with lengths that live on the device: nothing is uploaded or read back.  The kept samples are
    compared bit for bit, as tests/test_trim_gpu.py compares a batch with its entries alone (the statistics the gain is taken from
    are a maximum and float64 sums per frame)."""
    from text2speech_amd.audio import Resampler, Trimmer
    rs, tr = Resampler(22050, 16000, device=DEV), Trimmer(top_db=23, rescaling_max=0.9)
    gen = torch.Generator().manual_seed(44)
    env = torch.cat([torch.zeros(600), torch.ones(2400), torch.zeros(1096)])          # silence at both ends: the trim has work to do
    true = ((torch.rand(3, 4096, generator=gen) - 0.5) * env).to(DEV)
    decoy = ((torch.rand(3, 4096, generator=gen) - 0.5) * env.flip(0) * 0.5).to(DEV)
    buf, lengths = decoy.clone(), torch.tensor([4096, 3500, 3900]).to(DEV)

    def call():
        out, olen = rs.resample_batch(buf, lengths)
        cut, clen = tr.trim_batch(buf, lengths)
        return out, olen, cut, clen
    before_after("resample_batch + trim_batch, device lengths", call, buf, true, decoy)


def _pool_clips(seed):
    """three int16 clips at 22050 Hz with silence at both ends: the trim has work to do and keeps something of each"""
    gen = torch.Generator().manual_seed(seed)
    clips = []
    for n in (3000, 2205, 4410):
        env = torch.zeros(n)
        env[n // 5:n - n // 4] = 1.0
        clips.append(((torch.rand(n, generator=gen) - 0.5) * env * 20000).to(torch.int16))
    return clips


def test_pcm_pool_resample_rescale_trim():
    """resample, rescale and trim of an int16 pool (data.PcmPool: t2s_resample_table, the trim statistics, bounds and gather, their
    tables sent over without waiting for the copy).  The gated input is pool.pcm, the decoy another valid pool of the same clip
    lengths.  The resampler's filter is uploaded by a blocking copy and the cut points are read back: the gate is checked before
    the call.  int16 in, int16 out: bit for bit, as tests/test_trim_gpu.py and tests/test_resample_gpu.py compare pools."""
    from text2speech_amd.data import PcmPool
    pool = PcmPool(_pool_clips(45), 22050, device=DEV)
    true = pool.pcm.clone()
    decoy = PcmPool(_pool_clips(46), 22050, device=DEV).pcm.clone()

    def call():
        r = pool.resample(16000)
        t = r.rescale_trim(0.999, 23)
        return r.pcm, t.pcm, t.lengths
    before_after("PcmPool.resample + rescale_trim, 3 clips", call, pool.pcm, true, decoy, host_syncs=True)
