"""The stream contract of INTEGRATION.md section 4 at the C ABI, for the entry points that own helper streams: t2s_taco_decode_steps,
t2s_taco_decode_steps_w16 and t2s_taco_bptt_steps, called with a `stream` argument that is not the default stream.

The cases, the structs, the Guarded buffers, the float64 references and the bars (F32_NORM / F32_MAX of wg_bwd_util) are those of
tests/test_tacotron_fwd_kernels_gpu.py, tests/test_decode_w16_gpu.py and tests/test_tacotron_bwd_kernels_gpu.py: their runners are
executed as they are, with three of their module-level helpers replaced for the duration of a test -

  dev()     the upload of `memory` / `pmem` (the incoming gradient d_hc for the backward) yields a buffer that holds a DECOY, another
            seeded draw of the same shape and scale;
  _st()     the stream handed to the entry point is the test's own stream S; before the first call a gate (tests/stream_util.py) is
            enqueued on S and, behind it, the copies that make the buffers true;
  _sync()   asserts that the gate is still running - the entry points only enqueue - and then waits for S alone.

So a helper stream that did not wait for everything enqueued on S computes from the decoys and misses the float64 bars, and a
helper stream that S did not wait for at the end has its outputs read early.  Every case first runs on the default stream twice:
as it is (the timing of the gate, and the outputs the run on S must equal bit for bit) and with the decoys left in place, which
must FAIL the runner's checks - otherwise the test could not fail.

test_two_caller_streams_back_to_back hands two consecutive calls of one teacher-forced decode (decoder cells on the helper
stream) to two different caller streams A and B, B waiting for A as a caller of the C ABI has to: the second call may only start
once the first one's helper work has been joined into A."""
import ctypes
import time

import pytest
import torch

import stream_util as SU
import test_decode_w16_gpu as W
import test_tacotron_bwd_kernels_gpu as BW
import test_tacotron_fwd_kernels_gpu as K
from text2speech_amd import _lib
from wg_bwd_util import DEV, Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


class _Runner:
    """The replacements of one test.  mode: "time" (default stream, true inputs, events around the calls), "decoy" (default stream,
    decoys stay) or "gated" (streams of the test, gate, true inputs behind it)."""

    def __init__(self, decoys, streams=None):
        self.decoys = decoys            # [(host tensor of the case, seed)]
        self.mode = "time"
        self.streams = streams          # gated mode: the stream of the n-th call of a run (the last one repeats)
        self.reset()
        self.ms = None
        self.n_gate = 1
        self.outputs = {}               # mode -> bit patterns of every Guarded output, in creation order

    def reset(self):
        self.pending, self.guarded, self.gate, self.calls, self.e0 = [], [], None, 0, None

    # -- dev()
    def dev(self, t):
        for src, seed in self.decoys:
            if t is src:
                gen = torch.Generator().manual_seed(seed)
                decoy = (torch.randn(t.shape, generator=gen) * float(t.std())).to(DEV).contiguous()
                if self.mode == "time":
                    decoy.copy_(t.to(DEV))
                elif self.mode == "gated":
                    self.pending.append((decoy, t.to(DEV).contiguous()))
                return decoy
        return t.to(DEV).contiguous()

    # -- Guarded
    def guarded_cls(self):
        runner = self

        class Recorded(Guarded):
            def __init__(self, *shape, fill=None):
                super().__init__(*shape, fill=fill)
                runner.guarded.append(self)
        return Recorded

    # -- _st()
    def st(self):
        if self.mode != "gated":
            if self.e0 is None:
                torch.cuda.synchronize()
                self.e0 = torch.cuda.Event(enable_timing=True)
                self.t0 = time.perf_counter()
                self.e0.record()
            return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        s = self.streams[min(self.calls, len(self.streams) - 1)]
        if self.calls == 0:
            torch.cuda.current_stream().synchronize()       # the struct's buffers are filled: only the gated copies are pending
            self.gate = SU.Gate(s, self.n_gate)
            with torch.cuda.stream(s):
                for buf, true in self.pending:
                    buf.copy_(true, non_blocking=True)
            self.pending = []
        elif s is not self.streams[min(self.calls - 1, len(self.streams) - 1)]:
            s.wait_stream(self.streams[min(self.calls - 1, len(self.streams) - 1)])     # the caller's own duty at the C ABI
        self.calls += 1
        return ctypes.c_void_p(s.cuda_stream)

    # -- _sync()
    def sync(self):
        if self.mode != "gated":
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            host_ms = (time.perf_counter() - self.t0) * 1e3 if self.e0 is not None else 0.0
            torch.cuda.synchronize()
            if self.mode == "time" and self.e0 is not None:
                self.ms = max(self.e0.elapsed_time(e1), host_ms)       # as stream_util.timed: the longer of device and host time
        else:
            assert self.gate is not None
            self.gate.check()
            for s in self.streams:
                s.synchronize()
        self.outputs.setdefault(self.mode, []).extend(g.t.view(torch.int32).clone() for g in self.guarded)
        self.reset()


def _contract(monkeypatch, name, run, modules, decoys, two_streams=False, bit_equal=True, setup=None):
    """run() under the three modes.  modules: the test modules whose dev / Guarded / _st / _sync are replaced; setup(runner): further
    replacements of a test's own."""
    r = _Runner(decoys)
    for mod in modules:
        monkeypatch.setattr(mod, "dev", r.dev)
        monkeypatch.setattr(mod, "Guarded", r.guarded_cls())
        for name_, fn in (("_st", r.st), ("_sync", r.sync)):
            if hasattr(mod, name_):
                monkeypatch.setattr(mod, name_, fn)
    if setup is not None:
        setup(r)
    run()                                               # default stream: the reference outputs and the call's duration
    assert r.ms is not None and r.outputs["time"]
    r.mode = "decoy"
    with pytest.raises(AssertionError, match=r"(norm|max)-relative error .* >= "):      # the decoys miss the float64 bars (no
        run()                                                                            # guard word, no plan bit): the test can fail
    r.mode = "gated"
    r.n_gate = SU.gate_matmuls(r.ms)
    SU.log(name, r.ms, r.n_gate)
    S = torch.cuda.Stream(device=DEV)
    r.streams = [S, torch.cuda.Stream(device=DEV)] if two_streams else [S]
    with torch.cuda.stream(S):
        run()
    a, b = r.outputs["time"], r.outputs["gated"]
    differ = sum(0 if torch.equal(x, y) else 1 for x, y in zip(a, b))
    print("stream-contract %-46s %d of %d buffers differ in bits from the default-stream run" % (name, differ, len(a)))
    if bit_equal:
        assert len(a) == len(b) and differ == 0, "%s: %d of %d buffers differ from the default-stream run" % (name, differ, len(a))


# ------------------------------------------------------------------------------------------------ t2s_taco_decode_steps
def _decode(monkeypatch, lib, c, tag, **kw):
    _contract(monkeypatch, tag, lambda: K._run_decode(lib, c, tag), [K], [(c.memory, 901), (c.pmem, 902)], **kw)


def test_decode_small_serial(monkeypatch, lib):
    """the small autoregressive case: every launch on the caller's stream, no helper stream"""
    c = K._decode_case(K._DSMALL, K._CALLS_SMALL, 3, False, plan=dict(FUSED_ATT=True, Q_PARTS=True, PROJ_FUSED=True, SPLIT=False))
    _decode(monkeypatch, lib, c, "decode_steps[AR small B=3]")


def test_decode_reference_sizes_streamed(monkeypatch, lib):
    """reference sizes, B = 2, the streamed-gate chain"""
    c = K._decode_case(K._DREF, K._CALLS_REF, 2, False, stream=True, mask_steps=4,
                       plan=dict(STREAM_GATES=True, FOLD_PRE2=True, USE_PLOC=True, FUSED_ATT=True, Q_PARTS=True, PROJ_FUSED=True))
    _decode(monkeypatch, lib, c, "decode_steps[ref AR B=2 streamed]")


def test_decode_teacher_forced_helper_stream(monkeypatch, lib):
    """teacher forced with the saves at B = 3: the decoder cells run on the library's helper stream, in chunks of 16 steps"""
    c = K._decode_case(K._DSMALL, K._CALLS_SMALL, 3, True, saves=True, drops=True,
                       plan=dict(SPLIT=True, PACED=False, UNITS_2=True, FUSED_ATT=True))
    _decode(monkeypatch, lib, c, "decode_steps[TF B=3 helper stream]")


def test_two_caller_streams_back_to_back(monkeypatch, lib):
    """calls of 1 and 17 steps of the same decode from streams A and B: B's call spans two chunks of helper work and needs every
    decoder cell A's call left on the helper stream"""
    c = K._decode_case(K._DSMALL, ((0, 1), (1, 17)), 3, True, saves=True, drops=True,
                       plan=dict(SPLIT=True, PACED=False, UNITS_2=True, FUSED_ATT=True))
    _decode(monkeypatch, lib, c, "decode_steps[TF B=3, streams A then B]", two_streams=True)


# -------------------------------------------------------------------------------------------- t2s_taco_decode_steps_w16
@pytest.mark.parametrize("which", ["small", "ref-streamed", "small-streams-A-then-B"])
def test_decode_w16(monkeypatch, lib, which):
    """(the third case: the two calls of the small case, 7 and 11 steps, from caller streams A and B, B waiting for A.  The fp16
    entry point refuses teacher forcing, so it never takes the helper stream: what the case shows is the second call's state
    hand-over across two caller streams)"""
    c = (W._case(K._DREF, K._CALLS_REF, 2, True, mask_steps=4) if which == "ref-streamed" else W._case(K._DSMALL, K._CALLS_SMALL, 3, False))
    tag = "decode_steps_w16[%s]" % which
    _contract(monkeypatch, tag, lambda: W._run_both(lib, c, tag), [W, K], [(c.memory, 903), (c.pmem, 904)],
              two_streams=which.endswith("B"))


# ------------------------------------------------------------------------------------------------- t2s_taco_bptt_steps
@pytest.mark.parametrize("split", [False, True], ids=["one-call", "streams-A-then-B"])
def test_bptt_helper_stream(monkeypatch, lib, split):
    """B = 3, 18 steps (one past the chunk of 16): the decoder-cell chain on the helper stream, the attention chain on the caller's.
    The incoming gradient d_hc is the gated input; the case keeps it on the device, so the struct's pointer is redirected to a
    buffer of the test's own and the shared case stays as it is.  The slot sums are accumulated with atomics: not compared bit
    for bit, only against float64 at the bars of the runner.
    streams-A-then-B: the runner's one call over steps [18, 0) is issued as two, [18, 9) on stream A and [9, 0) on stream B with B
    waiting for A - the carries of step 9 come out of A's call, part of them from the helper stream it joined."""
    c = BW._bptt_case(128, 32, 31, 3, True)

    def setup(r):
        orig = BW._bptt_struct
        real = BW._lib

        def struct(case, form):
            bp, o, xbuf = orig(case, form)
            o.gated_d_hc = r.dev(c.d_hc)        # (kept alive with the outputs)
            bp.d_hc = BW._p(o.gated_d_hc)
            if not split:
                r.st()                          # the runner calls the entry point next, on the current stream: the gate goes in here
            return bp, o, xbuf
        monkeypatch.setattr(BW, "_bptt_struct", struct)
        if split:
            class TwoCalls:
                def __getattr__(self, name):
                    return getattr(real, name)

                @staticmethod
                def call(name, *args):
                    if name != "t2s_taco_bptt_steps":
                        return real.call(name, *args)
                    bp, t_hi, t_lo, _ = args
                    mid = (t_hi + t_lo) // 2
                    real.call(name, bp, t_hi, mid, r.st())      # r.st(): the gate before the first call, then stream A; B for the
                    return real.call(name, bp, mid, t_lo, r.st())   # second, after B.wait_stream(A)
            monkeypatch.setattr(BW, "_lib", TwoCalls())

    _contract(monkeypatch, "bptt_steps[B=3 fold%s]" % (", streams A then B" if split else ""), lambda: BW._run_bptt(c, "fold"), [BW],
              [(c.d_hc, 905)], bit_equal=False, setup=setup, two_streams=split)
