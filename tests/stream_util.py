"""Helpers of the stream-contract tests: a bounded delay on a stream, and inputs that become true only
behind it.

A gate is ordinary torch work - a chain of fp32 matmuls of one fixed size - whose length in milliseconds is turned into a number of
matmuls by one calibration per process (timed with events).  Nothing here spins on a flag or waits for the host: a gate drains by
itself, and a test whose gate had drained too early FAILS ("gate too short"), it neither passes nor skips."""
import functools
import math

import torch

GATE_N = 4096               # the matmul: [GATE_N, GATE_N] x [GATE_N, GATE_N] in fp32, 137 GFLOP
GATE_FACTOR = 5.0           # gate length over the duration of the call under test: covers enqueue-time jitter on a shared host
GATE_CAP_MS = 500.0         # per test
LOG = []                    # (test, call ms, gate ms, matmuls): printed by the tests, tabulated in profiles/stream_contract_tests.md


@functools.lru_cache(maxsize=None)
def matmul_ms(device="cuda:0"):
    """Milliseconds of one gate matmul on an idle device, measured once: the mean over a chain of 8 after a warm-up of 2."""
    a = torch.eye(GATE_N, device=device).roll(1, 0)         # a permutation: the chain's values stay what they are
    x = torch.ones(GATE_N, GATE_N, device=device)
    y = torch.empty_like(x)
    for _ in range(2):
        torch.mm(x, a, out=y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        torch.mm(x, a, out=y)
        torch.mm(y, a, out=x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 8


def gate_matmuls(call_ms, device="cuda:0"):
    """Matmuls of a gate for a call that took call_ms: GATE_FACTOR times as long, one at least, GATE_CAP_MS at most."""
    per = matmul_ms(device)
    return max(1, min(int(math.ceil(GATE_FACTOR * call_ms / per)), int(GATE_CAP_MS / per)))


class Gate:
    """n matmuls enqueued on `stream`, then the event `done`.  The operands are the gate's own, allocated on that stream."""

    def __init__(self, stream, n):
        self.stream, self.n = stream, int(n)
        with torch.cuda.stream(stream):
            a = torch.eye(GATE_N, device=stream.device).roll(1, 0)
            x = torch.ones(GATE_N, GATE_N, device=stream.device)
            y = torch.empty_like(x)
            for _ in range(self.n):
                torch.mm(x, a, out=y)
                x, y = y, x
            self.keep = (a, x, y)
            self.done = torch.cuda.Event()
            self.done.record(stream)

    def still_running(self):
        return not self.done.query()

    def check(self):
        assert self.still_running(), "gate too short: its %d matmuls (%.2f ms each) had drained" % (self.n, matmul_ms())


def behind_gate(stream, buf, true_value, n):
    """A gate of n matmuls on `stream`, then buf.copy_(true_value) on it: whoever reads `buf` without waiting for everything
    enqueued on `stream` so far finds the decoy it held before.  true_value lives on the device (the copy must not block the host).
    buf and true_value may be lists of tensors (a model's parameters)."""
    bufs, values = (buf, true_value) if isinstance(buf, (list, tuple)) else ([buf], [true_value])
    assert len(bufs) == len(values) and all(b.is_cuda and v.is_cuda for b, v in zip(bufs, values))
    gate = Gate(stream, n)
    with torch.cuda.stream(stream):
        for b, v in zip(bufs, values):
            b.copy_(v, non_blocking=True)
    return gate


def timed(fn):
    """(fn(), its duration in milliseconds) on the current stream, synchronised: the time between events around it or the host's
    time to issue it, whichever is longer - a gate has to outlast the enqueueing of the call, and a call of a few launches is
    over on the device before the host has returned from it."""
    import time
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return out, max(e0.elapsed_time(e1), host_ms)


def log(test, call_ms, n):
    row = (test, call_ms, n * matmul_ms(), n)
    LOG.append(row)
    print("stream-contract %-46s call %8.3f ms   gate %8.3f ms (%d matmuls of %.3f ms)" % (row + (matmul_ms(),)))
