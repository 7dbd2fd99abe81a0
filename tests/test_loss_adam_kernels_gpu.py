"""t2s_taco_loss, t2s_waveglow_loss (csrc/loss_ops.hip) and t2s_adam_table (csrc/train_ops.hip) called directly through the C ABI and
compared element by element with float64 on the same f32 operands (tests/tail_ref_util.py, pinned by tests/test_tail_ref_util_cpu.py).
Every output and scratch buffer is guarded, the reduction scratch is poisoned with NaN, and every bound comes from the arithmetic (the
losses) or from 4 x a float32 numpy emulation of the kernel's formula (Adam); the figures are in profiles/tail_kernel_tests.md."""
import ctypes

import numpy as np
import pytest
import torch

import tail_ref_util as R
from text2speech_amd import _lib
from wg_bwd_util import DEV, Guarded, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
S = R.GRID_STRIDE


def _st():
    return _lib.current_stream()


def _p(t):
    return _lib.ptr(t.t if isinstance(t, Guarded) else t)


def _bits(t):
    return (t.t if isinstance(t, Guarded) else t).view(torch.int32).clone()


def _partial(n_doubles, poison=None):
    """Guarded scratch of doubles: NaN everywhere (the sentinel twice is a NaN double too), or `poison`."""
    g = Guarded(2 * n_doubles)
    if poison is not None:
        g.t.view(torch.float64).fill_(poison)
    return g


def _elementwise(label, got, want, bound):
    got, want = R.f64(got).flatten(), R.f64(want).flatten()
    bound = torch.as_tensor(bound, dtype=torch.float64).flatten().expand_as(want)
    assert bool(torch.isfinite(got).all()), "%s: an element is not finite (never written?)" % label
    ratio = ((got - want).abs() / bound).max()
    print("PARITY %-58s worst |err| %.3e  worst err / bound %.3f" % (label, float((got - want).abs().max()), float(ratio)))
    assert float(ratio) <= 1.0, "%s: element-wise error is %.3f x its bound" % (label, float(ratio))


# ---------------------------------------------------------------------------------------------------------------------------------
def _taco_inputs(n_mel, n_gate, soft, seed):
    gen = torch.Generator().manual_seed(seed)
    mel, post, target = [torch.randn(n_mel, generator=gen) for _ in range(3)]
    gate = torch.rand(n_gate, generator=gen) * 6 - 3
    plant = torch.tensor([0.0, -0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4])[:n_gate]
    at = max(0, n_gate // 2 - 4) if n_gate > 8 else 0
    gate[at:at + plant.numel()] = plant
    gate_t = torch.full((n_gate,), 0.3) if soft else (torch.rand(n_gate, generator=gen) > 0.5).float()
    return mel, post, target, gate, gate_t, at


def _taco_call(ins, n_mel, n_gate, want=(True, True, True), poison=None):
    d = [Guarded(n) if w else None for n, w in zip((n_mel, n_mel, n_gate), want)]
    partial, out = _partial(256 * 3, poison), Guarded(3)
    mel, post, target, gate, gate_t = ins
    _lib.call("t2s_taco_loss", _p(mel), _p(post), _p(target), n_mel, _p(gate), _p(gate_t), n_gate,
              *[_p(g) if g is not None else None for g in d], _p(partial), _p(out), _st())
    torch.cuda.synchronize()
    for g, name in zip(d + [partial, out], ("d_mel", "d_post", "d_gate", "partial", "out")):
        if g is not None:
            g.assert_guards(name)
    assert bool(torch.isfinite(partial.t.view(torch.float64)).all()), "partial: a slot was not overwritten"
    return d, out


@pytest.mark.parametrize("n_mel,n_gate,soft", [(1, 37, False), (255, 1, True), (S, S + 1, False), (S + 1, 37, True),
                                               (3 * S + 17, S + 1, True)])
def test_taco_loss(n_mel, n_gate, soft):
    """Element counts below, at and above one grid stride (256 x 256), n_gate on either side of n_mel; gate logits +-3 with +-0, +-20,
    +-90 and +-1e4 planted (expf overflows at the last two: the gradient must come out finite, (0 or 1) - y over n_gate)."""
    _lib.load()
    cpu = _taco_inputs(n_mel, n_gate, soft, 11 * n_mel + n_gate)
    at = cpu[5]
    ins = [dev(t) for t in cpu[:5]]
    want_out, *want_d = R.taco_loss_ref(*cpu[:5])
    b = R.taco_loss_bounds(*cpu[:5])
    tag = "taco_loss n_mel %d n_gate %d %s" % (n_mel, n_gate, "soft" if soft else "0/1")
    d, out = _taco_call(ins, n_mel, n_gate)
    _elementwise(tag + " out[0..2]", out.t, want_out, b["out"])
    for g, w, key in zip(d, want_d, ("d_mel", "d_post", "d_gate")):
        _elementwise(tag + " " + key, g.t, w, b[key])
    if n_gate > 8:      # the overflowing logits: exactly the saturated sigmoid
        x, y = cpu[3][at + 6:at + 8], cpu[4][at + 6:at + 8]
        sat = ((x > 0).float() - y) * float(np.float32(1.0) / np.float32(n_gate))
        assert torch.equal(d[2].t[at + 6:at + 8].cpu(), sat)
    # each gradient pointer NULL in turn: the other two and the loss are bitwise the same
    full = [_bits(g) for g in d] + [_bits(out)]
    for skip in range(3):
        d2, out2 = _taco_call(ins, n_mel, n_gate, want=tuple(i != skip for i in range(3)))
        for i in range(3):
            if i != skip:
                assert torch.equal(_bits(d2[i]), full[i]), (skip, i)
        assert torch.equal(_bits(out2), full[3]), skip
    # the scratch is write-only: another poison, the same bits
    d3, out3 = _taco_call(ins, n_mel, n_gate, poison=1e300)
    assert all(torch.equal(_bits(g), f) for g, f in zip(d3 + [out3], full))


def _wg_call(z, log_s, log_det, sigma, with_dz, poison=None):
    n = len(log_s)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in log_s])
    sizes = (ctypes.c_size_t * max(n, 1))(*[t.numel() for t in log_s])
    d_z = Guarded(z.numel()) if with_dz else None
    partial, out = _partial(256 * 2, poison), Guarded(1)
    _lib.call("t2s_waveglow_loss", _p(z), z.numel(), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(sizes, ctypes.c_void_p), n,
              _p(log_det), sigma, _p(d_z) if with_dz else None, _p(partial), _p(out), _st())
    torch.cuda.synchronize()
    for g, name in ((d_z, "d_z"), (partial, "partial"), (out, "out")):
        if g is not None:
            g.assert_guards(name)
    assert bool(torch.isfinite(partial.t.view(torch.float64)).all()), "partial: a slot was not overwritten"
    return d_z, out


@pytest.mark.parametrize("n_flows,n_z,sigma", [(1, 255, 1.0), (12, 2 * S + 5, 0.6), (16, S + 1, 0.6), (16, S, 1.0)])
def test_waveglow_loss(n_flows, n_z, sigma):
    """1, 12 and 16 log_s tensors of different sizes in one call (1 and 65537 elements among them), negative log_det, two sigmas, with
    and without d_z.  The value is a difference of three sums: its error is bounded against their size, not against |loss|."""
    _lib.load()
    gen = torch.Generator().manual_seed(100 * n_flows + int(10 * sigma))
    sizes = ([S + 1] if n_flows == 1 else [1, S + 1, 255, S, 1000, 2 * S + 3, 37, 1, 4096, 511, 3, S - 1, 17, 2, S + 255, 129][:n_flows])
    z = torch.randn(n_z, generator=gen) * 1.3
    log_s = [torch.randn(n, generator=gen) * 0.4 - 0.05 for n in sizes]
    log_det = torch.randn(n_flows, generator=gen) * 300.0 - 50.0
    log_det[0] = -log_det[0].abs() - 1.0
    want, want_dz, scale = R.waveglow_loss_ref(z, log_s, log_det, sigma)
    b_loss, b_dz = R.waveglow_loss_bounds(scale, want_dz)
    zd, lsd, ldd = dev(z), [dev(t) for t in log_s], dev(log_det)
    tag = "waveglow_loss flows %d n_z %d sigma %.1f" % (n_flows, n_z, sigma)
    d_z, out = _wg_call(zd, lsd, ldd, sigma, True)
    print("       %s: loss %.6e, size of the three sums %.6e" % (tag, want, scale))
    _elementwise(tag + " out", out.t, [want], [b_loss])
    _elementwise(tag + " d_z", d_z.t, want_dz, b_dz)
    _, out2 = _wg_call(zd, lsd, ldd, sigma, False, poison=-1e300)
    assert torch.equal(_bits(out2), _bits(out))


def test_loss_refusals():
    """T2S_EINVAL and nothing written: n_flows 0 / 17, a NULL log_s entry, sigma 0 / negative / NaN, zero element counts, NULL required
    pointers."""
    lib = _lib.load()
    n = 64
    z, ld = torch.ones(n, device=DEV), torch.ones(17, device=DEV)
    ls = [torch.ones(8, device=DEV) for _ in range(17)]
    outs = [Guarded(n), _partial(512), Guarded(1)]
    before = [_bits(g) for g in outs]

    def wg(zz=z, n_z=n, k=2, null_at=None, lsp=True, szp=True, ldp=ld, sigma=1.0, partial=outs[1], out=outs[2]):
        ptrs = (ctypes.c_void_p * 17)(*[None if i == null_at else t.data_ptr() for i, t in enumerate(ls)])
        sizes = (ctypes.c_size_t * 17)(*[8] * 17)
        return lib.t2s_waveglow_loss(_p(zz) if zz is not None else None, n_z, ctypes.cast(ptrs, ctypes.c_void_p) if lsp else None,
                                     ctypes.cast(sizes, ctypes.c_void_p) if szp else None, k, _p(ldp) if ldp is not None else None,
                                     sigma, _p(outs[0]), _p(partial) if partial is not None else None,
                                     _p(out) if out is not None else None, _st())

    for kw in (dict(k=0), dict(k=17), dict(k=-1), dict(null_at=1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(n_z=0), dict(zz=None), dict(lsp=False), dict(szp=False), dict(ldp=None), dict(partial=None), dict(out=None)):
        assert wg(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for g, b in zip(outs, before):
        assert torch.equal(_bits(g), b), "a refused call wrote"
    assert wg(k=16) == 0                                     # the same call is accepted at the limit
    torch.cuda.synchronize()
    assert not torch.equal(_bits(outs[2]), before[2])
    outs = [Guarded(n), _partial(768), Guarded(3), Guarded(n), Guarded(n)]
    before = [_bits(g) for g in outs]
    ins = [torch.ones(n, device=DEV) for _ in range(5)]

    def taco(null_at=None, n_mel=n, n_gate=n, partial=outs[1], out=outs[2]):
        a = [None if i == null_at else _p(t) for i, t in enumerate(ins)]
        return lib.t2s_taco_loss(a[0], a[1], a[2], n_mel, a[3], a[4], n_gate, _p(outs[0]), _p(outs[3]), _p(outs[4]),
                                 _p(partial) if partial is not None else None, _p(out) if out is not None else None, _st())

    for kw in [dict(null_at=i) for i in range(5)] + [dict(n_mel=0), dict(n_gate=0), dict(partial=None), dict(out=None)]:
        assert taco(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for g, b in zip(outs, before):
        assert torch.equal(_bits(g), b), "a refused call wrote"
        g.assert_guards()


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
class _Job:
    def __init__(self, state):
        self.cpu = state                                           # f32 numpy (p, g, m, v)
        n = state[0].size
        self.n = n
        self.p, self.g, self.m, self.v = [Guarded(n, fill=torch.from_numpy(a)) for a in state]

    def read(self):
        return [t.t.cpu().numpy().copy() for t in (self.p, self.m, self.v)]

    def assert_guards(self, label):
        for t, name in ((self.p, "p"), (self.g, "g"), (self.m, "m"), (self.v, "v")):
            t.assert_guards("%s %s" % (label, name))


def _table(jobs):
    rows, blk = [], 0
    for j in jobs:
        rows.append([j.p.t.data_ptr(), j.g.t.data_ptr(), j.m.t.data_ptr(), j.v.t.data_ptr(), j.n, blk])
        blk += -(-j.n // 1024)
    return torch.tensor(rows, dtype=torch.int64).to(DEV), blk


def _adam(jobs, step, lr=R.ADAM_LR, betas=(0.9, 0.999), eps=1e-8, gscale=1.0, wd=0.0):
    table, blocks = _table(jobs)
    _lib.call("t2s_adam_table", _p(table), len(jobs), blocks, lr, betas[0], betas[1], eps, step, gscale, wd, _st())
    torch.cuda.synchronize()


def _adam_errors(job, before, hyper, label):
    """Worst element-wise relative error of (step, m, v) of one job against float64, and of the float32 emulation on the same state."""
    p0, g, m0, v0 = before
    p1, m1, v1 = job.read()
    job.assert_guards(label)
    ds, mr, vr = R.adam_ref(p0, g, m0, v0, *hyper)
    pe, me, ve = R.adam_emulate_f32(p0, g, m0, v0, *hyper)
    got = [float(R.relerr(p1.astype(np.float64) - p0.astype(np.float64), ds).max()), float(R.relerr(m1, mr).max()),
           float(R.relerr(v1, vr).max())]
    emu = [float(R.relerr(pe.astype(np.float64) - p0.astype(np.float64), ds).max()), float(R.relerr(me, mr).max()),
           float(R.relerr(ve, vr).max())]
    assert np.isfinite(p1).all() and np.isfinite(m1).all() and np.isfinite(v1).all(), label
    return got, emu


GEOMETRY = {"six": [1, 1023, 1024, 1025, 4097, 3], "six-reversed": [3, 4097, 1025, 1024, 1023, 1], "single": [4097], "33-of-1": [1] * 33}
GEOMETRY_HYPER = (R.ADAM_LR, 0.9, 0.999, 1e-8, 3, 1.0, 0.0)
_geometry_floor = []


def _geometry_states(name):
    return [R.adam_state(n, 3, 0.0, seed=50 + i, p_scale=R.ADAM_LR) for i, n in enumerate(GEOMETRY[name])]


def _geometry_emulation_floor():
    """Worst (step, m, v) error of the float32 emulation over the jobs of all four tables (33 one-element jobs alone are too few
    elements to give a worst case)."""
    if not _geometry_floor:
        worst = np.zeros(3)
        for name in GEOMETRY:
            for p, g, m, v in _geometry_states(name):
                ds, mr, vr = R.adam_ref(p, g, m, v, *GEOMETRY_HYPER)
                pe, me, ve = R.adam_emulate_f32(p, g, m, v, *GEOMETRY_HYPER)
                worst = np.maximum(worst, [R.relerr(pe.astype(np.float64) - p.astype(np.float64), ds).max(), R.relerr(me, mr).max(),
                                           R.relerr(ve, vr).max()])
        _geometry_floor.append(worst)
    return _geometry_floor[0]


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_adam_table_geometry(name):
    """Hand-built job tables: sizes either side of the 1024-element block in both orders, one job, and 33 one-element jobs (every block
    another job, so the binary search ends at every depth).  p, g, m, v of every job are separate guarded buffers: nothing past n is
    touched.  Step 3 from non-zero state, |p| <= lr; bound = 4 x the float32 emulation's worst error over these tables' jobs."""
    _lib.load()
    floor = _geometry_emulation_floor()
    jobs = [_Job(s) for s in _geometry_states(name)]
    _adam(jobs, 3)
    res = [_adam_errors(j, j.cpu, GEOMETRY_HYPER, "job %d (n %d)" % (i, j.n))[0] for i, j in enumerate(jobs)]
    got = np.array(res).max(axis=0)
    for k, what in enumerate(("step", "m", "v")):
        print("PARITY adam_table geometry %-13s %-4s device %.3e  emulation floor %.3e  bound %.3e" % (name, what, got[k], floor[k], 4 * floor[k]))
        assert got[k] <= 4 * floor[k], (what, got[k], floor[k])


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adam_table_arithmetic(step, weight_decay):
    """Steps 1 .. 100000 x two beta pairs x two eps x gscale 1 / 0.5, without and with weight decay: m, v and the step p_new - p_old
    element by element against float64 Adam on the f32 hyper-parameters.  Parameters start at zero (at 1e-2 with weight decay), so the
    subtraction does not swallow the step.  Bound: 4 x the worst error of the float32 emulation (bias corrections in double) over the
    whole grid - 1.4e-6 on the step without weight decay.  With the bias corrections in float (powf), as t2s_adam_table had them, the
    emulation is off by 3.6e-6 at step 2, beta2 = 0.999, and so was the device (profiles/tail_kernel_tests.md)."""
    _lib.load()
    floor = R.adam_emulation_floor(weight_decay)
    worst = np.zeros(3)
    for case in R.adam_cases():
        if case[0] != step:
            continue
        _, betas, eps, gs, seed = case
        job = _Job(R.adam_state(R.ADAM_N, step, weight_decay, seed))
        _adam([job], step, betas=betas, eps=eps, gscale=gs, wd=weight_decay)
        got, _ = _adam_errors(job, job.cpu, (R.ADAM_LR, betas[0], betas[1], eps, step, gs, weight_decay), str(case))
        print("PARITY adam_table step %6d betas %s eps %.0e gscale %.1f wd %.1f: step %.3e  m %.3e  v %.3e" %
              (step, betas, eps, gs, weight_decay, *got))
        worst = np.maximum(worst, got)
    for k, name in enumerate(("step", "m", "v")):
        print("PARITY adam_table step %6d wd %.1f worst %-4s %.3e  emulation floor %.3e  bound %.3e" %
              (step, weight_decay, name, worst[k], floor[k], 4 * floor[k]))
    for k, name in enumerate(("step", "m", "v")):
        assert worst[k] <= 4 * floor[k], "%s: %.3e > 4 x %.3e" % (name, worst[k], floor[k])


def test_adam_table_five_consecutive_steps():
    """Steps 1 .. 5 with the state carried on the device, against float64 carried on its own from the same start, and the float32
    emulation carried on its own for the bound (4 x its worst error at the same call).  The gradient of an element keeps its sign from
    call to call, so the first moment does not cancel."""
    _lib.load()
    n = 3000
    p0, g0, _, _ = R.adam_state(n, 1, 0.0, seed=9)
    job = _Job([p0, g0, np.zeros(n, np.float32), np.zeros(n, np.float32)])
    r = np.random.RandomState(10)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    pe, me, ve = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    prev = p0.copy()
    for step in range(1, 6):
        g = (g0 * (0.5 + r.uniform(size=n))).astype(np.float32)
        job.g.t.copy_(torch.from_numpy(g))
        _adam([job], step)
        p1, m1, v1 = job.read()
        job.assert_guards("call %d" % step)
        ds, m64, v64 = R.adam_ref(p64, g, m64, v64, R.ADAM_LR, 0.9, 0.999, 1e-8, step)
        p64 = p64 + ds
        pe_new, me, ve = R.adam_emulate_f32(pe, g, me, ve, R.ADAM_LR, 0.9, 0.999, 1e-8, step)
        emu = [float(R.relerr(pe_new.astype(np.float64) - pe.astype(np.float64), ds).max()), float(R.relerr(me, m64).max()),
               float(R.relerr(ve, v64).max())]
        got = [float(R.relerr(p1.astype(np.float64) - prev.astype(np.float64), ds).max()), float(R.relerr(m1, m64).max()),
               float(R.relerr(v1, v64).max())]
        pe, prev = pe_new, p1
        print("PARITY adam_table call %d of 5: step %.3e (emulation %.3e)  m %.3e (%.3e)  v %.3e (%.3e)" %
              (step, got[0], emu[0], got[1], emu[1], got[2], emu[2]))
        for k, name in enumerate(("step", "m", "v")):
            assert got[k] <= 4 * emu[k], (step, name, got[k], emu[k])


def test_adam_table_refusals():
    lib = _lib.load()
    job = _Job(R.adam_state(100, 2, 0.0, seed=1))
    table, blocks = _table([job])
    before = [_bits(t) for t in (job.p, job.m, job.v)]

    def call(tab=table, n_jobs=1, total=blocks, step=1):
        return lib.t2s_adam_table(_p(tab) if tab is not None else None, n_jobs, total, 1e-3, 0.9, 0.999, 1e-8, step, 1.0, 0.0, _st())

    for kw in (dict(step=0), dict(step=-1), dict(n_jobs=0), dict(total=0), dict(tab=None)):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t), b) for t, b in zip((job.p, job.m, job.v), before)), "a refused call wrote"
    job.assert_guards("refusals")
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(_bits(job.p), before[0])
