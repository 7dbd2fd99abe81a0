"""t2s_grad_norm_table, t2s_grad_scale_table and t2s_adam_table_clip (csrc/train_ops.hip) called directly through the C ABI on hand-built
job tables and compared with the float64 references of tests/grad_norm_ref.py (pinned by tests/test_grad_norm_ref_cpu.py).  Every device
buffer is guarded, the reduction scratch is poisoned with NaN, and the guards are checked after every call.  Bounds (H = 2^-24):
the norm 2 H relative - the squares are exact in double, the double sum of n terms is off by at most n 2^-53 (< 1e-9 here), root and
gscale product are in double, then one f32 rounding; the coefficient bit for bit from the device's norm; the clipped Adam step 4 x the
float32 emulation's own error, as tests/test_loss_adam_kernels_gpu.py has it.  The figures are in profiles/grad_norm_tests.md."""
import math

import numpy as np
import pytest
import torch

import grad_norm_ref as G
import tail_ref_util as R
from text2speech_amd import _lib
from wg_bwd_util import DEV, Guarded

pytestmark = pytest.mark.gpu
H = G.H


def _st():
    return _lib.current_stream()


def _nb():
    return _lib.load().t2s_grad_norm_partials()


class _Grads:
    """One guarded device buffer per gradient array; offset 1: every gradient starts one float into its buffer (4 bytes off the
    16-byte alignment), the float in front of it keeps the sentinel."""

    def __init__(self, arrays, offset=0):
        self.cpu = [np.asarray(a, dtype=np.float32) for a in arrays]
        self.offset = offset
        self.bufs = [Guarded(a.size + offset) for a in self.cpu]
        self.t = [b.t[offset:] for b in self.bufs]
        for t, a in zip(self.t, self.cpu):
            t.copy_(torch.tensor(a))
        rows, blk = [], 0
        for t in self.t:
            rows.append([0, t.data_ptr(), 0, 0, t.numel(), blk])
            blk += -(-t.numel() // 1024)
        self.table, self.n, self.blocks = torch.tensor(rows, dtype=torch.int64).to(DEV), len(rows), blk

    def read(self):
        return [t.cpu().numpy().copy() for t in self.t]

    def assert_guards(self, label):
        for i, b in enumerate(self.bufs):
            b.assert_guards("%s gradient %d" % (label, i))
            if self.offset:
                assert bool(b.untouched(b.t[:self.offset]).all()), "%s: wrote in front of gradient %d" % (label, i)


def _norm(gr, gscale=1.0, max_norm=1.0):
    """One t2s_grad_norm_table call into fresh guarded buffers: (out[4] as numpy f32, partial as numpy f64 bits, the out buffer)."""
    partial, out = Guarded(2 * _nb()), Guarded(4)
    partial.t.view(torch.float64).fill_(float("nan"))                  # (the f32 sentinel twice is a finite double)
    _lib.call("t2s_grad_norm_table", _lib.ptr(gr.table), gr.n, gr.blocks, gscale, max_norm, _lib.ptr(partial.t), _lib.ptr(out.t), _st())
    torch.cuda.synchronize()
    partial.assert_guards("partial")
    out.assert_guards("out")
    gr.assert_guards("norm")
    return out.t.cpu().numpy().copy(), partial.t.view(torch.int64).cpu().numpy().copy(), out


def _clip_buffer(values):
    c = Guarded(4)
    c.t.copy_(torch.tensor(values, dtype=torch.float32))
    return c


def _sizes():
    return {"one": (1,), "around-a-block": (1023, 1, 1025), "whole-blocks": (1024, 2049, 3), "wraps-the-grid": (1024 * _nb() + 1, 5)}


GEOMETRY = ["one", "around-a-block", "whole-blocks", "wraps-the-grid"]
_cache = {}


def _geometry(name):
    """The gradient arrays of one table (tail_ref_util.adam_state: magnitudes 1e-6 .. 1e3, exact zeros) and their float64 norm, once."""
    if name not in _cache:
        arrays = [R.adam_state(n, 1, 0.0, seed=300 + 7 * i + len(name))[1] for i, n in enumerate(_sizes()[name])]
        for a in arrays:
            a.setflags(write=False)
        _cache[name] = (arrays, G.norm_ref(arrays))
    return _cache[name]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off-by-one-float"])
@pytest.mark.parametrize("name", GEOMETRY)
def test_grad_norm_geometry(name, offset):
    """Job sizes either side of the 1024-element table block, whole blocks (the float4 path when aligned), and more table blocks than
    workgroups (the grid stride wraps); every gradient 16-byte aligned, or one float off (scalar path for every block)."""
    _lib.load()
    arrays, want = _geometry(name)
    gr = _Grads(arrays, offset)
    max_norm = float(np.float32(0.25 * want))               # clips to about a quarter, whatever the table's norm
    out, partial, _ = _norm(gr, 1.0, max_norm)
    err = abs(float(out[0]) - want) / want
    print("PARITY grad_norm %-15s offset %d: norm %.9e  float64 %.9e  err %.3f H (bound 2 H)" % (name, offset, out[0], want, err / H))
    assert err <= 2 * H
    assert out[1].tobytes() == G.clip_coef_f32(out[0], max_norm).tobytes(), (out, G.clip_coef_f32(out[0], max_norm))
    assert 0.2 < out[1] < 0.3 and out[2] == 0.0 and out[3] == 0.0
    assert not np.isnan(partial.view(np.float64)).any(), "partial: a slot was not overwritten"
    if gr.blocks < _nb():
        assert (partial[gr.blocks:] == 0).all(), "a workgroup without a table block must write +0.0"
    # the same data, the same bits
    out2, partial2, _ = _norm(gr, 1.0, max_norm)
    assert out2.tobytes() == out.tobytes() and partial2.tobytes() == partial.tobytes()
    # gscale 0.5 halves the norm; max_norm = +inf reports only
    out3, partial3, _ = _norm(gr, 0.5, math.inf)
    assert partial3.tobytes() == partial.tobytes()
    assert abs(float(out3[0]) - 0.5 * want) <= 2 * H * 0.5 * want
    assert out3[0] == np.float32(0.5) * out[0]          # halving is exact
    assert out3[1].tobytes() == np.float32(1.0).tobytes() and out3[2] == 0.0 and out3[3] == 0.0
    assert all(np.array_equal(a, b) for a, b in zip(gr.read(), arrays)), "the norm pass wrote a gradient"


def _value_case(arrays, max_norm=1.0):
    gr = _Grads(arrays)
    out, partial, _ = _norm(gr, 1.0, max_norm)
    assert not np.isnan(partial.view(np.float64)[gr.blocks:]).any()
    return out


def test_grad_norm_values():
    """Zeros, an overflowing norm, and a NaN at either end of the table."""
    _lib.load()
    out = _value_case([np.zeros(1025, np.float32), np.zeros(3, np.float32)])
    assert out[0] == 0.0 and out[1].tobytes() == np.float32(1.0).tobytes() and out[2] == 0.0 and out[3] == 0.0
    big = np.zeros(2049, np.float32)
    big[[5, 2048]] = 3e38                                    # sqrt(2) x 3e38 > the largest f32; the double sum does not overflow
    out = _value_case([big])
    assert np.isposinf(out[0]) and out[1] == 0.0 and out[2] == 1.0 and out[3] == 0.0
    out = _value_case([big], max_norm=math.inf)
    assert np.isposinf(out[0]) and np.isnan(out[1]) and out[2] == 1.0         # inf / inf, as torch has it
    sizes = (1024, 2049, 3)
    for where in ("first", "last"):
        arrays = [R.adam_state(n, 1, 0.0, seed=40 + i)[1] for i, n in enumerate(sizes)]
        if where == "first":
            arrays[0][0] = np.nan
        else:
            arrays[-1][-1] = np.nan
        out = _value_case(arrays)
        # (the formula on a NaN norm is a NaN; which NaN an operation produces is not specified, so it is not compared by bits)
        assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 1.0 and out[3] == 0.0, (where, out)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off-by-one-float"])
@pytest.mark.parametrize("name", GEOMETRY)
def test_grad_scale_table(name, offset):
    """g *= clip[1] with the coefficient the norm pass left on the device: every element is fl32(g * coef) exactly, nothing outside the
    gradients is written; then a coefficient of exactly 1 keeps every bit."""
    _lib.load()
    arrays, want = _geometry(name)
    gr = _Grads(arrays, offset)
    out, _, clip = _norm(gr, 1.0, float(np.float32(0.25 * want)))
    coef = out[1]
    assert 0.2 < coef < 0.3
    _lib.call("t2s_grad_scale_table", _lib.ptr(gr.table), gr.n, gr.blocks, _lib.ptr(clip.t), _st())
    torch.cuda.synchronize()
    gr.assert_guards("scale")
    clip.assert_guards("clip")
    assert clip.t.cpu().numpy().tobytes() == out.tobytes(), "the scale pass wrote its coefficient buffer"
    got = gr.read()
    for i, (a, b) in enumerate(zip(got, arrays)):
        assert a.tobytes() == (b * coef).astype(np.float32).tobytes(), "job %d" % i
    one = _clip_buffer([123.0, 1.0, 0.0, 0.0])
    _lib.call("t2s_grad_scale_table", _lib.ptr(gr.table), gr.n, gr.blocks, _lib.ptr(one.t), _st())
    torch.cuda.synchronize()
    gr.assert_guards("scale by 1")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gr.read(), got))


# ---------------------------------------------------------------------------------------------------------------------------------
# t2s_adam_table_clip
class _Job:
    def __init__(self, state):
        self.cpu = state                                           # f32 numpy (p, g, m, v)
        self.n = state[0].size
        self.p, self.g, self.m, self.v = [Guarded(self.n, fill=torch.from_numpy(a)) for a in state]
        rows = [[self.p.t.data_ptr(), self.g.t.data_ptr(), self.m.t.data_ptr(), self.v.t.data_ptr(), self.n, 0]]
        self.table, self.blocks = torch.tensor(rows, dtype=torch.int64).to(DEV), -(-self.n // 1024)

    def read(self):
        torch.cuda.synchronize()
        for t, name in ((self.p, "p"), (self.g, "g"), (self.m, "m"), (self.v, "v")):
            t.assert_guards(name)
        return [t.t.cpu().numpy().copy() for t in (self.p, self.m, self.v)]

    def adam(self, step, gscale=1.0, wd=0.0, clip=None, skip=0, betas=(0.9, 0.999), eps=1e-8):
        args = (_lib.ptr(self.table), 1, self.blocks, R.ADAM_LR, betas[0], betas[1], eps, step, gscale, wd)
        if clip is None:
            _lib.call("t2s_adam_table", *args, _st())
        else:
            _lib.call("t2s_adam_table_clip", *args, _lib.ptr(clip.t), skip, _st())
        return self.read()


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_table_clip_coefficient_one_is_adam_table(step, weight_decay):
    """(a) clip = [x, 1, 0, 0]: the same bits as t2s_adam_table on copies of the same state, n = 2049, gscale 1 and 0.5."""
    _lib.load()
    for gscale in (1.0, 0.5):
        state = R.adam_state(R.ADAM_N, step, weight_decay, seed=600 + step)
        want = _Job(state).adam(step, gscale, weight_decay)
        clip = _clip_buffer([7.5, 1.0, 0.0, 0.0])
        got = _Job(state).adam(step, gscale, weight_decay, clip=clip, skip=1)
        clip.assert_guards("clip")
        for a, b, name in zip(got, want, "pmv"):
            assert a.tobytes() == b.tobytes(), (name, gscale)
        assert not np.array_equal(got[0], state[0])


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_table_clip_is_scale_then_adam_table(step):
    """(b) gscale 1, coefficient 0.37: the same bits as t2s_grad_scale_table followed by t2s_adam_table.  Without weight decay: with it
    the compiler may contract g * coef + wd * p into one fused multiply-add, which the two-launch sequence, whose g * coef is rounded
    into memory, cannot reproduce (case (c) covers weight decay against float64)."""
    _lib.load()
    state = R.adam_state(R.ADAM_N, step, 0.0, seed=610 + step)
    clip = _clip_buffer([2.7, 0.37, 0.0, 0.0])
    got = _Job(state).adam(step, 1.0, 0.0, clip=clip)
    two = _Job(state)
    _lib.call("t2s_grad_scale_table", _lib.ptr(two.table), 1, two.blocks, _lib.ptr(clip.t), _st())
    want = two.adam(step, 1.0, 0.0)
    assert two.g.t.cpu().numpy().tobytes() == (state[1] * np.float32(0.37)).astype(np.float32).tobytes()
    for a, b, name in zip(got, want, "pmv"):
        assert a.tobytes() == b.tobytes(), name


CLIP_CASES = [(step, gscale, coef) for step in (1, 1000) for gscale, coef in ((1.0, 0.37), (0.5, 3.1e-4))]


def _clip_errors(case, weight_decay, device=None):
    step, gscale, coef = case
    p, g, m, v = R.adam_state(R.ADAM_N, step, weight_decay, seed=620 + step)
    hyper = (R.ADAM_LR, 0.9, 0.999, 1e-8, step, gscale, weight_decay, np.float32(coef))
    ds, mr, vr = G.clipped_adam_ref(p, g, m, v, *hyper)
    p1, m1, v1 = G.clipped_adam_emulate_f32(p, g, m, v, *hyper) if device is None else device((p, g, m, v))
    assert np.isfinite(p1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
    return np.array([R.relerr(p1.astype(np.float64) - p.astype(np.float64), ds).max(), R.relerr(m1, mr).max(), R.relerr(v1, vr).max()])


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adam_table_clip_arithmetic(weight_decay):
    """(c) m, v and the step p_new - p_old element by element against float64 Adam on the gradient times fl32(gscale * coef): steps 1
    and 1000, two (gscale, coefficient) pairs.  Bound: 4 x the worst error of the float32 emulation over the same cases."""
    _lib.load()
    floor = np.max([_clip_errors(c, weight_decay) for c in CLIP_CASES], axis=0)
    worst = np.zeros(3)
    for case in CLIP_CASES:
        step, gscale, coef = case
        clip = _clip_buffer([1.0, coef, 0.0, 0.0])
        got = _clip_errors(case, weight_decay, device=lambda s: _Job(s).adam(step, gscale, weight_decay, clip=clip))
        print("PARITY adam_table_clip step %4d gscale %.1f coef %.2e wd %.1f: step %.3e  m %.3e  v %.3e" % (step, gscale, coef, weight_decay, *got))
        worst = np.maximum(worst, got)
    for k, name in enumerate(("step", "m", "v")):
        print("PARITY adam_table_clip wd %.1f worst %-4s %.3e  emulation floor %.3e  bound %.3e" % (weight_decay, name, worst[k], floor[k], 4 * floor[k]))
    for k, name in enumerate(("step", "m", "v")):
        assert worst[k] <= 4 * floor[k], "%s: %.3e > 4 x %.3e" % (name, worst[k], floor[k])


def test_adam_table_clip_skips_a_nonfinite_step():
    """(d) flag 1 (what a NaN gradient leaves in the clip buffer): with skip_nonfinite p, m and v keep their bits; without it the NaN
    coefficient reaches every element, as it does in torch."""
    _lib.load()
    state = R.adam_state(R.ADAM_N, 3, 0.1, seed=630)
    clip = _clip_buffer([np.nan, np.nan, 1.0, 0.0])
    job = _Job(state)
    got = job.adam(3, 1.0, 0.1, clip=clip, skip=1)
    for a, b, name in zip(got, (state[0], state[2], state[3]), "pmv"):
        assert a.tobytes() == b.tobytes(), name
    got = job.adam(3, 1.0, 0.1, clip=clip, skip=0)
    for a, name in zip(got, "pmv"):
        assert np.isnan(a).all(), name
    # the flag alone decides: a finite coefficient with the flag set is skipped too, and a clear flag is not
    job = _Job(state)
    got = job.adam(3, 1.0, 0.1, clip=_clip_buffer([1.0, 0.5, 1.0, 0.0]), skip=1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (state[0], state[2], state[3])))
    got = job.adam(3, 1.0, 0.1, clip=_clip_buffer([1.0, 0.5, 0.0, 0.0]), skip=1)
    assert not any(a.tobytes() == b.tobytes() for a, b in zip(got, (state[0], state[2], state[3])))
