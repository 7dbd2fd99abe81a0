"""CPU side of the gradient-norm / clipping feature: the float64 references of tests/grad_norm_ref.py pinned against torch, the
learning-rate schedule's known answers, and what the new entry points and FusedAdam's constructor refuse - all without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import grad_norm_ref as G
import tail_ref_util as R
from text2speech_amd import _lib, build, optim

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _grads():
    return [R.adam_state(n, 1, 0.0, seed=70 + i)[1] for i, n in enumerate((1, 1023, 1025, 4097))]


@pytest.mark.parametrize("max_norm", [1.0, 1e9])
def test_norm_reference_matches_torch_float64(max_norm):
    """norm_ref against torch.nn.utils.clip_grad_norm_ on float64 copies to 1e-12, and the clipped gradients torch leaves against
    g * min(1, max_norm / (norm + 1e-6)) in float64 (the f32 coefficient of clip_coef_f32 is that value rounded as the kernel rounds
    it: within 3 H)."""
    grads = _grads()
    ps = [torch.zeros(g.size, dtype=torch.float64, requires_grad=True) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g.astype(np.float64))
    want = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    got = G.norm_ref(grads)
    assert abs(got - want) <= 1e-12 * want, (got, want)
    assert abs(G.norm_ref(grads, 0.5) - 0.5 * want) <= 1e-12 * want
    coef64 = min(1.0, max_norm / (want + 1e-6))
    for p, g in zip(ps, grads):
        assert np.allclose(p.grad.numpy(), g.astype(np.float64) * coef64, rtol=1e-12, atol=0.0)
    coef32 = G.clip_coef_f32(np.float32(got), max_norm)
    assert coef32.dtype == np.float32 and abs(float(coef32) - coef64) <= 3 * G.H * coef64
    assert (coef32 == 1.0) == (max_norm > got)


def test_clip_coefficient_special_values():
    f = np.float32
    assert G.clip_coef_f32(f(0.0), 1.0) == f(1.0)
    assert G.clip_coef_f32(f(123.0), math.inf) == f(1.0)
    assert np.isnan(G.clip_coef_f32(f(np.nan), 1.0))
    assert G.clip_coef_f32(f(np.inf), 1.0) == f(0.0)
    assert np.isnan(G.clip_coef_f32(f(np.inf), math.inf))      # inf / inf, as in torch
    assert G.clip_coef_f32(f(4.0), 1.0) == f(1.0) / (f(4.0) + f(1e-6))


def test_clipped_adam_reference_is_adam_on_the_scaled_gradient():
    p, g, m, v = R.adam_state(257, 3, 0.1, seed=5)
    hyper = (R.ADAM_LR, 0.9, 0.999, 1e-8, 3)
    a = G.clipped_adam_ref(p, g, m, v, *hyper, 0.5, 0.1, np.float32(0.37))
    b = R.adam_ref(p, g.astype(np.float64) * float(np.float32(0.5) * np.float32(0.37)), m, v, *hyper, 1.0, 0.1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_learning_rate_decay_known_answers():
    """train.py:62-67: init_lr * sqrt(w) * min(step * w^-1.5, step^-0.5), step = global_step + 1, w = 4000."""
    lr0 = 2e-3
    assert optim.learning_rate_decay(lr0, 0) == pytest.approx(lr0 / 4000, rel=1e-12)
    assert optim.learning_rate_decay(lr0, 3999) == pytest.approx(lr0, rel=1e-12)
    assert optim.learning_rate_decay(lr0, 15999) == pytest.approx(lr0 / 2, rel=1e-12)
    assert optim.learning_rate_decay(lr0, 99, warmup_steps=100.0) == pytest.approx(lr0, rel=1e-12)
    assert isinstance(optim.learning_rate_decay(lr0, 10), float)


def test_grad_norm_partials_is_pure_host(lib):
    assert lib.t2s_grad_norm_partials() > 0


def test_new_entry_points_refuse_without_gpu(lib):
    """T2S_EINVAL before anything touches the device: the pointers below are host memory no kernel may ever see."""
    mem = ctypes.create_string_buffer(256)
    ok = ctypes.cast(mem, ctypes.c_void_p)
    nan, big = float("nan"), 0x80000000

    def norm(jobs=ok, n_jobs=1, total=1, max_norm=1.0, partial=ok, out=ok):
        return lib.t2s_grad_norm_table(jobs, n_jobs, total, 1.0, max_norm, partial, out, None)

    for kw in (dict(jobs=None), dict(partial=None), dict(out=None), dict(n_jobs=0), dict(n_jobs=-1), dict(total=0), dict(total=-1),
               dict(total=big), dict(max_norm=nan), dict(max_norm=-1.0), dict(max_norm=-math.inf)):
        assert norm(**kw) == EINVAL, kw

    def scale(jobs=ok, n_jobs=1, total=1, clip=ok):
        return lib.t2s_grad_scale_table(jobs, n_jobs, total, clip, None)

    for kw in (dict(jobs=None), dict(clip=None), dict(n_jobs=0), dict(total=0), dict(total=big)):
        assert scale(**kw) == EINVAL, kw

    def adam(jobs=ok, n_jobs=1, total=1, step=1, clip=ok):
        return lib.t2s_adam_table_clip(jobs, n_jobs, total, 1e-3, 0.9, 0.999, 1e-8, step, 1.0, 0.0, clip, 0, None)

    for kw in (dict(jobs=None), dict(clip=None), dict(n_jobs=0), dict(total=0), dict(total=big), dict(step=0), dict(step=-1)):
        assert adam(**kw) == EINVAL, kw
    assert mem.raw == bytes(256)


def test_fused_adam_constructor_refuses_bad_max_grad_norm():
    p = [torch.zeros(3, requires_grad=True)]
    for bad in (-1.0, float("nan"), -math.inf):
        with pytest.raises(ValueError):
            optim.FusedAdam(p, max_grad_norm=bad)
    assert optim.FusedAdam(p).max_grad_norm is None
    assert optim.FusedAdam(p, max_grad_norm=0.0).max_grad_norm == 0.0
    assert optim.FusedAdam(p, max_grad_norm=math.inf).max_grad_norm == math.inf
    opt = optim.FusedAdam(p, skip_nonfinite=True)          # alone it implies report-only clipping
    assert opt.max_grad_norm == math.inf and opt.skip_nonfinite and opt.grad_norm is None and opt.found_nonfinite is None


def test_clip_grad_norm_refuses_what_it_cannot_do():
    p = torch.zeros(3, requires_grad=True)
    p.grad = torch.ones(3)
    with pytest.raises(_lib.T2SError):
        optim.clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(_lib.T2SError):
        optim.clip_grad_norm_([p], 1.0, norm_type=math.inf)
    with pytest.raises(_lib.T2SError):                      # a CPU gradient
        optim.clip_grad_norm_([p], 1.0)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], -1.0)
