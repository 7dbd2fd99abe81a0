"""FusedAdam(max_grad_norm=..., skip_nonfinite=...) and optim.clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam
on CPU float64 copies, the skipped non-finite step, the untouched default path, and one real WaveGlow step over gradient views into
the flat buckets.  H = 2^-24; the norm bound (2 H) is derived in tests/test_grad_norm_kernels_gpu.py, the step bound in
tests/test_waveglow_train_gpu.py::test_adam_step_matches_torch."""
import math

import numpy as np
import pytest
import torch

import grad_norm_ref as G
from text2speech_amd import _lib, optim, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = G.H
SHAPES = [(5,), (1030,), (3, 2048)]
MAX_NORM = 1.0


def _sets(grad_scale, seed=17):
    """Synthetic parameters (some near zero, so that the update's own error shows) and gradients of one overall size."""
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(*s, generator=gen) * 0.1 for s in SHAPES]
    ps[0][:3] = torch.tensor([0.0, 1e-5, -3e-4])
    gs = [torch.randn(*s, generator=gen) * grad_scale for s in SHAPES]
    gs[1][3::7] = 0.0
    return ps, gs


def _device_params(ps, gs):
    out = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    for p, g in zip(out, gs):
        p.grad = g.clone().to(DEV)
    return out


def _groups(params, **kw):
    return [dict(params=params[:2], lr=1e-3, **kw), dict(params=params[2:], lr=3e-4, **kw)]


@pytest.mark.parametrize("grad_scale", [0.5, 1e-4], ids=["norm-above-max", "norm-below-max"])
def test_three_clipped_steps_match_torch_float64(grad_scale):
    """Three steps of FusedAdam(max_grad_norm=1, weight_decay=1e-6) over two groups with different lr, the same gradients each step
    (norm ~ 40 or ~ 0.008), against clip_grad_norm_ + torch.optim.Adam in float64.  p_after - p_before element by element: 6 H on the
    parameter plus 36 H on the update (test_adam_step_matches_torch derives both) plus 2 H on the update for the coefficient."""
    _lib.load()
    ps, gs = _sets(grad_scale)
    want_norm = G.norm_ref([g.numpy() for g in gs])
    assert (want_norm > 10 * MAX_NORM) if grad_scale == 0.5 else (want_norm < 0.1 * MAX_NORM)
    params = _device_params(ps, gs)
    ref = [p.double().clone().requires_grad_(True) for p in ps]
    opt = optim.FusedAdam(_groups(params), weight_decay=1e-6, max_grad_norm=MAX_NORM)
    opt_ref = torch.optim.Adam(_groups(ref), weight_decay=1e-6)
    before = [r.detach().clone() for r in ref]
    for step in range(3):
        for r, g in zip(ref, gs):
            r.grad = g.double().clone()
        ref_norm = float(torch.nn.utils.clip_grad_norm_(ref, MAX_NORM))
        opt_ref.step()
        opt.step()
        got_norm, flag = float(opt.grad_norm), float(opt.found_nonfinite)
        print("PARITY FusedAdam clip step %d: grad_norm %.9e  float64 %.9e  err %.3f H (bound 2 H)" %
              (step + 1, got_norm, ref_norm, abs(got_norm - ref_norm) / ref_norm / H))
        assert abs(ref_norm - want_norm) <= 1e-12 * want_norm
        assert abs(got_norm - ref_norm) <= 2 * H * ref_norm and flag == 0.0
    torch.cuda.synchronize()
    for p, g in zip(params, gs):
        assert torch.equal(p.grad.cpu(), g), "FusedAdam.step() changed a gradient"
    worst = 0.0
    for p, r, b in zip(params, ref, before):
        got, want = p.detach().cpu().double() - b, r.detach() - b
        err = (got - want).abs()
        bound = 6 * H * (b.abs() + torch.maximum(got.abs(), want.abs())) + (36 + 2) * H * want.abs()
        worst = max(worst, float((err / (bound + 1e-300)).max()))
        assert bool((want != 0).any())
        assert bool((err <= bound).all()), "step differs from float64 torch by %.3f x its bound" % worst
    print("PARITY FusedAdam(max_grad_norm=1) three steps vs float64 torch, %s: worst err / bound %.3f" %
          ("clipping" if grad_scale == 0.5 else "not clipping", worst))


@pytest.mark.parametrize("grad_scale", [0.5, 1e-4], ids=["norm-above-max", "norm-below-max"])
def test_clip_grad_norm_scales_in_place_and_returns_the_norm(grad_scale):
    _lib.load()
    ps, gs = _sets(grad_scale, seed=23)
    params = _device_params(ps, gs)
    want = G.norm_ref([g.numpy() for g in gs])
    norm = optim.clip_grad_norm_(params, MAX_NORM)
    assert norm.is_cuda and norm.dim() == 0 and norm.dtype == torch.float32
    got = np.float32(norm.item())
    assert abs(float(got) - want) <= 2 * H * want
    coef = G.clip_coef_f32(got, MAX_NORM)
    assert (coef < 1.0) == (grad_scale == 0.5)
    for p, g in zip(params, gs):
        assert p.grad.cpu().numpy().tobytes() == (g.numpy() * coef).astype(np.float32).tobytes()
    # a second call (cached table) sees the clipped gradients (each rounded once: H, the norm 2 H, second order: 4 H); the norm
    # returned first is a tensor of its own
    norm2 = optim.clip_grad_norm_(params, MAX_NORM)
    assert abs(float(norm2) - float(coef) * want) <= 4 * H * float(coef) * want and np.float32(norm.item()) == got
    assert optim.clip_grad_norm_(params, MAX_NORM, error_if_nonfinite=True).is_cuda
    params[1].grad[7] = float("nan")
    with pytest.raises(RuntimeError):
        optim.clip_grad_norm_(params, MAX_NORM, error_if_nonfinite=True)
    with pytest.raises(_lib.T2SError):
        optim.clip_grad_norm_(params, MAX_NORM, norm_type=1)
    params[2].grad = params[2].grad.t().contiguous().t()            # not contiguous
    with pytest.raises(_lib.T2SError):
        optim.clip_grad_norm_(params, MAX_NORM)


def _state_bits(opt, params):
    return [t.detach().clone() for p in params for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]


def test_nonfinite_step_is_skipped_and_the_next_one_is_not():
    _lib.load()
    ps, gs = _sets(0.5, seed=29)
    params = _device_params(ps, gs)
    opt = optim.FusedAdam(_groups(params), skip_nonfinite=True)
    assert opt.max_grad_norm == math.inf
    opt.step()                                               # a clean step: the moments are no longer zero
    assert float(opt.found_nonfinite) == 0.0 and abs(float(opt.grad_norm) - G.norm_ref([g.numpy() for g in gs])) <= 2 * H * float(opt.grad_norm)
    before = _state_bits(opt, params)
    assert all(bool((opt.state[p]["exp_avg"] != 0).any()) for p in params)
    params[1].grad[1029] = float("nan")
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.found_nonfinite) == 1.0 and math.isnan(float(opt.grad_norm))
    for a, b in zip(_state_bits(opt, params), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a skipped step wrote"
    params[1].grad[1029] = 0.25
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.found_nonfinite) == 0.0 and math.isfinite(float(opt.grad_norm))
    after = _state_bits(opt, params)
    assert all(bool(torch.isfinite(a).all()) and not torch.equal(a, b) for a, b in zip(after, before))
    # the stated limit: the skipped step advanced the host step counter
    assert [g["step"] for g in opt.param_groups] == [3, 3]
    # without skip_nonfinite the NaN reaches every parameter, as with torch's clip_grad_norm_ + Adam
    params[1].grad[1029] = float("nan")
    opt2 = optim.FusedAdam(_groups(params), max_grad_norm=MAX_NORM)
    opt2.step()
    assert float(opt2.found_nonfinite) == 1.0 and all(bool(torch.isnan(p).all()) for p in params)


def test_default_path_calls_none_of_the_new_entry_points(monkeypatch):
    _lib.load()
    ps, gs = _sets(0.5, seed=31)
    names = []
    real = _lib.call

    def counting(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    plain = optim.FusedAdam(_groups(_device_params(ps, gs)))
    plain.step()
    plain.step()
    assert names == ["t2s_adam_table"] * 4 and plain.grad_norm is None and plain.found_nonfinite is None
    del names[:]
    clipped = optim.FusedAdam(_groups(_device_params(ps, gs)), max_grad_norm=MAX_NORM)
    clipped.step()
    assert names == ["t2s_grad_norm_table", "t2s_adam_table_clip", "t2s_adam_table_clip"]      # ONE norm over both groups


def test_one_real_waveglow_step_reports_the_norm_and_matches_plain_adam():
    """The 64-channel WaveGlow at 1 x 2048 samples: forward, loss, backward, FusedAdam(max_grad_norm=inf).step().  The table runs over
    gradient views into the flat buckets; the reported norm is within 2 H of the float64 norm of the .grad tensors, and every parameter
    has the bits a twin model stepped by a plain FusedAdam on the same gradients has."""
    from text2speech_amd.glow import WaveGlow, WaveGlowLoss
    _lib.load()
    cfg = synth.WAVEGLOW_SMALL
    mel, audio = synth.waveglow_inputs(1, 2048, seed=3)

    def model():
        m = WaveGlow(**cfg)
        m.load_state_dict(synth.waveglow_state(cfg))
        return m.to(DEV).train()

    m, twin = model(), model()
    WaveGlowLoss(1.0)(m((mel.to(DEV), audio.to(DEV)))).backward()
    torch.cuda.synchronize()
    for p, q in zip(m.parameters(), twin.parameters()):
        assert p.grad is not None
        q.grad = p.grad.detach().clone()
    want = G.norm_ref([p.grad.detach().cpu().numpy() for p in m.parameters()])
    opt = optim.FusedAdam(m.parameters(), lr=1e-3, max_grad_norm=math.inf)
    opt.step()
    optim.FusedAdam(twin.parameters(), lr=1e-3).step()
    torch.cuda.synchronize()
    got = float(opt.grad_norm)
    n = sum(p.numel() for p in m.parameters())
    print("PARITY FusedAdam(max_grad_norm=inf) on WaveGlow 64ch (%d parameters, %d elements): grad_norm %.9e  float64 %.9e  err %.3f H" %
          (len(list(m.parameters())), n, got, want, abs(got - want) / want / H))
    assert abs(got - want) <= 2 * H * want and float(opt.found_nonfinite) == 0.0
    for (name, p), q in zip(m.named_parameters(), twin.parameters()):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), name
