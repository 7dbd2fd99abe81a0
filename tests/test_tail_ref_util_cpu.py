"""CPU: pins tests/tail_ref_util.py, the float64 references behind the loss / Adam / audio / small-stage kernel tests - against the
audio oracle at the three golden STFT configurations, torch.nn.functional's MSE and BCE-with-logits, torch.optim.Adam in float64 - and
checks that a float32 evaluation of the kernels' formulas meets the bounds the GPU tests assert (the bounds come from the arithmetic,
not from what a kernel returns)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_ref_util as R
from oracle import audio_oracle as A


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_stft_references_vs_oracle(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "audio_stft.npz"))
    n_fft, hop, B, T = [int(v) for v in g[tag + "_cfg"]]
    audio = torch.from_numpy(g[tag + "_audio"])
    fwd_o, inv_o = A.stft_basis(n_fft, hop, n_fft)
    fwd, inv_t, win_sq = R.stft_operands(n_fft, hop, n_fft, "hann")
    c = n_fft // 2 + 1
    assert torch.equal(fwd, fwd_o[:, 0]) and torch.equal(inv_t[:, :2 * c], inv_o[:, 0].t())
    assert inv_t.size(1) == R.ru(2 * c, 16) and float(inv_t[:, 2 * c:].abs().max()) == 0.0
    # the oracle is one float32 evaluation, the helper's float32 evaluation another: both within the same floor of float64
    (ft, mag, ph), (e_ft, e_mag, _) = R.f32_floor(R.stft_transform_ref, audio, fwd, n_fft, hop)
    mag_o, ph_o = A.stft_transform(audio, fwd_o, n_fft, hop)
    assert mag.shape == mag_o.shape == (B, c, T // hop + 1)
    assert float((mag_o.double() - mag).abs().max()) <= 4 * e_mag
    big = mag > 1e3 * e_ft
    assert float(R.angle_diff(ph_o, ph)[big].max()) < 1e-3 + 2 * e_ft / float(mag[big].min())
    want, e_out = R.f32_floor(R.stft_inverse_ref, mag_o, ph_o, inv_t, n_fft, hop, win_sq)
    rec_o = A.stft_inverse(mag_o, ph_o, inv_o, n_fft, hop, n_fft)[:, 0]
    assert rec_o.shape == want.shape
    assert float((rec_o.double() - want).abs().max()) <= 4 * e_out
    # and against what the reference's own class produced
    assert float((torch.from_numpy(g[tag + "_mag"]).double() - mag).abs().max()) <= 4 * e_mag


def test_stft_inverse_reference_unusual_windows():
    """window=None (no normalisation), a centre-padded short window, and a hop past the window (window-sum-square 0 in places): the
    helper against the oracle's conv_transpose1d form."""
    gen = torch.Generator().manual_seed(5)
    for n_fft, hop, win, window, T in [(64, 16, 64, None, 256), (64, 16, 32, "hann", 256), (64, 48, 16, "hann", 480)]:
        audio = torch.rand(2, T, generator=gen) - 0.5
        fwd_o, inv_o = A.stft_basis(n_fft, hop, win, window)
        fwd, inv_t, win_sq = R.stft_operands(n_fft, hop, win, window)
        assert (win_sq is None) == (window is None)
        mag, ph = A.stft_transform(audio, fwd_o, n_fft, hop)
        want, e_out = R.f32_floor(R.stft_inverse_ref, mag, ph, inv_t, n_fft, hop, win_sq)
        rec = A.stft_inverse(mag, ph, inv_o, n_fft, hop, win, window)[:, 0]
        assert float((rec.double() - want).abs().max()) <= 4 * e_out, (n_fft, hop, win, window)
    ws = A.window_sumsquare("hann", 11, 48, 16, 64)
    assert (ws[32:-32] == 0).any() and (ws[32:-32] > 0).any()        # the (64, 48, 16) case does reach both branches


def test_mel_reference_vs_oracle():
    gen = torch.Generator().manual_seed(6)
    audio = torch.rand(2, 2048, generator=gen) * 1.8 - 0.9
    fwd_o, _ = A.stft_basis(1024, 256, 1024)
    basis = torch.from_numpy(A.mel_filterbank(22050, 1024, 80, 0.0, 8000.0))
    want = A.mel_spectrogram(audio, fwd_o, basis.numpy())
    mag, _ = A.stft_transform(audio, fwd_o)
    B, c, F_ = mag.shape
    magT = torch.zeros(B * F_, 528)
    magT[:, :c] = mag.transpose(1, 2).reshape(B * F_, c)
    bp = torch.zeros(80, 528)
    bp[:, :c] = basis
    got = R.mel_ref(magT, bp, B, F_, 1e-5)
    assert float((got - want.double()).abs().max()) < 1e-5
    assert torch.equal(R.mel_ref(magT, bp, B, F_, 0.0), (magT.double() @ bp.double().t()).view(B, F_, 80).transpose(1, 2))


def _loss_inputs(n_mel, n_gate, soft, seed):
    gen = torch.Generator().manual_seed(seed)
    mel, post, target = [torch.randn(n_mel, generator=gen) for _ in range(3)]
    gate = torch.rand(n_gate, generator=gen) * 6 - 3
    plant = torch.tensor([0.0, -0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4])[:n_gate]
    gate[:plant.numel()] = plant
    gate_t = torch.full((n_gate,), 0.3) if soft else (torch.rand(n_gate, generator=gen) > 0.5).float()
    return mel, post, target, gate, gate_t


@pytest.mark.parametrize("n_mel,n_gate,soft", [(255, 37, False), (R.GRID_STRIDE + 1, 1, True), (1, 1000, True)])
def test_taco_loss_reference_vs_torch(n_mel, n_gate, soft):
    mel, post, target, gate, gate_t = _loss_inputs(n_mel, n_gate, soft, n_mel + n_gate)
    out, d_mel, d_post, d_gate = R.taco_loss_ref(mel, post, target, gate, gate_t)
    leaves = [t.double().requires_grad_(True) for t in (mel, post, gate)]
    mel_loss = F.mse_loss(leaves[0], target.double()) + F.mse_loss(leaves[1], target.double())
    gate_loss = F.binary_cross_entropy_with_logits(leaves[2], gate_t.double())
    (mel_loss + gate_loss).backward()
    mel_loss, gate_loss = mel_loss.detach(), gate_loss.detach()
    assert abs(float(out[1]) - float(mel_loss)) <= 1e-13 * float(mel_loss)
    assert abs(float(out[2]) - float(gate_loss)) <= 1e-13 * float(gate_loss)
    assert abs(float(out[0]) - float(mel_loss + gate_loss)) <= 1e-13 * float(out[0])
    for got, leaf in zip((d_mel, d_post, d_gate), leaves):
        assert float((got - leaf.grad).abs().max()) <= 1e-15 + 1e-13 * float(leaf.grad.abs().max())
    assert bool(torch.isfinite(d_gate).all()) and bool(torch.isfinite(out).all())
    # the kernel's formulas in float32 meet the bounds the GPU test asserts
    b = R.taco_loss_bounds(mel, post, target, gate, gate_t)
    o32, *g32 = R.taco_loss_ref(mel, post, target, gate, gate_t, dtype=torch.float32)
    assert bool(((o32.float().double() - out).abs() <= b["out"]).all()), ((o32 - out).abs(), b["out"])
    for got, want, key in zip(g32, (d_mel, d_post, d_gate), ("d_mel", "d_post", "d_gate")):
        assert bool(((got.double() - want).abs() <= b[key]).all()), key


@pytest.mark.parametrize("sigma", [1.0, 0.6])
def test_waveglow_loss_reference(sigma):
    gen = torch.Generator().manual_seed(8)
    z = torch.randn(70001, generator=gen)
    log_s = [torch.randn(n, generator=gen) * 0.3 for n in (1, 65537, 300)]
    log_det = torch.randn(3, generator=gen) * 40
    loss, d_z, scale = R.waveglow_loss_ref(z, log_s, log_det, sigma)
    leaf = z.double().requires_grad_(True)
    sg = float(np.float32(sigma))
    want = ((leaf * leaf).sum() / (2 * sg * sg) - sum(t.double().sum() for t in log_s) - log_det.double().sum()) / z.numel()
    want.backward()
    assert abs(loss - float(want.detach())) <= 1e-13 * scale
    assert float((d_z - leaf.grad).abs().max()) <= 1e-13 * float(leaf.grad.abs().max())
    l32, d32, _ = R.waveglow_loss_ref(z, log_s, log_det, sigma, dtype=torch.float32)
    b_loss, b_dz = R.waveglow_loss_bounds(scale, d_z)
    assert abs(float(np.float32(l32)) - loss) <= b_loss
    assert bool(((d32.double() - d_z).abs() <= b_dz).all())


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adam_reference_vs_torch_float64(weight_decay):
    """Five consecutive steps with carried state: the helper's float64 Adam against torch.optim.Adam on float64 tensors."""
    lr, b1, b2, eps = [float(np.float32(a)) for a in (1e-3, 0.9, 0.999, 1e-8)]
    wd = float(np.float32(weight_decay))
    p0, g, _, _ = R.adam_state(500, 2, weight_decay, seed=3)
    ref = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.astype(np.float64), np.zeros(500), np.zeros(500)
    for step in range(1, 6):
        gk = g.astype(np.float64) * step
        ref.grad = torch.from_numpy(gk.copy())
        opt.step()
        ds, m, v = R.adam_ref(p, gk, m, v, lr, b1, b2, eps, step, 1.0, wd)
        p = p + ds
        assert float(np.abs(p - ref.detach().numpy()).max()) <= 1e-12 * float(np.abs(p).max() + lr)
    st = opt.state[ref]
    assert float(np.abs(m - st["exp_avg"].numpy()).max()) <= 1e-12 * float(np.abs(m).max())
    assert float(np.abs(v - st["exp_avg_sq"].numpy()).max()) <= 1e-12 * float(np.abs(v).max())
    # gscale multiplies the gradient first
    a = R.adam_ref(p0, g, m, v, lr, b1, b2, eps, 6, 0.5, wd)
    b = R.adam_ref(p0, 0.5 * g.astype(np.float64), m, v, lr, b1, b2, eps, 6, 1.0, wd)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_adam_emulation_floor_and_float_bias_correction():
    """The float32 emulation of the kernel's formula against float64 over the kernel test's grid.  With the bias corrections computed in
    double its worst element-wise step error is a few f32 roundings; with the float powf form every element of a step >= 2 at
    beta2 = 0.999 is off by 3e-6: ten times the floor, and outside the kernel test's bound of 4 x the floor."""
    step, m, v = R.adam_emulation_floor(0.0, bc_double=True)
    assert step < 5e-7 and m < 2e-7 and v < 2e-7, (step, m, v)
    old = R.adam_emulation_floor(0.0, bc_double=False)
    assert old[0] > 4 * step and old[1:] == (m, v), old
    case = (2, (0.9, 0.999), 1e-8, 1.0, 77)
    p, g, m0, v0 = R.adam_state(R.ADAM_N, 2, 0.0, 77)
    pe = R.adam_emulate_f32(p, g, m0, v0, R.ADAM_LR, 0.9, 0.999, 1e-8, 2, bc_double=False)[0]
    ds = R.adam_ref(p, g, m0, v0, R.ADAM_LR, 0.9, 0.999, 1e-8, 2)[0]
    e = R.relerr(pe.astype(np.float64), ds)
    assert float(np.median(e[ds != 0])) > 3e-6                       # systematic: the median element, not an outlier
    assert R.adam_case_errors(case, 0.0, True)[0] < 5e-7
    # weight decay moves p = 1e-2 by a step of 1e-3: the rounding of p, 2^-24 |p| / |step|, is part of that floor
    assert R.adam_emulation_floor(0.1, True)[0] < 2e-5


def test_small_stage_references():
    gen = torch.Generator().manual_seed(9)
    audio = torch.rand(2, 3 * 5 + 2, generator=gen)
    z = R.squeeze_ref(audio, 3, 5)
    assert z.shape == (2, 3, 5) and float(z[1, 2, 4]) == float(audio[1, 3 * 4 + 2])
    W = torch.randn(4, 4, generator=gen)
    zz = torch.randn(2, 6, 7, generator=gen)
    out, bound = R.convinv_ref(zz, W, 2)
    assert torch.equal(out[:, :2], zz[:, :2].double()) and float(bound[:, :2].abs().max()) == 0.0
    f32 = torch.einsum("ij,bjt->bit", W, zz[:, 2:])
    assert bool(((f32.double() - out[:, 2:]).abs() <= bound[:, 2:]).all())
