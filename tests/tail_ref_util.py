"""float64 references of the kernels either side of the hot path - the two losses (csrc/loss_ops.hip), Adam (csrc/train_ops.hip), the
audio front-end / back-end (csrc/audio_ops.hip) and the small WaveGlow stages - plus float32 evaluations of the same formulas on the
CPU, from which the kernel tests take their bounds.  Plain numpy / torch, no device: imported by tests/test_loss_adam_kernels_gpu.py,
tests/test_audio_kernels_gpu.py, tests/test_waveglow_small_kernels_gpu.py and pinned by tests/test_tail_ref_util_cpu.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

H = 2.0 ** -24                      # half a unit in the last place of an f32 of magnitude 1 (the relative error of one rounding)
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)
GRID_STRIDE = 256 * 256             # elements one sweep of the loss kernels' grid covers


def f64(t):
    if not torch.is_tensor(t):
        return torch.as_tensor(np.asarray(t, dtype=np.float64))      # (a list of Python floats would pass through float32)
    return t.detach().double().cpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# losses
def taco_loss_ref(mel, post, target, gate, gate_t, dtype=torch.float64):
    """include/t2s_hip.h, t2s_taco_loss, evaluated in `dtype` on the f32 inputs: (out[3], d_mel, d_post, d_gate).  float32 gives the
    kernel's own formulas (sums still in double, as the kernel keeps them)."""
    mel, post, target, gate, gate_t = [torch.as_tensor(t).to(dtype).flatten() for t in (mel, post, target, gate, gate_t)]
    n_mel, n_gate = mel.numel(), gate.numel()
    e0, e1 = mel - target, post - target
    terms = torch.clamp(gate, min=0) - gate * gate_t + torch.log1p(torch.exp(-gate.abs()))
    mel_loss = float((e0 * e0).double().sum()) / n_mel + float((e1 * e1).double().sum()) / n_mel
    gate_loss = float(terms.double().sum()) / n_gate
    if dtype == torch.float64:
        s_mel, s_gate = 2.0 / n_mel, 1.0 / n_gate
        sig = torch.sigmoid(gate)
    else:
        s_mel, s_gate = float(np.float32(2.0) / np.float32(n_mel)), float(np.float32(1.0) / np.float32(n_gate))
        sig = 1.0 / (1.0 + torch.exp(-gate))
    out = torch.tensor([mel_loss + gate_loss, mel_loss, gate_loss], dtype=torch.float64)
    return out, e0 * s_mel, e1 * s_mel, (sig - gate_t) * s_gate


def taco_loss_bounds(mel, post, target, gate, gate_t):
    """Element-wise bounds of t2s_taco_loss against taco_loss_ref in float64, from the arithmetic (H = one f32 rounding = 2^-24 relative):

    d_mel = fl(fl(mel - t) * fl(2 / n)): three roundings, 3 H relative; bound 4 H |want| (plus the smallest normal f32: below it a value
      has no relative accuracy).
    d_gate = fl((fl(1 / fl(1 + expf(-x))) - y) / n): expf is good to a unit in the last place = 2 H of e^-x, which moves the sigmoid s
      by at most 2 H s; the sum and the quotient add H each: |ds| <= 4 H s.  The subtraction, 1 / n and the product add 3 H of the
      result.  Bound (8 H s + 4 H |s - y|) / n: twice the worst case, because the library functions are not correctly rounded.  Where
      e^-x overflows f32 (x < -88.7) the kernel's s is exactly 0 and the true one is below the smallest normal f32: the same floor.
    mel loss: each term fl(fl(mel - t)^2) carries 3 H, all terms are positive and added in double, the result is rounded once: 4 H of
      the sum; bound 8 H.
    gate loss: a term is fl(fl(max(x, 0) - fl(x y)) + log1pf(expf(-|x|))): fl(x y) H |x y|, the difference H of itself (<= |x| + |x y|),
      log1pf o expf 4 H of its value (<= log 2), the sum H of the term: bound 4 H mean(|x| + 2 |x y| + 4 log 2 + term), and H of the
      value for the final rounding."""
    x, y = f64(gate).flatten(), f64(gate_t).flatten()
    out, d_mel, d_post, d_gate = taco_loss_ref(mel, post, target, gate, gate_t)
    s = torch.sigmoid(x)
    n_gate = x.numel()
    terms = torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    b_mel_loss = 8 * H * float(out[1])
    b_gate_loss = 4 * H * float((x.abs() + 2 * (x * y).abs() + 4 * math.log(2.0) + terms).sum()) / n_gate + H * float(out[2])
    return {
        "d_mel": 4 * H * d_mel.abs() + F32_MIN_NORMAL,
        "d_post": 4 * H * d_post.abs() + F32_MIN_NORMAL,
        "d_gate": (8 * H * s + 4 * H * (s - y).abs()) / n_gate + F32_MIN_NORMAL,
        "out": torch.tensor([b_mel_loss + b_gate_loss + H * float(out[0]), b_mel_loss, b_gate_loss], dtype=torch.float64),
    }


def waveglow_loss_ref(z, log_s, log_det, sigma, dtype=torch.float64):
    """t2s_waveglow_loss in `dtype`: (loss, d_z, scale) with scale = (|sum z^2 / 2 sigma^2| + |sum log_s| + |sum log_det|) / n_z, the size
    of the three sums whose difference the loss is.  sigma is the f32 value that is passed."""
    z = torch.as_tensor(z).to(dtype).flatten()
    n_z = z.numel()
    sg = float(np.float32(sigma))
    s0 = float((z * z).double().sum()) * (0.5 / (sg * sg))
    s1 = sum(float(f64(t).sum()) for t in log_s)
    s2 = float(f64(log_det).sum())
    if dtype == torch.float64:
        dz_scale = 1.0 / (sg * sg * n_z)
    else:
        dz_scale = float(np.float32(1.0) / (np.float32(sigma) * np.float32(sigma) * np.float32(n_z)))
    return (s0 - s1 - s2) / n_z, z * dz_scale, (abs(s0) + abs(s1) + abs(s2)) / n_z


def waveglow_loss_bounds(scale, d_z):
    """z^2 is one f32 product (H), log_s and log_det enter the double sums exactly, 1 / 2 sigma^2 is formed in double from the f32 sigma,
    the result is rounded to f32 once (H of |loss| <= scale): 2 H scale.  d_z = fl(z * fl(1 / fl(fl(sigma sigma) * n))): 4 H."""
    return 2 * H * scale, 4 * H * d_z.abs() + F32_MIN_NORMAL


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
def adam_ref(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0, weight_decay=0.0):
    """torch.optim.Adam's update in float64 on f32 state, with the f32 values of the hyper-parameters as the kernel receives them:
    (p_new - p, m_new, v_new)."""
    lr, b1, b2, eps, gscale, wd = [float(np.float32(a)) for a in (lr, b1, b2, eps, gscale, weight_decay)]
    p, g, m, v = [np.asarray(a, dtype=np.float64) for a in (p, g, m, v)]
    g = g * gscale
    if wd != 0.0:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    return -(lr / bc1) * m / (np.sqrt(v) / bc2s + eps), m, v


def adam_emulate_f32(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0, weight_decay=0.0, bc_double=True):
    """adam_table_kernel's expression (csrc/train_ops.hip) operation by operation in numpy float32: (p_new, m_new, v_new).
    bc_double: the two bias corrections 1 - beta^step in double and rounded once (what t2s_adam_table passes); False: in float with powf,
    as it was - 1 - powf(0.999f, 2) is 0.00199902 with 13 significant bits left after the cancellation."""
    f = np.float32
    lr, b1, b2, eps, gscale, wd = [f(a) for a in (lr, b1, b2, eps, gscale, weight_decay)]
    p, g, m, v = [np.asarray(a, dtype=f) for a in (p, g, m, v)]
    if bc_double:
        bc1, bc2s = f(1.0 - float(b1) ** step), f(math.sqrt(1.0 - float(b2) ** step))
    else:
        bc1, bc2s = f(1) - np.power(b1, f(step), dtype=f), np.sqrt(f(1) - np.power(b2, f(step), dtype=f), dtype=f)
    g = g * gscale
    if wd != f(0):
        g = g + wd * p
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    p = p - (lr / bc1) * m / (np.sqrt(v) / bc2s + eps)
    assert p.dtype == f and m.dtype == f and v.dtype == f
    return p, m, v


ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_BETAS = ((0.9, 0.999), (0.5, 0.9))
ADAM_EPS = (1e-8, 1e-3)
ADAM_GSCALE = (1.0, 0.5)
ADAM_LR = 1e-3
ADAM_N = 2049                       # two blocks and one element


def adam_state(n, step, weight_decay, seed, p_scale=None):
    """f32 (p, g, m, v) of one job.  Gradients: magnitudes 10^U(-6, 3), random signs, every 7th (from the 4th) an exact zero.  Moments (step > 1): the
    running means such gradients leave, m = g (0.5 + U) and v = g^2 (0.5 + U) (tiny non-zero values where g = 0) - a first moment of the
    gradient's sign, so that b1 m + (1 - b1) g does not cancel: a cancelling element has no relative accuracy in f32 or on the device,
    and would set the bound instead of the formula.  Parameters: zero, so that p_new - p is the step itself; with weight decay
    +-1e-2 (0.5 + U) with the gradient's sign; p_scale: +-p_scale U."""
    r = np.random.RandomState(seed)
    g = (10.0 ** r.uniform(-6, 3, n)) * r.choice([-1.0, 1.0], n)
    g[3::7] = 0.0
    sgn = np.where(g == 0, r.choice([-1.0, 1.0], n), np.sign(g))
    if step > 1:
        m = np.where(g == 0, sgn * 1e-4 * (0.5 + r.uniform(size=n)), g * (0.5 + r.uniform(size=n)))
        v = np.where(g == 0, 1e-8 * (0.5 + r.uniform(size=n)), g * g * (0.5 + r.uniform(size=n)))
    else:
        m, v = np.zeros(n), np.zeros(n)
    if weight_decay != 0.0:
        p = sgn * 1e-2 * (0.5 + r.uniform(size=n))
    elif p_scale:
        p = sgn * p_scale * r.uniform(size=n)
    else:
        p = np.zeros(n)
    return [a.astype(np.float32) for a in (p, g, m, v)]


def adam_cases():
    """The arithmetic grid of the kernel test: (step, (b1, b2), eps, gscale, seed)."""
    out = []
    for step in ADAM_STEPS:
        for betas in ADAM_BETAS:
            for eps in ADAM_EPS:
                for gs in ADAM_GSCALE:
                    out.append((step, betas, eps, gs, 1000 + len(out)))
    return out


def relerr(got, want):
    """Element-wise |got - want| / |want| (0 where both are 0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = np.abs(got - want)
    return np.where(d == 0, 0.0, d / np.maximum(np.abs(want), 1e-300))


def adam_case_errors(case, weight_decay, bc_double=True):
    """Worst element-wise relative error of the float32 emulation against float64 for one grid case: (step, m, v)."""
    step, (b1, b2), eps, gs, seed = case
    p, g, m, v = adam_state(ADAM_N, step, weight_decay, seed)
    pe, me, ve = adam_emulate_f32(p, g, m, v, ADAM_LR, b1, b2, eps, step, gs, weight_decay, bc_double)
    ds, mr, vr = adam_ref(p, g, m, v, ADAM_LR, b1, b2, eps, step, gs, weight_decay)
    return (float(relerr(pe.astype(np.float64) - p.astype(np.float64), ds).max()), float(relerr(me, mr).max()),
            float(relerr(ve, vr).max()))


_ADAM_FLOOR = {}


def adam_emulation_floor(weight_decay, bc_double=True):
    """Worst (step, m, v) error of the emulation over the whole grid.  The kernel test's bound is 4 x this (the device's sqrtf and
    division may differ from numpy's by a unit in the last place, and its compiler fuses multiply-adds)."""
    key = (weight_decay, bc_double)
    if key not in _ADAM_FLOOR:
        e = np.array([adam_case_errors(c, weight_decay, bc_double) for c in adam_cases()])
        _ADAM_FLOOR[key] = tuple(float(x) for x in e.max(axis=0))
    return _ADAM_FLOOR[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# audio
def ru(a, b):
    return -(-a // b) * b


def stft_operands(n_fft, hop, win_length, window, ld_rc=None):
    """The device operands as text2speech_amd.audio.STFT builds them (on the host): fwd [2c, n_fft], inv_t [n_fft, ld_rc] zero padded,
    win_sq [n_fft] or None."""
    from text2speech_amd.audio import STFT
    st = STFT(n_fft, hop, win_length, window)
    c = n_fft // 2 + 1
    fwd = st.forward_basis[:, 0, :].contiguous()
    inv_t = st._inv_basis_t
    if ld_rc is not None and ld_rc != inv_t.size(1):
        wide = torch.zeros(n_fft, ld_rc)
        wide[:, :2 * c] = inv_t[:, :2 * c]
        inv_t = wide
    return fwd, inv_t.contiguous(), (st._win_sq.clone() if window is not None else None)


def reflect_pad(audio, n_fft):
    B, T = audio.shape
    return F.pad(audio.view(B, 1, 1, T), (n_fft // 2, n_fft // 2, 0, 0), mode="reflect").view(B, T + n_fft)


def stft_transform_ref(audio, fwd, n_fft, hop, dtype=torch.float64):
    """t2s_stft_transform as a strided contraction in `dtype`: (ft [B, F, 2c], mag [B, c, F], phase [B, c, F]).  polar() of the result
    gives the form in which a phase is compared where the magnitude is small."""
    c = n_fft // 2 + 1
    xp = reflect_pad(audio, n_fft).to(dtype)
    fr = xp.unfold(1, n_fft, hop)                                   # [B, F, n_fft]
    ft = torch.einsum("bfk,rk->bfr", fr, fwd.to(dtype))
    re, im = ft[:, :, :c], ft[:, :, c:]
    mag = torch.sqrt(re * re + im * im).transpose(1, 2).contiguous()
    ph = torch.atan2(im, re).transpose(1, 2).contiguous()
    return ft, mag, ph


def polar(mag, ph):
    """(mag cos(phase), mag sin(phase)) in float64 from outputs of any precision: the real and imaginary parts again."""
    return f64(mag) * torch.cos(f64(ph)), f64(mag) * torch.sin(f64(ph))


def stft_polar_floor(audio, fwd, n_fft, hop):
    """Worst |mag cos(phase) - re|, |mag sin(phase) - im| of the float32 evaluation."""
    c = n_fft // 2 + 1
    ft = stft_transform_ref(audio, fwd, n_fft, hop)[0]
    _, mag32, ph32 = stft_transform_ref(audio, fwd, n_fft, hop, dtype=torch.float32)
    mc, ms = polar(mag32, ph32)
    return max(float((mc - ft[:, :, :c].transpose(1, 2)).abs().max()), float((ms - ft[:, :, c:].transpose(1, 2)).abs().max()))


def mel_ref(magT, mel_basis_p, B, F_, clip, dtype=torch.float64):
    """t2s_mel_from_mag: magT [B F, ld], mel_basis_p [n_mel, ld] -> [B, n_mel, F]; clip <= 0: the raw product."""
    prod = (magT.to(dtype) @ mel_basis_p.to(dtype).t()).view(B, F_, -1).transpose(1, 2).contiguous()
    if clip > 0:
        prod = torch.log(torch.clamp(prod, min=float(np.float32(clip))))
    return prod


def stft_inverse_ref(mag, ph, inv_t, n_fft, hop, win_sq, bias=None, strength=0.0, dtype=torch.float64):
    """t2s_stft_inverse: recombination (with the denoiser's clamp), frames = rc . inv_basis, overlap-add, division by the window-sum-
    square where it exceeds the smallest normal f32, n_fft / hop, trim: [B, hop (F - 1)]."""
    B, c, F_ = mag.shape
    m, p = mag.to(dtype), ph.to(dtype)
    if bias is not None:
        m = torch.clamp(m - bias.to(dtype).view(1, c, 1) * float(np.float32(strength)), min=0.0)
    rc = torch.cat([m * torch.cos(p), m * torch.sin(p)], dim=1)                       # [B, 2c, F]
    frames = torch.einsum("brf,kr->bfk", rc, inv_t[:, :2 * c].to(dtype))            # [B, F, n_fft]
    n = n_fft + hop * (F_ - 1)
    out = torch.zeros(B, n, dtype=dtype)
    wss = torch.zeros(n, dtype=dtype)
    for f in range(F_):
        out[:, f * hop:f * hop + n_fft] += frames[:, f]
        if win_sq is not None:
            wss[f * hop:f * hop + n_fft] += win_sq.to(dtype)
    if win_sq is not None:
        nz = wss > F32_MIN_NORMAL
        out[:, nz] = out[:, nz] / wss[nz]
        out = out * (float(n_fft) / hop)
    return out[:, n_fft // 2:n_fft // 2 + hop * (F_ - 1)].contiguous()


def f32_floor(fn, *args, **kw):
    """(float64 result, worst absolute element-wise error of the same evaluation in float32): the floor of exact-f32 arithmetic, from
    which a kernel test takes its bound (x 4: the device adds in another order)."""
    want = fn(*args, dtype=torch.float64, **kw)
    got = fn(*args, dtype=torch.float32, **kw)
    if isinstance(want, tuple):
        return want, tuple(float((g.double() - w).abs().max()) for g, w in zip(got, want))
    return want, float((got.double() - want).abs().max())


def angle_diff(a, b):
    """|a - b| on the circle."""
    d = (f64(a) - f64(b)).abs() % (2 * math.pi)
    return torch.minimum(d, 2 * math.pi - d)


# ---------------------------------------------------------------------------------------------------------------------------------
# small WaveGlow stages
def squeeze_ref(audio, G, L):
    """audio [B, T] -> z [B, G, L], z[b][g][t] = audio[b][G t + g]."""
    B = audio.size(0)
    return audio[:, :G * L].reshape(B, L, G).permute(0, 2, 1).contiguous()


def convinv_ref(z, W, c_off):
    """(float64 result, element-wise bound): channels [c_off, c_off + n) of z [B, G, L] times W [n, n].  An f32 dot product of n terms
    in any order is within n H sum |w_ij z_j| of the exact one (each product one rounding, each partial sum one; fused multiply-adds
    only lower it); bound (n + 1) H sum |w_ij| |z_j|."""
    n = W.size(0)
    z64, W64 = f64(z), f64(W)
    out = z64.clone()
    out[:, c_off:c_off + n] = torch.einsum("ij,bjt->bit", W64, z64[:, c_off:c_off + n])
    bound = torch.zeros_like(out)
    bound[:, c_off:c_off + n] = (n + 1) * H * torch.einsum("ij,bjt->bit", W64.abs(), z64[:, c_off:c_off + n].abs())
    return out, bound
