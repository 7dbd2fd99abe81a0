"""float64 references of the gradient-norm / clipping kernels (csrc/train_ops.hip: grad_norm_*_kernel, grad_scale_table_kernel,
adam_table_clip_kernel), pinned by tests/test_grad_norm_ref_cpu.py.  A plain module, imported by the tests."""
import math

import numpy as np

import tail_ref_util as R

H = R.H


def norm_ref(grads, gscale=1.0):
    """Global L2 norm of f32 gradient arrays times the f32 value of gscale, in float64.  The square of an f32 is exact in double and
    math.fsum adds them without error, so the only roundings are the root's and the product's (2^-53 each)."""
    total = math.fsum(math.fsum((np.asarray(g, dtype=np.float64).ravel() ** 2).tolist()) for g in grads)
    return math.sqrt(total) * float(np.float32(gscale))


def clip_coef_f32(norm, max_norm):
    """grad_norm_final_kernel's out[1] from its out[0]: min(1, max_norm / (norm + 1e-6)) operation by operation in numpy float32, as
    torch computes it on an f32 norm; torch.clamp(max=1) keeps a NaN."""
    f = np.float32
    with np.errstate(all="ignore"):
        c = f(max_norm) / (f(norm) + f(1e-6))
    return c if np.isnan(c) else min(f(1.0), c)


def clipped_gscale(gscale, coef):
    """The gradient scale adam_table_clip_kernel applies: fl32(gscale * clip[1])."""
    return np.float32(gscale) * np.float32(coef)


def clipped_adam_ref(p, g, m, v, lr, b1, b2, eps, step, gscale, weight_decay, coef):
    """float64 Adam on the clipped gradient: (p_new - p, m_new, v_new)."""
    return R.adam_ref(p, g, m, v, lr, b1, b2, eps, step, clipped_gscale(gscale, coef), weight_decay)


def clipped_adam_emulate_f32(p, g, m, v, lr, b1, b2, eps, step, gscale, weight_decay, coef):
    """The kernel's expression in numpy float32 on the clipped gradient: (p_new, m_new, v_new)."""
    return R.adam_emulate_f32(p, g, m, v, lr, b1, b2, eps, step, clipped_gscale(gscale, coef), weight_decay)
