"""Keyed sampling (include/t2s_hip.h, csrc/sampling.hip): random draws that are a function of (the entry's seed, the element's index
inside the entry) and of nothing else, made on the device straight into the buffers the kernels read.  An entry of a batch therefore
draws the same bits alone and in any batch - ``Tacotron.inference_batch(seeds=)``, ``WaveGlow.infer_batch(seeds=)``."""
import operator

import torch

from . import _lib

SEED_LIMIT = 1 << 63          # seeds lie in [0, 2^63): an int64 tensor holds them, and the kernels read the same bits as uint64


def check_seed(seed, what="seed"):
    """One seed as a Python int in [0, 2^63); raises ValueError otherwise."""
    try:
        seed = operator.index(seed)
    except TypeError:
        raise ValueError("%s must be an integer, got %r" % (what, type(seed).__name__)) from None
    if not 0 <= seed < SEED_LIMIT:
        raise ValueError("%s must lie in [0, 2^63), got %d" % (what, seed))
    return seed


def seeds_tensor(seeds, B, device, what="seeds"):
    """``seeds`` (a sequence of ints, or an int64 tensor on the host or the device) as a contiguous int64 [B] tensor on ``device``.
    Host values are checked: a wrong count or a value outside [0, 2^63) raises ValueError.  A device tensor is used as it is, with
    no read-back: its dtype and shape are checked, its values are not (a negative one is read as the unsigned value of its bits)."""
    if torch.is_tensor(seeds):
        if seeds.dtype != torch.int64:
            raise ValueError("%s: a tensor of seeds must be int64, got %s" % (what, seeds.dtype))
        if seeds.dim() != 1 or seeds.numel() != B:
            raise ValueError("%s has shape %s, the batch holds %d entries" % (what, tuple(seeds.shape), B))
        if seeds.is_cuda:
            if seeds.device != torch.device(device):
                raise ValueError("%s live on %s, the batch on %s" % (what, seeds.device, device))
            return seeds.detach().contiguous()
        if B and int(seeds.min()) < 0:
            raise ValueError("%s must lie in [0, 2^63), got %s" % (what, seeds.tolist()))
        return seeds.detach().to(device)
    try:
        vals = [check_seed(s, what) for s in seeds]
    except TypeError:
        raise ValueError("%s must be a sequence of integers or an int64 tensor, got %r" % (what, type(seeds).__name__)) from None
    if len(vals) != B:
        raise ValueError("%s holds %d values, the batch %d entries" % (what, len(vals), B))
    return torch.tensor(vals, dtype=torch.int64).to(device)


def sigmas_tensor(sigma, B, device, what="sigma"):
    """A per-entry temperature: ``sigma`` as (float for the scalar slot, float32 [B] device tensor or None).  Host values are checked
    (finite, >= 0); a device tensor is used as it is."""
    if not torch.is_tensor(sigma):
        return float(sigma), None
    if not sigma.is_floating_point() or sigma.dim() != 1 or sigma.numel() != B:
        raise ValueError("%s: a tensor must be floating point of shape [%d], got %s %s" % (what, B, sigma.dtype, tuple(sigma.shape)))
    if not sigma.is_cuda:
        if not bool(torch.isfinite(sigma).all()) or bool((sigma < 0).any()):
            raise ValueError("%s must be finite and >= 0, got %s" % (what, sigma.tolist()))
    elif sigma.device != torch.device(device):
        raise ValueError("%s lives on %s, the batch on %s" % (what, sigma.device, device))
    return 1.0, sigma.detach().to(device=device, dtype=torch.float32).contiguous()


def masks_keyed(n_steps, B, row, seeds, keep_prob, device):
    """uint8 [n_steps, B, row]: entry b's bytes are ``t2s_bernoulli_mask`` over n_steps * row elements under seeds[b]."""
    mk = torch.empty(n_steps, B, row, dtype=torch.uint8, device=device)
    _lib.call("t2s_bernoulli_mask_keyed", _lib.ptr(mk), n_steps, B, row, _lib.ptr(seeds), float(keep_prob), _lib.current_stream())
    return mk


def noise_keyed(z, seeds, sigma=1.0, sigmas=None):
    """Fill the contiguous f32 ``z`` [B, G, L] with sigma_b * unit Gaussian draws keyed by (seeds[b], channel, column): one launch."""
    B, G, L = z.shape
    assert z.dtype == torch.float32 and z.is_contiguous()
    _lib.call("t2s_wg_noise_keyed", _lib.ptr(z), B, G, L, _lib.ptr(seeds), float(sigma), _lib.ptr(sigmas), _lib.current_stream())
    return z


def noise_keyed_at(z, col0, seeds, sigma=1.0, sigmas=None, col0s=None):
    """Fill the contiguous f32 ``z`` [B, G, L] with the draws ``noise_keyed`` puts at columns [col0, col0 + L) of a longer buffer -
    a window of an utterance's noise (streaming.py).  ``col0s`` (int64 [B] on the device): one offset per entry instead."""
    B, G, L = z.shape
    assert z.dtype == torch.float32 and z.is_contiguous()
    _lib.call("t2s_wg_noise_keyed_at", _lib.ptr(z), B, G, L, int(col0), _lib.ptr(col0s), _lib.ptr(seeds), float(sigma),
              _lib.ptr(sigmas), _lib.current_stream())
    return z
