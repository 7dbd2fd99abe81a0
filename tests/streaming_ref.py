"""Shared by the streaming tests: the float64 oracle on a whole mel and on a window of it with the draws of the window's columns.

One [1, n_group, L] buffer of draws is sliced the way the engine assigns it (glow._Engine.noise_slices): the final n_remaining
channels at the back, in front of them the n_early_size channels re-attached at each early flow, in the inverse flow's order."""
import torch

from text2speech_amd import synth

CFG = synth.WAVEGLOW_SMALL
STRESS = dict(end_std=0.03, wn_gain=1.25)       # the stress weights of tests/test_waveglow_gpu.py
F = 260
SIGMA = 0.666
WINDOWS = ((0, 32), (110, 150), (230, 260))
ORACLE_BAR = 1e-3       # rel-L2 and max-rel against the float64 oracle (tests/test_waveglow_infer_batch_gpu.py)
SOLO_BAR = 1e-4         # rel-L2 against the existing HIP call


def rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def maxrel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def cols(cfg, frames):
    return frames * 256 // cfg["n_group"]


def noise_slices(cfg, z):
    """(final, [early draws in the inverse flow's order]) of a [B, n_group, L] buffer"""
    G, every, size = cfg["n_group"], cfg["n_early_every"], cfg["n_early_size"]
    early_ks = [k for k in reversed(range(cfg["n_flows"])) if k % every == 0 and k > 0]
    n_rem = G - size * len(early_ks)
    early = []
    for k in early_ks:
        c_off = size * (k // every)
        early.append(z[:, c_off - size:c_off])
    return z[:, G - n_rem:], early


def oracle(sd64, cfg, mel, z, lo=0, hi=None, sigma=SIGMA):
    """float64 audio [stride (hi - lo)] of the oracle on mel[:, :, lo:hi] with the draws z sliced to that run's columns"""
    from oracle import waveglow_oracle as O
    hi = mel.size(2) if hi is None else hi
    zz = z[:, :, cols(cfg, lo):cols(cfg, hi)].double()
    nf, ne = noise_slices(cfg, zz)
    with torch.no_grad():
        return O.waveglow_infer(sd64, cfg, mel[:, :, lo:hi].double(), nf, ne, sigma=sigma)[0]


def oracle_window(sd64, cfg, mel, z, f0, f1, halo, sigma=SIGMA):
    """the oracle's samples of frames [f0, f1) from a run on [f0 - left, f1 + right) clipped to the mel"""
    lo, hi = max(0, f0 - halo[0]), min(mel.size(2), f1 + halo[1])
    a = oracle(sd64, cfg, mel, z, lo, hi, sigma)
    return a[256 * (f0 - lo):256 * (f1 - lo)]


def double_state(sd):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
