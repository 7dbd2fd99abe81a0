"""Host-side helpers for the split-bf16 "plane" layout (text2speech_amd/csrc/t2s_common.h).

Pure tensor reshuffling (plumbing): used by tests and by host code that has to hand an
ordinary [B, C, L] f32 tensor to a kernel that consumes planes.
"""
import torch

from . import _lib


def split_bf16(x):
    """x (f32) -> (hi, lo) bf16 with hi = bf16(x), lo = bf16(x - hi)."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, lo


def split_f16(x):
    """x (f32) -> (hi, lo) fp16 with hi = fp16(x), lo = fp16(x - hi): the operand format of the fp16 vocoder planes (the _h16 entry
    points of include/t2s_hip.h).  |x| > 65504 overflows to inf."""
    hi = x.to(torch.float16)
    lo = (x - hi.to(torch.float32)).to(torch.float16)
    return hi, lo


def to_planes(x, halo, Lp=None, fmt="bf16"):
    """[B, C, L] f32 -> (hi, lo) planes [B, ceil(C/32), Lp, 32] bf16 (fmt = "f16": fp16), data rows at [halo, halo+L)."""
    if fmt not in ("bf16", "f16"):
        raise ValueError("to_planes: fmt is 'bf16' or 'f16', not %r" % (fmt,))
    B, C, L = x.shape
    if Lp is None:
        Lp = _lib.plane_rows(L, halo)
    nc = -(-C // 32)
    xp = torch.zeros(B, nc * 32, L, dtype=torch.float32, device=x.device)
    xp[:, :C] = x
    xp = xp.view(B, nc, 32, L).permute(0, 1, 3, 2)            # [B, nc, L, 32]
    hi, lo = split_bf16(xp) if fmt == "bf16" else split_f16(xp)
    ph = torch.zeros(B, nc, Lp, 32, dtype=hi.dtype, device=x.device)
    pl = torch.zeros_like(ph)
    ph[:, :, halo:halo + L] = hi
    pl[:, :, halo:halo + L] = lo
    return ph, pl


def from_planes(ph, pl, C, L, halo):
    """(hi, lo) planes -> [B, C, L] f32."""
    B, nc = ph.shape[:2]
    v = ph[:, :, halo:halo + L].to(torch.float32) + pl[:, :, halo:halo + L].to(torch.float32)
    return v.permute(0, 1, 3, 2).reshape(B, nc * 32, L)[:, :C].contiguous()


def from_f32_planes(p, C, L, halo):
    B, nc = p.shape[:2]
    return p[:, :, halo:halo + L].permute(0, 1, 3, 2).reshape(B, nc * 32, L)[:, :C].contiguous()


def start_window(a, taps):
    """[B, n_half, L] -> [B, taps * (n_half + 1), L]: the window the folded WN.start reads (include/t2s_hip.h, t2s_wg_start_window)
    as a channel-first tensor.  Channel tap * (n_half + 1) + j is a[j] at t + tap - taps // 2 (zero outside [0, L)); j = n_half is
    the ones-channel, 1 inside [0, L) and zero outside."""
    B, nh, L = a.shape
    x = torch.cat([a, torch.ones(B, 1, L, dtype=a.dtype, device=a.device)], 1)
    xp = torch.nn.functional.pad(x, (taps // 2, taps // 2))
    return torch.cat([xp[:, :, tap:tap + L] for tap in range(taps)], 1)


def start_fold_matrix(w_in, w_start, b_start):
    """Effective in_layers[0] weight [2C, C, taps], WN.start weight [C, n_half(, 1)] and bias [C] -> the composed weight
    [2C, taps * (n_half + 1)] in start_window's channel order: in_layers[0](start(a)) = start_fold_matrix . start_window(a) (+ bias)."""
    C = w_in.size(1)
    wb = torch.cat([w_start.reshape(C, -1), b_start.reshape(C, 1)], 1)
    return torch.einsum("mct,cj->mtj", w_in, wb).reshape(w_in.size(0), -1)


def start_fold_sets(x, is_weight, nwc, axis):
    """The four column sets of the folded WN.start (include/t2s_hip.h) for logical columns x (f32, the columns along `axis`, at most
    32 * nwc / 4 of them) -> (hi, lo) bf16 with 32 * nwc entries along `axis`.  With x = h + l + r: weights (h, l) | split(r) | (h, l) | (l, 0),
    window (h, l) | (h, l) | split(r) | (l, 0); 4 / nwc sets per 32-column chunk, unused columns zero."""
    h, l = split_bf16(x)
    rh, rl = split_bf16(x - (h.to(torch.float32) + l.to(torch.float32)))
    z = torch.zeros_like(l)
    sets = [(h, l), (rh, rl) if is_weight else (h, l), (h, l) if is_weight else (rh, rl), (l, z)]
    spc, ncol = 4 // nwc, x.size(axis)
    shape = list(x.shape)
    shape[axis] = 32 * nwc
    hi, lo = torch.zeros(shape, dtype=torch.bfloat16, device=x.device), torch.zeros(shape, dtype=torch.bfloat16, device=x.device)
    for s_, (a, b) in enumerate(sets):
        c0 = (s_ // spc) * 32 + (s_ % spc) * ncol
        hi.narrow(axis, c0, ncol).copy_(a)
        lo.narrow(axis, c0, ncol).copy_(b)
    return hi, lo
