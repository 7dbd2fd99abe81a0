"""Helpers of the WaveGlow backward kernel tests (tests/test_waveglow_bwd_kernels_gpu.py): error measures, guarded f32 outputs,
plane / packed-weight read-back, and the CPU emulation of the split-bf16 arithmetic.  A plain module, imported by the tests."""
import torch

from text2speech_amd import _lib, planes

DEV = "cuda:0"
GUARD = 1024                        # floats in front of and behind every f32 output
_SENTINEL_BITS = 0x7FC0BEEF         # a quiet NaN with a payload: an unwritten defined element is not finite, a guard is compared by bits
# bars (the project's own: tests/test_waveglow_gpu.py test_wn_layer / test_small_stages)
GEMM_NORM, GEMM_MAX = 2e-5, 1e-4
F32_NORM, F32_MAX = 1e-5, 1e-4


def dev(t):
    return t.to(DEV).contiguous()


def rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def maxrel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def check(label, got, want, norm_bar, max_bar):
    """Both error measures of one output against its float64 expectation; prints the figures before it asserts."""
    got = torch.as_tensor(got).double().cpu()
    want = torch.as_tensor(want).double().cpu()
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s: a defined element is not finite (never written?)" % label
    n, m = rel(got, want), maxrel(got, want)
    print("PARITY %-60s norm-rel %.3e  max-rel %.3e" % (label, n, m))
    assert n < norm_bar, "%s: norm-relative error %.3e >= %.1e" % (label, n, norm_bar)
    assert m < max_bar, "%s: max-relative error %.3e >= %.1e (norm-relative %.3e passes)" % (label, m, max_bar, n)
    return n, m


class Guarded:
    """An f32 device tensor of `shape` with GUARD floats either side, everything pre-filled with a NaN sentinel.  `.t` is the
    tensor (16-byte aligned), `.assert_guards()` checks that nothing outside it changed."""

    def __init__(self, *shape, fill=None):
        n = 1
        for s in shape:
            n *= int(s)
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), _SENTINEL_BITS, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + n].view(torch.float32).view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def assert_guards(self, label=""):
        assert bool((self.raw[:GUARD] == _SENTINEL_BITS).all()), "%s: wrote in front of the output" % label
        assert bool((self.raw[GUARD + self.n:] == _SENTINEL_BITS).all()), "%s: wrote behind the output" % label

    def untouched(self, view):
        """True where the elements of `view` (a view of .t) still hold the sentinel."""
        return view.view(torch.int32) == _SENTINEL_BITS


def rand_planes(gen, B, C, L, halo, scale=1.0):
    """Seeded randn [B, C, L] as device planes; returns ((hi, lo), float64 CPU values the planes hold)."""
    x = torch.randn(B, C, L, generator=gen) * scale
    pair = planes.to_planes(dev(x), halo)
    return pair, plane_values(pair, C, L, halo)


def plane_values(pair, C, L, halo, first=0):
    """float64 CPU [B, C, L] of channels [32 first, 32 first + C) of a (hi, lo) plane pair."""
    hi, lo = pair
    nc = -(-C // 32)
    v = hi[:, first:first + nc, halo:halo + L].double() + lo[:, first:first + nc, halo:halo + L].double()
    return v.permute(0, 1, 3, 2).reshape(v.size(0), nc * 32, L)[:, :C].contiguous().cpu()


def plane_rows(pair, first, n_chunks, shift, r0, r1):
    """float64 CPU [B, 32 n_chunks, r1 - r0]: channel-first values of plane rows [r0 + shift, r1 + shift) - what a weight-gradient
    GEMM reads from chunks [first, first + n_chunks) when the tap shift is folded into the pointer.  A pair of rank 2 ([Lp, 32]: a
    constant chunk with batch stride 0) gives B = 1."""
    hi, lo = pair
    if hi.dim() == 2:
        hi, lo = hi[None, None], lo[None, None]
    v = hi[:, first:first + n_chunks, r0 + shift:r1 + shift].double() + lo[:, first:first + n_chunks, r0 + shift:r1 + shift].double()
    return v.permute(0, 1, 3, 2).reshape(v.size(0), n_chunks * 32, r1 - r0).cpu()


def assert_halo_zero(pair, L, halo, label=""):
    for p in pair:
        assert float(p[:, :, :halo].float().abs().max()) == 0.0, "%s: rows in front of the data were written" % label
        assert float(p[:, :, halo + L:].float().abs().max()) == 0.0, "%s: rows behind the data were written" % label


def packed_values(A_hi, A_lo, rows, K, pair8=False):
    """float64 CPU [rows, K] of a packed GEMM A operand [K / 32][Mpad][32] (hi, lo): what the planes hold, rows back in channel
    order when they were packed in PERM_PAIR8 order (packed row 16 m + 4 q + e of a group of 32 = channel 8 q + 4 m + e)."""
    v = (A_hi.double() + A_lo.double()).cpu()                       # [nk, Mpad, 32]
    v = v.permute(1, 0, 2).reshape(v.size(1), -1)[:, :K]             # [Mpad, K]
    if pair8:
        c = torch.arange(rows)
        w = c & 31
        v = v[(c & ~31) + ((w >> 2) & 1) * 16 + (w >> 3) * 4 + (w & 3)]
    return v[:rows].contiguous()


def split3_floor(a, b, eq):
    """The floor of the kernels' arithmetic on the CPU: operands a, b (float64 values that planes hold, i.e. hi + lo exactly) are
    split into hi + lo, the three products hi.hi + hi.lo + lo.hi are contracted by `eq` in float64 and compared with the exact
    contraction.  Returns (norm-relative, max-relative)."""
    def split(x):
        hi = x.to(torch.float32).to(torch.bfloat16).double()
        return hi, x - hi
    ah, al = split(a)
    bh, bl = split(b)
    exact = torch.einsum(eq, a, b)
    emu = torch.einsum(eq, ah, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, al, bh)
    return rel(emu, exact), maxrel(emu, exact)


def wn_eff(v, g):
    """weight_norm written out: w = g v / |v| per output row (g None: w = v)."""
    if g is None:
        return v
    return v * (g / v.flatten(1).norm(dim=1)).view(-1, *([1] * (v.dim() - 1)))
