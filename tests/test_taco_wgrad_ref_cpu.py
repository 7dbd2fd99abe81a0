"""The float64 restatements of the Tacotron weight gradients in tests/taco_ref_util.py (shift_items, with_ones, items_wgrad,
conv1d_wgrad, context_wgrad) against torch autograd of the layers they stand for, in float64 on the CPU.  They are the expectations
of tests/test_tacotron_wgrad_kernels_gpu.py; a mistake in one of them would be a mistake in what the kernels are held to."""
import torch
import torch.nn.functional as F

import taco_ref_util as R

TOL = 1e-12


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_shift_items_is_the_previous_step():
    B, T, C = 3, 4, 2
    h = torch.arange(T * B * C, dtype=torch.float64).view(T, B, C) + 1
    prev = R.shift_items(h.view(T * B, C), B).view(T, B, C)
    assert torch.equal(prev[0], torch.zeros(B, C, dtype=torch.float64))
    assert torch.equal(prev[1:], h[:-1])
    assert torch.equal(R.shift_items(h.view(T * B, C), 0), h.view(T * B, C))
    assert torch.equal(R.shift_items(h.view(T * B, C), T * B + 5), torch.zeros(T * B, C, dtype=torch.float64))


def test_items_wgrad_is_linear_autograd():
    """y = [x | h_prev] W^T + b over (step, batch) items: W's gradient in columns [0, C), b's in the ones column; sub-ranges of the
    items (the split-K slabs) add up to the whole, an empty range is zeros."""
    gen = torch.Generator().manual_seed(1)
    B, T, O, C1, C2 = 3, 11, 6, 5, 4
    items = T * B
    x = torch.randn(items, C1, generator=gen, dtype=torch.float64)
    h = torch.randn(items, C2, generator=gen, dtype=torch.float64)
    dy = torch.randn(items, O, generator=gen, dtype=torch.float64)
    W = torch.randn(O, C1 + C2, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(O, generator=gen, dtype=torch.float64, requires_grad=True)
    hp = torch.zeros(T, B, C2, dtype=torch.float64)
    hp[1:] = h.view(T, B, C2)[:-1]
    y = F.linear(torch.cat([x, hp.view(items, C2)], 1), W, b)
    dW, db = torch.autograd.grad((y * dy).sum(), [W, b])
    P = R.items_wgrad(dy, torch.cat([x, R.shift_items(h, B)], 1))
    assert P.shape == (O, C1 + C2 + 1)
    assert _rel(P[:, :-1], dW) < TOL and _rel(P[:, -1], db) < TOL
    parts = [R.items_wgrad(dy, torch.cat([x, R.shift_items(h, B)], 1), lo, min(lo + 7, items)) for lo in range(0, items, 7)]
    assert _rel(sum(parts), P) < TOL
    assert torch.equal(R.items_wgrad(dy, torch.cat([x, h], 1), items, items), torch.zeros(O, C1 + C2 + 1, dtype=torch.float64))


def test_conv1d_wgrad_is_conv1d_autograd():
    gen = torch.Generator().manual_seed(2)
    for Kt, T in ((5, 9), (1, 4), (3, 2)):
        B, Cin, Cout = 2, 3, 4
        x = torch.randn(B, Cin, T, generator=gen, dtype=torch.float64)
        dy = torch.randn(B, Cout, T, generator=gen, dtype=torch.float64)
        W = torch.randn(Cout, Cin, Kt, generator=gen, dtype=torch.float64, requires_grad=True)
        b = torch.randn(Cout, generator=gen, dtype=torch.float64, requires_grad=True)
        dW, db = torch.autograd.grad((F.conv1d(x, W, b, padding=Kt // 2) * dy).sum(), [W, b])
        gW, gb = R.conv1d_wgrad(dy, x, Kt)
        assert gW.shape == dW.shape and _rel(gW, dW) < TOL and _rel(gb, db) < TOL


def test_context_wgrad_is_autograd():
    gen = torch.Generator().manual_seed(3)
    B, T, T_in, E = 2, 7, 5, 3
    align = torch.randn(B, T, T_in, generator=gen, dtype=torch.float64)
    dctx = torch.randn(T, B, E, generator=gen, dtype=torch.float64)
    memory = torch.randn(B, T_in, E, generator=gen, dtype=torch.float64, requires_grad=True)
    ctx = torch.einsum("bti,bie->tbe", align, memory)
    dmem, = torch.autograd.grad((ctx * dctx).sum(), [memory])
    assert _rel(R.context_wgrad(align, dctx), dmem) < TOL
