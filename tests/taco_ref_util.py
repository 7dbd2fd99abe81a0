"""Plain restatements of the Tacotron decoder's pieces, in whatever floating type their arguments have (float64 for the references,
float32 for the floors), shared by tests/test_tacotron_bwd_kernels_gpu.py, tests/test_tacotron_fwd_kernels_gpu.py and
tests/test_tacotron_wgrad_kernels_gpu.py.  A plain module, imported by the tests; nothing here touches the library."""
import torch
import torch.nn.functional as F


def lstm(x_full, W, bias, c_prev):
    """One LSTMCell on [x | h] with W = [W_ih | W_hh], bias = b_ih + b_hh (torch gate order i, f, g, o): the pre-activations, the
    activated gates, the new cell state and the new h."""
    z = x_full @ W.t() + bias
    i, f, g, o = z.chunk(4, 1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return z, torch.cat([i, f, g, o], 1), c, o * torch.tanh(c)


def att_step(q, pmem, memory, w_prev, wc_prev, K, D, v, lengths):
    """tacotron.py:124-166,379: f = conv1d([w_prev; wc_prev], K); e = v . tanh(q + D f + pmem), -inf from `length` on;
    w = softmax(e); ctx = w . memory; wc = wc_prev + w."""
    T = pmem.size(1)
    f = F.conv1d(torch.stack([w_prev, wc_prev], 1), K, padding=K.size(2) // 2)              # [B, F, T]
    e = torch.tanh(q[:, None, :] + f.transpose(1, 2) @ D.t() + pmem) @ v
    e = e.masked_fill(torch.arange(T)[None, :] >= lengths[:, None], float("-inf"))
    w = torch.softmax(e, 1)
    return w, torch.einsum("bt,bte->be", w, memory), wc_prev + w


# ---- weight gradients of the train step (tests/test_tacotron_wgrad_kernels_gpu.py): what the time-major planes, the ones column and
# the split-K GEMM compute together, written as plain sums.  tests/test_taco_wgrad_ref_cpu.py pins each against torch autograd.

def shift_items(x, shift):
    """[items, C] -> row i holds x[i - shift], zeros for i < shift: with items ordered (step, batch) and shift = B, the previous
    step's value of the same batch entry (h_{t-1}, zero at step 0)."""
    out = torch.zeros_like(x)
    if shift < x.size(0):
        out[shift:] = x[:x.size(0) - shift]
    return out


def with_ones(x):
    """[..., items, C] -> [..., items, C + 1]: a column of ones behind the inputs; its weight-gradient column is the bias gradient."""
    return torch.cat([x, torch.ones(*x.shape[:-1], 1, dtype=x.dtype)], -1)


def items_wgrad(dy, x, lo=0, hi=None):
    """P[m][n] = sum over items lo <= i < hi of dy[i][m] * [x | 1][i][n]: the weight gradient of y = x W^T + b over those items
    (columns [0, C)) and the bias gradient (column C).  An empty range gives zeros."""
    hi = dy.size(0) if hi is None else hi
    return dy[lo:hi].t() @ with_ones(x)[lo:hi]


def conv1d_wgrad(dy, x, Kt):
    """dy [B, Cout, T], x [B, Cin, T] -> (dW [Cout, Cin, Kt], db [Cout]) of y = conv1d(x, W, b, padding = Kt // 2):
    dW[o][c][k] = sum_{b,t} dy[b][o][t] * x[b][c][t + k - Kt // 2], x zero outside [0, T)."""
    T = x.size(2)
    xp = F.pad(x, (Kt // 2, Kt // 2))
    dW = torch.stack([torch.einsum("bot,bct->oc", dy, xp[:, :, k:k + T]) for k in range(Kt)], 2)
    return dW, dy.sum((0, 2))


def context_wgrad(align, dctx):
    """align [B, T, T_in], dctx [T, B, E] -> d_memory [B, T_in, E] of ctx[t][b] = sum_i align[b][t][i] * memory[b][i]."""
    return torch.einsum("bti,tbe->bie", align, dctx)


# ragged lengths per batch size: the longest entry fills T, one entry is 1 where there are three or more
LEN = {1: lambda T: [T], 2: lambda T: [T, max(1, T - 7)], 3: lambda T: [T, max(1, T - 7), 1],
       9: lambda T: [T, max(1, T - 7), max(1, T // 2), T, max(1, T - 15), 1, max(1, T - 2), max(1, T // 3), T]}


def ragged(B, T):
    """LEN[B](T) where the table has B, else the nine-entry pattern repeated."""
    if B in LEN:
        return LEN[B](T)
    return [LEN[9](T)[i % 9] for i in range(B)]
