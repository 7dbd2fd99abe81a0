"""Plain restatements of the Tacotron decoder's pieces, in whatever floating type their arguments have (float64 for the references,
float32 for the floors), shared by tests/test_tacotron_bwd_kernels_gpu.py and tests/test_tacotron_fwd_kernels_gpu.py.  A plain
module, imported by the tests; nothing here touches the library."""
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


# ragged lengths per batch size: the longest entry fills T, one entry is 1 where there are three or more
LEN = {1: lambda T: [T], 2: lambda T: [T, max(1, T - 7)], 3: lambda T: [T, max(1, T - 7), 1],
       9: lambda T: [T, max(1, T - 7), max(1, T // 2), T, max(1, T - 15), 1, max(1, T - 2), max(1, T // 3), T]}


def ragged(B, T):
    """LEN[B](T) where the table has B, else the nine-entry pattern repeated."""
    if B in LEN:
        return LEN[B](T)
    return [LEN[9](T)[i % 9] for i in range(B)]
