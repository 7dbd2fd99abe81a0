"""The float64 BiLSTM recurrence helper (oracle/tacotron_oracle.py::bilstm_recurrence) against torch.nn.LSTM(bidirectional=True)
in double over pack_padded_sequence: the kernel-level GPU tests of the encoder recurrence (tests/test_bilstm_kernels_gpu.py) rest
on it, so it is pinned here to an implementation it shares no code with."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from oracle import tacotron_oracle as O


@pytest.mark.parametrize("B,T,T_out,C,H,lens", [
    (5, 11, 9, 12, 16, [9, 7, 7, 3, 1]),       # ragged, descending, a one-step entry, T_out < T (the batch tuple's max_len)
    (1, 6, 6, 5, 8, None),                     # no lengths: every entry T long
    (3, 5, 5, 7, 256, [5, 4, 1]),              # the kernels' H
])
def test_bilstm_recurrence_matches_torch_lstm(B, T, T_out, C, H, lens):
    gen = torch.Generator().manual_seed(B * 1000 + T * 10 + H)
    lstm = torch.nn.LSTM(C, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.8 / H ** 0.5))
    x = torch.randn(B, T, C, generator=gen, dtype=torch.float64, requires_grad=True)
    lengths = torch.full((B,), T) if lens is None else torch.tensor(lens)
    d_out = torch.randn(B, T_out, 2 * H, generator=gen, dtype=torch.float64)

    # torch: packed sequence, padded back to T_out rows
    packed = pack_padded_sequence(x, lengths, batch_first=True)
    y, (h_n, c_n) = lstm(packed)
    y, _ = pad_packed_sequence(y, batch_first=True, total_length=T_out)
    (y * d_out).sum().backward()

    # the helper: gx = W_ih x + b_ih + b_hh of both directions, [B][T][8H]
    sfx = ("_l0", "_l0_reverse")
    w_ih = [getattr(lstm, "weight_ih" + s).detach() for s in sfx]
    w_hh = [getattr(lstm, "weight_hh" + s).detach() for s in sfx]
    bias = [(getattr(lstm, "bias_ih" + s) + getattr(lstm, "bias_hh" + s)).detach() for s in sfx]
    xd = x.detach()
    gx = torch.cat([xd @ w_ih[d].t() + bias[d] for d in range(2)], 2)
    r = O.bilstm_recurrence(gx, w_hh[0], w_hh[1], None if lens is None else lengths, T_out, d_out=d_out)
    assert r["out"].dtype == torch.float64 and tuple(r["out"].shape) == (B, T_out, 2 * H)
    assert tuple(r["gates"].shape) == (B, T, 2, 4 * H) and tuple(r["c"].shape) == (B, T, 2, H)
    assert tuple(r["dgx"].shape) == (B, T, 8 * H) and tuple(r["hprev"].shape) == (B, T, 2 * H)
    tol = 1e-12

    assert float((r["out"] - y.detach()).abs().max()) < tol
    # final states: forward direction at t = len - 1, reverse direction at t = 0
    last = lengths - 1
    bi = torch.arange(B)
    assert float((r["c"][bi, last, 0] - c_n[0].detach()).abs().max()) < tol
    assert float((r["c"][:, 0, 1] - c_n[1].detach()).abs().max()) < tol
    assert float((r["out"][bi, last, :H] - h_n[0].detach()).abs().max()) < tol

    # every step's gates and cell state: a torch.nn.LSTMCell walk per entry and direction
    for d in range(2):
        cell = torch.nn.LSTMCell(C, H).double()
        with torch.no_grad():
            cell.weight_ih.copy_(w_ih[d]); cell.weight_hh.copy_(w_hh[d])
            cell.bias_ih.copy_(bias[d]); cell.bias_hh.zero_()
        for b in range(B):
            n = int(lengths[b])
            h = torch.zeros(1, H, dtype=torch.float64)
            c = torch.zeros(1, H, dtype=torch.float64)
            for t in (range(n) if d == 0 else range(n - 1, -1, -1)):
                z = (xd[b:b + 1, t] @ w_ih[d].t() + bias[d] + h @ w_hh[d].t())[0]      # (before h moves on)
                with torch.no_grad():
                    h, c = cell(xd[b:b + 1, t], (h, c))
                want = torch.cat((torch.sigmoid(z[:H]), torch.sigmoid(z[H:2 * H]), torch.tanh(z[2 * H:3 * H]), torch.sigmoid(z[3 * H:])))
                assert float((r["gates"][b, t, d] - want).abs().max()) < tol, (b, t, d)
                assert float((r["c"][b, t, d] - c[0].detach()).abs().max()) < tol, (b, t, d)
    assert not r["gates"][~r["valid"]].any() and not r["c"][~r["valid"]].any()

    # dgx and hprev through what they are for: d x = sum_d dgx_d W_ih_d, d W_hh_d = sum_{b,t} dgx_d (x) hprev_d, d b = sum dgx_d
    dgx, hp = r["dgx"], r["hprev"]
    assert not dgx[~r["valid"]].any() and not hp[~r["valid"]].any()
    dx = sum(dgx[..., d * 4 * H:(d + 1) * 4 * H] @ w_ih[d] for d in range(2))
    assert float((dx - x.grad).abs().max()) < tol * max(1.0, float(x.grad.abs().max()))
    for d, s in enumerate(sfx):
        g = dgx[..., d * 4 * H:(d + 1) * 4 * H].reshape(-1, 4 * H)
        dW = g.t() @ hp[..., d * H:(d + 1) * H].reshape(-1, H)
        ref_w, ref_b = getattr(lstm, "weight_hh" + s).grad, getattr(lstm, "bias_hh" + s).grad
        assert float((dW - ref_w).abs().max()) < tol * max(1.0, float(ref_w.abs().max())), s
        assert float((g.sum(0) - ref_b).abs().max()) < tol * max(1.0, float(ref_b.abs().max())), s
    # hprev is zero at each direction's first step
    assert not hp[:, 0, :H].any() and not hp[bi, last, H:].any()
