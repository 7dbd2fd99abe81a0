"""The encoder BiLSTM recurrence kernels through the C ABI against the float64 helper (oracle/tacotron_oracle.py::bilstm_recurrence,
itself pinned to torch.nn.LSTM by tests/test_oracle_bilstm_cpu.py): the split kernels (t2s_taco_encoder_lstm_split / _bwd_split:
four workgroups per (element, direction) exchanging h / d_h per step through tagged granules) and the one-workgroup kernels
(t2s_taco_encoder_lstm / _bwd), at the shapes where the split grid needs more than one residency round, at the longest sequence
the 12 tag bits allow, and with entries longer than the output's rows (T_out)."""
import pytest
import torch

from oracle import tacotron_oracle as O
from text2speech_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 256
NAN_BITS = 0x7FC00000


def _inputs(B, T, T_out, seed):
    gen = torch.Generator().manual_seed(seed)
    gx = torch.randn(B, T, 8 * H, generator=gen) * 0.5
    whh = [torch.randn(4 * H, H, generator=gen) * 0.06 for _ in range(2)]     # [4H][H], torch's weight_hh layout
    d_out = torch.randn(B, T_out, 2 * H, generator=gen)
    return gx, whh, d_out


def _xbuf(B):
    return torch.zeros(_lib.load().t2s_taco_lstm_xbuf_bytes(B) // 8, dtype=torch.int64, device=DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _check_xbuf(xbuf, what):
    """After every launch on a split buffer: its error word says whether a bounded hand-off wait expired."""
    torch.cuda.synchronize()
    if int(xbuf[-1].item()) != 0:
        pytest.fail("%s: a hand-off wait of the split kernel expired (its results are invalid)" % what)


def _fwd(split, gx_d, whhT_d, len32, B, T, T_out, out, xbuf=None, epoch=0):
    """One forward launch; gates / c start as NaN, so a row the kernel should write and did not shows."""
    gs, cs = _nan(B, T, 2, 4 * H), _nan(B, T, 2, H)
    args = [_lib.ptr(gx_d), _lib.ptr(whhT_d[0]), _lib.ptr(whhT_d[1]), _lib.ptr(len32), _lib.ptr(out), B, T, H, T_out, _lib.ptr(gs),
            _lib.ptr(cs)]
    if split:
        _lib.call("t2s_taco_encoder_lstm_split", *args, _lib.ptr(xbuf), epoch, _lib.current_stream())
        _check_xbuf(xbuf, "forward, epoch %#x" % epoch)
    else:
        _lib.call("t2s_taco_encoder_lstm", *args, _lib.current_stream())
        torch.cuda.synchronize()
    return gs, cs


def _bwd(split, d_out, out, gs, cs, whh_d, len32, B, T, T_out, xbuf=None, epoch=0):
    dgx, hp = _nan(B, T, 8 * H), _nan(B, T, 2 * H)
    args = [_lib.ptr(d_out), _lib.ptr(out), _lib.ptr(gs), _lib.ptr(cs), _lib.ptr(whh_d[0]), _lib.ptr(whh_d[1]), _lib.ptr(len32),
            _lib.ptr(dgx), _lib.ptr(hp), B, T, H, T_out]
    if split:
        _lib.call("t2s_taco_encoder_lstm_bwd_split", *args, _lib.ptr(xbuf), epoch, _lib.current_stream())
        _check_xbuf(xbuf, "BPTT, epoch %#x" % epoch)
    else:
        _lib.call("t2s_taco_encoder_lstm_bwd", *args, _lib.current_stream())
        torch.cuda.synchronize()
    return dgx, hp


def _shifted(out, lens, T):
    """hprev as the BPTT must produce it from the forward's `out` [B][T_out][2H]: a copy (no arithmetic) of the direction's
    previous step, zero at its first step; rows past the length are the caller's (NaN here)."""
    B, T_out, _ = out.shape
    o = torch.cat((out, torch.zeros(B, T + 1 - T_out, 2 * H, device=out.device)), 1)
    hp = torch.cat((torch.cat((torch.zeros(B, 1, H, device=out.device), o[:, :T - 1, :H]), 1), o[:, 1:T + 1, H:]), 2)
    valid = (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).to(out.device)
    return torch.where(valid[..., None], hp, torch.full_like(hp, float("nan"))), valid


def _assert_fwd(what, out, gs, cs, ref, T_out):
    valid = ref["valid"].to(DEV)
    err_o = float((out.double() - ref["out"].to(DEV)).abs().max())
    err_g = float((gs[valid].double() - ref["gates"].to(DEV)[valid]).abs().max())
    err_c = float((cs[valid].double() - ref["c"].to(DEV)[valid]).abs().max())
    assert err_o <= 2e-5 and err_g <= 2e-5 and err_c <= 2e-5, (what, err_o, err_g, err_c)
    # rows past each entry's length are not the kernel's: left as they were
    assert torch.isnan(gs[~valid]).all() and torch.isnan(cs[~valid]).all(), what


def _assert_bwd(what, dgx, hp, out, lens, ref, T):
    want_hp, valid = _shifted(out, lens, T)
    assert torch.equal(hp[valid], want_hp[valid]), what                  # bitwise: a copy of the forward's own h
    assert torch.isnan(hp[~valid]).all() and torch.isnan(dgx[~valid]).all(), what
    rd = ref["dgx"].to(DEV)[valid]
    rel = float((dgx[valid].double() - rd).norm() / rd.norm())
    assert rel <= 1e-4, (what, rel)


def _both_vs_float64(B, T, lens, epochs=(1,), seed=0):
    """Both kernel families, forward then BPTT, against one float64 reference.  The split kernels run once per epoch on one buffer
    per direction of use (as the engine keeps them): a later epoch must not match anything an earlier launch left."""
    T_out = T if lens is None else max(lens)
    gx, whh, d_out = _inputs(B, T, T_out, seed or B * 131 + T)
    ref = O.bilstm_recurrence(gx, whh[0], whh[1], lens, T_out, d_out=d_out)
    gx_d, d_out_d = gx.to(DEV), d_out.to(DEV)
    whh_d = [w.to(DEV) for w in whh]
    whhT_d = [w.t().contiguous() for w in whh_d]
    len32 = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    lens_l = [T] * B if lens is None else lens
    out = _nan(B, T_out, 2 * H)
    gs, cs = _fwd(False, gx_d, whhT_d, len32, B, T, T_out, out)
    _assert_fwd("one-workgroup forward", out, gs, cs, ref, T_out)
    dgx, hp = _bwd(False, d_out_d, out, gs, cs, whh_d, len32, B, T, T_out)
    _assert_bwd("one-workgroup BPTT", dgx, hp, out, lens_l, ref, T)
    xf, xb = _xbuf(B), _xbuf(B)
    for e in epochs:
        out = _nan(B, T_out, 2 * H)
        gs, cs = _fwd(True, gx_d, whhT_d, len32, B, T, T_out, out, xf, e)
        _assert_fwd("split forward, epoch %#x" % e, out, gs, cs, ref, T_out)
    for e in epochs:
        dgx, hp = _bwd(True, d_out_d, out, gs, cs, whh_d, len32, B, T, T_out, xb, e)
        _assert_bwd("split BPTT, epoch %#x" % e, dgx, hp, out, lens_l, ref, T)


def _ragged(B, T):
    """Descending lengths from T down to 1 (both ends present)."""
    if B == 1:
        return [T]
    return sorted([T] + [max(1, T - (i * (T - 1) + B - 2) // (B - 1)) for i in range(1, B)], reverse=True)


@pytest.mark.parametrize("B,T", [
    (32, 48),     # 256 blocks: the last shape that is one residency round
    (33, 40),     # 288 blocks: the 33rd element's groups in a second round; 66 groups, not a multiple of 8
    (40, 64),     # 320 blocks
    (64, 64),     # 512 blocks: two full rounds
])
def test_bilstm_kernels_vs_float64_past_one_residency_round(B, T):
    """Forward out / gates / c within 2e-5 absolute and BPTT dgx within 1e-4 relative (L2) of float64, hprev bitwise the kernel's
    own forward h shifted by a step, for both the split and the one-workgroup kernels, ragged lengths including 1 and T.  (The bars
    come from the split-vs-one-workgroup test; measured on an MI355X at B = 32 / 64 and at T = 4094: at most 5.3e-7 absolute
    forward, 1.6e-7 relative dgx.)"""
    lens = _ragged(B, T)
    assert lens[0] == T and lens[-1] == 1
    _both_vs_float64(B, T, lens, epochs=(1, 2))


def test_bilstm_kernels_longest_tagged_sequence():
    """T = 4094, the longest sequence whose step numbers fit the tag's 12 bits (t2s_taco_encoder_lstm_split rejects T >= 4095),
    at the last epoch (0xFFFFF: tags up to 0xFFFFFFFE) and then epoch 1 on the same buffers."""
    _both_vs_float64(1, 4094, None, epochs=(0xFFFFF, 1), seed=7)


@pytest.mark.parametrize("B,T,T_out,lens", [
    (5, 40, 30, [40, 36, 31, 30, 12]),     # some entries past T_out, others inside
    (3, 48, 24, [48, 40, 25]),             # every entry past T_out: the last one's overrun would land in the guard band
])
def test_bilstm_kernels_clamp_lengths_to_t_out(B, T, T_out, lens):
    """lengths[b] > T_out (a stale max_len at the module level): all four kernels must treat such an entry as T_out long.
    out (forward), d_out and out (read by the BPTT) are the first B entries of NaN-filled buffers with one spare entry and
    (T - T_out) rows after them: the band stays bitwise NaN (nothing wrote there), and the results equal the float64 reference
    on lengths.clamp(max=T_out) - a read past T_out would have pulled NaN or another entry's rows in."""
    item, guard_n = T_out * 2 * H, (T - T_out) * 2 * H + T_out * 2 * H
    clamped = [min(n, T_out) for n in lens]
    gx, whh, d_out = _inputs(B, T, T_out, 977 + B)
    ref = O.bilstm_recurrence(gx, whh[0], whh[1], clamped, T_out, d_out=d_out)
    gx_d = gx.to(DEV)
    whh_d = [w.to(DEV) for w in whh]
    whhT_d = [w.t().contiguous() for w in whh_d]
    len32 = torch.tensor(lens, dtype=torch.int32, device=DEV)

    def banded(fill=None):
        buf = _nan(B * item + guard_n)
        if fill is not None:
            buf[:B * item] = fill.reshape(-1)
        return buf, buf[:B * item].view(B, T_out, 2 * H)

    def band_is_nan(buf):
        return bool((buf[B * item:].view(torch.int32) == NAN_BITS).all())

    for split in (False, True):
        name = "split" if split else "one-workgroup"
        xf, xb = (_xbuf(B), _xbuf(B)) if split else (None, None)
        ob, out = banded()
        gs, cs = _fwd(split, gx_d, whhT_d, len32, B, T, T_out, out, xf, 1)
        assert band_is_nan(ob), "%s forward wrote past its output" % name
        _assert_fwd(name + " forward", out, gs, cs, ref, T_out)
        db, d_o = banded(d_out.to(DEV))
        rb, o_r = banded(out)
        dgx, hp = _bwd(split, d_o, o_r, gs, cs, whh_d, len32, B, T, T_out, xb, 1)
        assert band_is_nan(db) and band_is_nan(rb), name
        assert torch.isfinite(dgx[ref["valid"].to(DEV)]).all(), "%s BPTT read past T_out" % name
        _assert_bwd(name + " BPTT", dgx, hp, o_r, clamped, ref, T)
