"""The small WaveGlow stages called directly at more than the one shape of test_small_stages: t2s_small_logdet_inv (n = 1 .. 16, row
exchanges, negative determinants), its _batch and _batch_host forms, t2s_wg_convinv and t2s_wg_audio_squeeze (both directions).
References: torch.linalg in float64 and the float64 product (tests/tail_ref_util.py); every output is a guarded allocation."""
import ctypes

import pytest
import torch

import tail_ref_util as R
from text2speech_amd import _lib
from wg_bwd_util import DEV, Guarded, dev

pytestmark = pytest.mark.gpu
EINVAL = -1
H = R.H


def _st():
    return _lib.current_stream()


def _p(t):
    if t is None:
        return None
    return _lib.ptr(t.t if isinstance(t, Guarded) else t)


def _bits(t):
    return (t.t if isinstance(t, Guarded) else t).view(torch.int32).clone()


def _matrix(kind, n, gen):
    if kind == "random":                        # orthogonal x diagonal in [0.5, 1.5]: condition number <= 3
        W = torch.linalg.qr(torch.randn(n, n, generator=gen))[0] @ torch.diag(torch.rand(n, generator=gen) + 0.5)
    else:                                       # a scaled cyclic shift: zero diagonal (n > 1), every column needs a row exchange
        W = torch.zeros(n, n)
        for i in range(n):
            W[i, (i + 1) % n] = 0.5 + float(torch.rand(1, generator=gen))
    W = W.float().contiguous()
    return W


def _with_sign(W, positive):
    if (torch.linalg.det(W.double()) > 0) != positive:
        W = W.clone()
        W[0] = -W[0]
    return W


def _check_logdet_inv(tag, W, scale, logdet, inv):
    """The kernel eliminates in double and rounds the results to f32 once: H of each value, plus what double Gauss-Jordan leaves on a
    matrix of condition number <= 3 (1e-12 of the largest entry is generous)."""
    W64 = W.double()
    n = W.size(0)
    if inv is not None:
        want = torch.linalg.inv(W64)
        err = (inv.t.cpu().double() - want).abs()
        bound = H * want.abs() + 1e-12 * float(want.abs().max())
        print("PARITY %-58s worst err / bound %.3f" % (tag + " inverse", float((err / bound).max())))
        assert bool((err <= bound).all()), tag
        inv.assert_guards(tag)
    if logdet is not None:
        sign, logabs = torch.linalg.slogdet(W64)
        got = float(logdet.t.cpu()[0])
        if sign > 0:
            want = scale * float(logabs)
            print("PARITY %-58s |err| %.3e  bound %.3e" % (tag + " logdet", abs(got - want), H * abs(want) + 1e-12 * scale * n))
            assert abs(got - want) <= H * abs(want) + 1e-12 * scale * n, (tag, got, want)
        else:
            assert got != got, "%s: logdet of a matrix with negative determinant is %r, not NaN" % (tag, got)
        logdet.assert_guards(tag)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 15, 16])
@pytest.mark.parametrize("kind", ["random", "shift"])
def test_small_logdet_inv(kind, n):
    _lib.load()
    gen = torch.Generator().manual_seed(100 * n + len(kind))
    for positive in (True, False):
        W = _with_sign(_matrix(kind, n, gen), positive)
        if kind == "shift" and n > 1:
            assert float(W.diagonal().abs().max()) == 0.0
        Wd = dev(W)
        for scale in (1.0, 100.0):
            tag = "small_logdet_inv %s n %d det %s scale %g" % (kind, n, "+" if positive else "-", scale)
            logdet, inv = Guarded(1), Guarded(n, n)
            _lib.call("t2s_small_logdet_inv", _p(Wd), n, scale, _p(logdet), _p(inv), _st())
            torch.cuda.synchronize()
            _check_logdet_inv(tag, W, scale, logdet, inv)
            only_ld, only_inv = Guarded(1), Guarded(n, n)
            _lib.call("t2s_small_logdet_inv", _p(Wd), n, scale, _p(only_ld), None, _st())
            _lib.call("t2s_small_logdet_inv", _p(Wd), n, scale, None, _p(only_inv), _st())
            torch.cuda.synchronize()
            assert torch.equal(_bits(only_ld), _bits(logdet)) and torch.equal(_bits(only_inv), _bits(inv)), tag
            only_ld.assert_guards(tag)
            only_inv.assert_guards(tag)
    lib = _lib.load()
    out = Guarded(1)
    assert lib.t2s_small_logdet_inv(_p(Wd), 17, 1.0, _p(out), None, _st()) == EINVAL
    assert lib.t2s_small_logdet_inv(_p(Wd), 0, 1.0, _p(out), None, _st()) == EINVAL
    assert lib.t2s_small_logdet_inv(_p(Wd), n, 1.0, None, None, _st()) == EINVAL
    assert lib.t2s_small_logdet_inv(None, n, 1.0, _p(out), None, _st()) == EINVAL
    torch.cuda.synchronize()
    assert bool(out.untouched(out.t).all())


class _SmallMatJob(ctypes.Structure):
    _fields_ = [("W", ctypes.c_void_p), ("logdet_out", ctypes.c_void_p), ("inv_out", ctypes.c_void_p), ("n", ctypes.c_long)]


def _jobs(sizes, seed):
    """Matrices (some with a negative determinant, some shifts), their single-call results, and fresh guarded outputs per job."""
    gen = torch.Generator().manual_seed(seed)
    Ws, single, outs = [], [], []
    for i, n in enumerate(sizes):
        W = _with_sign(_matrix("shift" if i % 4 == 3 else "random", n, gen), i % 3 != 2)
        Wd = dev(W)
        ld, inv = Guarded(1), Guarded(n, n)
        _lib.call("t2s_small_logdet_inv", _p(Wd), n, 7.0, _p(ld), _p(inv), _st())
        Ws.append(Wd)
        single.append((_bits(ld), _bits(inv)))
        outs.append((Guarded(1), Guarded(n, n)))
    torch.cuda.synchronize()
    return Ws, single, outs


def _assert_same(single, outs):
    torch.cuda.synchronize()
    for i, ((ld0, inv0), (ld, inv)) in enumerate(zip(single, outs)):
        assert torch.equal(_bits(ld), ld0) and torch.equal(_bits(inv), inv0), "job %d differs from the single-matrix call" % i
        ld.assert_guards("job %d logdet" % i)
        inv.assert_guards("job %d inverse" % i)


def test_small_logdet_inv_batch_device_table():
    """12 jobs of sizes 8, 8, 8, 8, 6, 6, 6, 6, 4, 4, 4, 4 in a device table: bit for bit the single-matrix call.  (The device-table
    form cannot validate n: it is never handed one out of range.)"""
    _lib.load()
    sizes = [8] * 4 + [6] * 4 + [4] * 4
    Ws, single, outs = _jobs(sizes, 21)
    table = torch.tensor([[W.data_ptr(), ld.t.data_ptr(), inv.t.data_ptr(), n] for W, (ld, inv), n in zip(Ws, outs, sizes)],
                         dtype=torch.int64).to(DEV)
    _lib.call("t2s_small_logdet_inv_batch", _p(table), len(sizes), 7.0, _st())
    _assert_same(single, outs)
    lib = _lib.load()
    assert lib.t2s_small_logdet_inv_batch(None, 12, 7.0, _st()) == EINVAL
    assert lib.t2s_small_logdet_inv_batch(_p(table), 0, 7.0, _st()) == EINVAL


def test_small_logdet_inv_batch_host_table():
    """16 jobs by value; 17 jobs, n = 17, n = 0 and a NULL W are refused with nothing written."""
    lib = _lib.load()
    sizes = [1, 2, 3, 8, 15, 16, 4, 6, 8, 8, 5, 7, 16, 12, 2, 9]
    Ws, single, outs = _jobs(sizes, 22)

    def table(patch=None, n_entries=17):
        t = (_SmallMatJob * 17)()
        for i in range(min(n_entries, 16)):
            t[i] = _SmallMatJob(Ws[i].data_ptr(), outs[i][0].t.data_ptr(), outs[i][1].t.data_ptr(), sizes[i])
        if n_entries > 16:
            t[16] = t[0]
        for i, (field, value) in (patch or {}).items():
            setattr(t[i], field, value)
        return t

    def call(t, n_jobs):
        return lib.t2s_small_logdet_inv_batch_host(ctypes.cast(t, ctypes.c_void_p), n_jobs, 7.0, _st())

    assert call(table(), 17) == EINVAL
    assert call(table({3: ("n", 17)}), 16) == EINVAL
    assert call(table({15: ("n", 0)}), 16) == EINVAL
    assert call(table({5: ("W", None)}), 16) == EINVAL
    assert call(table(), 0) == EINVAL
    assert lib.t2s_small_logdet_inv_batch_host(None, 16, 7.0, _st()) == EINVAL
    torch.cuda.synchronize()
    for ld, inv in outs:
        assert bool(ld.untouched(ld.t).all()) and bool(inv.untouched(inv.t).all()), "a refused call wrote"
    assert call(table(), 16) == 0
    _assert_same(single, outs)


@pytest.mark.parametrize("L", [1, 255, 256, 257])
@pytest.mark.parametrize("n_rem,c_off", [(2, 0), (2, 6), (8, 0), (16, 0), (8, 8)])
def test_wg_convinv(n_rem, c_off, L):
    """B = 2; channels outside [c_off, c_off + n_rem) keep their bits; W, then the inverse the kernel computed, gives z back."""
    _lib.load()
    B, G = 2, max(c_off + n_rem, 8)
    gen = torch.Generator().manual_seed(1000 * n_rem + 10 * c_off + L)
    W = _matrix("random", n_rem, gen)
    z = torch.randn(B, G, L, generator=gen)
    want, bound = R.convinv_ref(z, W, c_off)
    zg, Wd = Guarded(B, G, L, fill=z), dev(W)
    inv = Guarded(n_rem, n_rem)
    _lib.call("t2s_wg_convinv", _p(zg), _p(Wd), B, G, c_off, n_rem, L, _st())
    _lib.call("t2s_small_logdet_inv", _p(Wd), n_rem, 1.0, None, _p(inv), _st())
    torch.cuda.synchronize()
    zg.assert_guards("convinv")
    got = zg.t.cpu()
    rest = torch.ones(G, dtype=torch.bool)
    rest[c_off:c_off + n_rem] = False
    assert torch.equal(got[:, rest].view(torch.int32), z[:, rest].contiguous().view(torch.int32)), "a channel outside the range changed"
    err = (got.double() - want).abs()[:, ~rest]
    ratio = float((err / bound[:, ~rest]).max())
    print("PARITY wg_convinv n_rem %2d c_off %d L %3d: worst |err| %.3e  worst err / bound %.3f" % (n_rem, c_off, L, float(err.max()), ratio))
    assert ratio <= 1.0
    # back through the kernel's own inverse: the bound of the second product on what the first one returned, plus the first product's
    # error carried through |W^-1|, plus the rounding of W^-1 itself (H |W^-1| |W| |z|)
    back, bound2 = R.convinv_ref(got, inv.t.cpu(), c_off)
    Wi = torch.linalg.inv(W.double()).abs()
    carried = torch.einsum("ij,bjt->bit", Wi, bound[:, ~rest]) + H * torch.einsum("ij,bjt->bit", Wi @ W.double().abs(), z[:, ~rest].double().abs())
    _lib.call("t2s_wg_convinv", _p(zg), _p(inv), B, G, c_off, n_rem, L, _st())
    torch.cuda.synchronize()
    zg.assert_guards("convinv back")
    err = (zg.t.cpu().double() - z.double()).abs()
    assert float(err[:, rest].max()) == 0.0 if bool(rest.any()) else True
    ratio = float((err[:, ~rest] / (bound2[:, ~rest] + carried)).max())
    print("PARITY wg_convinv n_rem %2d c_off %d L %3d: W then W^-1, worst |z' - z| %.3e  worst err / bound %.3f" %
          (n_rem, c_off, L, float(err.max()), ratio))
    assert ratio <= 1.0
    lib = _lib.load()
    before = _bits(zg)
    for args in ((B, G, G - n_rem + 1, n_rem, L), (B, G, -1, n_rem, L), (B, 32, 0, 17, L), (B, G, c_off, 0, L), (0, G, c_off, n_rem, L),
                 (B, G, c_off, n_rem, 0)):
        assert lib.t2s_wg_convinv(_p(zg), _p(Wd), *args, _st()) == EINVAL, args
    torch.cuda.synchronize()
    assert torch.equal(_bits(zg), before)


@pytest.mark.parametrize("L", [1, 257])
@pytest.mark.parametrize("G", [2, 8, 16])
@pytest.mark.parametrize("tail", [0, 5])
def test_wg_audio_squeeze_both_directions(G, L, tail):
    """T = G L and T = G L + 5, B = 2.  Both directions move bits; unsqueeze leaves the tail of audio alone; unsqueeze after squeeze is
    the identity."""
    _lib.load()
    B, T = 2, G * L + tail
    gen = torch.Generator().manual_seed(G * 1000 + L + tail)
    audio = torch.randn(B, T, generator=gen)
    audio_d = Guarded(B, T, fill=audio)
    z = Guarded(B, G, L)
    _lib.call("t2s_wg_audio_squeeze", _p(audio_d), _p(z), B, T, G, L, 0, _st())
    torch.cuda.synchronize()
    z.assert_guards("squeeze")
    audio_d.assert_guards("squeeze (audio is read only)")
    assert torch.equal(_bits(z).cpu(), R.squeeze_ref(audio, G, L).view(torch.int32))
    assert torch.equal(_bits(audio_d).cpu(), audio.view(torch.int32))
    back = Guarded(B, T)
    _lib.call("t2s_wg_audio_squeeze", _p(back), _p(z), B, T, G, L, 1, _st())
    torch.cuda.synchronize()
    back.assert_guards("unsqueeze")
    assert torch.equal(_bits(back)[:, :G * L].cpu(), audio[:, :G * L].contiguous().view(torch.int32))
    if tail:
        assert bool(back.untouched(back.t[:, G * L:]).all()), "unsqueeze wrote the tail of audio"
    lib = _lib.load()
    assert lib.t2s_wg_audio_squeeze(_p(back), _p(z), B, G * L - 1, G, L, 1, _st()) == EINVAL
    assert lib.t2s_wg_audio_squeeze(_p(back), None, B, T, G, L, 1, _st()) == EINVAL
