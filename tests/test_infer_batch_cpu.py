"""WaveGlow.infer_batch without a device: the four _ragged entry points (include/t2s_hip.h) refuse a null `lengths`, null planes
and bad geometry with T2S_EINVAL before anything touches the device - the pointers below are made up and 16-byte aligned, so a
launch would fault - and infer_batch refuses host tensors as infer does."""
import ctypes

import pytest
import torch

from text2speech_amd import _lib, synth


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _p(i):
    """a made-up, distinct, 16-byte-aligned pointer"""
    return ctypes.c_void_p(0x10000 * (i + 1))


B, G, C, L, HALO = 2, 8, 128, 40, 128


def _start(lib, **ch):
    a = dict(z=_p(0), w=_p(1), bias=_p(2), B=B, n_group=G, c_off=0, n_half=4, C=C, L=L, Lp=_lib.plane_rows(L, HALO), halo=HALO,
             X_hi=_p(3), X_lo=_p(4), taps=3, win_chunks=2, W_hi=_p(5), W_lo=_p(6), lengths=_p(7), stream=None)
    a.update(ch)
    return lib.t2s_wg_start_ragged(*a.values())


def _res(lib, **ch):
    a = dict(A_hi=_p(0), A_lo=_p(1), bias=_p(2), acts_hi=_p(3), acts_lo=_p(4), X_hi=_p(5), X_lo=_p(6), B=B, C=C, L=L,
             Lp=_lib.plane_rows(L, HALO), halo=HALO, Mpad=256, pair8=1, lengths=_p(7), stream=None)
    a.update(ch)
    return lib.t2s_wg_res_only_ragged(*a.values())


def _res_start(lib, **ch):
    a = dict(A_hi=_p(0), A_lo=_p(1), bias=_p(2), acts_hi=_p(3), acts_lo=_p(4), z=_p(5), w_start=_p(6), b_start=_p(7), n_group=G,
             c_off=0, n_half=4, X_hi=_p(8), X_lo=_p(9), B=B, C=C, L=L, Lp=_lib.plane_rows(L, HALO), halo=HALO, Mpad=256,
             lengths=_p(10), stream=None)
    a.update(ch)
    return lib.t2s_wg_res_only_start_ragged(*a.values())


def _boundary(lib, **ch):
    a = dict(z_in=_p(0), z_out=_p(1), fold_acc=_p(2), nslots=8, bes=_p(3), n_layers=3, b_end=_p(4), log_s=_p(5), c_off_prev=0,
             n_half_prev=4, W=_p(6), c_off=0, n_rem=8, n_half=4, B=B, n_group=G, L=L, Lp=_lib.plane_rows(L, HALO), halo=HALO, taps=3,
             win_chunks=2, W_hi=_p(7), W_lo=_p(8), lengths=_p(9), stream=None)
    a.update(ch)
    return lib.t2s_wg_flow_boundary_ragged(*a.values())


def test_ragged_entry_points_refuse_bad_arguments(lib):
    Lp = _lib.plane_rows(L, HALO)
    bad = {
        # the window form, then (W_hi = W_lo = NULL) the plain form; one window plane without the other is refused too
        _start: [dict(lengths=None), dict(X_hi=None), dict(X_lo=None), dict(W_hi=None), dict(W_lo=None), dict(z=None), dict(w=None),
                 dict(bias=None), dict(B=0), dict(L=0), dict(C=0), dict(n_half=0), dict(n_half=9), dict(c_off=6), dict(c_off=-1),
                 dict(taps=4), dict(win_chunks=3), dict(taps=5), dict(C=32), dict(Lp=256),
                 dict(W_hi=None, W_lo=None, lengths=None), dict(W_hi=None, W_lo=None, X_hi=None), dict(W_hi=None, W_lo=None, X_lo=None),
                 dict(W_hi=None, W_lo=None, Lp=256), dict(W_hi=None, W_lo=None, B=0), dict(W_hi=None, W_lo=None, n_half=9),
                 dict(W_hi=None, W_lo=None, X_hi=ctypes.c_void_p(0x10008))],
        _res: [dict(lengths=None), dict(X_hi=None), dict(X_lo=None), dict(acts_hi=None), dict(acts_lo=None), dict(A_hi=None),
               dict(A_lo=None), dict(bias=None), dict(bias=ctypes.c_void_p(0x10004)), dict(C=0), dict(C=6), dict(C=48), dict(Mpad=300),
               dict(Mpad=0), dict(C=288), dict(Lp=Lp + 256), dict(Lp=Lp - 256), dict(B=0), dict(L=0)],
        _res_start: [dict(lengths=None), dict(X_hi=None), dict(X_lo=None), dict(acts_hi=None), dict(A_lo=None), dict(bias=None), dict(z=None),
                     dict(w_start=None), dict(b_start=None), dict(n_half=5), dict(n_half=0), dict(c_off=6), dict(c_off=-1), dict(C=144),
                     dict(C=0), dict(Mpad=300), dict(C=288), dict(Lp=Lp + 256), dict(B=0), dict(L=0)],
        _boundary: [dict(lengths=None), dict(W_hi=None), dict(W_lo=None), dict(z_in=None), dict(z_out=None), dict(z_out=_p(0)),
                    dict(n_half_prev=5), dict(c_off_prev=2), dict(bes=None), dict(b_end=None), dict(nslots=0), dict(c_off=2, n_rem=7),
                    dict(n_rem=17), dict(n_half=5), dict(taps=5), dict(taps=4), dict(win_chunks=3), dict(taps=35, n_half=1, win_chunks=4),
                    dict(Lp=Lp - 256), dict(B=0), dict(L=0), dict(n_group=17), dict(c_off=6, n_rem=2, n_half=4), dict(halo=-1)],
    }
    for fn, cases in bad.items():
        for ch in cases:
            assert fn(lib, **ch) == -1, "%s accepted %r" % (fn.__name__, ch)


def test_infer_batch_refuses_host_tensors():
    """before any validation of the lengths or any launch: the error infer() raises for a host tensor"""
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**synth.WAVEGLOW_SMALL).eval()
    mel = torch.zeros(2, 80, 4)
    with pytest.raises(_lib.T2SError, match="no CPU fallback"):
        m.infer_batch(mel, torch.tensor([4, 2]))
    with pytest.raises(_lib.T2SError, match="no CPU fallback"):
        m.infer(mel)
