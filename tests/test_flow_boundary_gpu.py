"""One kernel per flow boundary and x0 rebuilt in the layer-0 residual GEMM on the GPU: t2s_wg_flow_boundary
against the three launches it replaces and against the window planes' definition, t2s_wg_res_only_start against t2s_wg_start +
t2s_wg_res_only(pair8 = 1), then WN.forward, forward() and infer() on the new path against T2S_FLOW_BOUNDARY=0, the goldens and the
CPU oracle - at the bars tests/test_edge_cases_gpu.py (2e-5 between two kernel paths over the same inputs), test_waveglow_gpu.py and
test_start_fold_gpu.py apply.
Measured on MI355X: every kernel-against-kernel and on-against-off comparison below came out bit-equal (rel 0.0: z_out, log_s, the X
planes, forward z / log_s, infer audio, WN.forward); z against the goldens 3.95e-6 / 3.80e-6 on either path, infer audio 2.70e-6;
stress weights z rel 1.4e-4, max 2.2e-4, worst log_s 1.5e-4 against the f32 oracle."""
import os

import numpy as np
import pytest
import torch

from text2speech_amd import _lib, planes, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FB_TC = 64          # columns per workgroup of flow_boundary_kernel (csrc/waveglow_ops.hip)


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _maxrel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _build(cfg, sd=None):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg) if sd is None else sd, strict=True)
    return m.to(DEV).eval()


def _window_want(z, c_off, nh, taps, nwc, Lp, halo):
    """the window planes by their definition (include/t2s_hip.h): the four column sets of the taps of z[:, c_off:c_off+nh]"""
    B, _, L = z.shape
    hi, lo = planes.start_fold_sets(planes.start_window(z[:, c_off:c_off + nh], taps), False, nwc, 1)
    wh = torch.zeros(B, nwc, Lp, 32, dtype=torch.bfloat16, device=z.device)
    wl = torch.zeros_like(wh)
    wh[:, :, halo:halo + L] = hi.view(B, nwc, 32, L).permute(0, 1, 3, 2)
    wl[:, :, halo:halo + L] = lo.view(B, nwc, 32, L).permute(0, 1, 3, 2)
    return wh, wl


# (c_off, n_half) of the flow before (None: the first flow, no coupling) -> (c_off, n_half) of this flow
_GEOMS = [((0, 4), (0, 4)), ((0, 4), (2, 3)), ((4, 2), (6, 1)), (None, (0, 4))]
# the last two: one column fewer and one more than a workgroup's FB_TC (3 x 64 is the exact fit)
_SHAPES = [(2, 300, 3), (1, 2051, 3), (3, 64, 3), (1, 5, 5), (2, 1, 3), (1, FB_TC - 1, 3), (1, FB_TC + 1, 3)]


@pytest.mark.parametrize("prev,cur", _GEOMS)
@pytest.mark.parametrize("B,L,taps", _SHAPES)
def test_boundary_kernel_vs_the_three_it_replaces(B, L, taps, prev, cur):
    """t2s_wg_flow_boundary against t2s_wg_end_fold_affine -> t2s_wg_convinv -> t2s_wg_start_window on a copy: z_out (all G
    channels) and log_s at rel-L2 2e-5 (printed with whether they are bit-equal, which is expected: same sums in the same order);
    the window planes bit-for-bit the four column sets of the z_out the kernel itself wrote, rows outside [0, L) and unused columns
    zero; the input buffer unchanged.  Then the window-only form (no coupling, no convolution) against t2s_wg_start_window's window
    planes, bit for bit."""
    _lib.load()
    G, C, halo, nslots, nl = 8, 128, 128, 8, 3
    c_off, nh = cur
    n_rem = G - c_off
    ncol = taps * (nh + 1)
    nwc = 2 if 2 * ncol <= 32 else 4
    gen = torch.Generator().manual_seed(1000 * L + 10 * taps + c_off)
    z = torch.randn(B, G, L, generator=gen).to(DEV)
    fold_acc = (0.1 * torch.randn(nslots, B, 8, L, generator=gen)).to(DEV)
    bes = (0.1 * torch.randn(nl, 8, generator=gen)).to(DEV)
    W = torch.randn(8, 8, generator=gen)[:n_rem, :n_rem].contiguous().to(DEV)
    ws = torch.randn(C, nh, generator=gen).to(DEV)
    bs = torch.randn(C, generator=gen).to(DEV)
    Lp = _lib.plane_rows(L, halo)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    st = _lib.current_stream()
    # the three launches, on a copy
    z_ref = z.clone()
    ls_ref = None
    if prev is not None:
        c_off_p, nh_p = prev
        b_end = (0.1 * torch.randn(2 * nh_p, generator=gen)).to(DEV)
        ls_ref = torch.zeros(B, nh_p, L, device=DEV)
        _lib.call("t2s_wg_end_fold_affine", _lib.ptr(fold_acc), nslots, _lib.ptr(bes), nl, _lib.ptr(b_end), _lib.ptr(z_ref),
                  _lib.ptr(ls_ref), None, B, G, c_off_p, nh_p, L, 0, st)
    _lib.call("t2s_wg_convinv", _lib.ptr(z_ref), _lib.ptr(W), B, G, c_off, n_rem, L, st)
    Xh, Xl = torch.zeros(B, C // 32, Lp, 32, **bf), torch.zeros(B, C // 32, Lp, 32, **bf)
    Wh_ref, Wl_ref = torch.zeros(B, nwc, Lp, 32, **bf), torch.zeros(B, nwc, Lp, 32, **bf)
    _lib.call("t2s_wg_start_window", _lib.ptr(z_ref), _lib.ptr(ws), _lib.ptr(bs), B, G, c_off, nh, C, L, Lp, halo, _lib.ptr(Xh),
              _lib.ptr(Xl), taps, nwc, _lib.ptr(Wh_ref), _lib.ptr(Wl_ref), st)
    # the one launch
    z_in = z.clone()
    z_out = torch.full((B, G, L), float("nan"), device=DEV)
    Wh, Wl = torch.zeros(B, nwc, Lp, 32, **bf), torch.zeros(B, nwc, Lp, 32, **bf)
    if prev is not None:
        ls = torch.zeros(B, nh_p, L, device=DEV)
        _lib.call("t2s_wg_flow_boundary", _lib.ptr(z_in), _lib.ptr(z_out), _lib.ptr(fold_acc), nslots, _lib.ptr(bes), nl,
                  _lib.ptr(b_end), _lib.ptr(ls), c_off_p, nh_p, _lib.ptr(W), c_off, n_rem, nh, B, G, L, Lp, halo, taps, nwc,
                  _lib.ptr(Wh), _lib.ptr(Wl), st)
    else:
        _lib.call("t2s_wg_flow_boundary", _lib.ptr(z_in), _lib.ptr(z_out), None, 0, None, 0, None, None, 0, 0, _lib.ptr(W),
                  c_off, n_rem, nh, B, G, L, Lp, halo, taps, nwc, _lib.ptr(Wh), _lib.ptr(Wl), st)
    torch.cuda.synchronize()
    assert torch.equal(z_in, z), "the input buffer changed"
    assert bool(torch.isfinite(z_out).all())
    dz = _rel(z_out, z_ref)
    print("boundary %s -> %s, B %d L %d taps %d: z_out rel %.2e (bit-equal %s)" % (prev, cur, B, L, taps, dz, torch.equal(z_out, z_ref)))
    assert dz < 2e-5, dz
    if prev is not None:
        dl = _rel(ls, ls_ref)
        print("    log_s rel %.2e (bit-equal %s)" % (dl, torch.equal(ls, ls_ref)))
        assert dl < 2e-5, dl
    wh, wl = _window_want(z_out, c_off, nh, taps, nwc, Lp, halo)
    assert torch.equal(Wh, wh) and torch.equal(Wl, wl)
    assert float(Wh[:, :, :halo].float().abs().max()) == 0.0 and float(Wh[:, :, halo + L:].float().abs().max()) == 0.0
    assert float(Wl[:, :, :halo].float().abs().max()) == 0.0 and float(Wl[:, :, halo + L:].float().abs().max()) == 0.0
    # window-only form on the finished columns: what t2s_wg_start_window wrote from them
    Wh2, Wl2 = torch.zeros_like(Wh), torch.zeros_like(Wl)
    z_keep = z_ref.clone()
    _lib.call("t2s_wg_flow_boundary", _lib.ptr(z_ref), None, None, 0, None, 0, None, None, 0, 0, None, c_off, n_rem, nh, B, G, L, Lp,
              halo, taps, nwc, _lib.ptr(Wh2), _lib.ptr(Wl2), st)
    torch.cuda.synchronize()
    assert torch.equal(Wh2, Wh_ref) and torch.equal(Wl2, Wl_ref)
    assert torch.equal(z_ref, z_keep)


@pytest.fixture(scope="module")
def packed_res():
    """The engine's own pack (t2s_pack_conv_weight_table with the residual rows in the PAIR8 order) of a two-layer WN at C = 128 (one
    full 128-row tile) and C = 160 (a second, partial one): layer 0's residual operand of flow 0."""
    out = {}
    for C in (128, 160):
        cfg = dict(synth.WAVEGLOW_SMALL, n_flows=1, WN_config=dict(n_layers=2, n_channels=C, kernel_size=3))
        m = _build(cfg)
        eng = m._eng()
        eng.pack_weights(torch.device(DEV), force=True, res_pair8=True, start_fold=True)
        torch.cuda.synchronize()
        assert eng.packed["res_pair8"]
        ly = eng.packed["flows"][0]["layers"][0]
        out[C] = (m, ly["A2h"], ly["A2l"], ly["b2"], ly["Mpad2"])
    return out


@pytest.mark.parametrize("c_off,nh", [(0, 4), (2, 3), (6, 1)])
@pytest.mark.parametrize("B,L", [(2, 300), (1, 257), (3, 5), (1, 1)])
@pytest.mark.parametrize("C", [128, 160])
def test_res_only_start_vs_start_then_res_only(packed_res, C, B, L, c_off, nh):
    """t2s_wg_res_only_start (x0 rebuilt in the epilogue, X planes only written) against t2s_wg_start followed by
    t2s_wg_res_only(pair8 = 1) in place, on random acts planes: the X planes, hi + lo joined, at rel-L2 2e-5 - bit-equality is
    printed and expected, the value added being the re-rounded x0 - and rows outside [0, L) stay zero."""
    _, A2h, A2l, b2, Mpad2 = packed_res[C]
    G, halo = 8, 128
    gen = torch.Generator().manual_seed(100 * L + 10 * c_off + C)
    z = torch.randn(B, G, L, generator=gen).to(DEV)
    ws = torch.randn(C, nh, generator=gen).to(DEV)
    bs = torch.randn(C, generator=gen).to(DEV)
    acts = torch.randn(B, C, L, generator=gen).to(DEV)
    Lp = _lib.plane_rows(L, halo)
    Ah, Al = planes.to_planes(acts, halo, Lp)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    st = _lib.current_stream()
    Xh0, Xl0 = torch.zeros(B, C // 32, Lp, 32, **bf), torch.zeros(B, C // 32, Lp, 32, **bf)
    _lib.call("t2s_wg_start", _lib.ptr(z), _lib.ptr(ws), _lib.ptr(bs), B, G, c_off, nh, C, L, Lp, halo, _lib.ptr(Xh0), _lib.ptr(Xl0), st)
    _lib.call("t2s_wg_res_only", _lib.ptr(A2h), _lib.ptr(A2l), _lib.ptr(b2), _lib.ptr(Ah), _lib.ptr(Al), _lib.ptr(Xh0), _lib.ptr(Xl0),
              B, C, L, Lp, halo, Mpad2, 1, st)
    Xh, Xl = torch.zeros_like(Xh0), torch.zeros_like(Xl0)
    _lib.call("t2s_wg_res_only_start", _lib.ptr(A2h), _lib.ptr(A2l), _lib.ptr(b2), _lib.ptr(Ah), _lib.ptr(Al), _lib.ptr(z),
              _lib.ptr(ws), _lib.ptr(bs), G, c_off, nh, _lib.ptr(Xh), _lib.ptr(Xl), B, C, L, Lp, halo, Mpad2, st)
    torch.cuda.synchronize()
    got, want = planes.from_planes(Xh, Xl, C, L, halo), planes.from_planes(Xh0, Xl0, C, L, halo)
    d = _rel(got, want)
    print("res_only_start C %d B %d L %d (c_off %d, n_half %d): rel %.2e (planes bit-equal %s)"
          % (C, B, L, c_off, nh, d, torch.equal(Xh, Xh0) and torch.equal(Xl, Xl0)))
    assert float(want.abs().max()) > 0.0
    assert d < 2e-5, d
    for p in (Xh, Xl):
        assert float(p[:, :, :halo].float().abs().max()) == 0.0 and float(p[:, :, halo + L:].float().abs().max()) == 0.0


def _both(monkeypatch, fn):
    """fn() on the one-launch boundaries, then with T2S_FLOW_BOUNDARY=0; each run asserts the path it took"""
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("T2S_FLOW_BOUNDARY", flag)
        out[flag] = fn(flag == "1")
    monkeypatch.delenv("T2S_FLOW_BOUNDARY")
    return out["1"], out["0"]


@pytest.mark.parametrize("name,batch,n,seed", [
    ("waveglow_small_fwd", 2, 4096, 31),
    ("waveglow_small_ragged_fwd", 3, 2400, 32),
])
def test_forward_small_on_vs_off_golden_oracle(monkeypatch, golden_dir, name, batch, n, seed):
    """forward() at the small config on the new path: test_waveglow_gpu.py::test_forward_small_vs_golden's bars (z rel 1e-4 against
    the golden and the oracle, log_s 1e-3, log_det rtol 1e-4), and on against T2S_FLOW_BOUNDARY=0 at 2e-5 on z and the worst log_s."""
    from oracle import waveglow_oracle as O
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = synth.WAVEGLOW_SMALL
    m = _build(cfg)
    eng = m._eng()
    mel, audio = synth.waveglow_inputs(batch, n, seed=seed)

    def run(on):
        with torch.no_grad():
            out = m((mel.to(DEV), audio.to(DEV)))
        torch.cuda.synchronize()
        assert bool(eng.last_path.boundary) == on and bool(eng.packed["start_fold"])
        return out
    (z, log_s, log_det), (z0, log_s0, _) = _both(monkeypatch, run)
    with torch.no_grad():
        zo, lso, ldo = O.waveglow_forward(synth.waveglow_state(cfg), cfg, mel, audio)
    d = _rel(z, z0)
    dls = max(_rel(a, b) for a, b in zip(log_s, log_s0))
    print("%s: boundary on vs off z rel %.2e (bit-equal %s), worst log_s rel %.2e; z vs golden on %.2e off %.2e"
          % (name, d, torch.equal(z, z0), dls, _rel(z, g["z"]), _rel(z0, g["z"])))
    assert _rel(z, g["z"]) < 1e-4 and _maxrel(z, g["z"]) < 1e-3
    assert _rel(z, zo) < 1e-4
    np.testing.assert_allclose([float(x) for x in log_det], g["log_det"], rtol=1e-4, atol=1e-2)
    for k, ls in enumerate(log_s):
        assert _rel(ls, lso[k]) < 1e-3, "flow %d log_s" % k
    assert d < 2e-5 and dls < 2e-5, (d, dls)


def test_infer_small_on_vs_off_golden(monkeypatch, golden_dir):
    """infer() (the window-only boundary and the rebuilt x0; its reverse coupling and inverse convolution keep their kernels) on
    waveglow_small_infer_s0666: the golden at 1e-3, on against off at 2e-5."""
    g = np.load(os.path.join(golden_dir, "waveglow_small_infer_s0666.npz"))
    cfg = synth.WAVEGLOW_SMALL
    m = _build(cfg)
    eng = m._eng()
    gen = torch.Generator().manual_seed(41)
    mel = torch.randn(2, 80, 12, generator=gen)
    noise = (torch.from_numpy(g["noise_final"]), [torch.from_numpy(g[f"noise_early_{i}"]) for i in range(2)])

    def run(on):
        a = m.infer(mel.to(DEV), sigma=0.666, noise=noise)
        assert bool(eng.last_path.boundary) == on and bool(eng.packed["start_fold"])
        return a
    a_on, a_off = _both(monkeypatch, run)
    d = _rel(a_on, a_off)
    print("infer s0666: boundary on vs off audio rel %.2e (bit-equal %s); vs golden on %.2e off %.2e"
          % (d, torch.equal(a_on, a_off), _rel(a_on, g["audio"]), _rel(a_off, g["audio"])))
    assert tuple(a_on.shape) == g["audio"].shape
    assert _rel(a_on, g["audio"]) < 1e-3 and _maxrel(a_on, g["audio"]) < 1e-3
    assert d < 2e-5, d


def test_wn_forward_on_vs_off(monkeypatch):
    """WN[k].forward for flows 0, 5, 11 (n_half 4, 3, 2) at B = 2, L = 600: on against off at 2e-5."""
    cfg = synth.WAVEGLOW_SMALL
    m = _build(cfg)
    eng = m._eng()
    gen = torch.Generator().manual_seed(3)
    B, L = 2, 600
    for k in (0, 5, 11):
        n_half = m.WN[k].start.in_channels
        audio = torch.randn(B, n_half, L, generator=gen)
        spect = torch.randn(B, 640, L, generator=gen)

        def run(on):
            got = m.WN[k]((audio.to(DEV), spect.to(DEV)))
            assert bool(eng.last_path.boundary) == on
            return got
        on, off = _both(monkeypatch, run)
        d = _rel(on, off)
        print("WN[%d] (n_half %d): boundary on vs off rel %.2e (bit-equal %s)" % (k, n_half, d, torch.equal(on, off)))
        assert float(off.abs().max()) > 0.0
        assert d < 2e-5, (k, d)


def test_stress_weights_vs_oracle():
    """the stress weights of test_waveglow_gpu.py::test_stress_weights_forward_and_infer_vs_oracle (WN.end std 0.03, every weight-norm
    gain x 1.25, config.json defaults, 2 x 4096 samples) on the new path at that test's bar: z and every log_s within 1e-3 (rel-L2
    and max for z) of the f32 oracle."""
    from oracle import waveglow_oracle as O
    cfg = synth.WAVEGLOW_DEFAULT
    sd = synth.waveglow_state(cfg, end_std=0.03, wn_gain=1.25)
    m = _build(cfg, sd)
    eng = m._eng()
    mel, audio = synth.waveglow_inputs(2, 4096, seed=31)
    with torch.no_grad():
        z, log_s, _ = m((mel.to(DEV), audio.to(DEV)))
        torch.cuda.synchronize()
        assert bool(eng.last_path.boundary)
        zo, lso, _ = O.waveglow_forward(sd, cfg, mel, audio)
    assert max(float(l.abs().max()) for l in lso) > 2.5          # the stress is real
    rz, mz = _rel(z, zo), _maxrel(z, zo)
    worst_ls = max(_rel(x, y) for x, y in zip(log_s, lso))
    print("stress weights, one-launch boundaries: z rel %.1e max %.1e, worst log_s rel %.1e" % (rz, mz, worst_ls))
    assert rz < 1e-3 and mz < 1e-3, (rz, mz)
    assert worst_ls < 1e-3, worst_ls


def test_second_shorter_forward_matches_a_fresh_model():
    """Two forwards of different length on one model, the second shorter: its result is bit for bit a fresh model's, so neither
    the second z buffer nor the window planes carry anything over; and the first call's outputs are still what they were (the
    returned z is the caller's tensor, not a workspace buffer)."""
    cfg = synth.WAVEGLOW_SMALL
    m = _build(cfg)
    mel1, audio1 = synth.waveglow_inputs(2, 4096, seed=7)
    mel2, audio2 = synth.waveglow_inputs(2, 2400, seed=8)
    with torch.no_grad():
        z1, ls1, _ = m((mel1.to(DEV), audio1.to(DEV)))
        z1c, ls1c = z1.clone(), [t.clone() for t in ls1]
        z2, ls2, _ = m((mel2.to(DEV), audio2.to(DEV)))
        assert bool(m._eng().last_path.boundary)
        z2f, ls2f, _ = _build(cfg)((mel2.to(DEV), audio2.to(DEV)))
        z1b, _, _ = m((mel1.to(DEV), audio1.to(DEV)))           # same shape as the first call again
    torch.cuda.synchronize()
    assert torch.equal(z2, z2f)
    for a, b in zip(ls2, ls2f):
        assert torch.equal(a, b)
    assert torch.equal(z1, z1c) and torch.equal(z1b, z1c)
    for a, b in zip(ls1, ls1c):
        assert torch.equal(a, b)


def test_argument_validation_without_launching():
    """Every broken rule returns T2S_EINVAL before anything is launched (the pointers are real, the valid tuple is the one the
    kernel tests run)."""
    lib = _lib.load()
    B, G, L, halo, taps, nwc, C = 1, 8, 40, 128, 3, 2, 128
    Lp = _lib.plane_rows(L, halo)
    z, z2 = torch.zeros(B, G, L, device=DEV), torch.zeros(B, G, L, device=DEV)
    acc, bes, b_end = torch.zeros(8, B, 8, L, device=DEV), torch.zeros(3, 8, device=DEV), torch.zeros(8, device=DEV)
    ls, W = torch.zeros(B, 4, L, device=DEV), torch.eye(8, device=DEV)
    Wh = torch.zeros(B, 4, Lp, 32, dtype=torch.bfloat16, device=DEV)
    Wl = torch.zeros_like(Wh)
    P = _lib.ptr

    def boundary(**ch):
        a = dict(z_in=P(z), z_out=P(z2), fold_acc=P(acc), nslots=8, bes=P(bes), n_layers=3, b_end=P(b_end), log_s=P(ls), c_off_prev=0,
                 n_half_prev=4, W=P(W), c_off=0, n_rem=8, n_half=4, B=B, n_group=G, L=L, Lp=Lp, halo=halo, taps=taps, win_chunks=nwc,
                 W_hi=P(Wh), W_lo=P(Wl), stream=None)
        a.update(ch)
        return lib.t2s_wg_flow_boundary(*a.values())
    bad = [dict(W_hi=None), dict(W_lo=None), dict(z_in=None), dict(z_out=None), dict(z_out=P(z)), dict(n_half_prev=5),
           dict(c_off_prev=2), dict(bes=None), dict(b_end=None), dict(nslots=0), dict(c_off=2, n_rem=7), dict(n_rem=17),
           dict(n_half=5, taps=3, win_chunks=2), dict(taps=5, win_chunks=2), dict(taps=4), dict(win_chunks=3), dict(taps=35, n_half=1, win_chunks=4),
           dict(Lp=Lp - 256), dict(B=0), dict(L=0), dict(n_group=17), dict(c_off=6, n_rem=2, n_half=4), dict(halo=-1)]
    # the tuple the broken ones are made from is itself accepted (real pointers: the launch is harmless)
    assert boundary(stream=_lib.current_stream()) == 0
    for ch in bad:
        assert boundary(**ch) == -1, "t2s_wg_flow_boundary accepted %r" % (ch,)
    # the window-only form needs no z_out
    assert lib.t2s_wg_flow_boundary(P(z), None, None, 0, None, 0, None, None, 0, 0, None, 0, 8, 4, B, G, L, Lp, halo, taps, nwc, P(Wh),
                                    P(Wl), _lib.current_stream()) == 0

    A = torch.zeros(C // 32, 256, 32, dtype=torch.bfloat16, device=DEV)
    bias, ws, bs = torch.zeros(256, device=DEV), torch.zeros(C, 4, device=DEV), torch.zeros(C, device=DEV)
    X = torch.zeros(B, C // 32, Lp, 32, dtype=torch.bfloat16, device=DEV)
    acts = torch.zeros_like(X)

    def res(**ch):
        a = dict(A_hi=P(A), A_lo=P(A), bias=P(bias), acts_hi=P(acts), acts_lo=P(acts), z=P(z), w_start=P(ws), b_start=P(bs), n_group=G, c_off=0,
                 n_half=4, X_hi=P(X), X_lo=P(X), B=B, C=C, L=L, Lp=Lp, halo=halo, Mpad=256, stream=None)
        a.update(ch)
        return lib.t2s_wg_res_only_start(*a.values())
    assert res(stream=_lib.current_stream()) == 0
    for ch in [dict(X_hi=None), dict(X_lo=None), dict(acts_hi=None), dict(A_lo=None), dict(bias=None), dict(z=None), dict(w_start=None),
               dict(b_start=None), dict(n_half=5), dict(n_half=0), dict(c_off=6), dict(c_off=-1), dict(C=144), dict(C=0), dict(Mpad=300),
               dict(C=288), dict(Lp=Lp + 256), dict(B=0), dict(L=0)]:
        assert res(**ch) == -1, "t2s_wg_res_only_start accepted %r" % (ch,)
    torch.cuda.synchronize()
